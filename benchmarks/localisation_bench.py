"""The localisation test on the device (te_localisation_f32) beside its torch restatement, in one process on the same tensors.

    python benchmarks/localisation_bench.py [--rounds 9] [--window-ms 50] [--warmup 3] [--skip-model] [--out F]

Prints one JSON line (and writes it to --out):
  * metrics: scoring 128 pairs (64 images x 2 classes sharing 64 label maps) and 1 pair of 224 x 224, mask mode.  heat is
    ops.heatmap of seeded random [P,196] patch maps (bilinear maps have real ties), labels are seeded regions of three
    classes with a tenth of the pixels ignored.  ``kernel`` is ops.localisation_metrics, ``torch`` is
    localisation.reference_metrics on the same DEVICE tensors (one sort per pair).  The versions alternate, --rounds timed
    windows each of at least --window-ms (host clock between two device synchronisations), after warming every shape;
    reported: median, min and max seconds per call.  ``bytes_algorithmic`` = P HW 4 + B HW 8 is what the algorithm has to
    read (every map and every label map once); ``hbm_fraction_of_8TBps`` is that over the kernel's median call time over
    8 TB/s -- a call time (enqueue included), so a floor of the kernel's own share.
  * evaluator: one LocalisationEvaluator.update (one generate_classes pass of K = 2 classes, one heat-map launch, one scoring
    launch) behind vit_base_patch16_224 at batch 64, against ``old``: two generate_LRP calls, one per class, the same
    heat-map launch and the torch scoring; ``explain_only`` is the generate_classes pass alone.
``range_below_old`` is true when the slowest window of the new path is faster than the fastest window of the old one;
``not_slower_beyond_old_spread`` when the new median exceeds the old one by no more than the spread of the old windows.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks._models import vit_b16  # noqa: E402
from benchmarks._timing import HBM_BYTES_PER_S, alternate, summary, wall_window  # noqa: E402  (the wall-window protocol)

DEV = "cuda:0"


def _verdict(old, new):
    return {"speedup_of_medians": round(statistics.median(old) / statistics.median(new), 2),
            "range_below_old": bool(max(new) < min(old)),
            "not_slower_beyond_old_spread": bool(statistics.median(new) <= statistics.median(old) + (max(old) - min(old)))}


def regions(B, side, n_classes, g):
    """label maps [B,side,side]: a class per 16 x 16 cell, a tenth of the pixels ignored"""
    cells = torch.randint(n_classes, (B, side // 16, side // 16), generator=g)
    lab = cells.repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    lab[torch.rand((B, side, side), generator=g) < 0.1] = -1
    return lab


def inputs(B, K, seed=0):
    from transformer_explainability_amd import ops
    g = torch.Generator().manual_seed(seed + B)
    maps = torch.rand((B * K, 196), generator=g).to(DEV)
    heat = ops.heatmap(maps, scale=16, normalise=True)[:, 0].contiguous()
    return dict(heat=heat, labels=regions(B, 224, 3, g).to(DEV), target_id=torch.arange(K).repeat(B).to(DEV),
                image_index=torch.arange(B).repeat_interleave(K).to(DEV))


def bench_metrics(rounds, window, warmup):
    from transformer_explainability_amd import localisation as L, ops
    res = {}
    for B, K in ((64, 2), (1, 1)):
        case = inputs(B, K)
        got, ref = ops.localisation_metrics(**case), L.reference_metrics(**case)
        t = alternate({"kernel": lambda: ops.localisation_metrics(**case), "torch": lambda: L.reference_metrics(**case)},
                      rounds, window, warmup)
        P, HW = B * K, 224 * 224
        nbytes = P * HW * 4 + B * HW * 8
        k = summary(t["kernel"])
        k.update(bytes_algorithmic=nbytes, hbm_fraction_of_8TBps=round(nbytes / statistics.median(t["kernel"]) / HBM_BYTES_PER_S, 4))
        rel = ((got[1] - ref[1]).abs() / ref[1].abs().clamp(min=1e-300)).max()
        res[f"pairs{P}.images{B}.224x224"] = {"kernel": k, "torch": summary(t["torch"]), **_verdict(t["torch"], t["kernel"]),
                                              "stats_equal": bool(torch.equal(got[0], ref[0])),
                                              "max_rel_energy_kernel_minus_torch": float(rel)}
    return res


def old_update(ev, lrp, x, labels, classes):
    """What a tree without generate_classes and without the kernel does for the same totals: one generate_LRP per class, the
    heat-map launch, the torch scoring on the device."""
    from transformer_explainability_amd import localisation as L, ops
    B, K = classes.shape
    maps = torch.stack([lrp.generate_LRP(x, index=classes[:, k], start_layer=1).detach().reshape(B, -1) for k in range(K)], 1)
    heat = ops.heatmap(maps.reshape(B * K, -1), scale=ev.scale, normalise=True)[:, 0]
    cls = classes.reshape(-1)
    stats, energy = L.reference_metrics(heat, labels=labels, target_id=cls,
                                        image_index=torch.arange(B, device=x.device).repeat_interleave(K))
    ev.add(stats, energy, cls)
    return stats, energy


def bench_evaluator(rounds, window, warmup, B=64, K=2):
    from transformer_explainability_amd import localisation as L
    from transformer_explainability_amd.generators import LRP
    from transformer_explainability_amd.sweep import normalize
    lrp = LRP(vit_b16())
    g = torch.Generator().manual_seed(B)
    x = normalize(torch.rand((B, 3, 224, 224), generator=g).to(DEV))
    labels = regions(B, 224, 1000, g).to(DEV)
    # the two classes of an image: the labels of two of its pixels (an ignored pixel gives class 0, which may have no pixel:
    # that pair is then not counted)
    classes = torch.stack([labels[:, 8, 8].clamp(min=0), labels[:, 120, 120].clamp(min=0)], 1).contiguous()
    ev_new, ev_old = L.LocalisationEvaluator(1000), L.LocalisationEvaluator(1000)
    t = alternate({"new": lambda: ev_new.update(lrp, x, labels=labels, classes=classes, start_layer=1),
                   "old": lambda: old_update(ev_old, lrp, x, labels, classes),
                   "explain_only": lambda: lrp.generate_classes(x, classes=classes, methods=("transformer_attribution",),
                                                                start_layer=1)}, rounds, window, warmup)
    lrp.check()
    row = {k: {"images_per_s": round(B / statistics.median(v), 1), **summary(v, 1e3, "ms")} for k, v in t.items()}
    row.update(_verdict(t["old"], t["new"]))
    row["summary_new"], row["summary_old"] = ev_new.summary(), ev_old.summary()
    return {f"update.vit_base_patch16_224.batch{B}.classes{K}": row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=50.0, help="least duration of a timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "localisation", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    window = partial(wall_window, min_s=a.window_ms / 1e3)
    res["metrics"] = bench_metrics(a.rounds, window, a.warmup)
    if not a.skip_model:
        res["evaluator"] = bench_evaluator(a.rounds, window, a.warmup)
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
