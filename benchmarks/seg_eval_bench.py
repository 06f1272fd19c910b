"""The segmentation test on the device (te_seg_metrics_f32) beside the path it replaces, in one process on the same tensors.

    python benchmarks/seg_eval_bench.py [--batches 1,8,64] [--rounds 9] [--window-ms 50] [--warmup 3] [--skip-model] [--only new|old] [--out F]

Prints one JSON line (and writes it to --out):
  * metrics: one SegmentationEvaluator.update_from_heat per batch of 224 x 224 maps at every --batches size.  heat / mask
    are ops.heatmap of seeded random [B,196] patch maps (bilinear maps have real ties), labels are seeded with 30 %
    foreground.  ``old`` is the update a tree without the kernel performs on CUDA tensors: the four torch functions of
    segmentation.py and the six reads of the running totals; ``new`` is the kernel and its one device-to-host copy;
    ``kernel_only`` is ops.seg_metrics without the copy.  The versions alternate, --rounds timed windows each of at least
    --window-ms (host clock between two device synchronisations: the old path is bound by its own host reads), after
    warming every shape; reported: median, min and max seconds per update.  ``range_below_old`` is true when the slowest
    window of the new path is faster than the fastest window of the old one; ``not_slower_beyond_old_spread`` when the new
    median exceeds the old one by no more than the spread (max - min) of the old windows.
  * evaluator: images per second of SegmentationEvaluator.update behind LRP(vit_base_patch16_224).generate_LRP(x,
    start_layer=1) at batch 64, old and new alternating in the same way.
For a kernel table run the script under ``rocprofv3 --kernel-trace --memory-copy-trace --stats -- python
benchmarks/seg_eval_bench.py --rounds 1 --window-ms 1 --warmup 1 --skip-model --batches 64 --only new`` and again with
``--only old``: one version alone, and ``calls`` says how many updates the launches and copies of the trace belong to.
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


def old_update_from_heat(ev, heat, mask, labels):
    """SegmentationEvaluator.update_from_heat as it is for CPU tensors, which a tree without the kernel also runs on CUDA ones"""
    from transformer_explainability_amd import segmentation as sg
    correct, labeled = sg.pixel_accuracy(mask, labels)
    inter, union = sg.intersection_union(mask, labels)
    ap, f1 = sg.average_precision(heat, labels), sg.row_f1(mask, labels)
    ev.total_correct += int(correct.sum())
    ev.total_label += int(labeled.sum())
    ev.total_inter += inter.sum(0).cpu().numpy()
    ev.total_union += union.sum(0).cpu().numpy()
    ev.total_ap += [float(v) for v in ap.cpu()]
    ev.total_f1 += [r for r in f1.cpu().numpy()]
    return correct, labeled, inter, union, ap, f1


def old_update(ev, image, labels):
    from transformer_explainability_amd import segmentation as sg
    maps = ev.explain(image).detach()
    heat, mask = sg.foreground_split(maps.reshape(maps.shape[0], -1), ev.scale)
    return old_update_from_heat(ev, heat, mask, labels)


def _verdict(t):
    old, new = t["old"], t["new"]
    return {"speedup_of_medians": round(statistics.median(old) / statistics.median(new), 2),
            "range_below_old": bool(max(new) < min(old)),
            "not_slower_beyond_old_spread": bool(statistics.median(new) <= statistics.median(old) + (max(old) - min(old)))}


def inputs(B, seed=0):
    from transformer_explainability_amd import ops, segmentation as sg
    g = torch.Generator().manual_seed(seed + B)
    maps = torch.rand((B, 196), generator=g).to("cuda:0")
    labels = (torch.rand((B, 224, 224), generator=g) > 0.7).long().to("cuda:0")
    heat, mask = ops.heatmap(maps, scale=16, normalise=True, with_mask=True)
    return maps, heat[:, 0], mask[:, 0], sg.foreground_split(maps), labels


def _counted(fn, calls, name):
    def run():
        calls[name] = calls.get(name, 0) + 1
        return fn()
    return run


def bench_one_version(batches, rounds, window, warmup, only):
    """--only: one version by itself (for a profiler), with the number of updates it made"""
    from transformer_explainability_amd import segmentation as sg
    res = {}
    for B in batches:
        _, heat, mask, (heat_c, mask_c), labels = inputs(B)
        ev, calls = sg.SegmentationEvaluator(None), {}
        fn = (lambda: ev.update_from_heat(heat, mask, labels)) if only == "new" else \
            (lambda: old_update_from_heat(ev, heat_c, mask_c, labels))
        t = alternate({only: _counted(fn, calls, only)}, rounds, window, warmup)
        res[f"update_from_heat.B{B}.224x224"] = {only: summary(t[only]), "calls": calls}
    return res


def bench_metrics(batches, rounds, window, warmup):
    from transformer_explainability_amd import ops, segmentation as sg
    res = {}
    for B in batches:
        _, heat, mask, (heat_c, mask_c), labels = inputs(B)
        ev_new, ev_old = sg.SegmentationEvaluator(None), sg.SegmentationEvaluator(None)
        got, ref = ev_new.update_from_heat(heat, mask, labels), old_update_from_heat(ev_old, heat_c, mask_c, labels)
        t = alternate({"new": lambda: ev_new.update_from_heat(heat, mask, labels),
                       "old": lambda: old_update_from_heat(ev_old, heat_c, mask_c, labels),
                       "kernel_only": lambda: ops.seg_metrics(heat, mask, labels)}, rounds, window, warmup)
        # what the kernel must move: the three inputs once, the sort elements written once and, per radix pass, read and
        # written once (8 B each, 2 H W per image), the run scan's two reads, the outputs
        P = 224 * 224
        nbytes = B * (P * (4 + 4 + 8) + 2 * P * 8 * (1 + 2 * 4 + 2) + (7 + 224) * 8)
        k = summary(t["kernel_only"])
        k.update(bytes_moved=nbytes, hbm_fraction_of_8TBps=round(nbytes / statistics.median(t["kernel_only"]) / HBM_BYTES_PER_S, 4))
        row = {"new": summary(t["new"]), "old": summary(t["old"]), "kernel_only": k, **_verdict(t),
               "integers_equal": bool(all(torch.equal(a, b) for a, b in zip(got[:4], ref[:4])) and torch.equal(got[5], ref[5])),
               "max_abs_ap_new_minus_old": float((got[4] - ref[4]).abs().max())}
        res[f"update_from_heat.B{B}.224x224"] = row
        ev_new.total_ap.clear(), ev_new.total_f1.clear(), ev_old.total_ap.clear(), ev_old.total_f1.clear()
    return res


def bench_evaluator(rounds, window, warmup, B=64):
    from transformer_explainability_amd import segmentation as sg
    from transformer_explainability_amd.generators import LRP
    from transformer_explainability_amd.sweep import normalize
    lrp = LRP(vit_b16())
    g = torch.Generator().manual_seed(B)
    x = normalize(torch.rand((B, 3, 224, 224), generator=g).to("cuda:0"))
    labels = (torch.rand((B, 224, 224), generator=g) > 0.7).long().to("cuda:0")
    explain = lambda im: lrp.generate_LRP(im, start_layer=1)      # noqa: E731
    ev_new, ev_old = sg.SegmentationEvaluator(explain), sg.SegmentationEvaluator(explain)
    t = alternate({"new": lambda: ev_new.update(x, labels), "old": lambda: old_update(ev_old, x, labels),
                   "explain_only": lambda: explain(x)}, rounds, window, warmup)
    lrp.check()
    row = {k: {"images_per_s": round(B / statistics.median(v), 1), **summary(v, 1e3, "ms")} for k, v in t.items()}
    row.update(_verdict(t))
    row["summary_new"], row["summary_old"] = ev_new.summary(), ev_old.summary()
    return {f"update.vit_base_patch16_224.batch{B}": row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=50.0, help="least duration of a timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--only", choices=["new", "old"], default=None, help="run one version of the metrics alone (profiling)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "seg_eval", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    batches = [int(b) for b in a.batches.split(",")]
    window = partial(wall_window, min_s=a.window_ms / 1e3)
    if a.only:
        res["metrics"] = bench_one_version(batches, a.rounds, window, a.warmup, a.only)
    else:
        res["metrics"] = bench_metrics(batches, a.rounds, window, a.warmup)
    if not a.skip_model and not a.only:
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
