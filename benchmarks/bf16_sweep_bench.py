"""The evaluation pipeline on a bf16 ViT-B/16 beside the fp32 model, in one process on the same images.

    python benchmarks/bf16_sweep_bench.py [--batches 64,32] [--steps 5] [--warmup 2] [--rounds 9] [--window-ms 50] [--skip-models] [--out F]

Prints one JSON line (and writes it to --out):
  * kernels: te_perturb_bf16 at B = 64, 3 x 224 x 224, S = 10 against the path a tree without it offers for the same
    tensor (te_perturb_f32 followed by .to(bfloat16)), and te_attn_headmean_bf16 at (64, 12, 197) and (32, 12, 512)
    against the torch expression it replaces (attn.mean(dim=1).float()).  The two versions alternate, --rounds timed
    windows each (device events around about --window-ms of calls, after warm-up); reported: the median, min and max per-call time of
    each version, and for the new kernels the bytes they must move over the median time as a fraction of the 8 TB/s HBM
    peak.  ``faster_beyond_spread`` is true when the slowest window of the new path is faster than the fastest window of
    the old one.
  * sweep: maps/s of SaliencySweep("transformer_attribution").explain on fp32 images for the bf16 and the fp32 model at the
    sweep's batch shapes, the models alternating.
  * perturbation: seconds per PerturbationEvaluator.update at batch 64 (10 x 64 forwards) for both models.
For a kernel table run the script under ``rocprofv3 --kernel-trace --stats -- python benchmarks/bf16_sweep_bench.py
--steps 1 --warmup 1 --rounds 2``.
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
from benchmarks._timing import HBM_BYTES_PER_S, alternate, event_window, summary  # noqa: E402  (the event-window protocol)

BF = torch.bfloat16


def _summary(ts, nbytes=None):
    med = statistics.median(ts)
    out = summary(ts)
    if nbytes is not None:
        out["bytes_that_must_move"] = int(nbytes)
        out["GB_per_s"] = round(nbytes / med / 1e9, 1)
        out["hbm_fraction_of_8TBps"] = round(nbytes / med / HBM_BYTES_PER_S, 3)
    return out


def _ab(new, old, nbytes, rounds, window_s, warmup):
    for fn in (new, old):
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    inner = max(20, int(window_s / max(event_window(old, 20), 1e-6)))      # calls per window: about window_s of device time
    t = alternate({"new": new, "old": old}, rounds, partial(event_window, n=inner), 0)
    return {"new": _summary(t["new"], nbytes), "old": _summary(t["old"]), "calls_per_window": inner,
            "speedup_of_medians": round(statistics.median(t["old"]) / statistics.median(t["new"]), 3),
            "faster_beyond_spread": bool(max(t["new"]) < min(t["old"]))}


def bench_kernels(rounds, window_s, warmup):
    from transformer_explainability_amd import ops
    d = "cuda:0"
    g = torch.Generator().manual_seed(0)
    res = {}
    B, C, HW, S = 64, 3, 224 * 224, 10
    data = torch.rand((B, C, 224, 224), generator=g).to(d)
    vis = torch.rand((B, HW), generator=g).to(d)
    ks = [0] + [int(HW * f) for f in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)]
    mean = std = (0.5, 0.5, 0.5)
    same = bool(torch.equal(ops.perturb(vis, data, ks, mean, std, out_dtype=BF), ops.perturb(vis, data, ks, mean, std).to(BF)))
    # bf16 form: every step inside the thread, so the image and the relevance row are read once
    nbytes = S * B * C * HW * 2 + B * C * HW * 4 + B * HW * 4
    r = _ab(lambda: ops.perturb(vis, data, ks, mean, std, out_dtype=BF),
            lambda: ops.perturb(vis, data, ks, mean, std).to(BF), nbytes, rounds, window_s, warmup)
    r["outputs_equal"] = same
    r["note"] = "times include the selection kernel (shared by both paths); old = te_perturb_f32 + .to(bfloat16)"
    res["perturb_bf16.B64.3x224x224.S10"] = r
    del data, vis
    for (B, H, N) in ((64, 12, 197), (32, 12, 512)):
        attn = torch.softmax(torch.randn((B, H, N, N), generator=g).to(d), -1).to(BF)
        out = torch.empty((B, N, N), dtype=torch.float32, device=d)
        diff = float((ops.attn_headmean(attn) - attn.mean(dim=1).float()).abs().max())
        nbytes = B * H * N * N * 2 + B * N * N * 4
        r = _ab(lambda: ops.attn_headmean(attn, out=out), lambda: attn.mean(dim=1).float(), nbytes, rounds, window_s, warmup)
        r["max_abs_new_minus_old"] = diff        # (the old path rounds the mean to bf16)
        r["note"] = "old = attn.mean(dim=1).float()"
        res[f"attn_headmean_bf16.B{B}.H{H}.N{N}"] = r
        del attn, out
    torch.cuda.empty_cache()
    return res


def bench_models(batches, steps, warmup, rounds):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd.generators import LRP
    from transformer_explainability_amd.perturbation import PerturbationEvaluator
    from transformer_explainability_amd.sweep import SaliencySweep, normalize
    models = {"bf16": vit_b16(BF), "fp32": vit_b16(torch.float32)}
    sweeps = {k: SaliencySweep("transformer_attribution", lrp=LRP(m)) for k, m in models.items()}
    res = {"sweep": {}, "perturbation": {}}
    for B in batches:
        x = normalize(torch.rand((B, 3, 224, 224), generator=torch.Generator().manual_seed(B)).to("cuda:0"))
        t = alternate({k: (lambda s=s: s.explain(x)) for k, s in sweeps.items()}, rounds, partial(event_window, n=steps), warmup)
        row = {k: {"maps_per_s": round(B / statistics.median(v), 1), "step_ms_median": round(statistics.median(v) * 1e3, 2),
                   "step_ms_min": round(min(v) * 1e3, 2), "step_ms_max": round(max(v) * 1e3, 2)} for k, v in t.items()}
        row["bf16_over_fp32"] = round(statistics.median(t["fp32"]) / statistics.median(t["bf16"]), 3)
        res["sweep"][f"transformer_attribution.batch{B}"] = row
    for s in sweeps.values():
        s.lrp.check()
    B = 64
    data = torch.rand((B, 3, 224, 224), generator=torch.Generator().manual_seed(1)).to("cuda:0")
    vis = seeded_randn((B, 1, 224, 224), 2).to("cuda:0")
    target = torch.arange(B, device="cuda:0") % 1000
    evs = {k: PerturbationEvaluator(m, num_samples=B * (warmup + rounds * steps)) for k, m in models.items()}
    t = alternate({k: (lambda e=e: e.update(data, vis, target)) for k, e in evs.items()}, rounds, partial(event_window, n=steps),
                  warmup)
    row = {k: {"seconds_per_update_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
           for k, v in t.items()}
    row["bf16_over_fp32"] = round(statistics.median(t["fp32"]) / statistics.median(t["bf16"]), 3)
    res["perturbation"]["update.batch64"] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,32")
    ap.add_argument("--steps", type=int, default=5, help="calls per timed window of the model-level measurements")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=50.0, help="device time per timed window of the kernel measurements")
    ap.add_argument("--skip-models", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "bf16_sweep", "rounds": a.rounds, "kernel_window_ms": a.window_ms, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    res["kernels"] = bench_kernels(a.rounds, a.window_ms / 1e3, max(a.warmup, 3))
    if not a.skip_models:
        res.update(bench_models([int(b) for b in a.batches.split(",")], a.steps, a.warmup, a.rounds))
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
