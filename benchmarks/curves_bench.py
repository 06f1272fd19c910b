"""The deletion / insertion curve kernels (csrc/te_curves.hip) beside the torch restatement of the same definitions (curves.py),
in one process on the same device tensors.

    python benchmarks/curves_bench.py [--rounds 5] [--window-ms 200] [--warmup 2] [--skip-model] [--model-rounds 3] [--out F]

Configuration: ViT-B/16, batch 64, 224 x 224, 224 pixels per step (S = 224: 225 images per sample and curve), fp32 and bf16
images, chunks of 8 steps (max_forward_batch 512).  Prints one JSON line (and writes it to --out, default
profiles/curves_bench.json):
  * inputs: building every image of ONE insertion curve from the blurred image -- ``kernel`` is ops.pixel_ranks +
    ops.gaussian_blur + 29 ops.curve_inputs launches, ``torch`` is reference_ranks + reference_blur (RISE's fp32 conv2d) + 29
    reference_inputs calls on the same device tensors; every chunk is dropped as soon as it is built, as the evaluator does.
  * update: one CurveEvaluator.update (both curves, 2 x 225 x 64 forwards of the classifier) beside the restatement's loop with
    the same classifier: how much of the protocol the input building is.
  * compose: one ops.curve_inputs launch of 8 steps alone: its algorithmic bytes (the images written, image, substrate and
    ranks read once) over its time, as a share of the 8 TB/s of the data sheet; the measured copy rate of the part, 6.29 TB/s,
    is the practical ceiling.
The versions alternate, --rounds timed windows each (host clock between two device synchronisations) after a warm-up;
reported: median, min and max.  The yardstick of every time is the torch restatement on the device; no ratio is promised,
the result is written down whichever way it falls.
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
from benchmarks._timing import (HBM_BYTES_PER_S, MEASURED_COPY_BYTES_PER_S, alternate, summary,  # noqa: E402
                                wall_window)                                  # (the wall-window protocol)

B, C, H, W, STEP, CHUNK = 64, 3, 224, 224, 224, 8
MEAN = STD = (0.5, 0.5, 0.5)
BF = torch.bfloat16


def _pair(t, new="kernel", old="torch"):
    return {new: summary(t[new], 1e3, "ms", 3), old: summary(t[old], 1e3, "ms", 3),
            "torch_over_kernel_medians": round(statistics.median(t[old]) / statistics.median(t[new]), 2),
            "kernel_range_below_torch": bool(max(t[new]) < min(t[old]))}


def inputs():
    g = torch.Generator().manual_seed(0)
    data = torch.rand((B, C, H, W), generator=g).to("cuda:0")
    small = torch.rand((B, 1, 14, 14), generator=g)
    vis = torch.nn.functional.interpolate(small, size=(H, W), mode="bilinear", align_corners=False).to("cuda:0")
    target = (torch.arange(B) % 1000).to("cuda:0")
    return data, vis, target


def kernel_inputs(data, vis, dtype, consume=None):
    from transformer_explainability_amd import curves, ops
    S = curves.n_steps(H * W, STEP)
    ranks = ops.pixel_ranks(vis)
    blurred = ops.gaussian_blur(data, 11, 5.0, MEAN, STD)
    for s0 in range(0, S + 1, CHUNK):
        x = ops.curve_inputs(data, ranks, STEP, s0, min(CHUNK, S + 1 - s0), "insertion", substrate=blurred, mean=MEAN, std=STD,
                             out_dtype=dtype)
        if consume is not None:
            consume(x, s0)


def torch_inputs(data, vis, dtype, consume=None):
    from transformer_explainability_amd import curves
    S = curves.n_steps(H * W, STEP)
    ranks = curves.reference_ranks(vis)
    blurred = curves.reference_blur(data, 11, 5.0, MEAN, STD, dtype=torch.float32)
    for s0 in range(0, S + 1, CHUNK):
        x = curves.reference_inputs(data, ranks, STEP, s0, min(CHUNK, S + 1 - s0), "insertion", substrate=blurred, mean=MEAN,
                                    std=STD, out_dtype=dtype)
        if consume is not None:
            consume(x, s0)


def bench_inputs(rounds, window, warmup):
    from transformer_explainability_amd import curves, ops
    data, vis, _ = inputs()
    res = {}
    same_ranks = bool(torch.equal(ops.pixel_ranks(vis), curves.reference_ranks(vis)))
    for name, dtype in (("fp32", torch.float32), ("bf16", BF)):
        t = alternate({"kernel": lambda: kernel_inputs(data, vis, dtype), "torch": lambda: torch_inputs(data, vis, dtype)},
                      rounds, window, warmup)
        row = _pair(t)
        row["ranks_equal"] = same_ranks
        res[f"insertion.B{B}.{H}x{W}.step{STEP}.{name}"] = row
    return res


def bench_compose(rounds, window, warmup):
    from transformer_explainability_amd import ops
    data, vis, _ = inputs()
    ranks = ops.pixel_ranks(vis)
    blurred = ops.gaussian_blur(data, 11, 5.0, MEAN, STD)
    res = {}
    for name, dtype, size in (("fp32", torch.float32, 4), ("bf16", BF, 2)):
        fn = lambda: ops.curve_inputs(data, ranks, STEP, 100, CHUNK, "insertion", substrate=blurred, mean=MEAN, std=STD,  # noqa: E731
                                      out_dtype=dtype)
        t = alternate({"kernel": fn}, rounds, window, warmup)["kernel"]
        nbytes = CHUNK * B * C * H * W * size + 2 * B * C * H * W * 4 + B * H * W * 4
        med = statistics.median(t)
        row = summary(t, 1e6, "us", 3)
        row.update(algorithmic_bytes=nbytes, TB_per_s=round(nbytes / med / 1e12, 3),
                   share_of_8TBps=round(nbytes / med / HBM_BYTES_PER_S, 3),
                   share_of_measured_copy_rate_6_29TBps=round(nbytes / med / MEASURED_COPY_BYTES_PER_S, 3),
                   note="host clock over a window of back-to-back calls: launch and allocation of the output included")
        res[f"curve_inputs.B{B}.{H}x{W}.{CHUNK}steps.{name}"] = row
    return res


@torch.no_grad()
def restatement_update(model, data, vis, target, dtype):
    """CurveEvaluator.update spelled with the restatements, on device tensors: both curves"""
    from transformer_explainability_amd import curves
    S = curves.n_steps(H * W, STEP)
    ranks = curves.reference_ranks(vis)
    blurred = curves.reference_blur(data, 11, 5.0, MEAN, STD, dtype=torch.float32)
    out = {}
    for mode, sub in (("deletion", dict(fill=[0.0] * C)), ("insertion", dict(substrate=blurred))):
        prob = torch.empty((S + 1, B), dtype=torch.float64, device=data.device)
        for s0 in range(0, S + 1, CHUNK):
            n_s = min(CHUNK, S + 1 - s0)
            x = curves.reference_inputs(data, ranks, STEP, s0, n_s, mode, mean=MEAN, std=STD, out_dtype=dtype, **sub)
            prob[s0:s0 + n_s] = curves.reference_scores(model(x.reshape(n_s * B, C, H, W)), target)
        out[mode] = (prob, curves.reference_auc(prob))
    return out


def bench_update(rounds):
    from transformer_explainability_amd import curves
    data, vis, target = inputs()
    res = {}
    for name, dtype in (("bf16", BF), ("fp32", torch.float32)):
        model = vit_b16(dtype)

        def kernel():
            ev = curves.CurveEvaluator(model, step=STEP, mean=MEAN, std=STD, max_forward_batch=CHUNK * B)
            ev.update(data, vis, target)
            return ev
        t = alternate({"kernel": kernel, "torch": lambda: restatement_update(model, data, vis, target, dtype)}, rounds,
                      partial(wall_window, min_s=0.0), 1)
        row = {"kernel": summary(t["kernel"], 1.0, "s", 3), "torch": summary(t["torch"], 1.0, "s", 3),
               "torch_over_kernel_medians": round(statistics.median(t["torch"]) / statistics.median(t["kernel"]), 3),
               "kernel_range_below_torch": bool(max(t["kernel"]) < min(t["torch"])),
               "forwards_per_update": 2 * 225 * B}
        row["mean_auc"] = kernel().summary()
        res[f"update.vit_base_patch16_224.batch{B}.step{STEP}.{name}"] = row
        del model
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=200.0, help="least duration of a timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--model-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "curves_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "curves", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    window = partial(wall_window, min_s=a.window_ms / 1e3)
    res["inputs"] = bench_inputs(a.rounds, window, a.warmup)
    res["compose"] = bench_compose(a.rounds, window, a.warmup)
    if not a.skip_model:
        res["update"] = bench_update(a.model_rounds)
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
