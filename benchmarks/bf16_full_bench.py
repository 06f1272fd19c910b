"""method="full" on a bf16 ViT-B/16: the z^B rule of the patch embedding on bf16 operands against the fp32 kernel.

    python benchmarks/bf16_full_bench.py [--part rule|call|all] [--batch 64] [--rounds 5] [--steps 10] [--warmup 3]

Prints one JSON line.  The new and the old path ALTERNATE in one process (round r times the new path, then the old one, on
the same tensors); the figures are the medians over the rounds, device-event timing after warm-up.
  rule  the rule alone at ViT-B/16 shape (T = batch * 196, K = E = 768): ops.conv2d_zb_relprop on the bf16 X / W
        (te_conv2d_zb_relprop_bf16, weight planes cached) against te_conv2d_zb_relprop_f32 on fp32 copies of the same
        operands with Y = their fp32 convolution, both made once outside the timed region; `fp32_upcast_route_ms` is what a
        bf16 model would pay on that route per call (the two copies, the convolution and the kernel).
  call  LRP(model).generate_LRP(x, method="full") of the bf16 model against the fp32 model.
For a kernel table run the script under ``rocprofv3 --kernel-trace --stats -- python benchmarks/bf16_full_bench.py --part rule
--rounds 1 --steps 2 --warmup 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks._models import vit_b16  # noqa: E402
from benchmarks._timing import event_window  # noqa: E402  (event windows, but warmed anew before every window: not `alternate`)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return event_window(fn, steps) * 1e3


def _rewarmed_rounds(fns, rounds, steps, warmup):
    """{name: median ms over the rounds}, the paths taking turns inside every round, each warmed again before its window"""
    ms = {name: [] for name in fns}
    for r in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, steps, warmup if r == 0 else 1))
    return {name: round(statistics.median(v), 4) for name, v in ms.items()}, {name: [round(x, 4) for x in v] for name, v in ms.items()}


def bench_rule(a, res):
    import torch.nn.functional as F
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import ops
    B, p, E = a.batch, 16, 768
    X = seeded_randn((B, 3, 224, 224), 1).to("cuda:0").to(torch.bfloat16)
    g = torch.Generator().manual_seed(2)
    W = (torch.randn(E, 3, p, p, generator=g) * 0.02).to("cuda:0").to(torch.bfloat16)
    cam = torch.randn(B, 197, E, generator=g).to("cuda:0")
    R = cam[:, 1:].unflatten(1, (14, 14)).permute(0, 3, 1, 2)          # the view PatchEmbed.relprop hands over
    Xf, Wf = X.float(), W.float()
    Yf = F.conv2d(Xf, Wf, stride=p)
    cache = {}
    fns = {"bf16_rule_ms": lambda: ops.conv2d_zb_relprop(R, X, W, None, cache=cache),
           "fp32_kernel_on_upcast_operands_ms": lambda: ops.conv2d_zb_relprop(R, Xf, Wf, Yf),
           "fp32_upcast_route_ms": lambda: ops.conv2d_zb_relprop(R, X.float(), W.float(),
                                                                 F.conv2d(X.float(), W.float(), stride=p))}
    med, runs = _rewarmed_rounds(fns, a.rounds, a.steps, a.warmup)
    T, K = B * 196, 3 * p * p
    res["rule"] = {"shape": {"T": T, "K": K, "E": E}, **med, "rounds_ms": runs,
                   "bf16_vs_fp32_kernel": round(med["fp32_kernel_on_upcast_operands_ms"] / med["bf16_rule_ms"], 3),
                   "bf16_mfma_TFLOP_per_s": round(14.0 * T * K * E / (med["bf16_rule_ms"] * 1e-3) / 1e12, 1)}


def bench_call(a, res):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd.generators import LRP
    x32 = seeded_randn((a.batch, 3, 224, 224), 1).to("cuda:0")
    x16 = x32.to(torch.bfloat16)
    l16, l32 = LRP(vit_b16(torch.bfloat16)), LRP(vit_b16(torch.float32))
    fns = {"bf16_model_ms": lambda: l16.generate_LRP(x16, method="full"),
           "fp32_model_ms": lambda: l32.generate_LRP(x32, method="full")}
    med, runs = _rewarmed_rounds(fns, a.rounds, a.steps, a.warmup)
    res["call"] = {**med, "rounds_ms": runs, "bf16_maps_per_s": round(a.batch / med["bf16_model_ms"] * 1e3, 1),
                   "fp32_maps_per_s": round(a.batch / med["fp32_model_ms"] * 1e3, 1),
                   "bf16_speedup_vs_fp32": round(med["fp32_model_ms"] / med["bf16_model_ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["rule", "call", "all"], default="all")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"config": "vit_b16_224", "method": "full", "batch": a.batch, "rounds": a.rounds, "steps": a.steps,
           "warmup": a.warmup}
    if a.part in ("rule", "all"):
        bench_rule(a, res)
    if a.part in ("call", "all"):
        bench_call(a, res)
    res["build_id"] = te._lib.build_id()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
