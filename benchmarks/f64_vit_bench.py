"""fp64 vs fp32 explanation step of ViT-B/16 (224 x 224, batch 8) in one process on the same images, modes alternating.

    python benchmarks/f64_vit_bench.py [--batch 8] [--rounds 5] [--warmup 2] [--rules] [--cpu-oracle on|off] [--only f64]

Prints one JSON line:
  * ms per step of LRP(model.double()).generate_LRP(x.double()) and of LRP(model).generate_LRP(x) (package defaults), measured
    A B A B ... with HIP events around every single step after a joint warm-up; median, min and max over the rounds;
  * --rules: every relprop C-ABI call of ONE fp64 step bracketed by HIP events (ops.KERNEL_TIMER) with its algorithmic
    flops and bytes -- for "linear_f64" flops = the fp64 MFMA work executed (the Z-pass issues the + and the - product,
    the C-pass the two weight signs: 4 x 2 T in out per rule);
  * --cpu-oracle on: wall time of the CPU oracle in double (oracle.relprop_oracle.vit_relprop, 16 threads) for ONE sample
    of the same batch on the fp64 model's own cache -- the comparator this path replaces -- and the normalised error of
    the device map against it.
For the per-kernel table run one mode alone under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats -- python benchmarks/f64_vit_bench.py --only f64 --rounds 2 --warmup 1 --cpu-oracle off
The two Linear passes are the instantiations 1 (Z-pass) and 2 (C-pass) of gemm64_kernel; instantiation 0 is the attention
rules' product.  Their fp64 MFMA work per ViT-B/16 step is printed as "linear_pass_flops" so that achieved TF/s follows from
the trace's total time per kernel.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

import torch  # noqa: E402


def _model(dtype):
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import vit
    m = vit.vit_base_patch16_224().eval()
    synthetic_init(m, 0)
    return m.to("cuda:0").to(dtype)


def _one(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "rounds": len(ms)}


def _linear_pass_flops(batch):
    """fp64 MFMA flops executed per pass of the Linear rules of one ViT-B/16 step (last block on the class-token rows)."""
    n, c = 197, 768
    layers = [(c, 3 * c), (c, c), (c, 4 * c), (4 * c, c)]                     # (in, out): qkv, proj, fc1, fc2
    dense = sum(2.0 * batch * n * i * o for i, o in layers) * 11
    last = 2.0 * batch * n * c * 3 * c + sum(2.0 * batch * i * o for i, o in layers[1:]) + 2.0 * batch * c * 1000
    return 2.0 * (dense + last)                                                # two products per pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rules", action="store_true")
    ap.add_argument("--cpu-oracle", choices=["on", "off"], default="on")
    ap.add_argument("--only", choices=["both", "f64"], default="both")
    a = ap.parse_args()

    import transformer_explainability_amd as te
    from bf16_vit_bench import _RuleTimer
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    te._lib.require_device()
    x32 = seeded_randn((a.batch, 3, 224, 224), 1).to("cuda:0")
    x64 = x32.double()
    res = {"config": "vit_b16_224", "batch": a.batch, "warmup": a.warmup, "start_layer": 1,
           "linear_pass_flops": _linear_pass_flops(a.batch)}

    m64 = _model(torch.float64)
    lrp64 = LRP(m64)
    f64 = lambda: lrp64.generate_LRP(x64, start_layer=1)      # noqa: E731
    modes = [("f64", f64)]
    if a.only == "both":
        m32 = _model(torch.float32)
        lrp32 = LRP(m32)
        modes.append(("fp32", lambda: lrp32.generate_LRP(x32, start_layer=1)))
    for _ in range(a.warmup):
        for _, fn in modes:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in modes}
    for _ in range(a.rounds):
        for name, fn in modes:
            ms[name].append(_one(fn))
    for name in ms:
        res[name + "_step"] = _summary(ms[name])
    if a.only == "both":
        lrp32.check()
        res["f64_over_fp32"] = round(res["f64_step"]["median_ms"] / res["fp32_step"]["median_ms"], 2)
    if a.rules:
        timer = _RuleTimer()
        ops.KERNEL_TIMER = timer
        try:
            f64()
            timer.flush()
        finally:
            ops.KERNEL_TIMER = None
        res["f64_rules"] = timer.table()
    if a.cpu_oracle == "on":
        from oracle import model_cache
        from oracle import relprop_oracle as O
        from unittest import mock
        torch.set_num_threads(16)
        out = f64().detach().double().cpu()
        index = m64.head.Y.detach().argmax(-1).cpu()
        with model_cache.sliced_relprop_state(m64, 0, a.batch), \
                mock.patch.object(model_cache, "_cpu", lambda t: None if t is None else t.detach().double().cpu()):
            cache = model_cache.vit_cache_from_model(m64)
        oh = torch.zeros((1, m64.head.Y.shape[1]), dtype=torch.float64)
        oh[0, index[0]] = 1.0
        t0 = time.perf_counter()
        ref = O.vit_relprop(oh, cache, num_heads=12, start_layer=1)["map"]
        res["cpu_oracle_fp64_one_sample_s"] = round(time.perf_counter() - t0, 3)
        res["cpu_oracle_threads"] = torch.get_num_threads()
        got = out[:1]
        norm = lambda m: (m - m.min()) / (m.max() - m.min())      # noqa: E731
        res["normalised_max_abs_vs_oracle"] = float((norm(got) - norm(ref)).abs().max())
    res["build_id"] = te._lib.build_id()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
