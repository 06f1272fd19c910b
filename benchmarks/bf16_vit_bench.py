"""bf16 vs fp32 explanation step of ViT-B/16 (224 x 224, batch 64) in one process on the same images.

    python benchmarks/bf16_vit_bench.py [--batch 64] [--steps 10] [--warmup 3] [--rules]

Prints one JSON line: maps/s of LRP(model).generate_LRP(x) for the model in bf16 (the bf16 relprop kernels) and in fp32
(twice: the package defaults, and with the fused fp32 producers bench.py uses), and for the bf16 model with the fused bf16
producers (ops.USE_FUSED_PRODUCERS, csrc/te_attn_bf16.hip); device-event timing after warm-up.  --only bf16 / bf16_fused
runs that one line alone (a kernel trace of one mode).
--rules adds, for the bf16 step, every relprop C-ABI call bracketed by HIP events (ops.KERNEL_TIMER) with its ALGORITHMIC
flops and bytes: time, achieved GB/s and the HBM fraction (8 TB/s) per rule.  For a kernel table run the script under
``rocprofv3 --kernel-trace --stats -- python benchmarks/bf16_vit_bench.py --steps 2 --warmup 1``.
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def _model(dtype):
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import vit
    m = vit.vit_base_patch16_224().eval()
    synthetic_init(m, 0)
    return m.to("cuda:0").to(dtype)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / steps


class _RuleTimer:
    def __init__(self):
        self.rows = collections.defaultdict(lambda: [0, 0.0, 0.0, 0.0])      # calls, seconds, flops, bytes
        self.pending = []

    @contextlib.contextmanager
    def __call__(self, name, flops, nbytes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.pending.append((name, flops, nbytes, a, b))

    def flush(self):
        torch.cuda.synchronize()
        for name, flops, nbytes, a, b in self.pending:
            r = self.rows[name]
            r[0] += 1
            r[1] += a.elapsed_time(b) / 1e3
            r[2] += flops
            r[3] += nbytes
        self.pending.clear()

    def table(self):
        out = {}
        for name, (n, s, f, nb) in sorted(self.rows.items(), key=lambda kv: -kv[1][1]):
            out[name] = {"calls": n, "ms": round(s * 1e3, 3), "algorithmic_bytes": nb,
                         "GB_per_s": round(nb / s / 1e9, 1) if s > 0 else None,
                         "hbm_fraction": round(nb / s / HBM_BYTES_PER_S, 3) if s > 0 else None,
                         "TFLOP_per_s": round(f / s / 1e12, 1) if s > 0 else None}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rules", action="store_true")
    ap.add_argument("--only", choices=["all", "bf16", "bf16_fused"], default="all")
    a = ap.parse_args()

    import transformer_explainability_amd as te
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    te._lib.require_device()
    x32 = seeded_randn((a.batch, 3, 224, 224), 1).to("cuda:0")
    res = {"config": "vit_b16_224", "batch": a.batch, "steps": a.steps, "warmup": a.warmup}

    m16 = _model(torch.bfloat16)
    x16 = x32.to(torch.bfloat16)
    lrp16 = LRP(m16)
    t16 = None
    if a.only in ("all", "bf16"):
        t16 = _time(lambda: lrp16.generate_LRP(x16, start_layer=1), a.steps, a.warmup)
        res["bf16_maps_per_s"] = round(a.batch / t16, 1)
        res["bf16_step_ms"] = round(t16 * 1e3, 2)
    if a.only in ("all", "bf16_fused"):
        was = ops.USE_FUSED_PRODUCERS
        ops.USE_FUSED_PRODUCERS = True
        try:
            t16f = _time(lambda: lrp16.generate_LRP(x16, start_layer=1), a.steps, a.warmup)
            assert all(b.attn._fused_anchor is not None for b in m16.blocks), "the bf16 blocks did not take the fused route"
        finally:
            ops.USE_FUSED_PRODUCERS = was
        res["bf16_fused_producers_maps_per_s"] = round(a.batch / t16f, 1)
        res["bf16_fused_producers_step_ms"] = round(t16f * 1e3, 2)
    if a.only != "all":
        res["build_id"] = te._lib.build_id()
        print(json.dumps(res), flush=True)
        return
    t16 = min(t16, t16f)
    if a.rules:
        timer = _RuleTimer()
        ops.KERNEL_TIMER = timer
        try:
            lrp16.generate_LRP(x16, start_layer=1)
            timer.flush()
        finally:
            ops.KERNEL_TIMER = None
        res["bf16_rules"] = timer.table()
    del m16, lrp16
    torch.cuda.empty_cache()

    m32 = _model(torch.float32)
    lrp32 = LRP(m32)
    t32 = _time(lambda: lrp32.generate_LRP(x32, start_layer=1), a.steps, a.warmup)
    res["fp32_maps_per_s"] = round(a.batch / t32, 1)
    res["fp32_step_ms"] = round(t32 * 1e3, 2)
    was = ops.USE_FUSED_PRODUCERS
    ops.USE_FUSED_PRODUCERS = True
    try:
        t32f = _time(lambda: lrp32.generate_LRP(x32, start_layer=1), a.steps, a.warmup)
    finally:
        ops.USE_FUSED_PRODUCERS = was
    lrp32.check()
    res["fp32_fused_producers_maps_per_s"] = round(a.batch / t32f, 1)
    res["fp32_fused_producers_step_ms"] = round(t32f * 1e3, 2)
    res["bf16_speedup_vs_fp32_best"] = round(min(t32, t32f) / t16, 3)
    res["build_id"] = te._lib.build_id()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
