"""bf16 vs fp32 explanation step of BERT-base (512 tokens, batch 32, every other sample padded in its last 64 tokens: the
inputs of test_config3_bert_base_512_batch32) in one process on the same inputs.

    python benchmarks/bf16_bert_bench.py [--batch 32] [--steps 10] [--warmup 3] [--rules]

Prints one JSON line: sequences/s of Generator(model).generate_LRP(ids, mask, start_layer=0) for the model in bf16 (the bf16
relprop kernels; forward and backward on stock PyTorch, and again with the fused bf16 producers of csrc/te_attn_bf16.hip,
ops.USE_FUSED_PRODUCERS), eager and replayed as a GraphedCall, and in fp32 with the package
defaults (eager) and with the fused fp32 producers bench.py --config bert_base_512 uses (eager and GraphedCall); device-event
timing after warm-up.  --rules adds, for the bf16 step, every relprop C-ABI call bracketed by HIP events
(ops.KERNEL_TIMER) with its ALGORITHMIC flops and bytes.  For a kernel table run the script under
``rocprofv3 --kernel-trace --stats -- python benchmarks/bf16_bert_bench.py --steps 2 --warmup 1``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

import torch  # noqa: E402

from bf16_vit_bench import _RuleTimer, _time  # noqa: E402


def _model(dtype):
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import bert
    m = bert.BertForSequenceClassification(bert.BertConfigLite(num_labels=2)).eval()
    synthetic_init(m, 0)
    return m.to("cuda:0").to(dtype)


def _inputs(B, N=512):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 20000, (B, N), generator=g)
    mask = torch.ones(B, N)
    mask[::2, N - 64:] = 0
    return ids.to("cuda:0"), mask.to("cuda:0")


def _eager_and_graphed(gen, ids, mask, a, res, key):
    from transformer_explainability_amd.generators import GraphedCall
    B = ids.shape[0]
    step = lambda i, m: gen.generate_LRP(i, m, start_layer=0)      # noqa: E731
    t = _time(lambda: step(ids, mask), a.steps, a.warmup)
    res[f"{key}_seq_per_s"] = round(B / t, 1)
    res[f"{key}_step_ms"] = round(t * 1e3, 2)
    g = GraphedCall(step, (ids, mask))
    tg = _time(lambda: g(ids, mask), a.steps, a.warmup)
    res[f"{key}_graphed_seq_per_s"] = round(B / tg, 1)
    res[f"{key}_graphed_step_ms"] = round(tg * 1e3, 2)
    del g
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return min(t, tg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rules", action="store_true")
    ap.add_argument("--only", choices=["all", "bf16", "bf16_fused"], default="all")      # one line alone: a kernel trace of one mode
    a = ap.parse_args()

    import transformer_explainability_amd as te
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import Generator
    te._lib.require_device()
    ids, mask = _inputs(a.batch)
    res = {"config": "bert_base_512", "batch": a.batch, "padded": "every other sample, last 64 tokens",
           "steps": a.steps, "warmup": a.warmup}

    m16 = _model(torch.bfloat16)
    gen16 = Generator(m16)
    t16 = float("inf")
    if a.only in ("all", "bf16"):
        t16 = _eager_and_graphed(gen16, ids, mask, a, res, "bf16")
    if a.only in ("all", "bf16_fused"):
        was = ops.USE_FUSED_PRODUCERS
        ops.USE_FUSED_PRODUCERS = True
        try:
            t16 = min(t16, _eager_and_graphed(gen16, ids, mask, a, res, "bf16_fused_producers"))
            assert all(l.attention.self._fused_anchor is not None for l in m16.bert.encoder.layer), \
                "the bf16 layers did not take the fused route"
        finally:
            ops.USE_FUSED_PRODUCERS = was
    if a.only != "all":
        res["build_id"] = te._lib.build_id()
        print(json.dumps(res), flush=True)
        return
    if a.rules:
        timer = _RuleTimer()
        ops.KERNEL_TIMER = timer
        try:
            gen16.generate_LRP(ids, mask, start_layer=0)
            timer.flush()
        finally:
            ops.KERNEL_TIMER = None
        res["bf16_rules"] = timer.table()
    gen16.check()
    del m16, gen16
    torch.cuda.empty_cache()

    m32 = _model(torch.float32)
    gen32 = Generator(m32)
    t32 = _time(lambda: gen32.generate_LRP(ids, mask, start_layer=0), a.steps, a.warmup)
    res["fp32_seq_per_s"] = round(a.batch / t32, 1)
    res["fp32_step_ms"] = round(t32 * 1e3, 2)
    was = ops.USE_FUSED_PRODUCERS
    ops.USE_FUSED_PRODUCERS = True
    try:
        t32f = _eager_and_graphed(gen32, ids, mask, a, res, "fp32_fused_producers")
    finally:
        ops.USE_FUSED_PRODUCERS = was
    gen32.check()
    res["bf16_speedup_vs_fp32_best"] = round(min(t32, t32f) / t16, 3)
    res["build_id"] = te._lib.build_id()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
