"""generate_attnlrp on a bf16 model beside the same call on the fp32 model and beside generate_LRP on the bf16 model: one
process, the same weights and inputs, windows alternating.

    python benchmarks/attnlrp_bf16_bench.py [--configs vit_b16 bert_base] [--steps 5] [--rounds 5] [--warmup 2]
                                            [--producers fused|stock] [--out profiles/attnlrp_bf16_bench.json]

Two configurations: ViT-B/16 (224 x 224) at batch 64 and BERT-base at 512 tokens x 32.  Per configuration the three calls are
warmed up together, then timed A B C A B C ...: one window = ``--steps`` calls between two HIP events, ended by a synchronise;
reported are the median, minimum and maximum ms per call over the ``--rounds`` windows of each call and the ratios of the
medians.  Then one bf16 generate_attnlrp call runs with every rule call of the chain bracketed by HIP events
(ops.KERNEL_TIMER): the per-kernel table, with the ALGORITHMIC flops and bytes of each binding.  No speed is claimed anywhere:
the file holds what was measured.  The result is printed as one JSON line and written to ``--out``.
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import json
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks._models import bert_base, vit_b16  # noqa: E402
from benchmarks._timing import alternate, event_window, summary  # noqa: E402  (the event-window protocol)

BF16 = torch.bfloat16


def _vit_b16(batch):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd.generators import LRP
    x32 = seeded_randn((batch, 3, 224, 224), 1).to("cuda:0")
    x16 = x32.to(BF16)
    g32, g16 = LRP(vit_b16()), LRP(vit_b16(BF16))
    return (g32, g16), {"attnlrp_bf16": lambda: g16.generate_attnlrp(x16), "attnlrp_fp32": lambda: g32.generate_attnlrp(x32),
                        "LRP_bf16": lambda: g16.generate_LRP(x16, start_layer=0)}


def _bert_base(batch, tokens=512):
    from transformer_explainability_amd.generators import Generator
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30000, (batch, tokens), generator=g).to("cuda:0")
    mask = torch.ones(batch, tokens)
    mask[::2, tokens - tokens // 8:] = 0.0                     # every other sample padded
    mask = mask.to("cuda:0")
    g32, g16 = Generator(bert_base()), Generator(bert_base(BF16))
    return (g32, g16), {"attnlrp_bf16": lambda: g16.generate_attnlrp(ids, mask), "attnlrp_fp32": lambda: g32.generate_attnlrp(ids, mask),
                        "LRP_bf16": lambda: g16.generate_LRP(ids, mask, start_layer=0)}


CONFIGS = {"vit_b16": (_vit_b16, 64), "bert_base": (_bert_base, 32)}


class _RuleTimer:
    """ops.KERNEL_TIMER: HIP events around every rule call; rows by binding, slowest first"""

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

    def table(self):
        torch.cuda.synchronize()
        for name, flops, nbytes, a, b in self.pending:
            r = self.rows[name]
            r[0], r[1], r[2], r[3] = r[0] + 1, r[1] + a.elapsed_time(b) / 1e3, r[2] + flops, r[3] + nbytes
        self.pending.clear()
        return {name: {"calls": n, "ms": round(s * 1e3, 3), "GB_per_s": round(nb / s / 1e9, 1) if s > 0 else None,
                       "TFLOP_per_s": round(f / s / 1e12, 1) if s > 0 else None}
                for name, (n, s, f, nb) in sorted(self.rows.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=sorted(CONFIGS), default=["vit_b16", "bert_base"])
    ap.add_argument("--steps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per call")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="0: the configuration's own (64 / 32)")
    ap.add_argument("--producers", choices=["stock", "fused"], default="fused")
    ap.add_argument("--tuned-gemms", choices=["on", "off"], default="on")
    ap.add_argument("--weight-side", choices=["transposed", "inplace"], default="transposed",
                    help="te_attnlrp_linear_bf16's weight operand: the cached W^T (ops.ALRP_WEIGHT_T) or W read in place")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attnlrp_bf16_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    from transformer_explainability_amd import ops
    te._lib.require_device()
    ops.USE_FUSED_PRODUCERS = a.producers == "fused"
    ops.ALRP_WEIGHT_T = a.weight_side == "transposed"
    tuned = te.enable_tuned_gemms() if a.tuned_gemms == "on" else False
    res = {"producers": a.producers, "weight_side": a.weight_side, "tuned_gemms": bool(tuned), "steps_per_window": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.configs:
        make, batch = CONFIGS[name]
        batch = a.batch or batch
        gens, modes = make(batch)
        for _ in range(a.warmup):
            for fn in modes.values():
                fn()
        ts = alternate(modes, a.rounds, partial(event_window, n=a.steps), 0)      # (warmed above, the three calls in turn)
        for gen in gens:
            gen.check()                                        # no x6 hand-over was lost in any timed call
        finite = {m: bool(torch.isfinite(fn()).all()) for m, fn in modes.items()}
        entry = {"batch": batch, "finite": finite, **{m: summary(v, 1e3, "ms", 3) for m, v in ts.items()}}
        med = lambda m: entry[m]["median_ms"]      # noqa: E731
        entry["attnlrp_bf16_over_attnlrp_fp32"] = round(med("attnlrp_bf16") / med("attnlrp_fp32"), 3)
        entry["attnlrp_bf16_over_LRP_bf16"] = round(med("attnlrp_bf16") / med("LRP_bf16"), 3)
        timer = _RuleTimer()
        ops.KERNEL_TIMER = timer
        try:
            modes["attnlrp_bf16"]()
            entry["attnlrp_bf16_rule_calls"] = timer.table()
        finally:
            ops.KERNEL_TIMER = None
        res["configs"][name] = entry
        del gens, modes
        torch.cuda.empty_cache()
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
