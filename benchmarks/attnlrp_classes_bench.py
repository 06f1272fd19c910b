"""AttnLRP for several classes of the same batch: K single calls against ONE generate_attnlrp_classes call, and the class
entries of csrc/te_attnlrp.hip against K launches of their parents, in one process.

    python benchmarks/attnlrp_classes_bench.py [--configs vit_b16.fp32 vit_b16.bf16 bert_base.fp32] [--ks 2,5] [--steps 2]
                                               [--rounds 5] [--warmup 1] [--skip-kernels] [--out F]
    python benchmarks/attnlrp_classes_bench.py --profile-call vit_b16.fp32 --ks 5      (the one call alone, for a profiler)

ViT-B/16 224 x 224 at batch 64 (fp32, bf16) and BERT-base 512 tokens x 32 (fp32; max(K) labels); the K largest logits of every
sample in a device tensor.  Per configuration and K the versions take turns (benchmarks/_timing.py: --rounds windows of
--steps calls between HIP events, after --warmup untimed calls of every version), medians reported with the min / max window:

  (a) k_single_calls   K generate_attnlrp calls, one per class column
  (b) chunk1           generate_attnlrp_classes(chunk=1): one forward pass, K chains on the kernels of (a)
  (c) one_call         generate_attnlrp_classes: one forward pass, one chain with a class axis
  forward              the forward pass alone (no_grad)
  peak allocated bytes of one single call and of (c)

The yardstick of (c) is (a) - (K - 1) x forward: the K single calls less the forward passes the one call does not run; the row
says "met" or "missed by x %".  (c) against (b) is what the class axis itself buys; the row gives the ratio, both spreads
and whether the difference of the medians lies inside them.  No ratio is promised.  The script FAILS (exit status 1, after
writing the result) only if a map of the one call differs from the single call's.

Kernel level: te_alrpk_damp / _act (GELU) / _layernorm at [K, 64 x 197, 768] and [K, 64 x 197, 3072] and te_alrpk_token_relevance
at [K, 64, 197, 768], each against K launches of its parent on the slices, with the achieved bytes/s on the algorithmic bytes
(damp / act: (2K + 1) 4 n against 3K 4 n; layernorm: 2K 4 n either way; token sums: (K + 1) 4 n against 2K 4 n) beside the
copy rate measured on the part.  One JSON line is printed and written to --out (default profiles/attnlrp_classes_bench.json)."""
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
from benchmarks._timing import MEASURED_COPY_BYTES_PER_S, alternate, event_window, summary  # noqa: E402
from benchmarks.classes_bench import _peak_bytes  # noqa: E402
from benchmarks.sweep_all_bench import _same  # noqa: E402

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _vit(dtype, Ks):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd.generators import LRP
    x = seeded_randn((64, 3, 224, 224), 1).to("cuda:0").to(dtype)
    gen = LRP(vit_b16(dtype))
    return (gen, lambda: gen.model(x), lambda idx: gen.generate_attnlrp(x, index=idx),
            lambda c, **kw: gen.generate_attnlrp_classes(x, classes=c, **kw))


def _bert(dtype, Ks, B=32, N=512):
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import bert
    from transformer_explainability_amd.generators import Generator
    model = bert.BertForSequenceClassification(bert.BertConfigLite(num_labels=max(Ks))).eval()
    synthetic_init(model, 0)
    model.to("cuda:0").to(dtype)
    ids = torch.randint(1000, 30000, (B, N), generator=torch.Generator().manual_seed(N)).to("cuda:0")
    mask = torch.ones((B, N), device="cuda:0")
    mask[B // 2:, N - N // 4:] = 0                   # half of the batch padded
    gen = Generator(model)
    return (gen, lambda: model(input_ids=ids, attention_mask=mask)[0], lambda idx: gen.generate_attnlrp(ids, mask, index=idx),
            lambda c, **kw: gen.generate_attnlrp_classes(ids, mask, classes=c, **kw))


CONFIGS = {"vit_b16.fp32": (_vit, torch.float32), "vit_b16.bf16": (_vit, torch.bfloat16), "bert_base.fp32": (_bert, torch.float32)}


def _spread(ts):
    return min(ts), max(ts)


def _row(K, times, single, one_call, equal, a):
    med = {n: statistics.median(v) for n, v in times.items()}
    yardstick = med["k_single_calls"] - (K - 1) * med["forward"]
    over = med["one_call"] / yardstick
    (b_lo, b_hi), (c_lo, c_hi) = _spread(times["chunk1"]), _spread(times["one_call"])
    row = {n + "_ms": summary(v, 1e3, "ms", 3) for n, v in times.items()}
    row.update(K=K, yardstick_ms=round(yardstick * 1e3, 3), one_call_over_yardstick=round(over, 4),
               yardstick="met" if over <= 1.0 else f"missed by {round((over - 1.0) * 100, 1)} %",
               one_call_over_k_single_calls=round(med["one_call"] / med["k_single_calls"], 4),
               one_call_over_chunk1=round(med["one_call"] / med["chunk1"], 4),
               class_axis_saves_ms=round((med["chunk1"] - med["one_call"]) * 1e3, 3),
               # the windows of (b) and (c) overlap: the difference of the medians is not told apart from the spread
               class_axis_inside_the_window_spread=bool(c_hi >= b_lo and b_hi >= c_lo),
               peak_bytes_single_call=_peak_bytes(lambda: single(0)), peak_bytes_one_call=_peak_bytes(one_call),
               bitwise_equal_to_single_calls=equal, calls_per_window=a.steps, warmup_calls=a.warmup, windows_per_version=a.rounds)
    return row


def bench_config(name, Ks, a):
    make, dtype = CONFIGS[name]
    gen, forward_of, single_of, classes_of = make(dtype, Ks)
    rows, ok = {}, True
    with torch.no_grad():
        logits = forward_of().float()

    def forward():
        with torch.no_grad():
            return forward_of()
    for K in Ks:
        classes = torch.topk(logits, K).indices.contiguous()
        single = lambda k, c=classes: single_of(c[:, k])                          # noqa: E731
        one_call = lambda c=classes: classes_of(c)                                # noqa: E731
        got = one_call().maps["attnlrp"]
        equal = all(_same(got[:, k], single(k)) for k in range(K))
        del got
        fns = {"k_single_calls": lambda: [single(k) for k in range(K)], "chunk1": lambda c=classes: classes_of(c, chunk=1),
               "one_call": one_call, "forward": forward}
        times = alternate(fns, a.rounds, partial(event_window, n=a.steps), a.warmup)
        rows[f"K{K}"] = _row(K, times, single, one_call, equal, a)
        ok = ok and equal
    gen.check()
    del gen
    torch.cuda.empty_cache()
    return rows, ok


def bench_kernels(Ks, a):
    """every class entry against K launches of its parent on the slices of the same G"""
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import ops
    dev, rows_n, out = "cuda:0", 64 * 197, {}
    for K in Ks:
        for C in (768, 3072):
            n = rows_n * C
            G = seeded_randn((K, rows_n, C), K + C).to(dev)
            Y = seeded_randn((rows_n, C), C).to(dev)
            gamma, buf = seeded_randn((C,), 3).to(dev), torch.empty_like(G)
            rstd = ops.alrp_row_rstd(Y, 1e-6)
            legs = {"damp": (lambda g, o: ops.alrp_damp(g, Y, 1e-6, out=o), (2 * K + 1) * 4.0 * n, 3 * K * 4.0 * n),
                    "act_gelu": (lambda g, o: ops.alrp_act(g, Y, "gelu", out=o), (2 * K + 1) * 4.0 * n, 3 * K * 4.0 * n),
                    "layernorm": (lambda g, o: ops.alrp_layernorm(g, gamma, rstd, out=o), 2 * K * 4.0 * n, 2 * K * 4.0 * n)}
            if C == 768:
                x0, G4 = Y.view(64, 197, C), G.view(K, 64, 197, C)
                legs["token_relevance"] = (None, (K + 1) * 4.0 * n, 2 * K * 4.0 * n)
            for rule, (fn, bytes_classes, bytes_parent) in legs.items():
                if rule == "token_relevance":
                    fns = {"classes": lambda: ops.alrp_token_relevance(x0, G4, skip_first=True),
                           "k_parent_launches": lambda: [ops.alrp_token_relevance(x0, G4[k], skip_first=True) for k in range(K)]}
                else:
                    fns = {"classes": lambda fn=fn: fn(G, buf),
                           "k_parent_launches": lambda fn=fn: [fn(G[k], buf[k]) for k in range(K)]}
                ts = alternate(fns, a.rounds, partial(event_window, n=a.kernel_steps), a.warmup)
                med = {m: statistics.median(v) for m, v in ts.items()}
                row = {m + "_us": summary(v) for m, v in ts.items()}
                row.update(classes_over_k_parent_launches=round(med["classes"] / med["k_parent_launches"], 4),
                           algorithmic_MB_classes=round(bytes_classes / 1e6, 1), algorithmic_MB_k_parent_launches=round(bytes_parent / 1e6, 1),
                           classes_TB_per_s=round(bytes_classes / med["classes"] / 1e12, 3),
                           k_parent_launches_TB_per_s=round(bytes_parent / med["k_parent_launches"] / 1e12, 3),
                           classes_share_of_measured_copy_rate=round(bytes_classes / med["classes"] / MEASURED_COPY_BYTES_PER_S, 4))
                out[f"{rule}.K{K}.rows{rows_n}.C{C}"] = row
            del G, Y, buf
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=sorted(CONFIGS), default=["vit_b16.fp32", "vit_b16.bf16", "bert_base.fp32"])
    ap.add_argument("--ks", default="2,5")
    ap.add_argument("--steps", type=int, default=2, help="calls per timed window")
    ap.add_argument("--kernel-steps", type=int, default=10, help="launches per timed window of the kernel level")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per version (the versions take turns)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--profile-call", choices=sorted(CONFIGS), help="run the one call alone (3 calls at max(K)) and exit")
    ap.add_argument("--producers", choices=["stock", "fused"], default="fused")
    ap.add_argument("--tuned-gemms", choices=["on", "off"], default="on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attnlrp_classes_bench.json"))
    a = ap.parse_args()
    Ks = tuple(int(k) for k in a.ks.split(","))

    import transformer_explainability_amd as te
    from transformer_explainability_amd import ops
    te._lib.require_device()                         # no device: fail, never time the host
    ops.USE_FUSED_PRODUCERS = a.producers == "fused"
    tuned = te.enable_tuned_gemms() if a.tuned_gemms == "on" else False
    if a.profile_call:
        make, dtype = CONFIGS[a.profile_call]
        gen, forward_of, _, classes_of = make(dtype, Ks)
        with torch.no_grad():
            classes = torch.topk(forward_of().float(), max(Ks)).indices.contiguous()
        for _ in range(3):
            classes_of(classes)
        torch.cuda.synchronize()
        gen.check()
        return
    res = {"bench": "attnlrp_classes", "device": torch.cuda.get_device_name(0), "producers": a.producers, "tuned_gemms": bool(tuned),
           "measured_copy_TB_per_s": MEASURED_COPY_BYTES_PER_S / 1e12, "configs": {}}
    ok = True
    for name in a.configs:
        rows, good = bench_config(name, Ks, a)
        res["configs"][name] = rows
        ok = ok and good
    if not a.skip_kernels:
        res["kernels"] = bench_kernels(Ks, a)
    res["passed"] = ok
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not ok:
        sys.exit("attnlrp_classes_bench FAILED: a map of the one call differs from the single call's")


if __name__ == "__main__":
    main()
