"""Several classes of the same batch: K single calls against ONE generate_classes call, in one process.

    python benchmarks/classes_bench.py [--batch 64] [--bert-batch 32] [--seq 512] [--dtypes fp32,bf16] [--ks 2,5] [--steps 2]
                                       [--warmup 1] [--rounds 5] [--skip-vit] [--skip-bert] [--out F]

  * ViT-B/16, 224 x 224, batch 64, per dtype: ``LRP.generate_LRP(method="transformer_attribution", start_layer=1)``.
  * BERT-base, 512 tokens, batch 32 (fp32): ``Generator.generate_LRP(start_layer=0)``.

Per configuration and K (the K largest logits of every sample, held in a device tensor), the versions taking turns --
--rounds timed windows each, --steps calls per window, device events around a window that ends in a synchronise, after
--warmup untimed calls of every version:

  (a) k_single_calls   K single calls, one per class column
  (b) one_call         one ``generate_classes(classes=[B,K])``
  (c) forward          one forward pass alone under the settings of the pass (autograd graph built, the GELU-backward
                       plane hand-off open)
  (d) peak allocated bytes of (b) and of one single call (torch.cuda.max_memory_allocated over one call each)

The yardstick of (b) is (a) - (K - 1) x (c): the K single calls less the forward passes the one call does not run.  Medians
over the windows, and the min / max window of every version.  No ratio is promised; the script FAILS (exit status 1, after
writing the result) only if a map of the one call differs from the single call's on the same batch.
One JSON line is printed and written to --out (default profiles/classes_bench.json).
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
from benchmarks._timing import alternate, event_window  # noqa: E402  (the event-window protocol)
from benchmarks.sweep_all_bench import _ms, _same  # noqa: E402


def _peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return int(peak)


def _row(K, single, one_call, times, equal, steps, warmup, rounds):
    """single(k) / one_call(): the calls whose peak memory is taken; times: {version: [s per call]} -> the result row."""
    med = {n: statistics.median(v) for n, v in times.items()}
    yardstick = med["k_single_calls"] - (K - 1) * med["forward"]
    return {"K": K, "k_single_calls_ms": _ms(times["k_single_calls"]), "one_call_ms": _ms(times["one_call"]),
            "forward_ms": _ms(times["forward"]),
            "yardstick_ms": round(yardstick * 1e3, 3),                 # (a) - (K - 1) x (c)
            "one_call_over_k_single_calls": round(med["one_call"] / med["k_single_calls"], 4),
            "one_call_over_yardstick": round(med["one_call"] / yardstick, 4),
            "saved_ms": round((med["k_single_calls"] - med["one_call"]) * 1e3, 3),
            "saved_over_skipped_forwards": round((med["k_single_calls"] - med["one_call"]) / ((K - 1) * med["forward"]), 4),
            "peak_bytes_one_call": _peak_bytes(one_call), "peak_bytes_single_call": _peak_bytes(lambda: single(0)),
            "bitwise_equal_to_single_calls": equal,
            "calls_per_window": steps, "warmup_calls": warmup, "windows_per_version": rounds}


def _bench(Ks, logits_of, single_of, one_call_of, forward, name, steps, warmup, rounds):
    rows, ok = {}, True
    with torch.no_grad():
        logits = logits_of().float()
    for K in Ks:
        classes = torch.topk(logits, K).indices.contiguous()
        single = lambda k, c=classes: single_of(c[:, k])                         # noqa: E731
        one_call = lambda c=classes: one_call_of(c)                              # noqa: E731
        got = one_call().maps[name]
        equal = all(_same(got[:, k], single(k)) for k in range(K))
        del got
        fns = {"k_single_calls": lambda: [single(k) for k in range(K)], "one_call": one_call, "forward": forward}
        times = alternate(fns, rounds, partial(event_window, n=steps), warmup)
        rows[f"K{K}"] = _row(K, single, one_call, times, equal, steps, warmup, rounds)
        ok = ok and equal
    return rows, ok


def bench_vit(dtype, B, Ks, steps, warmup, rounds):
    from transformer_explainability_amd import generators as G
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.sweep import normalize
    model = vit_b16(dtype)
    lrp = G.LRP(model)
    x = normalize(torch.rand((B, 3, 224, 224), generator=torch.Generator().manual_seed(B)).to("cuda:0")).to(dtype)

    def forward():
        with ops.gelu_backward_plane_handoff():
            return model(x)
    rows, ok = _bench(Ks, lambda: model(x),
                      lambda idx: lrp.generate_LRP(x, index=idx, method="transformer_attribution", start_layer=1),
                      lambda c: lrp.generate_classes(x, classes=c, methods=("transformer_attribution",), start_layer=1),
                      forward, "transformer_attribution", steps, warmup, rounds)
    lrp.check()
    del model, lrp
    torch.cuda.empty_cache()
    return rows, ok


def bench_bert(B, N, Ks, steps, warmup, rounds):
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import bert, ops
    from transformer_explainability_amd import generators as G
    model = bert.BertForSequenceClassification(bert.BertConfigLite(num_labels=max(Ks))).eval()
    synthetic_init(model, 0)
    model.to("cuda:0")
    g = torch.Generator().manual_seed(N)
    ids = torch.randint(1000, 30000, (B, N), generator=g).to("cuda:0")
    mask = torch.ones((B, N), device="cuda:0")
    mask[B // 2:, N - N // 4:] = 0                   # half of the batch padded
    gen = G.Generator(model)

    def forward():
        with ops.gelu_backward_plane_handoff():
            return model(input_ids=ids, attention_mask=mask)[0]
    rows, ok = _bench(Ks, lambda: model(input_ids=ids, attention_mask=mask)[0],
                      lambda idx: gen.generate_LRP(ids, mask, index=idx, start_layer=0),
                      lambda c: gen.generate_classes(ids, mask, classes=c, methods=("LRP",), start_layer=0),
                      forward, "LRP", steps, warmup, rounds)
    gen.check()
    del model, gen
    torch.cuda.empty_cache()
    return rows, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--bert-batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--ks", default="2,5")
    ap.add_argument("--steps", type=int, default=2, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls of every version before the windows")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per version (the versions take turns)")
    ap.add_argument("--skip-vit", action="store_true")
    ap.add_argument("--skip-bert", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classes_bench.json"))
    a = ap.parse_args()
    Ks = tuple(int(k) for k in a.ks.split(","))

    import transformer_explainability_amd as te
    te._lib.require_device()                         # no device: fail, never time the host
    res = {"bench": "classes", "device": torch.cuda.get_device_name(0), "configs": {}}
    ok = True
    if not a.skip_vit:
        for name in a.dtypes.split(","):
            dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[name]
            rows, good = bench_vit(dtype, a.batch, Ks, a.steps, a.warmup, a.rounds)
            res["configs"][f"vit_b16_224.batch{a.batch}.{name}.transformer_attribution.start_layer1"] = rows
            ok = ok and good
    if not a.skip_bert:
        rows, good = bench_bert(a.bert_batch, a.seq, Ks, a.steps, a.warmup, a.rounds)
        res["configs"][f"bert_base.seq{a.seq}.batch{a.bert_batch}.fp32.LRP.start_layer0"] = rows
        ok = ok and good
    res["passed"] = ok
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not ok:
        sys.exit("classes_bench FAILED: a map of the one call differs from the single call's")


if __name__ == "__main__":
    main()
