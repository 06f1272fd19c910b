"""Several explanation methods of the same batch: one call per method against ONE pass for all of them, in one process.

    python benchmarks/sweep_all_bench.py [--batch 64] [--bert-batch 32] [--seq 512] [--dtypes fp32,bf16] [--steps 3]
                                         [--warmup 1] [--rounds 5] [--skip-vit] [--skip-bert] [--out F]

  * ViT-B/16, 224 x 224, batch 64, per dtype: the five sweep methods that run on the "ours" model (rollout, lrp,
    transformer_attribution, attn_last_layer, attn_gradcam; the baselines built on the same model object), each through
    ``SaliencySweep(method).explain``, then ``SaliencySweepAll(the five).explain`` (sweep.py).
  * BERT-base, 512 tokens, batch 32 (fp32): the six ``Generator.generate_*`` methods one by one, then ``Generator.generate_all``.

The versions take turns: --rounds timed windows each, --steps calls per window, device events around a window that ends in a
synchronise, after --warmup untimed calls of every version.  Reported per configuration (medians over the windows, and the
min / max window of every version): the sum of the single calls, the one pass, their ratio, the dearest single method, and
the time of every method's TAIL alone (the part that runs after forward, backward and relprop; every timed tail call
follows a full pass without a synchronise in between, as it does inside a call).  No ratio is promised.  The yardstick of the one pass is the dearest single method of the same run: the
script FAILS (exit status 1, after writing the result) unless

    one pass  <=  dearest single method + the tails of the other methods,

all measured in this run, and unless every entry of the one pass is bit for bit what the single call returned on the same
batch (the tails read only what the pass left on the model; the kernels are deterministic).
One JSON line is printed and written to --out (default profiles/sweep_all_bench.json).
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

from benchmarks._models import bert_base, vit_b16  # noqa: E402
from benchmarks._timing import alternate, event_window, summary  # noqa: E402  (the event-window protocol)

VIT_METHODS = ("rollout", "lrp", "transformer_attribution", "attn_last_layer", "attn_gradcam")
BERT_METHODS = ("LRP", "LRP_last_layer", "full_lrp", "attn_last_layer", "rollout", "attn_gradcam")
_ms = partial(summary, scale=1e3, unit="ms", digits=3)


def _tails_in_context(pass_fn, tail_fns, rounds, warmup):
    """{name: [seconds of one tail call]}: every timed tail call follows a full pass WITHOUT a synchronise in between, as a
    tail does inside a single call and inside the one pass -- its operands were written a whole pass ago and its launches
    queue up behind the pass (a tail timed in a tight loop of its own re-reads what it has just read)."""
    for fn in tail_fns.values():
        for _ in range(warmup):
            pass_fn()
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in tail_fns}
    for _ in range(rounds):
        for name, fn in tail_fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pass_fn()
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / 1e3)
    return times


def _same(a, b):
    a, b = a.detach(), b.detach()
    return bool(a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b))
                and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


def _report(single, tails, one_pass, equal, steps, warmup, rounds):
    """single / tails: {method: [s per call]}, one_pass: [s per call] -> the result row and whether the run passes."""
    med = {m: statistics.median(v) for m, v in single.items()}
    tail = {m: statistics.median(v) for m, v in tails.items()}
    dearest = max(med, key=med.get)
    allowed = med[dearest] + sum(t for m, t in tail.items() if m != dearest)
    one = statistics.median(one_pass)
    ok = bool(one <= allowed and all(equal.values()))
    row = {"single_ms": {m: _ms(v) for m, v in single.items()}, "tail_ms": {m: _ms(v) for m, v in tails.items()},
           "one_pass_ms": _ms(one_pass), "sum_of_singles_ms": round(sum(med.values()) * 1e3, 3),
           "sum_over_one_pass": round(sum(med.values()) / one, 3), "dearest_single": dearest,
           "dearest_single_ms": round(med[dearest] * 1e3, 3),
           "one_pass_over_dearest_single": round(one / med[dearest], 3),
           "allowed_ms": round(allowed * 1e3, 3),       # the dearest single method + the other methods' tails
           "within_allowed": bool(one <= allowed), "bitwise_equal_to_single_calls": equal,
           "calls_per_window": steps, "warmup_calls": warmup, "windows_per_version": rounds}
    return row, ok


def bench_vit(dtype, B, steps, warmup, rounds):
    from transformer_explainability_amd import generators as G
    from transformer_explainability_amd import sweep as S
    from transformer_explainability_amd import vit
    model = vit_b16(dtype)
    lrp, base = G.LRP(model), G.Baselines(model)
    x = S.normalize(torch.rand((B, 3, 224, 224), generator=torch.Generator().manual_seed(B)).to("cuda:0"))
    singles = {m: S.SaliencySweep(m, lrp=lrp, baselines=base) for m in VIT_METHODS}
    sweep_all = S.SaliencySweepAll(VIT_METHODS, lrp=lrp, baselines=base)
    assert [k for k, _, _ in sweep_all.groups] == ["lrp"]
    want = {m: s.explain(x).clone() for m, s in singles.items()}
    got = sweep_all.explain(x)
    equal = {m: _same(got[m], want[m]) for m in VIT_METHODS}
    del want, got
    fns = {m: (lambda s=s: s.explain(x)) for m, s in singles.items()}
    fns["one_pass"] = lambda: sweep_all.explain(x)
    t = alternate(fns, rounds, partial(event_window, n=steps), warmup)
    # the tails alone, each behind a pass that has just populated the caches it reads (a tail changes none of them)
    H = x.shape[-1]
    tail_fns = {
        "rollout": lambda: S._heat(G.attn_rollout_tail(model, 1), B, H),
        "lrp": lambda: S._heat(vit.relprop_tail(model, "transformer_attribution", None, False, 1), B, H),
        "transformer_attribution": lambda: S._heat(vit.relprop_tail(model, "grad", None, False, 1), B, H),
        "attn_last_layer": lambda: S._heat(vit.relprop_tail(model, "last_layer_attn"), B, H),
        "attn_gradcam": lambda: S._heat(G.cam_attn_tail(model), B, H)}
    tails = _tails_in_context(lambda: sweep_all.explain(x), tail_fns, rounds, warmup)
    lrp.check()
    one_pass = t.pop("one_pass")
    del model, lrp, base, singles, sweep_all
    torch.cuda.empty_cache()
    return _report(t, tails, one_pass, equal, steps, warmup, rounds)


def bench_bert(B, N, steps, warmup, rounds):
    from transformer_explainability_amd import generators as G
    model = bert_base()
    g = torch.Generator().manual_seed(N)
    ids = torch.randint(1000, 30000, (B, N), generator=g).to("cuda:0")
    mask = torch.ones((B, N), device="cuda:0")
    mask[B // 2:, N - N // 4:] = 0                   # half of the batch padded
    gen = G.Generator(model)
    fns = {"LRP": lambda: gen.generate_LRP(ids, mask), "LRP_last_layer": lambda: gen.generate_LRP_last_layer(ids, mask),
           "full_lrp": lambda: gen.generate_full_lrp(ids, mask), "attn_last_layer": lambda: gen.generate_attn_last_layer(ids, mask),
           "rollout": lambda: gen.generate_rollout(ids, mask), "attn_gradcam": lambda: gen.generate_attn_gradcam(ids, mask)}
    want = {m: fn().clone() for m, fn in fns.items()}
    got = gen.generate_all(ids, mask, BERT_METHODS)
    equal = {m: _same(got[m], want[m]) for m in BERT_METHODS}
    del want, got
    fns["one_pass"] = lambda: gen.generate_all(ids, mask, BERT_METHODS)
    t = alternate(fns, rounds, partial(event_window, n=steps), warmup)
    held = {}

    def whole_pass():                                # every cache populated + the relevance of the encoder input
        held["cam"] = gen._pass(ids, mask, None, 0, "all", True, False)[1]

    tail_fns = {"LRP": lambda: G.lrp_tail(model, 11), "LRP_last_layer": lambda: G.lrp_last_layer_tail(model),
                "full_lrp": lambda: G.full_lrp_tail(held["cam"]), "attn_last_layer": lambda: G.attn_last_layer_tail(model),
                "rollout": lambda: G.rollout_tail(model, 0), "attn_gradcam": lambda: G.attn_gradcam_tail(model)}
    tails = _tails_in_context(whole_pass, tail_fns, rounds, warmup)
    gen.check()
    one_pass = t.pop("one_pass")
    del model, gen, held
    torch.cuda.empty_cache()
    return _report(t, tails, one_pass, equal, steps, warmup, rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--bert-batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--steps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls of every version before the windows")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per version (the versions take turns)")
    ap.add_argument("--skip-vit", action="store_true")
    ap.add_argument("--skip-bert", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_all_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()                         # no device: fail, never time the host
    res = {"bench": "sweep_all", "device": torch.cuda.get_device_name(0), "configs": {}}
    ok = True
    if not a.skip_vit:
        for name in a.dtypes.split(","):
            dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[name]
            row, good = bench_vit(dtype, a.batch, a.steps, a.warmup, a.rounds)
            res["configs"][f"vit_b16_224.batch{a.batch}.{name}"] = row
            ok = ok and good
    if not a.skip_bert:
        row, good = bench_bert(a.bert_batch, a.seq, a.steps, a.warmup, a.rounds)
        res["configs"][f"bert_base.seq{a.seq}.batch{a.bert_batch}.fp32"] = row
        ok = ok and good
    res["passed"] = ok
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    if not ok:
        bad = {k: {"one_pass_ms": r["one_pass_ms"]["median_ms"], "allowed_ms": r["allowed_ms"],
                   "equal": r["bitwise_equal_to_single_calls"]} for k, r in res["configs"].items()}
        sys.exit(f"sweep_all_bench FAILED: the one pass is dearer than the dearest single method plus the other methods' "
                 f"tails, or its maps differ from the single calls: {bad}")


if __name__ == "__main__":
    main()
