"""The rationale test on the device (te_rationale_metrics_f32, te_token_erase) beside the loop it replaces, in one process on
the same tensors.

    python benchmarks/rationale_eval_bench.py [--batches 1,8,32] [--rounds 9] [--window-ms 50] [--warmup 3] [--skip-model] [--out F]

Prints one JSON line (and writes it to --out):
  * metrics: one RationaleEvaluator.update_from_scores per batch of 512-wordpiece documents at every --batches size (1 is the
    reference's batch size).  Scores are seeded normal values (about half of them tie at 0 under the clamp), words have 1-3
    wordpieces, 20 % of the words are human rationale.  ``old`` is the reference's loop restated in torch on CUDA tensors: per
    document the clamp and the word pooling, sixteen topk calls (bert_pipeline.py:567-569) with the set arithmetic of
    metrics.py:168-199 on their index lists, and the soft scores of the torch function, one document at a time with a host
    round trip each.  ``new`` is the evaluator's device path (one kernel, results stay on the device); ``torch_batched`` the
    evaluator's torch functions on the same CUDA tensors (device_path=False).  The versions alternate, --rounds timed windows
    each of at least --window-ms (host clock between two device synchronisations), after warming every shape; reported:
    median, min and max seconds per update.  ``not_slower_beyond_old_spread``: the new median exceeds the old one by no more
    than the spread (max - min) of the old windows -- the condition under which the device path stays the default.
  * erase: ops.token_erase against rationale.token_erase_torch for the five default thresholds, same scheme.
  * evaluator: documents per second of RationaleEvaluator.update behind Generator(BERT-base).generate_LRP(start_layer=0) at
    batch 32, 512 wordpieces, old and new alternating in the same way, and the explanation alone.
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

from benchmarks._models import bert_base  # noqa: E402
from benchmarks._timing import alternate, summary, wall_window  # noqa: E402  (the wall-window protocol)

KS = list(range(5, 85, 5))


def old_update_from_scores(totals, scores, word_ids, truth):
    """the reference's per-document loop (batch size 1), restated in torch on CUDA tensors"""
    from transformer_explainability_amd import rationale as rt
    n_max = truth.shape[1]
    for b in range(scores.shape[0]):
        cam = scores[b:b + 1].clamp(min=0)                                   # bert_pipeline.py:552
        ws, nw = rt.word_scores(cam, word_ids[b:b + 1], n_max, clamp=False)  # :563
        n = int(nw)                                                          # len(cam): a host read
        cam_w, t = ws[0, :n], truth[b, :n]
        gold = set(torch.nonzero(t).flatten().tolist())
        for i, k in enumerate(KS):
            _, indices = cam_w.topk(k=min(k, n))                             # :569
            pred = set(indices.tolist())                                     # :570-574 + metrics.py:171-174
            totals["tp"][i] += len(gold & pred)
            totals["pred"][i] += len(pred)
        totals["truth"] += len(gold)
        totals["soft"].append(rt.soft_scores(ws, nw, truth[b:b + 1])[0].cpu())   # metrics.py:242-253, per document
    return totals


def new_totals():
    return {"tp": [0] * len(KS), "pred": [0] * len(KS), "truth": 0, "soft": []}


def _verdict(t):
    old, new = t["old"], t["new"]
    return {"speedup_of_medians": round(statistics.median(old) / statistics.median(new), 2),
            "range_below_old": bool(max(new) < min(old)),
            "not_slower_beyond_old_spread": bool(statistics.median(new) <= statistics.median(old) + (max(old) - min(old)))}


def inputs(B, N=512, seed=0):
    """(scores, word_ids, truth, input_ids, attention_mask) on the device"""
    g = torch.Generator().manual_seed(seed + B)
    scores = torch.randn((B, N), generator=g)
    word_ids = torch.full((B, N), -1, dtype=torch.int32)
    mask = torch.zeros((B, N), dtype=torch.int64)
    for b in range(B):
        length = int(torch.randint(N * 3 // 4, N + 1, (1,), generator=g))
        pieces = torch.randint(1, 4, (N,), generator=g).tolist()
        i, w = 1, 0
        while i < length - 1:
            n = min(pieces[w], length - 1 - i)
            word_ids[b, i:i + n] = w
            i, w = i + n, w + 1
        mask[b, :length] = 1
    truth = torch.rand((B, N), generator=g) < 0.2
    ids = torch.randint(1000, 20000, (B, N), generator=g) * mask
    return tuple(t.to("cuda:0") for t in (scores, word_ids, truth, ids, mask))


def _clear(ev):
    for name in ("_counts", "_truth_n", "_soft", "_probs", "_word_scores", "_n_words", "_order", "_n_rationale"):
        getattr(ev, name).clear()


def bench_metrics(batches, rounds, window, warmup):
    from transformer_explainability_amd import ops, rationale as rt
    res = {}
    for B in batches:
        scores, wid, truth, ids, mask = inputs(B)
        ev_new = rt.RationaleEvaluator(None, ks=KS)
        ev_torch = rt.RationaleEvaluator(None, ks=KS, device_path=False)
        got = ev_new.update_from_scores(scores, wid, truth)
        ref = ev_torch.update_from_scores(scores, wid, truth)
        old = old_update_from_scores(new_totals(), scores, wid, truth)
        counts = got["counts"].cpu().long()
        same = (counts[:, :, 0].sum(0).tolist() == old["tp"] and counts[:, :, 1].sum(0).tolist() == old["pred"]
                and torch.equal(got["counts"], ref["counts"]) and torch.equal(got["order"], ref["order"]))
        totals = new_totals()

        def run_new():
            _clear(ev_new)
            ev_new.update_from_scores(scores, wid, truth)

        def run_torch():
            _clear(ev_torch)
            ev_torch.update_from_scores(scores, wid, truth)

        def run_old():
            totals["soft"].clear()
            old_update_from_scores(totals, scores, wid, truth)

        t = alternate({"new": run_new, "old": run_old, "torch_batched": run_torch,
                       "kernel_only": lambda: ops.rationale_metrics(scores, wid, truth, KS)}, rounds, window, warmup)
        res[f"update_from_scores.B{B}.512"] = {
            "new": summary(t["new"]), "old": summary(t["old"]), "torch_batched": summary(t["torch_batched"]),
            "kernel_only": summary(t["kernel_only"]), **_verdict(t), "integers_equal": bool(same),
            "max_abs_soft_new_minus_old": float((got["soft"].cpu() - torch.stack(old["soft"])).abs().max())}
        fr = rt.THRESHOLDS
        e_new = ops.token_erase(ids, mask, wid, got["order"], got["n_words"], fr)
        e_old = rt.token_erase_torch(ids, mask, wid, got["order"], got["n_words"], fr)
        te = alternate({"new": lambda: ops.token_erase(ids, mask, wid, got["order"], got["n_words"], fr),
                        "old": lambda: rt.token_erase_torch(ids, mask, wid, got["order"], got["n_words"], fr)},
                       rounds, window, warmup)
        res[f"token_erase.B{B}.512"] = {"new": summary(te["new"]), "old": summary(te["old"]), **_verdict(te),
                                        "equal": bool(all(torch.equal(a, b) for a, b in zip(e_new, e_old)))}
    return res


def bench_evaluator(rounds, window, warmup, B=32, N=512):
    from transformer_explainability_amd import rationale as rt
    from transformer_explainability_amd.generators import Generator
    gen = Generator(bert_base())
    _, wid, truth, ids, mask = inputs(B, N, seed=7)
    fmask = mask.float()
    explain = lambda i, a, x: gen.generate_LRP(i, a, index=x, start_layer=0)      # noqa: E731
    ev_new = rt.RationaleEvaluator(explain, ks=KS)
    totals = new_totals()

    def run_new():
        _clear(ev_new)
        ev_new.update(ids, fmask, wid, truth)

    def run_old():
        totals["soft"].clear()
        old_update_from_scores(totals, explain(ids, fmask, None).detach(), wid, truth)

    t = alternate({"new": run_new, "old": run_old, "explain_only": lambda: explain(ids, fmask, None)}, rounds, window, warmup)
    gen.check()
    row = {k: {"documents_per_s": round(B / statistics.median(v), 1), **summary(v, 1e3, "ms")} for k, v in t.items()}
    row.update(_verdict(t))
    return {f"update.bert_base.batch{B}.{N}": row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=50.0, help="least duration of a timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "rationale_eval", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    window = partial(wall_window, min_s=a.window_ms / 1e3)
    res["metrics"] = bench_metrics([int(b) for b in a.batches.split(",")], a.rounds, window, a.warmup)
    if not a.skip_model:
        res["evaluator"] = bench_evaluator(a.rounds, window, a.warmup)
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
