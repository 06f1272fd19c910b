#!/usr/bin/env python
"""Generate tests/golden/rationale.npz by running the UNMODIFIED reference's own functions on the CPU.

    python tests/golden/make_golden_rationale.py          # needs the reference checkout (oracle/ref_harness.REFERENCE_ROOT)

32 seeded synthetic documents of 180-420 words, tokenised by a toy id -> wordpiece table into 512 wordpieces ([CLS] ...
[SEP] [PAD]...; the longer documents are truncated, some in the middle of a word), seeded relevance per wordpiece, seeded
human rationale spans over the WHOLE document (so some rationale words lie beyond the truncation), seeded class
probabilities of the original and the erased inputs.  Data only.  The expected values come from:

  ref_word_scores   bert_pipeline.scores_per_word_from_scores_per_token(words, toy tokenizer, input_ids, clamp(scores, 0))
  hard_*            metrics.score_hard_rationale_predictions(truth, pred) per k, pred = cam.topk(k) as bert_pipeline.py:567-574
                    (per document: hard_doc, hard_tp; all documents: hard_micro, hard_macro)
  soft_*            metrics.score_soft_tokens (per document: soft_doc; all documents: soft_all)
  aopc_*, comp, suff  metrics.compute_aopc_scores / metrics.score_classifications on the recorded probabilities

CONDITION (asserted below, not a tolerance): every document has >= 81 scored words, both classes among them, and its k-th and
(k+1)-th largest word scores differ for every k in ks -- so the reference's topk does not depend on the order of ties.
"""
import contextlib
import importlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from oracle import ref_harness as rh  # noqa: E402

D, N = 32, 512
KS = list(range(5, 85, 5))
THRESHOLDS = [0.01, 0.05, 0.1, 0.2, 0.5]
PAD, UNK, CLS, SEP, FIRST = 0, 100, 101, 102, 1000
LETTERS = "abcdefghijklmnopqrstuvwxyz"


class ToyTokenizer:
    def __init__(self, table):
        self.table = table

    def convert_ids_to_tokens(self, ids):
        return [self.table[int(i)] for i in ids]


def main():
    rh.load_reference_bert()                    # the gensim stub and the transformers shims
    with rh.reference_on_path():
        pipeline = importlib.import_module("BERT_rationale_benchmark.models.pipeline.bert_pipeline")
        metrics = importlib.import_module("BERT_rationale_benchmark.metrics")
        utils = importlib.import_module("BERT_rationale_benchmark.utils")
    rng = np.random.RandomState(20260)
    torch.manual_seed(20260)

    # vocabulary of words and of wordpieces
    vocab = sorted({"".join(rng.choice(list(LETTERS), size=rng.randint(1, 10))) for _ in range(600)})
    table = {PAD: "[PAD]", UNK: "[UNK]", CLS: "[CLS]", SEP: "[SEP]"}
    piece_id = {}

    def pid(text):
        if text not in piece_id:
            piece_id[text] = FIRST + len(piece_id)
            table[piece_id[text]] = text
        return piece_id[text]

    doc_words, input_ids, attention_mask = [], np.full((D, N), PAD, np.int64), np.zeros((D, N), np.int64)
    for d in range(D):
        words = [vocab[i] for i in rng.randint(0, len(vocab), size=rng.randint(180, 421))]
        ids = [CLS]
        for w in words:
            cuts = sorted(set(rng.randint(1, len(w), size=rng.randint(0, 3)).tolist())) if len(w) > 1 else []
            parts = [w[a:b] for a, b in zip([0] + cuts, cuts + [len(w)])]
            ids += [pid(p if j == 0 else "##" + p) for j, p in enumerate(parts)]
        ids = ids[:N - 1] + [SEP]
        input_ids[d, :len(ids)] = ids
        attention_mask[d, :len(ids)] = 1
        doc_words.append(words)
    tok = ToyTokenizer(table)
    scores = (torch.randn(D, N) + 0.3).float()
    cam = scores.clamp(min=0)                                                            # bert_pipeline.py:552

    L = max(len(w) for w in doc_words)
    word_index = {w: i for i, w in enumerate(vocab)}
    words_arr = np.full((D, L), -1, np.int32)
    truth_full = np.zeros((D, L), np.uint8)
    ref_ws, n_words = np.zeros((D, N), np.float32), np.zeros((D,), np.int32)
    for d, words in enumerate(doc_words):
        words_arr[d, :len(words)] = [word_index[w] for w in words]
        for _ in range(rng.randint(3, 9)):                                               # rationale spans
            a = rng.randint(0, len(words) - 1)
            truth_full[d, a:min(len(words), a + rng.randint(1, 25))] = 1
        with contextlib.redirect_stdout(io.StringIO()):
            ws = pipeline.scores_per_word_from_scores_per_token(words, tok, torch.from_numpy(input_ids[d]), cam[d])
        assert ws.dtype == torch.float32
        n_words[d] = len(ws)
        ref_ws[d, :len(ws)] = ws.numpy()
        s = np.sort(ws.numpy())[::-1]
        assert len(ws) >= 81 and all(s[k - 1] != s[k] for k in KS), d                    # the CONDITION
        t = truth_full[d, :len(ws)]
        assert 0 < t.sum() < len(ws), d
    assert (n_words < np.array([len(w) for w in doc_words])).any(), "no truncated document"

    # hard rationales, scored by metrics.py
    K = len(KS)
    hard_doc, hard_tp = np.zeros((D, K, 3)), np.zeros((D, K), np.int64)
    hard_micro, hard_macro = np.zeros((K, 3)), np.zeros((K, 3))
    truth_rats = [[metrics.Rationale(f"ann{d}", f"doc{d}", int(t), int(t) + 1) for t in np.nonzero(truth_full[d, :len(doc_words[d])])[0]]
                  for d in range(D)]
    with contextlib.redirect_stdout(io.StringIO()):
        for i, k in enumerate(KS):
            preds = []
            for d in range(D):
                _, indices = torch.from_numpy(ref_ws[d, :n_words[d]]).topk(k=k)          # bert_pipeline.py:569
                pred = [metrics.Rationale(f"ann{d}", f"doc{d}", int(j), int(j) + 1) for j in indices.tolist()]
                preds.append(pred)
                one = metrics.score_hard_rationale_predictions(truth_rats[d], pred)
                assert one["instance_micro"] == one["instance_macro"]
                hard_doc[d, i] = [one["instance_micro"][c] for c in ("p", "r", "f1")]
                hard_tp[d, i] = len(set(truth_rats[d]) & set(pred))
            both = metrics.score_hard_rationale_predictions(sum(truth_rats, []), sum(preds, []))
            hard_micro[i] = [both["instance_micro"][c] for c in ("p", "r", "f1")]
            hard_macro[i] = [both["instance_macro"][c] for c in ("p", "r", "f1")]

    # soft scores
    paired = [metrics.PositionScoredDocument(f"ann{d}", f"doc{d}", tuple(float(v) for v in ref_ws[d, :n_words[d]]),
                                             tuple(bool(v) for v in truth_full[d, :n_words[d]])) for d in range(D)]
    names = ("auprc", "average_precision", "roc_auc_score")
    soft_doc = np.array([[metrics.score_soft_tokens([p])[c] for c in names] for p in paired])
    soft_all = np.array([metrics.score_soft_tokens(paired)[c] for c in names])

    # faithfulness numbers from recorded probabilities
    T = len(THRESHOLDS)
    probs = torch.softmax(torch.randn(D, 2 * T + 1, 2) * 1.5, -1).float().numpy()
    labels = ["NEG", "POS"]
    dist = lambda row: {labels[c]: float(row[c]) for c in range(2)}                      # noqa: E731
    h = THRESHOLDS.index(0.1)
    instances = [{"annotation_id": f"ann{d}", "classification": labels[int(probs[d, 0].argmax())],
                  "classification_scores": dist(probs[d, 0]),
                  "comprehensiveness_classification_scores": dist(probs[d, 1 + h]),
                  "sufficiency_classification_scores": dist(probs[d, 1 + T + h]),
                  "thresholded_scores": [{"threshold": t, "comprehensiveness_classification_scores": dist(probs[d, 1 + i]),
                                          "sufficiency_classification_scores": dist(probs[d, 1 + T + i])}
                                         for i, t in enumerate(THRESHOLDS)]} for d in range(D)]
    _, comp_aopc, comp_points, suff_aopc, suff_points = metrics.compute_aopc_scores(instances, THRESHOLDS)
    annotations = [utils.Annotation(f"ann{d}", "", frozenset(), labels[d % 2]) for d in range(D)]
    cls = metrics.score_classifications(instances, annotations, {}, THRESHOLDS)
    assert cls["comprehensiveness_aopc"] == comp_aopc

    pieces = np.array([table.get(i, "") for i in range(max(table) + 1)])
    out = os.path.join(HERE, "rationale.npz")
    np.savez_compressed(
        out, vocab=np.array(vocab), pieces=pieces, doc_words=words_arr, truth_full=truth_full, input_ids=input_ids,
        attention_mask=attention_mask, scores=scores.numpy(), ref_word_scores=ref_ws[:, :int(n_words.max())],
        ref_n_words=n_words, ks=np.array(KS, np.int64), hard_doc=hard_doc, hard_tp=hard_tp, hard_micro=hard_micro,
        hard_macro=hard_macro, soft_doc=soft_doc, soft_all=soft_all, thresholds=np.array(THRESHOLDS), probs=probs,
        aopc_comp=np.float64(comp_aopc), aopc_comp_points=np.array(comp_points), aopc_suff=np.float64(suff_aopc),
        aopc_suff_points=np.array(suff_points), comp=np.float64(cls["comprehensiveness"]), suff=np.float64(cls["sufficiency"]))
    print(out, os.path.getsize(out), "bytes;", D, "documents,", int(n_words.min()), "-", int(n_words.max()), "scored words")


if __name__ == "__main__":
    main()
