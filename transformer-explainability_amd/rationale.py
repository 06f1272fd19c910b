"""Rationale test of a BERT relevance vector, SURVEY.md section 8(f): ERASER Movie Reviews, token F1 at top-k.  Mirror of
the rationale production of BERT_rationale_benchmark/models/pipeline/bert_pipeline.py:547-582 and of the scores of
BERT_rationale_benchmark/metrics.py (hard rationales :168-215, soft scores :217-253, AOPC :255-282, comprehensiveness /
sufficiency :301-313), without the dataset / tokenizer loading, the training loop, the LaTeX rendering and the CLI.

Per document the reference clamps the relevance at 0, pools it per word through a character alignment, calls torch.topk
sixteen times (k = 5 .. 80), writes one result file per k, and a second program (metrics.py) scores the files with sets of
dataclasses and scikit-learn.  On the MI355X all of that is ONE te_rationale_metrics_f32 launch per batch
(ops.rationale_metrics, a workgroup per document), and the erased inputs of ERASER's two faithfulness numbers come out of
ONE te_token_erase launch (ops.token_erase); results stay on the device until ``summary()`` / ``write_results()``.  The torch
functions below are the CPU path and the restatement the kernels are tested against.

Semantics, and where they differ from the reference:
  * ties: words are ranked by descending score, EQUAL SCORES IN ASCENDING WORD INDEX.  torch.topk leaves ties unspecified,
    and after the clamp every non-positive word ties at 0 (the rule te_perturb documents for pixels);
  * k > n_words: the reference's topk raises; here pred_k = min(k, n_words);
  * a NaN score counts as 0 (scikit-learn raises on NaN; the explanation path never produces one);
  * bert_pipeline.py:566-574 never empties ``hard_rationales`` between the k, so its file for k holds the top-5, top-10,
    ... top-k lists one after another; metrics.py reads them into a set, which is the top-k set.  ``write_results`` writes
    that set once;
  * a document whose truth has one class only is left out of auprc, average_precision and roc_auc_score alike
    (metrics.py:229-240 leaves it out of the latter two; its AUPRC is undefined);
  * THE REFERENCE TREE HAS NO PRODUCER for the erased inputs metrics.py:255-313 consumes.  This package's definition: for a
    fraction t the rationale of a document is its first min(n_words, max(1, ceil(t n_words))) ranked words; the
    comprehensiveness input drops every wordpiece of those words, the sufficiency input keeps only those; [CLS], [SEP] and
    [UNK] (word id -1, mask 1) are always kept; kept tokens move to the left in their order, the rest is padding.  The single
    pair of ``comprehensiveness_classification_scores`` / ``sufficiency_classification_scores`` metrics.py:301-313 reads is
    the pair of ``hard_threshold`` (default 0.1, else the last threshold).
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from . import ops

KS = tuple(range(5, 85, 5))                                  # bert_pipeline.py:567
THRESHOLDS = (0.01, 0.05, 0.1, 0.2, 0.5)                     # metrics.py:610
SPECIAL_TOKENS = ("[CLS]", "[SEP]", "[UNK]", "[PAD]")        # bert_pipeline.py:104


def word_ids_from_wordpieces(words, pieces):
    """The character alignment of bert_pipeline.py:96-138 as a word index per wordpiece: ``words`` the document's words,
    ``pieces`` = tokenizer.convert_ids_to_tokens(input_ids) -> a list of len(pieces) ints, -1 for the special tokens and for
    wordpieces past the last word.  Max-pooling the scores over equal indices is scores_per_word_from_scores_per_token.
    Raises ValueError where the reference asserts (the characters of the wordpieces of a word, the last scored word
    excepted, are not that word) and when a wordpiece would straddle two words (the reference would then count its score
    for both)."""
    ids = [-1] * len(pieces)
    built = []                                   # the characters assigned to every scored word
    w, used = 0, 0
    for i, piece in enumerate(pieces):
        if piece in SPECIAL_TOKENS:
            continue
        text = piece.replace("##", "")
        if not text:
            continue
        while w < len(words) and used == len(words[w]):
            if len(words[w]) == 0:
                raise ValueError(f"word {w} is empty: it has no character to align")
            w, used = w + 1, 0
        if w >= len(words):
            break                                # wordpieces past the last word score nothing (:120-122)
        if used + len(text) > len(words[w]):
            raise ValueError(f"wordpiece {i} ({piece!r}) straddles words {w} ({words[w]!r}) and {w + 1}")
        if w == len(built):
            built.append("")
        built[w] += text
        ids[i] = w
        used += len(text)
    if built[:-1] != list(words[:len(built) - 1]) and len(built) > 1:
        bad = next(j for j in range(len(built) - 1) if built[j] != words[j])
        raise ValueError(f"the wordpieces of word {bad} spell {built[bad]!r}, the document has {words[bad]!r}")
    return ids


# ------------------------------------------------------------------------------------------------ torch functions
def word_scores(scores, word_ids, n_max, clamp=True):
    """bert_pipeline.py:552 + :96-138 for a batch: scores [B,N], word_ids [B,N] (-1 = no word; ids >= n_max are ignored) ->
    (word scores fp32 [B,n_max]: the maximum over the word's wordpieces, 0 for a word without one and past n_words;
    n_words int32 [B] = highest word id + 1).  NaN counts as 0."""
    s = scores.float()
    s = torch.where(torch.isnan(s), torch.zeros_like(s), s)
    if clamp:
        s = s.clamp(min=0)
    wid = word_ids.long()
    valid = (wid >= 0) & (wid < n_max)
    slot = torch.where(valid, wid, torch.full_like(wid, n_max))               # column n_max collects the rest
    B = s.shape[0]
    pooled = torch.full((B, n_max + 1), float("-inf"), device=s.device).scatter_reduce(1, slot, s, "amax")
    pieces = torch.zeros((B, n_max + 1), dtype=torch.int32, device=s.device).scatter_add(1, slot, torch.ones_like(slot, dtype=torch.int32))
    n_words = torch.where(valid, wid + 1, torch.zeros_like(wid)).amax(1).to(torch.int32)
    inside = torch.arange(n_max, device=s.device).unsqueeze(0) < n_words.unsqueeze(1)
    out = torch.where((pieces[:, :n_max] > 0) & inside, pooled[:, :n_max], torch.zeros((), device=s.device))
    return out + 0.0, n_words                                                 # (-0 -> +0)


def _ranking(ws, n_words):
    """word indices by descending score, ties in ascending index, the words past n_words last: int64 [B,n_max]"""
    o1 = torch.sort(ws, dim=1, descending=True, stable=True).indices
    beyond = o1 >= n_words.long().unsqueeze(1)
    o2 = torch.sort(beyond.to(torch.uint8), dim=1, stable=True).indices
    return o1.gather(1, o2)


def topk_counts(ws, n_words, truth, ks):
    """bert_pipeline.py:567-574 + the per-document counts of metrics.py:168-199: ws [B,n_max] word scores, n_words [B],
    truth [B,n_max] -> (order int32 [B,n_max]: the ranking, -1 at and past n_words; counts int32 [B,len(ks),2] =
    (tp_k, pred_k) with pred_k = min(k, n_words))."""
    n_max = ws.shape[1]
    rank = torch.arange(n_max, device=ws.device).unsqueeze(0)
    inside = rank < n_words.long().unsqueeze(1)
    order = _ranking(ws, n_words)
    hit = (truth.gather(1, order) != 0) & inside
    tp_at = torch.cumsum(hit.to(torch.int32), 1, dtype=torch.int32)
    out = []
    for k in ks:
        pred = n_words.to(torch.int32).clamp(max=int(k))
        tp = tp_at.gather(1, (pred.long() - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
        out.append(torch.stack([torch.where(pred > 0, tp, torch.zeros_like(tp)), pred], 1))
    return torch.where(inside, order, torch.full_like(order, -1)).to(torch.int32), torch.stack(out, 1)


def soft_scores(ws, n_words, truth):
    """metrics.py:217-253 per document (sklearn.average_precision_score, auc(*precision_recall_curve), roc_auc_score of the
    word scores against truth over the n_words words) -> float64 [B,4] = AP, AUPRC, ROC-AUC, npos; the three scores are 0
    for a document of one class.  One scan over the runs of equal scores in descending order: with (tp_i, n_i) at the end of
    run i, P_i = tp_i / n_i, R_i = tp_i / npos, F_i = (n_i - tp_i) / nneg, P_0 = 1, R_0 = F_0 = 0:
    AP = sum (R_i - R_{i-1}) P_i, AUPRC = sum (R_i - R_{i-1}) (P_i + P_{i-1}) / 2, ROC-AUC = sum (F_i - F_{i-1}) (R_i + R_{i-1}) / 2."""
    B, n_max = ws.shape
    dev = ws.device
    rank = torch.arange(n_max, device=dev).unsqueeze(0).expand(B, n_max)
    nw = n_words.long().unsqueeze(1)
    inside = rank < nw
    order = _ranking(ws, n_words)
    s = ws.gather(1, order)
    hit = (truth.gather(1, order) != 0) & inside
    tp = torch.cumsum(hit.long(), 1)
    n = rank + 1
    nxt = torch.cat([s[:, 1:], s[:, -1:]], 1)
    end = inside & ((n == nw) | (nxt != s))                                   # last element of every run of equal scores
    last_end = torch.cummax(torch.where(end, rank, torch.full_like(rank, -1)), 1).values
    prev = torch.cat([torch.full((B, 1), -1, dtype=torch.long, device=dev), last_end[:, :-1]], 1)      # previous run's end
    has_prev = prev >= 0
    tp_prev = torch.where(has_prev, tp.gather(1, prev.clamp(min=0)), torch.zeros_like(tp))
    n_prev = prev + 1
    npos = torch.where(nw > 0, tp.gather(1, (nw - 1).clamp(min=0)), torch.zeros_like(nw))
    nneg = nw - npos
    both = (npos > 0) & (nneg > 0)
    dpos, dneg = npos.clamp(min=1).double(), nneg.clamp(min=1).double()
    P, R, F = tp.double() / n.double(), tp.double() / dpos, (n - tp).double() / dneg
    Pp = torch.where(has_prev, tp_prev.double() / n_prev.clamp(min=1).double(), torch.ones((), dtype=torch.float64, device=dev))
    Rp, Fp = tp_prev.double() / dpos, (n_prev - tp_prev).double() / dneg
    use = (end & both).double()
    ap = ((R - Rp) * P * use).sum(1)
    pr = ((R - Rp) * ((P + Pp) / 2.0) * use).sum(1)
    roc = ((F - Fp) * ((R + Rp) / 2.0) * use).sum(1)
    return torch.stack([ap, pr, roc, npos.squeeze(1).double()], 1)


def rationale_sizes(n_words, fractions):
    """min(n_words, max(1, ceil(t n_words))) words per fraction t (fp64), 0 for a document without words: int32 [T,B]"""
    nw = n_words.double().unsqueeze(0)
    t = torch.tensor([float(f) for f in fractions], dtype=torch.float64, device=n_words.device).unsqueeze(1)
    m = torch.minimum(torch.ceil(t * nw).clamp(min=1.0), nw)
    return m.to(torch.int32)


def token_erase_torch(input_ids, attention_mask, word_ids, order, n_words, fractions, pad_id=0):
    """ops.token_erase in torch (the CPU path, and what the kernel is tested against): -> (ids_out int64 [2,T,B,N],
    mask_out int64 [2,T,B,N], n_rationale int32 [T,B]); see the module docstring for the definition."""
    B, N = input_ids.shape
    n_max = order.shape[1]
    dev = input_ids.device
    m = rationale_sizes(n_words, fractions)                                              # [T,B]
    T = m.shape[0]
    ranks = torch.arange(n_max, device=dev).unsqueeze(0).expand(B, n_max)
    o = order.long()
    listed = (o >= 0) & (o < n_max) & (ranks < n_words.long().unsqueeze(1))
    rank_of = torch.full((B, n_max + 1), n_max + 1, dtype=torch.long, device=dev)
    rank_of.scatter_(1, torch.where(listed, o, torch.full_like(o, n_max)), torch.where(listed, ranks, torch.full_like(ranks, n_max + 1)))
    wid = word_ids.long()
    has_word = (wid >= 0) & (wid < n_max)
    tok_rank = rank_of[:, :n_max].gather(1, wid.clamp(0, max(n_max - 1, 0)))
    rat = has_word.unsqueeze(0) & (tok_rank.unsqueeze(0) < m.long().unsqueeze(2))        # [T,B,N]
    on = (attention_mask != 0).unsqueeze(0)
    keep = torch.stack([on & ~rat, on & ((wid < 0).unsqueeze(0) | rat)], 0)              # [2,T,B,N]
    pos = torch.cumsum(keep.long(), -1) - 1
    slot = torch.where(keep, pos, torch.full_like(pos, N))
    ids_out = torch.full((2, T, B, N + 1), int(pad_id), dtype=torch.int64, device=dev)
    ids_out.scatter_(-1, slot, input_ids.long().view(1, 1, B, N).expand(2, T, B, N))
    mask_out = torch.zeros((2, T, B, N + 1), dtype=torch.int64, device=dev)
    mask_out.scatter_(-1, slot, torch.ones_like(slot))
    ids_out[..., N] = int(pad_id)
    return ids_out[..., :N].contiguous(), mask_out[..., :N].contiguous(), m


# ------------------------------------------------------------------------------------------------ host arithmetic
def _f1(p, r):
    """metrics.py:100-103"""
    if p == 0 or r == 0:
        return 0
    return 2 * p * r / (p + r)


def hard_scores(tp, pred, truth_n):
    """score_hard_rationale_predictions (metrics.py:168-215) from the integer counts of the documents (sequences of python
    ints): the quotients are python's int / int, i.e. fp64, as the reference's len(...) / len(...)."""
    tp, pred, truth_n = [int(v) for v in tp], [int(v) for v in pred], [int(v) for v in truth_n]
    micro_p = sum(tp) / sum(pred) if sum(pred) > 0 else 0
    micro_r = sum(tp) / sum(truth_n) if sum(truth_n) > 0 else 0
    inst = []
    for a, b, c in zip(tp, pred, truth_n):
        p = a / b if b > 0 else 0
        r = a / c if c > 0 else 0
        inst.append((p, r, _f1(p, r)))
    n = len(inst)
    return {"instance_micro": {"p": micro_p, "r": micro_r, "f1": _f1(micro_p, micro_r)},
            "instance_macro": {"p": sum(i[0] for i in inst) / n, "r": sum(i[1] for i in inst) / n,
                               "f1": sum(i[2] for i in inst) / n}}


def aopc_scores(probs, n_thresholds):
    """_instances_aopc (metrics.py:255-275) for both keys + :301-313 per threshold: probs float64 [D, 2 T + 1, C] (copy 0 the
    original, then T comprehensiveness and T sufficiency copies) -> (comp [D,T], suff [D,T]) differences of the predicted
    class's probability."""
    probs = np.asarray(probs, dtype=np.float64)
    T = int(n_thresholds)
    kls = probs[:, 0].argmax(-1)
    d = np.arange(probs.shape[0])
    beta0 = probs[d, 0, kls]
    comp = beta0[:, None] - probs[d[:, None], 1 + np.arange(T)[None], kls[:, None]]
    suff = beta0[:, None] - probs[d[:, None], 1 + T + np.arange(T)[None], kls[:, None]]
    return comp, suff


class RationaleEvaluator:
    """Running results of the rationale test.  ``explain(input_ids, attention_mask, index) -> relevance [B,N]`` is any BERT
    generator of this package (e.g. ``lambda i, m, x: gen.generate_LRP(i, m, index=x, start_layer=0)``); ``classifier``
    (optional, ``classifier(input_ids=..., attention_mask=...) -> logits`` or a tuple starting with them) switches the two
    faithfulness numbers on.  On CUDA tensors ``update`` / ``update_from_scores`` run the kernels and perform NO
    device-to-host copy; CPU tensors (and ``device_path=False``) take the torch functions."""

    def __init__(self, explain, ks=KS, clamp=True, classifier=None, thresholds=THRESHOLDS, max_forward_batch=256,
                 pad_id=0, hard_threshold=None, device_path=True):
        self.explain, self.classifier = explain, classifier
        self.ks = [int(k) for k in ks]
        self.clamp = bool(clamp)
        self.thresholds = [float(t) for t in thresholds]
        if not 1 <= len(self.ks) <= 16 or min(self.ks) <= 0:
            raise ValueError("RationaleEvaluator takes 1..16 positive rationale sizes")
        if classifier is not None and (not 1 <= len(self.thresholds) <= 8 or not all(0.0 < t <= 1.0 for t in self.thresholds)):
            raise ValueError("RationaleEvaluator takes 1..8 thresholds in (0, 1]")
        if hard_threshold is None:
            hard_threshold = 0.1 if 0.1 in self.thresholds else self.thresholds[-1]
        if classifier is not None and float(hard_threshold) not in self.thresholds:
            raise ValueError(f"hard_threshold {hard_threshold} is not one of the thresholds {self.thresholds}")
        self.hard_index = self.thresholds.index(float(hard_threshold)) if float(hard_threshold) in self.thresholds else 0
        self.max_forward_batch = int(max_forward_batch)
        self.pad_id = int(pad_id)
        self.device_path = bool(device_path)
        self._counts, self._truth_n, self._soft, self._probs = [], [], [], []
        self._word_scores, self._n_words, self._order, self._n_rationale = [], [], [], []

    # ------------------------------------------------------------------------------------------
    def _forward(self, ids, mask):
        outs = []
        for i in range(0, ids.shape[0], self.max_forward_batch):
            out = self.classifier(input_ids=ids[i:i + self.max_forward_batch],
                                  attention_mask=mask[i:i + self.max_forward_batch])
            out = out.logits if hasattr(out, "logits") else out
            outs.append(out[0] if isinstance(out, (tuple, list)) else out)
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)

    def update(self, input_ids, attention_mask, word_ids, truth, truth_total=None, index=None):
        """One batch: input_ids / attention_mask [B,N], word_ids [B,N] (word_ids_from_wordpieces per document), truth
        [B,Wmax] bool, truth_total [B] (optional) = the document's rationale words INCLUDING those beyond the truncation to
        N wordpieces, which count as missed recall as in metrics.py; index: the explained class (None = the predicted)."""
        scores = self.explain(input_ids, attention_mask, index).detach()
        return self.update_from_scores(scores, word_ids, truth, truth_total, input_ids, attention_mask)

    @staticmethod
    def update_all(evaluators, generator, input_ids, attention_mask, word_ids, truth, truth_total=None, index=None,
                   start_layer=11, rollout_start_layer=0):
        """One batch for SEVERAL methods: ``evaluators`` = {Generator.generate_all name: RationaleEvaluator}; ONE
        ``generator.generate_all`` serves every method's relevance (one forward pass, at most one backward pass and one
        relprop chain), then each evaluator's ``update_from_scores`` runs as in ``update``.  The faithfulness forwards
        stay per method: the erased inputs differ.  -> {name: what update returns}."""
        scores = generator.generate_all(input_ids, attention_mask, tuple(evaluators), index=index,
                                        start_layer=start_layer, rollout_start_layer=rollout_start_layer)
        return {name: ev.update_from_scores(scores[name].detach(), word_ids, truth, truth_total, input_ids, attention_mask)
                for name, ev in evaluators.items()}

    @torch.no_grad()
    def update_from_scores(self, scores, word_ids, truth, truth_total=None, input_ids=None, attention_mask=None):
        scores = scores.float()
        truth = truth if truth.dtype in (torch.bool, torch.uint8) else truth != 0
        on_device = scores.is_cuda and self.device_path
        if on_device:
            ws, nw, order, counts, soft = ops.rationale_metrics(scores, word_ids, truth, self.ks, clamp=self.clamp)
        else:
            ws, nw = word_scores(scores, word_ids, truth.shape[1], clamp=self.clamp)
            order, counts = topk_counts(ws, nw, truth, self.ks)
            soft = soft_scores(ws, nw, truth)
        truth_n = soft[:, 3].to(torch.int64) if truth_total is None else truth_total.to(soft.device, torch.int64)
        out = {"word_scores": ws, "n_words": nw, "order": order, "counts": counts, "soft": soft, "truth_n": truth_n}
        if self.classifier is not None:
            if input_ids is None or attention_mask is None:
                raise ValueError("the faithfulness numbers need input_ids and attention_mask")
            erase = ops.token_erase if on_device else token_erase_torch
            ids_out, mask_out, n_rat = erase(input_ids, attention_mask, word_ids, order, nw, self.thresholds,
                                             pad_id=self.pad_id)
            B, N = input_ids.shape
            T = len(self.thresholds)
            ids = torch.cat([input_ids.to(torch.int64).reshape(1, B, N), ids_out.reshape(2 * T, B, N)], 0)
            mask = torch.cat([attention_mask.to(torch.int64).reshape(1, B, N), mask_out.reshape(2 * T, B, N)], 0)
            logits = self._forward(ids.reshape(-1, N), mask.reshape(-1, N)).float()
            probs = torch.softmax(logits, dim=-1).reshape(2 * T + 1, B, -1).transpose(0, 1)      # [B, 2T+1, C]
            out.update(erased_ids=ids_out, erased_mask=mask_out, n_rationale=n_rat, probs=probs)
            self._probs.append(probs)
            self._n_rationale.append(n_rat.transpose(0, 1))
        self._counts.append(counts)
        self._truth_n.append(truth_n)
        self._soft.append(soft)
        self._word_scores.append(ws)
        self._n_words.append(nw)
        self._order.append(order)
        return out

    # ------------------------------------------------------------------------------------------
    def _host(self, parts):
        return torch.cat([p.reshape(p.shape[0], -1) if p.dim() > 1 else p for p in parts], 0).cpu().numpy() if parts else None

    def summary(self):
        """{"hard": {k: {"instance_micro": {p, r, f1}, "instance_macro": {p, r, f1}}}, "auprc", "average_precision",
        "roc_auc_score"} and, with a classifier, "comprehensiveness", "sufficiency", their "_aopc" and "_aopc_points" and
        "aopc_thresholds" -- the names of metrics.py."""
        if not self._counts:
            raise RuntimeError("RationaleEvaluator.summary() before any update")
        K = len(self.ks)
        counts = self._host(self._counts).reshape(-1, K, 2)
        truth_n = self._host(self._truth_n)
        soft = self._host(self._soft).reshape(-1, 4)
        nw = self._host(self._n_words)
        out = {"hard": {k: hard_scores(counts[:, i, 0], counts[:, i, 1], truth_n) for i, k in enumerate(self.ks)}}
        both = (soft[:, 3] > 0) & (soft[:, 3] < nw)
        kept = soft[both]
        for j, name in enumerate(("average_precision", "auprc", "roc_auc_score")):
            out[name] = float(np.average(kept[:, j])) if len(kept) else 0.0
        if self._probs:
            T = len(self.thresholds)
            probs = torch.cat(self._probs, 0).double().cpu().numpy()
            comp, suff = aopc_scores(probs, T)
            out["aopc_thresholds"] = list(self.thresholds)
            out["comprehensiveness"] = float(np.average(comp[:, self.hard_index]))
            out["sufficiency"] = float(np.average(suff[:, self.hard_index]))
            out["comprehensiveness_aopc"] = float(np.average(comp))
            out["comprehensiveness_aopc_points"] = np.average(comp, axis=0).tolist()
            out["sufficiency_aopc"] = float(np.average(suff))
            out["sufficiency_aopc_points"] = np.average(suff, axis=0).tolist()
        return out

    def write_results(self, directory, doc_ids, class_names=None, doc_lengths=None):
        """Per k one ``identifier_results_{k}.json`` in the layout of bert_pipeline.py:575-582 (one JSON object per line:
        the top-k words as one-token spans), and ``instances.jsonl`` with, per document, the hard rationale of
        ``hard_threshold``, the word scores as ``soft_rationale_predictions`` (0 up to doc_lengths[d] when given: metrics.py
        wants one value per document token) and, with a classifier, ``classification``, ``classification_scores``,
        ``comprehensiveness_classification_scores``, ``sufficiency_classification_scores`` and ``thresholded_scores`` in the
        field layout metrics.py reads -- so that ERASER's own script can score the files.  Returns the file paths."""
        os.makedirs(directory, exist_ok=True)
        doc_ids = [str(d) for d in doc_ids]
        nw = self._host(self._n_words)
        if len(doc_ids) != len(nw):
            raise ValueError(f"{len(doc_ids)} document ids for {len(nw)} documents")
        order = [row for part in self._order for row in part.cpu().numpy()]
        scores = [row for part in self._word_scores for row in part.cpu().numpy()]
        paths = []
        for k in self.ks:
            paths.append(os.path.join(directory, f"identifier_results_{k}.json"))
            with open(paths[-1], "w") as f:
                for d, doc in enumerate(doc_ids):
                    spans = [{"start_token": int(w), "end_token": int(w) + 1} for w in order[d][:min(k, int(nw[d]))]]
                    f.write(json.dumps({"annotation_id": doc, "rationales": [{"docid": doc, "hard_rationale_predictions": spans}]}) + "\n")
        probs = torch.cat(self._probs, 0).double().cpu().numpy() if self._probs else None
        n_rat = self._host(self._n_rationale).reshape(len(nw), -1) if self._n_rationale else None
        T = len(self.thresholds)
        paths.append(os.path.join(directory, "instances.jsonl"))
        with open(paths[-1], "w") as f:
            for d, doc in enumerate(doc_ids):
                n = int(nw[d])
                soft = [float(v) for v in scores[d][:n]]
                if doc_lengths is not None:
                    soft = (soft + [0.0] * max(0, int(doc_lengths[d]) - n))[:int(doc_lengths[d])]
                m = int(n_rat[d, self.hard_index]) if n_rat is not None else min(n, max(1, math.ceil(0.1 * n))) if n else 0
                inst = {"annotation_id": doc,
                        "rationales": [{"docid": doc, "soft_rationale_predictions": soft,
                                        "hard_rationale_predictions": [{"start_token": int(w), "end_token": int(w) + 1}
                                                                       for w in order[d][:m]]}]}
                if probs is not None:
                    names = list(class_names) if class_names is not None else (
                        ["NEG", "POS"] if probs.shape[2] == 2 else [str(c) for c in range(probs.shape[2])])
                    dist = lambda row: {names[c]: float(row[c]) for c in range(len(names))}       # noqa: E731
                    inst["classification"] = names[int(probs[d, 0].argmax())]
                    inst["classification_scores"] = dist(probs[d, 0])
                    inst["comprehensiveness_classification_scores"] = dist(probs[d, 1 + self.hard_index])
                    inst["sufficiency_classification_scores"] = dist(probs[d, 1 + T + self.hard_index])
                    inst["thresholded_scores"] = [{"threshold": t, "comprehensiveness_classification_scores": dist(probs[d, 1 + i]),
                                                   "sufficiency_classification_scores": dist(probs[d, 1 + T + i])}
                                                  for i, t in enumerate(self.thresholds)]
                f.write(json.dumps(inst) + "\n")
        return paths
