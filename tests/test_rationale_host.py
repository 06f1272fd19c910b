"""Host-side checks of the rationale test (no GPU needed): te_rationale_metrics_workspace_bytes / te_rationale_metrics_f32 /
te_token_erase are declared, exported and bound and their limits answer before any device call; ops refuses what has no
kernel with a TeError; the torch functions of rationale.py -- the CPU path, and the yardstick of tests/test_gpu_rationale.py
-- reproduce the reference's own results in tests/golden/rationale.npz: integers and per-document P / R / F1 exactly.

Soft scores (AP, AUPRC, ROC-AUC).  ``kernel_order_soft`` below restates the kernel's summation in numpy: thread t adds the runs
t and t + 1024, a shfl_down tree over the 64 lanes of a wave, then the 16 waves in sequence.  Over the input classes of the
GPU test (``make_case``: random / zero-clamped / heavily tied scores, N in {64, 512, 2048}, word ids with gaps; 40 seeds each)
its largest difference from scikit-learn 1.7.2 measured on the CPU is 2.22e-16 (one ulp of a score in [0.5, 1)); SOFT_BAR is
four times that, 8.9e-16 (the margin covers fp64 contraction on the device).  The torch function ``soft_scores`` is held to the same bar."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from host_util import header_args, lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rationale.npz")
NEW_SYMBOLS = ["te_rationale_metrics_workspace_bytes", "te_rationale_metrics_f32", "te_token_erase"]
SOFT_MEASURED = 2.22e-16
SOFT_BAR = 4 * SOFT_MEASURED
KINDS = ["random", "clamped", "tied"]


def rt():
    from transformer_explainability_amd import rationale
    return rationale


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ shared with the GPU test
def make_case(kind, B, N, seed):
    """(scores fp32 [B,N], word_ids int32 [B,N], truth bool [B,N]) on the CPU: [CLS], words of 1-3 wordpieces, [SEP], padding;
    every eleventh word id is skipped (a word without a wordpiece); 'clamped' scores are about half negative (they tie at 0
    under clamp=True), 'tied' scores take nine levels."""
    g = torch.Generator().manual_seed(seed)
    scores = torch.randn((B, N), generator=g)
    if kind == "tied":
        scores = (scores * 2).round().clamp(-2, 2) / 2
    elif kind not in ("random", "clamped"):
        raise ValueError(kind)
    word_ids = torch.full((B, N), -1, dtype=torch.int32)
    for b in range(B):
        length = int(torch.randint(max(3, N // 2), N + 1, (1,), generator=g))
        pieces = torch.randint(1, 4, (N,), generator=g).tolist()
        i, w = 1, 0
        while i < length - 1:
            n = min(pieces[w % N], length - 1 - i)
            word_ids[b, i:i + n] = w
            i += n
            w += 2 if w % 11 == 10 else 1
    truth = torch.rand((B, N), generator=g) < 0.2
    return scores.float(), word_ids, truth


def kernel_order_soft(ws, n_words, truth):
    """numpy restatement of the kernel's soft scores IN ITS SUMMATION ORDER, one document: ws [W] fp32, truth [W] ->
    (AP, AUPRC, ROC-AUC, npos)."""
    nw = int(n_words)
    s, t = np.asarray(ws[:nw], np.float32) + np.float32(0), np.asarray(truth[:nw]) != 0
    order = np.lexsort((np.arange(nw), -s.astype(np.float64)))             # descending score, ascending index
    s, t = s[order], t[order]
    tp_at = np.cumsum(t)
    npos = int(tp_at[-1]) if nw else 0
    if npos == 0 or npos == nw:
        return 0.0, 0.0, 0.0, float(npos)
    end = np.ones(nw, bool)
    end[:-1] = s[1:] != s[:-1]
    n = (np.nonzero(end)[0] + 1).astype(np.int64)
    tp = tp_at[end].astype(np.int64)
    n_prev, tp_prev = np.concatenate([[0], n[:-1]]), np.concatenate([[0], tp[:-1]])
    dpos, dneg = np.float64(npos), np.float64(nw - npos)
    P, R, F = tp / n.astype(np.float64), tp / dpos, (n - tp) / dneg
    Pp = np.where(n_prev > 0, tp_prev / np.maximum(n_prev, 1).astype(np.float64), 1.0)
    Rp, Fp = tp_prev / dpos, (n_prev - tp_prev) / dneg
    terms = np.stack([(R - Rp) * P, (R - Rp) * ((P + Pp) / 2.0), (F - Fp) * ((R + Rp) / 2.0)], 1)
    acc = np.zeros((1024, 3))
    for k in range(len(n)):                                                 # thread k % 1024: run k, then run k + 1024
        acc[k % 1024] += terms[k]
    lanes = acc.reshape(16, 64, 3).copy()
    for off in (32, 16, 8, 4, 2, 1):                                        # te_wave_sum: v[l] += v[l + off]
        lanes[:, :64 - off] = lanes[:, :64 - off] + lanes[:, off:]
    total = np.zeros(3)
    for w in range(16):
        total = total + lanes[w, 0]
    return float(total[0]), float(total[1]), float(total[2]), float(npos)


def sklearn_soft(ws, n_words, truth):
    from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_auc_score
    nw = int(n_words)
    s, t = np.asarray(ws[:nw], np.float64), (np.asarray(truth[:nw]) != 0).astype(int)
    precision, recall, _ = precision_recall_curve(t, s)
    return average_precision_score(t, s), auc(recall, precision), roc_auc_score(t, s)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_declared_exported_bound(lib):
    from transformer_explainability_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == header_args(name), name
    assert header_args("te_rationale_metrics_f32") == 17 and header_args("te_token_erase") == 15
    header = open(os.path.join(ROOT, "include", "te_relprop.h")).read()
    assert "#define TE_RATIONALE_MAX_KS 16" in header and "#define TE_TOKEN_ERASE_MAX_FRACTIONS 8" in header
    assert _lib.TE_RATIONALE_MAX_KS == 16 and _lib.TE_TOKEN_ERASE_MAX_FRACTIONS == 8 and _lib.TE_RATIONALE_CLAMP == 1
    build = open(os.path.join(ROOT, "transformer-explainability_amd", "build.py")).read()
    assert '"te_rationale.hip"' in build


def test_header_comment_states_the_semantics():
    header = open(os.path.join(ROOT, "include", "te_relprop.h")).read()
    block = header[header.index("rationale test of a BERT relevance vector"):header.index("int te_token_erase")]
    for cite in ("bert_pipeline.py:547-582", "metrics.py:168-215", "ASCENDING WORD INDEX", "min(k, n_words)", "NaN rule",
                 "NO PRODUCER", "this project's", "ceil(t * n_words)"):
        assert cite in block, cite


def test_workspace_query(lib):
    q = lib.te_rationale_metrics_workspace_bytes
    for bad in ((0, 512, 512), (-1, 512, 512), (4, 0, 512), (4, 512, 0), (4, -3, 512), (4, 2049, 512), (4, 512, 2049),
                (65536, 512, 512)):
        assert q(*bad) == 0, bad
    sizes = [q(B, 512, 512) for B in (1, 2, 8, 64, 65535)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert q(1, 1, 1) > 0 and q(3, 2048, 2048) > 0


def test_rationale_metrics_validates_on_the_host(lib):
    """Every refusal below comes before any HIP call (the pointers are never dereferenced; this host has no device)."""
    f = lib.te_rationale_metrics_f32
    p = ctypes.c_void_p(256)
    B, N, W = 2, 64, 64
    ks = (ctypes.c_int64 * 16)(*range(5, 85, 5))
    ws = lib.te_rationale_metrics_workspace_bytes(B, N, W)
    assert ws > 0
    ok = [p, p, p, p, p, p, p, p, B, N, W, ks, 16, 1, p, ws, None]
    for i in list(range(8)) + [11]:                      # a null pointer
        args = list(ok)
        args[i] = None
        assert f(*args) == -1, i
    for i in (8, 9, 10, 12):                             # non-positive sizes, n_ks = 0
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert f(*args) == -1, (i, v)
    args = list(ok)
    args[12] = 17                                        # ks holds 16 entries, none is read
    assert f(*args) == -1
    for bad_k in (0, -5):
        args = list(ok)
        args[11] = (ctypes.c_int64 * 16)(*([5] * 15 + [bad_k]))
        assert f(*args) == -1, bad_k
    args = list(ok)
    args[13] = 2                                         # an unknown flag bit
    assert f(*args) == -1
    big = 1 << 40
    for i, v in ((9, 2049), (10, 2049), (8, 65536), (9, 1 << 40)):
        args = list(ok)
        args[i], args[15] = v, big
        assert f(*args) == -3, (i, v)
    for short in (ws - 1, 0):
        args = list(ok)
        args[15] = short
        assert f(*args) == -2
    args = list(ok)
    args[14] = None
    assert f(*args) == -2


def test_token_erase_validates_on_the_host(lib):
    f = lib.te_token_erase
    p = ctypes.c_void_p(256)
    fr = (ctypes.c_double * 8)(0.01, 0.05, 0.1, 0.2, 0.5, 0.6, 0.7, 1.0)
    ok = [p, p, p, p, p, p, p, p, 2, 64, 64, fr, 5, 0, None]
    for i in list(range(8)) + [11]:
        args = list(ok)
        args[i] = None
        assert f(*args) == -1, i
    for i in (8, 9, 10, 12):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert f(*args) == -1, (i, v)
    args = list(ok)
    args[12] = 9
    assert f(*args) == -1
    for bad in (0.0, -0.1, 1.5, float("nan")):
        args = list(ok)
        args[11] = (ctypes.c_double * 8)(0.1, bad, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1)
        assert f(*args) == -1, bad
    for i, v in ((9, 2049), (10, 2049), (8, 65536)):
        args = list(ok)
        args[i] = v
        assert f(*args) == -3, (i, v)


def test_ops_refuse_cpu_tensors_and_wrong_dtypes():
    from transformer_explainability_amd import ops, TeError
    scores, word_ids, truth = make_case("random", 2, 64, 1)
    with pytest.raises(TeError, match="CPU"):
        ops.rationale_metrics(scores, word_ids, truth, [5, 10])
    with pytest.raises(TeError, match="float32"):
        ops.rationale_metrics(scores.double(), word_ids, truth, [5])
    with pytest.raises(TeError, match="integer word ids"):
        ops.rationale_metrics(scores, word_ids.float(), truth, [5])
    with pytest.raises(TeError, match="truth"):
        ops.rationale_metrics(scores, word_ids, truth.float(), [5])
    ids = torch.zeros(2, 64, dtype=torch.long)
    order, n_words = torch.zeros(2, 64, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TeError, match="CPU"):
        ops.token_erase(ids, torch.ones_like(ids), word_ids, order, n_words, [0.1])
    with pytest.raises(TeError, match="integer"):
        ops.token_erase(ids.float(), torch.ones_like(ids), word_ids, order, n_words, [0.1])
    with pytest.raises(TeError, match="integer"):
        ops.token_erase(ids, torch.ones_like(ids), word_ids, order.float(), n_words, [0.1])


# ------------------------------------------------------------------------------------------------ the golden documents
def golden_documents(g):
    """(word_ids int32 [D,N] from word_ids_from_wordpieces, truth bool [D,Wmax] over the scored words, truth_total [D])"""
    r = rt()
    D, N = g["input_ids"].shape
    Wmax = g["ref_word_scores"].shape[1]
    wid = np.full((D, N), -1, np.int32)
    for d in range(D):
        words = [str(g["vocab"][i]) for i in g["doc_words"][d] if i >= 0]
        pieces = [str(g["pieces"][i]) for i in g["input_ids"][d]]
        wid[d] = r.word_ids_from_wordpieces(words, pieces)
    truth = torch.from_numpy(g["truth_full"][:, :Wmax].astype(bool))
    truth = truth & (torch.arange(Wmax).unsqueeze(0) < torch.from_numpy(g["ref_n_words"]).unsqueeze(1))
    return torch.from_numpy(wid), truth, torch.from_numpy(g["truth_full"].astype(np.int64).sum(1))


def test_word_ids_reproduce_the_references_pooled_scores(golden):
    r = rt()
    wid, truth, _ = golden_documents(golden)
    ws, nw = r.word_scores(torch.from_numpy(golden["scores"]), wid, truth.shape[1], clamp=True)
    assert torch.equal(nw, torch.from_numpy(golden["ref_n_words"]))
    assert torch.equal(ws, torch.from_numpy(golden["ref_word_scores"]))
    assert (wid[:, 0] == -1).all() and int(wid.max()) + 1 == int(nw.max())
    assert (golden["ref_n_words"] < (golden["doc_words"] >= 0).sum(1)).any()          # some documents are truncated


def test_hard_rationales_against_the_reference(golden):
    """Integers and the per-document / micro P, R, F1 are exact.  The macro averages are sums of the per-document values: the
    reference adds them in the iteration order of a set of string tuples, which changes from process to process, so they
    are compared within D ulp of 1 (D = 32 documents, values in [0, 1])."""
    r = rt()
    wid, truth, truth_total = golden_documents(golden)
    ks = [int(k) for k in golden["ks"]]
    ws, nw = r.word_scores(torch.from_numpy(golden["scores"]), wid, truth.shape[1], clamp=True)
    order, counts = r.topk_counts(ws, nw, truth, ks)
    assert order.dtype == torch.int32 and counts.dtype == torch.int32 and counts.shape == (32, 16, 2)
    assert torch.equal(counts[:, :, 0].long(), torch.from_numpy(golden["hard_tp"]))
    assert torch.equal(counts[:, :, 1].long(), torch.tensor(ks).expand(32, 16))
    D = counts.shape[0]
    for i, k in enumerate(ks):
        for d in range(D):
            one = r.hard_scores([counts[d, i, 0]], [counts[d, i, 1]], [truth_total[d]])["instance_micro"]
            assert [one["p"], one["r"], one["f1"]] == list(golden["hard_doc"][d, i]), (k, d)
        both = r.hard_scores(counts[:, i, 0], counts[:, i, 1], truth_total)
        assert [both["instance_micro"][c] for c in ("p", "r", "f1")] == list(golden["hard_micro"][i]), k
        macro = np.array([both["instance_macro"][c] for c in ("p", "r", "f1")])
        assert np.abs(macro - golden["hard_macro"][i]).max() <= D * np.finfo(np.float64).eps, k


def test_soft_scores_against_the_reference(golden):
    r = rt()
    wid, truth, _ = golden_documents(golden)
    ws, nw = r.word_scores(torch.from_numpy(golden["scores"]), wid, truth.shape[1], clamp=True)
    soft = r.soft_scores(ws, nw, truth).numpy()
    ref = golden["soft_doc"]                                                           # auprc, ap, roc per document
    err = np.abs(soft[:, [1, 0, 2]] - ref).max()
    ko = np.array([kernel_order_soft(ws[d].numpy(), nw[d], truth[d].numpy()) for d in range(32)])
    err_ko = np.abs(ko[:, [1, 0, 2]] - ref).max()
    print(f"golden: max|soft_scores - ref| {err:.3e}  max|kernel order - ref| {err_ko:.3e}")
    assert err <= SOFT_BAR and err_ko <= SOFT_BAR
    assert np.array_equal(soft[:, 3], truth.sum(1).numpy())
    ev = r.RationaleEvaluator(explain=None)
    ev.update_from_scores(torch.from_numpy(golden["scores"]), wid, truth)
    s = ev.summary()
    got = np.array([s["auprc"], s["average_precision"], s["roc_auc_score"]])
    assert np.abs(got - golden["soft_all"]).max() <= SOFT_BAR


@pytest.mark.parametrize("kind", KINDS)
def test_soft_scores_against_sklearn(kind):
    pytest.importorskip("sklearn")
    r = rt()
    worst = worst_ko = 0.0
    for N, B in ((64, 6), (512, 4), (2048, 2)):
        scores, wid, truth = make_case(kind, B, N, seed=100 + N)
        for clamp in (True, False):
            ws, nw = r.word_scores(scores, wid, N, clamp=clamp)
            soft = r.soft_scores(ws, nw, truth).numpy()
            for b in range(B):
                ref = np.array(sklearn_soft(ws[b].numpy(), nw[b], truth[b].numpy()))
                worst = max(worst, np.abs(soft[b, :3] - ref).max())
                ko = np.array(kernel_order_soft(ws[b].numpy(), nw[b], truth[b].numpy()))
                worst_ko = max(worst_ko, np.abs(ko[:3] - ref).max())
                assert ko[3] == soft[b, 3]
    print(f"{kind}: max|soft_scores - sklearn| {worst:.3e}  max|kernel order - sklearn| {worst_ko:.3e}")
    assert worst <= SOFT_BAR and worst_ko <= SOFT_BAR


def test_tie_rule_k_beyond_n_words_single_class_and_nan():
    r = rt()
    nan = float("nan")
    #            CLS  w0   w0   w1   w2   w3   w3   w4   SEP  PAD
    scores = torch.tensor([[9.0, 0.5, -1.0, 0.5, nan, 0.25, 0.5, -3.0, 9.0, 9.0]])
    wid = torch.tensor([[-1, 0, 0, 1, 2, 3, 3, 4, -1, -1]], dtype=torch.int32)
    truth = torch.tensor([[0, 1, 0, 1, 0, 0, 0, 0]], dtype=torch.bool)
    ws, nw = r.word_scores(scores, wid, 8, clamp=True)
    assert ws.tolist() == [[0.5, 0.5, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0]] and nw.tolist() == [5]     # NaN counts as 0
    order, counts = r.topk_counts(ws, nw, truth, [1, 2, 3, 4, 5, 80])
    assert order.tolist() == [[0, 1, 3, 2, 4, -1, -1, -1]]                 # ties in ascending word index
    assert counts.tolist() == [[[0, 1], [1, 2], [2, 3], [2, 4], [2, 5], [2, 5]]]               # k = 80 > n_words: clipped
    ws2, _ = r.word_scores(scores, wid, 8, clamp=False)
    assert ws2.tolist() == [[0.5, 0.5, 0.0, 0.5, -3.0, 0.0, 0.0, 0.0]]
    soft = r.soft_scores(ws, nw, truth)
    assert soft[0, 3] == 2.0 and 0.0 < float(soft[0, 0]) <= 1.0
    for one_class in (torch.zeros(1, 8, dtype=torch.bool), torch.tensor([[1, 1, 1, 1, 1, 0, 0, 0]], dtype=torch.bool)):
        soft = r.soft_scores(ws, nw, one_class)
        assert soft[0, :3].tolist() == [0.0, 0.0, 0.0] and float(soft[0, 3]) in (0.0, 5.0)
    ev = r.RationaleEvaluator(explain=None, ks=[2])
    ev.update_from_scores(scores, wid, torch.zeros(1, 8, dtype=torch.bool))
    s = ev.summary()                                                        # the only document is discarded
    assert s["auprc"] == 0.0 and s["hard"][2]["instance_micro"] == {"p": 0.0, "r": 0, "f1": 0}
    empty = r.word_scores(scores, torch.full_like(wid, -1), 8)              # a document without words
    assert empty[1].tolist() == [0] and r.topk_counts(empty[0], empty[1], truth, [5])[1].tolist() == [[[0, 0]]]


def test_word_ids_from_wordpieces_raises_where_the_reference_asserts():
    r = rt()
    words = ["unbelievable", "film", "!"]
    pieces = ["[CLS]", "un", "##believ", "##able", "film", "!", "[SEP]", "[PAD]"]
    assert r.word_ids_from_wordpieces(words, pieces) == [-1, 0, 0, 0, 1, 2, -1, -1]
    assert r.word_ids_from_wordpieces(words, pieces[:4] + ["fi", "[SEP]"]) == [-1, 0, 0, 0, 1, -1]    # truncated in a word
    assert r.word_ids_from_wordpieces(words[:1], pieces) == [-1, 0, 0, 0, -1, -1, -1, -1]             # wordpieces past the words
    with pytest.raises(ValueError, match="straddles"):
        r.word_ids_from_wordpieces(words, ["[CLS]", "un", "##believ", "##ablefi", "lm", "!", "[SEP]"])
    with pytest.raises(ValueError, match="spell"):
        r.word_ids_from_wordpieces(words, ["[CLS]", "un", "##believ", "##abel", "film", "!", "[SEP]"])
    with pytest.raises(ValueError):                                         # [UNK] hides a word's characters
        r.word_ids_from_wordpieces(["a", "xyz", "film", "!"], ["[CLS]", "a", "[UNK]", "film", "!", "[SEP]"])


def test_token_erase_torch_definition():
    r = rt()
    ids = torch.tensor([[101, 11, 12, 13, 100, 14, 15, 102, 0, 0],
                        [101, 21, 22, 23, 24, 25, 26, 27, 28, 102]])
    mask = (ids != 0).long()
    wid = torch.tensor([[-1, 0, 0, 1, -1, 2, 3, -1, -1, -1],
                        [-1, 0, 1, 1, 2, 3, 4, 5, 5, -1]], dtype=torch.int32)
    order = torch.tensor([[1, 3, 0, 2, -1, -1], [5, 4, 3, 2, 1, 0]], dtype=torch.int32)
    nw = torch.tensor([4, 6], dtype=torch.int32)
    ids_out, mask_out, m = r.token_erase_torch(ids, mask, wid, order, nw, [0.01, 0.5, 1.0], pad_id=0)
    assert m.tolist() == [[1, 1], [2, 3], [4, 6]] and ids_out.shape == (2, 3, 2, 10) and ids_out.dtype == torch.int64
    assert ids_out[0, 0, 0].tolist() == [101, 11, 12, 100, 14, 15, 102, 0, 0, 0]       # word 1 dropped
    assert ids_out[1, 0, 0].tolist() == [101, 13, 100, 102, 0, 0, 0, 0, 0, 0]          # only word 1 ([UNK] stays)
    assert ids_out[0, 1, 0].tolist() == [101, 11, 12, 100, 14, 102, 0, 0, 0, 0]        # words 1, 3 dropped
    assert ids_out[0, 2, 0].tolist() == [101, 100, 102, 0, 0, 0, 0, 0, 0, 0]           # the whole text is the rationale
    assert ids_out[1, 2, 0].tolist() == ids[0].tolist() and mask_out[1, 2, 0].tolist() == mask[0].tolist()
    assert ids_out[0, 1, 1].tolist() == [101, 21, 22, 23, 24, 102, 0, 0, 0, 0]         # words 5, 4, 3 dropped
    assert ids_out[1, 1, 1].tolist() == [101, 25, 26, 27, 28, 102, 0, 0, 0, 0]
    assert torch.equal(mask_out, (torch.arange(10) < mask_out.sum(-1, keepdim=True)).long())
    assert torch.equal(r.rationale_sizes(torch.tensor([0, 1, 81, 300]), [0.01, 0.05]),
                       torch.tensor([[0, 1, 1, 3], [0, 1, 5, 15]], dtype=torch.int32))


def test_aopc_against_the_reference(golden):
    r = rt()
    T = len(golden["thresholds"])
    comp, suff = r.aopc_scores(golden["probs"], T)
    assert float(np.average(comp)) == float(golden["aopc_comp"]) and float(np.average(suff)) == float(golden["aopc_suff"])
    assert np.average(comp, axis=0).tolist() == golden["aopc_comp_points"].tolist()
    assert np.average(suff, axis=0).tolist() == golden["aopc_suff_points"].tolist()
    h = list(golden["thresholds"]).index(0.1)
    assert float(np.average(comp[:, h])) == float(golden["comp"]) and float(np.average(suff[:, h])) == float(golden["suff"])


class ToyClassifier(torch.nn.Module):
    """logits from the bag of the unmasked ids: changes whenever a token is erased"""

    def __init__(self, vocab=8192, classes=2):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.table = torch.nn.Parameter(torch.randn((vocab, classes), generator=g) * 0.3)

    def forward(self, input_ids, attention_mask):
        return ((self.table[input_ids % self.table.shape[0]] * attention_mask.unsqueeze(-1)).sum(1),)


def test_evaluator_cpu_path_and_write_results_round_trip(golden, tmp_path):
    r = rt()
    wid, truth, truth_total = golden_documents(golden)
    ids, mask = torch.from_numpy(golden["input_ids"]), torch.from_numpy(golden["attention_mask"])
    scores = torch.from_numpy(golden["scores"])
    ev = r.RationaleEvaluator(lambda i, m, x: scores[:16] if i.shape[0] == 16 and bool((i == ids[:16]).all()) else scores[16:],
                              classifier=ToyClassifier().eval(), max_forward_batch=50)
    out = ev.update(ids[:16], mask[:16], wid[:16], truth[:16], truth_total[:16])
    ev.update(ids[16:], mask[16:], wid[16:], truth[16:], truth_total[16:])
    assert out["erased_ids"].shape == (2, 5, 16, 512) and out["probs"].shape == (16, 11, 2)
    assert torch.equal(out["n_rationale"], r.rationale_sizes(out["n_words"], r.THRESHOLDS))
    s = ev.summary()
    for i, k in enumerate(golden["ks"]):                                   # the hard scores are the reference's
        assert [s["hard"][int(k)]["instance_micro"][c] for c in ("p", "r", "f1")] == list(golden["hard_micro"][i])
    assert s["aopc_thresholds"] == list(r.THRESHOLDS) and len(s["comprehensiveness_aopc_points"]) == 5
    # erasing everything but the rationale / the rationale changes the prediction: both numbers are nonzero here
    assert s["comprehensiveness_aopc"] != 0.0 and s["sufficiency_aopc"] != 0.0

    doc_ids = [f"doc{d}" for d in range(32)]
    lengths = (golden["doc_words"] >= 0).sum(1)
    paths = ev.write_results(str(tmp_path), doc_ids, doc_lengths=lengths)
    assert [os.path.basename(p) for p in paths] == [f"identifier_results_{k}.json" for k in golden["ks"]] + ["instances.jsonl"]
    for i, k in enumerate(golden["ks"]):                                   # bert_pipeline.py:575-582
        rows = [json.loads(line) for line in open(paths[i])]
        assert len(rows) == 32
        for d, row in enumerate(rows):
            assert row["annotation_id"] == doc_ids[d] and row["rationales"][0]["docid"] == doc_ids[d]
            spans = row["rationales"][0]["hard_rationale_predictions"]
            assert len(spans) == k and all(sp["end_token"] == sp["start_token"] + 1 for sp in spans)
            tp = sum(int(golden["truth_full"][d, sp["start_token"]]) for sp in spans)
            assert tp == golden["hard_tp"][d, i]
    inst = [json.loads(line) for line in open(paths[-1])]
    probs = np.array([[[row["classification_scores"][c] for c in ("NEG", "POS")]]
                      + [[t["comprehensiveness_classification_scores"][c] for c in ("NEG", "POS")] for t in row["thresholded_scores"]]
                      + [[t["sufficiency_classification_scores"][c] for c in ("NEG", "POS")] for t in row["thresholded_scores"]]
                      for row in inst])
    comp, suff = r.aopc_scores(probs, 5)                                   # what metrics.py would compute from the file
    assert float(np.average(comp)) == s["comprehensiveness_aopc"] and float(np.average(suff)) == s["sufficiency_aopc"]
    for d, row in enumerate(inst):
        assert [t["threshold"] for t in row["thresholded_scores"]] == list(r.THRESHOLDS)
        assert row["classification"] == ("NEG", "POS")[int(np.argmax(probs[d, 0]))]
        assert row["comprehensiveness_classification_scores"] == row["thresholded_scores"][2]["comprehensiveness_classification_scores"]
        soft = row["rationales"][0]["soft_rationale_predictions"]
        assert len(soft) == lengths[d]
        assert np.array_equal(np.float32(soft[:golden["ref_n_words"][d]]), golden["ref_word_scores"][d, :golden["ref_n_words"][d]])
