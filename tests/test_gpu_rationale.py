"""-m gpu: ops.rationale_metrics (te_rationale_metrics_f32) and ops.token_erase (te_token_erase) against the torch functions of
rationale.py applied to the same tensors ON THE CPU -- the yardstick of every case, never the kernel's own output -- and
against the reference's own results in tests/golden/rationale.npz.  word_scores, n_words, order, counts, npos and every erased
input must be exact.  The soft scores (AP, AUPRC, ROC-AUC) are held to SOFT_BAR = 8.9e-16: a numpy restatement of the kernel's
summation order differs from scikit-learn by at most 2.22e-16 over these input classes on the CPU
(tests/test_rationale_host.py says how that was measured), and the bar is four times that."""
import numpy as np
import pytest
import torch

from gpu_util import dev, record
from host_util import bits
from test_rationale_host import GOLDEN, KINDS, SOFT_BAR, golden_documents, kernel_order_soft, make_case

pytestmark = pytest.mark.gpu

KS = list(range(5, 85, 5))


def rt():
    from transformer_explainability_amd import rationale
    return rationale


def ops():
    from transformer_explainability_amd import ops as o
    return o


def restate(scores, word_ids, truth, ks, clamp=True):
    """The torch functions on CPU tensors: (word_scores, n_words, order, counts, soft)."""
    r = rt()
    assert not scores.is_cuda and not word_ids.is_cuda and not truth.is_cuda
    ws, nw = r.word_scores(scores, word_ids, truth.shape[1], clamp=clamp)
    order, counts = r.topk_counts(ws, nw, truth, ks)
    return ws, nw, order, counts, r.soft_scores(ws, nw, truth)


def run(scores, word_ids, truth, ks, clamp=True):
    d = dev()
    return ops().rationale_metrics(scores.to(d), word_ids.to(d), truth.to(d), ks, clamp=clamp)


def compare(name, got, ref):
    ws, nw, order, counts, soft = (t.cpu() for t in got)
    rws, rnw, rorder, rcounts, rsoft = ref
    assert ws.dtype == torch.float32 and nw.dtype == torch.int32 and order.dtype == torch.int32
    assert counts.dtype == torch.int32 and soft.dtype == torch.float64
    for a, b in ((ws, rws), (nw, rnw), (order, rorder), (counts, rcounts), (soft, rsoft)):
        assert a.shape == b.shape, name
    err = float((soft[:, :3] - rsoft[:, :3]).abs().max())
    print(f"{name}: max|soft - torch on the CPU| {err:.3e}")
    record(name, soft_max_abs=err, exact=bool(torch.equal(order, rorder) and torch.equal(counts, rcounts)))
    assert torch.equal(nw, rnw), name
    assert torch.equal(ws, rws), name
    assert torch.equal(order, rorder), name
    assert torch.equal(counts, rcounts), name
    assert torch.equal(soft[:, 3], rsoft[:, 3]), name
    assert torch.isfinite(soft).all() and err <= SOFT_BAR, (name, err)
    return soft


def test_golden_reference_results():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    wid, truth, _ = golden_documents(g)
    ks = [int(k) for k in g["ks"]]
    got = run(torch.from_numpy(g["scores"]), wid, truth, ks)
    ws, nw, order, counts, soft = (t.cpu() for t in got)
    assert torch.equal(nw, torch.from_numpy(g["ref_n_words"]))
    assert torch.equal(ws, torch.from_numpy(g["ref_word_scores"]))
    assert torch.equal(counts[:, :, 0].long(), torch.from_numpy(g["hard_tp"]))
    assert torch.equal(counts[:, :, 1].long(), torch.tensor(ks).expand(32, 16))
    err = float(np.abs(soft.numpy()[:, [1, 0, 2]] - g["soft_doc"]).max())
    print(f"golden: max|soft - ref| {err:.3e}")
    assert err <= SOFT_BAR
    compare("rationale_golden", got, restate(torch.from_numpy(g["scores"]), wid, truth, ks))


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("N,B", [(64, 6), (512, 4), (2048, 3)])
@pytest.mark.parametrize("kind", KINDS)
def test_against_torch_on_cpu(kind, N, B, clamp):
    scores, wid, truth = make_case(kind, B, N, seed=7 + N)
    ref = restate(scores, wid, truth, KS, clamp)
    soft = compare(f"rationale_{kind}_{N}_{'clamp' if clamp else 'raw'}", run(scores, wid, truth, KS, clamp), ref)
    for b in range(B):                           # the numpy restatement of the kernel's order: the same bits are expected
        ko = kernel_order_soft(ref[0][b].numpy(), ref[1][b], truth[b].numpy())
        assert max(abs(float(soft[b, j]) - ko[j]) for j in range(3)) <= SOFT_BAR


@pytest.mark.parametrize("kind", KINDS)
def test_two_thousand_words(kind):
    """One wordpiece per word: 2046 words in 2048 tokens, the longest sort, both halves of the ranks in use; and 1025 words."""
    scores, _, truth = make_case(kind, 3, 2048, seed=13)
    wid = (torch.arange(2048, dtype=torch.int32) - 1).repeat(3, 1)
    wid[:, -1] = -1
    wid[1, 1026:] = -1
    wid[2] = torch.flip(wid[2], [0])             # the word ids need not ascend along the text
    compare(f"rationale_{kind}_2046_words", run(scores, wid, truth, KS),
            restate(scores, wid, truth, KS))
    ks = [1, 64, 1023, 1024, 1025, 2045, 2046, 2047]
    compare(f"rationale_{kind}_2046_words_large_k", run(scores, wid, truth, ks, clamp=False),
            restate(scores, wid, truth, ks, clamp=False))


def test_word_ids_of_another_integer_dtype_and_a_narrow_truth():
    scores, wid, truth = make_case("tied", 3, 512, seed=3)
    wid = wid.clamp(max=199)                     # Wmax = 200 < N: everything beyond is folded into the last word
    truth = truth[:, :200].contiguous()
    compare("rationale_int64_ids", run(scores, wid.long(), truth.to(torch.uint8), [1, 7, 200, 4000]),
            restate(scores, wid, truth, [1, 7, 200, 4000]))
    wid[wid >= 150] = 900                        # ids >= Wmax are ignored
    compare("rationale_ids_beyond", run(scores, wid, truth, [5]), restate(scores, wid, truth, [5]))


def test_k_beyond_n_words_single_class_nan_and_empty_documents():
    scores, wid, truth = make_case("clamped", 5, 64, seed=9)
    scores[0, 3:9] = float("nan")
    truth[1] = False                             # single class: no positive
    truth[2] = True                              # single class: all positive
    wid[3] = -1                                  # a document without words
    scores[4] = -1.0                             # everything ties at 0 under the clamp
    got = run(scores, wid, truth, [1, 30, 64, 100])
    compare("rationale_edge_cases", got, restate(scores, wid, truth, [1, 30, 64, 100]))
    ws, nw, order, counts, soft = (t.cpu() for t in got)
    assert soft[1, :3].tolist() == [0, 0, 0] and soft[2, :3].tolist() == [0, 0, 0] and soft[1, 3] == 0
    assert int(nw[3]) == 0 and counts[3].tolist() == [[0, 0]] * 4 and (order[3] == -1).all() and (ws[3] == 0).all()
    n4 = int(nw[4])
    assert order[4, :n4].tolist() == list(range(n4)) and counts[4, 3, 1] == n4          # ascending index; k = 100 clipped


@pytest.fixture(scope="module")
def batch20():
    scores, wid, truth = make_case("clamped", 20, 512, seed=21)
    truth[5] = False
    wid[6] = -1
    d = dev()
    return scores.to(d), wid.to(d), truth.to(d)


def test_batch_equals_its_samples_bit_for_bit(batch20):
    scores, wid, truth = batch20
    first = ops().rationale_metrics(scores, wid, truth, KS)
    again = ops().rationale_metrics(scores, wid, truth, KS)
    for a, b in zip(first, again):
        assert torch.equal(bits(a), bits(b))
    for b in range(scores.shape[0]):
        alone = ops().rationale_metrics(scores[b:b + 1], wid[b:b + 1], truth[b:b + 1], KS)
        for whole, one in zip(first, alone):
            assert torch.equal(bits(whole[b:b + 1]), bits(one)), b
    compare("rationale_batch20", first, restate(scores.cpu(), wid.cpu(), truth.cpu(), KS))


def test_graph_capture_replays_bit_for_bit():
    """No host synchronisation inside the calls: a HIP graph captures both, and the replay is the eager call."""
    from transformer_explainability_amd.generators import GraphedCall
    d = dev()
    first = [t.to(d) for t in make_case("random", 4, 512, seed=31)]
    other = [t.to(d) for t in make_case("tied", 4, 512, seed=32)]
    ids = torch.randint(1000, 2000, (4, 512), generator=torch.Generator().manual_seed(5)).to(d)

    def both(scores, wid, truth):
        out = ops().rationale_metrics(scores, wid, truth, KS)
        mask = (wid >= 0).long()
        mask[:, 0] = 1
        return (*out, *ops().token_erase(ids, mask, wid, out[2], out[1], rt().THRESHOLDS, pad_id=0))

    graphed = GraphedCall(both, first)
    for inputs in (first, other, first):
        replay = [t.clone() for t in graphed(*inputs)]
        eager = both(*inputs)
        for a, b in zip(replay, eager):
            assert torch.equal(bits(a), bits(b))
    compare("rationale_graph_replay", replay[:5], restate(*(t.cpu() for t in first), KS))


def erase_case(B, N, seed):
    """ids, mask, word ids with [UNK]s (word id -1, mask 1) inside the text and padding behind it, on the CPU"""
    scores, wid, truth = make_case("clamped", B, N, seed)
    g = torch.Generator().manual_seed(seed + 1)
    ids = torch.randint(1000, 30000, (B, N), generator=g)
    last = (wid >= 0).long().cumsum(1).argmax(1)               # position of the last wordpiece
    mask = (torch.arange(N).unsqueeze(0) <= (last + 1).unsqueeze(1)).long()           # ... then [SEP], then padding
    unk = (torch.rand((B, N), generator=g) < 0.03) & (mask == 1)
    wid = torch.where(unk, torch.full_like(wid, -1), wid)
    ids = torch.where(unk, torch.full_like(ids, 100), ids)
    ids[:, 0] = 101
    ids[mask == 0] = 0
    return scores, wid, truth, ids, mask


@pytest.mark.parametrize("N,B", [(64, 5), (512, 4), (2048, 2)])
def test_token_erase_against_torch_on_cpu(N, B):
    r = rt()
    scores, wid, truth, ids, mask = erase_case(B, N, seed=40 + N)
    ws, nw, order, _, _ = restate(scores, wid, truth, [5])
    fractions = [0.01, 0.05, 0.1, 0.2, 0.5, 0.999, 1.0]       # 1.0: the rationale is the whole text
    ref = r.token_erase_torch(ids, mask, wid, order, nw, fractions, pad_id=7)
    d = dev()
    got = ops().token_erase(ids.to(d), mask.to(d), wid.to(d), order.to(d), nw.to(d), fractions, pad_id=7)
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b)
    whole = got[0][0, -1].cpu()                                # comprehensiveness at t = 1: only [CLS] / [UNK] / [SEP] are left
    assert all(set(whole[b][got[1][0, -1, b].cpu() == 1].tolist()) <= {100, 101, ids[b, int(mask[b].sum()) - 1].item()} for b in range(B))
    assert torch.equal(got[0][1, -1].cpu(), torch.where(mask == 1, ids, torch.full_like(ids, 7)))       # sufficiency at t = 1: the input
    # other integer dtypes, a bool mask
    again = ops().token_erase(ids.to(d).int(), mask.to(d).bool(), wid.to(d).long(), order.to(d).long(), nw.to(d).long(),
                              fractions, pad_id=7)
    for a, b in zip(again, got):
        assert torch.equal(a, b)


def small_bert():
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=30000, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                              intermediate_size=256, max_position_embeddings=64, num_labels=2)
    torch.manual_seed(11)
    model = bert.BertForSequenceClassification(cfg).eval()
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return model.to(dev())


def test_evaluator_kernels_against_torch_path_without_a_device_to_host_copy():
    """A seeded small BERT explains and classifies; kernels vs torch functions ON THE SAME CUDA TENSORS: identical erased
    inputs and hard summaries.  ``update`` runs under torch.cuda.set_sync_debug_mode("error"): any device-to-host copy or
    other synchronising call raises."""
    from transformer_explainability_amd.generators import Generator
    r = rt()
    d = dev()
    model = small_bert()
    gen = Generator(model)
    seen = []

    def explain(ids, mask, index):
        seen.append(gen.generate_LRP(ids, mask, index=index, start_layer=0).detach().clone())
        return seen[-1]

    _, wid, truth, ids, mask = (t.to(d) for t in erase_case(6, 64, seed=77))
    ks = [1, 5, 10, 40]
    warm = r.RationaleEvaluator(explain, ks=ks, classifier=model, max_forward_batch=32)
    warm.update(ids, mask, wid, truth)                          # lazy initialisation happens here, outside the check
    ev = r.RationaleEvaluator(explain, ks=ks, classifier=model, max_forward_batch=32)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ev.update(ids, mask, wid, truth)
        out2 = ev.update(ids[:3], mask[:3], wid[:3], truth[:3], truth_total=truth[:3].sum(1) + 2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.is_cuda for t in out.values()) and all(t.is_cuda for t in out2.values())
    assert all(t.is_cuda for part in (ev._counts, ev._soft, ev._probs, ev._truth_n) for t in part)

    ref = r.RationaleEvaluator(explain=None, ks=ks, classifier=model, max_forward_batch=32, device_path=False)
    a = ref.update_from_scores(seen[-2], wid, truth, None, ids, mask)
    ref.update_from_scores(seen[-1], wid[:3], truth[:3], truth[:3].sum(1) + 2, ids[:3], mask[:3])
    for key in ("word_scores", "n_words", "order", "counts", "truth_n", "erased_ids", "erased_mask", "n_rationale"):
        assert a[key].is_cuda and out[key].dtype == a[key].dtype and torch.equal(out[key], a[key]), key
    assert float((out["soft"] - a["soft"]).abs().max()) <= SOFT_BAR
    assert torch.equal(out["probs"], a["probs"])                # the same inputs through the same classifier
    s, t = ev.summary(), ref.summary()
    assert s["hard"] == t["hard"]
    for key in ("comprehensiveness", "sufficiency", "comprehensiveness_aopc", "sufficiency_aopc",
                "comprehensiveness_aopc_points", "sufficiency_aopc_points"):
        assert s[key] == t[key], key
    for key in ("auprc", "average_precision", "roc_auc_score"):
        assert abs(s[key] - t[key]) <= SOFT_BAR, key
    # and the torch functions on the CPU
    cpu = restate(seen[-2].cpu(), wid.cpu(), truth.cpu(), ks)
    compare("rationale_evaluator", [out[k] for k in ("word_scores", "n_words", "order", "counts", "soft")], cpu)
