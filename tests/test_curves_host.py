"""CPU: the deletion / insertion curves' definitions (curves.py restates include/te_relprop.h in torch) against scipy, sklearn
and the oracle's perturbation test; what every te_curve_* / te_blur_* / te_pixel_rank_* entry point refuses on the host, before
any HIP call; and CurveEvaluator on CPU tensors against a literal per-image loop."""
import os

import numpy as np
import pytest
import torch

from curves_inputs import MEAN, STD, Stub, images, relevance, tie_example
from host_util import lib, status  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def curves():
    from transformer_explainability_amd import curves
    return curves


# ------------------------------------------------------------------------------------------------ the definitions
@pytest.mark.parametrize("klen,nsig", [(11, 5), (3, 0.8), (31, 5), (1, 2)])
def test_taps_are_scipys(klen, nsig):
    ndimage = pytest.importorskip("scipy.ndimage")
    taps = curves().gaussian_taps(klen, nsig)
    assert taps.dtype == np.float64 and taps.shape == (klen,)
    delta = np.zeros(klen)
    delta[klen // 2] = 1.0
    assert np.abs(taps - ndimage.gaussian_filter1d(delta, nsig)).max() <= 1e-15
    delta2 = np.zeros((klen, klen))
    delta2[klen // 2, klen // 2] = 1.0
    assert np.abs(np.outer(taps, taps) - ndimage.gaussian_filter(delta2, nsig)).max() <= 1e-15      # RISE's gkern


@pytest.mark.parametrize("klen,nsig", [(11, 5), (3, 0.8), (31, 5), (1, 2)])
def test_taps_sum_to_one_and_are_symmetric(klen, nsig):
    taps = curves().gaussian_taps(klen, nsig)
    assert abs(taps.sum() - 1.0) <= 1e-15
    # (mirror positions fold the same weights in another order: equal to the rounding of at most 2 R + 1 additions)
    assert np.abs(taps - taps[::-1]).max() <= 4 * 2.0 ** -53
    assert (taps > 0).all()
    with pytest.raises(ValueError):
        curves().gaussian_taps(klen + 1, nsig)


def test_reference_ranks_on_ties_zeros_and_infinities():
    vis = tie_example()
    ranks = curves().reference_ranks(vis)
    assert ranks.dtype == torch.int32 and ranks.shape == vis.shape
    n = vis.shape[1]
    for b in range(vis.shape[0]):
        assert sorted(ranks[b].tolist()) == list(range(n))                       # a permutation
        by_rank = torch.empty(n)
        by_rank[ranks[b].long()] = vis[b]
        assert bool((by_rank[1:] <= by_rank[:-1]).all()), by_rank                # non-increasing
    # equal values (and -0 == +0) in ascending pixel index
    row = ranks[0].tolist()
    assert row[4] == 0 and row[3] < row[9] and row[0] < row[5] < row[10]
    assert row[1] < row[2] < row[7] < row[11] and row[6] == n - 1
    assert ranks[1].tolist() == list(range(n - 1, -1, -1))


def test_reference_auc_is_sklearns():
    metrics = pytest.importorskip("sklearn.metrics")
    g = torch.Generator().manual_seed(3)
    for S in (1, 2, 17, 225):
        prob = torch.rand((S + 1, 4), generator=g, dtype=torch.float64)
        got = curves().reference_auc(prob)
        x = np.arange(S + 1) / S
        want = np.array([metrics.auc(x, prob[:, b].numpy()) for b in range(4)])
        assert np.abs(got.numpy() - want).max() <= (S + 2) * 2.0 ** -53 * np.abs(want).max() * 4


def test_reference_inputs_deletion_to_black_is_the_perturbation_test():
    """25 x 40 pixels, 100 per step: the images 1 .. 9 are the oracle's perturbation test at 100 .. 900 pixels, value for value."""
    from oracle import relprop_oracle as O
    c = curves()
    data, vis = images(2, 3, 25, 40), relevance(2, 1000)
    vis[0, 100:140] = vis[0, 7]                                                  # ties across a step boundary
    ranks = c.reference_ranks(vis)
    fill = c.substrate_fill("black", 3, MEAN, STD)
    got = c.reference_inputs(data, ranks, 100, 0, 11, "deletion", fill=fill, mean=MEAN, std=STD)
    want = O.perturb(vis, data, list(range(100, 1000, 100)), MEAN, STD)
    assert got.shape == (11, 2, 3, 25, 40) and got.dtype == torch.float32
    assert torch.equal(got[1:10], want)
    assert torch.equal(got[0], c.normalise(data, MEAN, STD))
    assert torch.equal(got[10], torch.tensor(fill).reshape(1, 3, 1, 1).expand(2, 3, 25, 40))
    # insertion is the complement; a chunk equals the slice of the whole
    ins = c.reference_inputs(data, ranks, 100, 0, 11, "insertion", fill=fill, mean=MEAN, std=STD)
    assert torch.equal(ins[0], got[10]) and torch.equal(ins[10], got[0])
    assert torch.equal(c.reference_inputs(data, ranks, 100, 3, 4, "insertion", fill=fill, mean=MEAN, std=STD), ins[3:7])
    bf = c.reference_inputs(data, ranks, 100, 0, 11, "deletion", fill=fill, mean=MEAN, std=STD, out_dtype=torch.bfloat16)
    assert torch.equal(bf, got.to(torch.bfloat16))


def test_reference_blur_of_an_impulse_is_the_kernel():
    c = curves()
    data = torch.zeros(1, 1, 15, 17)
    data[0, 0, 7, 8] = 1.0
    taps = c.gaussian_taps(11, 5).astype(np.float32).astype(np.float64)
    got = c.reference_blur(data, 11, 5)
    assert got.dtype == torch.float64
    assert np.abs(got[0, 0, 2:13, 3:14].numpy() - np.outer(taps, taps)).max() <= 1e-17


# ------------------------------------------------------------------------------------------------ refusals on the host
P = 4096      # a fake non-null, 16-byte-aligned address: every call below returns before the first HIP call


def test_entry_points_reject_on_the_host(lib):
    import ctypes
    from transformer_explainability_amd import _lib
    INVALID, WORKSPACE, UNSUPPORTED = _lib.TE_ERR_INVALID_ARG, _lib.TE_ERR_WORKSPACE, _lib.TE_ERR_UNSUPPORTED
    assert _lib.TE_BLUR_MAX_TAPS == 63 and lib.te_version() >= 702
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    taps = (ctypes.c_float * 63)(*([1.0 / 63] * 63))

    blur = dict(data=P, out=P, B=2, C=3, H=16, W=16, taps=taps, klen=11, mean=f3, std_=f3, stream=None)
    f = "te_blur_normalised_f32"
    assert tuple(blur) == _lib.PARAMS[f]
    assert [status(lib, f, blur, data=None), status(lib, f, blur, out=None), status(lib, f, blur, taps=None)] == [INVALID] * 3
    assert [status(lib, f, blur, klen=10), status(lib, f, blur, klen=0), status(lib, f, blur, B=0), status(lib, f, blur, W=0)] == [INVALID] * 4
    assert [status(lib, f, blur, klen=65), status(lib, f, blur, C=5), status(lib, f, blur, H=1025, W=1024)] == [UNSUPPORTED] * 3

    n = 1000
    ws_bytes = lib.te_pixel_rank_workspace_bytes(2, n)
    assert ws_bytes >= 2 * 2 * n * 8
    assert [lib.te_pixel_rank_workspace_bytes(*a) for a in ((0, n), (2, 0), (2, (1 << 20) + 1), (65536, n))] == [0] * 4
    assert lib.te_pixel_rank_workspace_bytes(1, 1 << 20) >= 2 * 8 << 20
    rank = dict(vis=P, rank=P, B=2, n=n, ws=P, ws_bytes=ws_bytes, stream=None)
    f = "te_pixel_rank_f32"
    assert tuple(rank) == _lib.PARAMS[f]
    assert [status(lib, f, rank, vis=None), status(lib, f, rank, rank=None), status(lib, f, rank, n=0)] == [INVALID] * 3
    assert [status(lib, f, rank, n=(1 << 20) + 1), status(lib, f, rank, B=65536)] == [UNSUPPORTED] * 2
    assert [status(lib, f, rank, ws=None), status(lib, f, rank, ws_bytes=ws_bytes - 256)] == [WORKSPACE] * 2

    for f in ("te_curve_inputs_f32", "te_curve_inputs_bf16"):
        inp = dict(data=P, substrate=P, fill=None, rank=P, out=P, B=2, C=3, HW=n, step=300, s0=0, n_s=5, insertion=0, mean=f3,
                   std_=f3, stream=None)                                         # S = 4: the images 0 .. 4
        assert tuple(inp) == _lib.PARAMS[f]
        assert [status(lib, f, inp, data=None), status(lib, f, inp, rank=None), status(lib, f, inp, out=None),
                status(lib, f, inp, substrate=None)] == [INVALID] * 4             # no substrate and no fill
        assert [status(lib, f, inp, step=0), status(lib, f, inp, step=-3), status(lib, f, inp, s0=-1), status(lib, f, inp, n_s=0),
                status(lib, f, inp, insertion=2)] == [INVALID] * 5
        assert [status(lib, f, inp, n_s=6), status(lib, f, inp, s0=1), status(lib, f, inp, s0=5, n_s=1)] == [INVALID] * 3
        assert [status(lib, f, inp, HW=(1 << 20) + 1), status(lib, f, inp, C=5), status(lib, f, inp, B=65536)] == [UNSUPPORTED] * 3

    tgt = P
    for f in ("te_curve_scores_f32", "te_curve_scores_bf16"):
        sc = dict(logits=P, target=tgt, prob=P, B=2, K=10, s0=0, n_s=3, stream=None)
        assert tuple(sc) == _lib.PARAMS[f]
        assert [status(lib, f, sc, logits=None), status(lib, f, sc, target=None), status(lib, f, sc, prob=None)] == [INVALID] * 3
        assert [status(lib, f, sc, K=0), status(lib, f, sc, B=0), status(lib, f, sc, s0=-1), status(lib, f, sc, n_s=0)] == [INVALID] * 4
        assert status(lib, f, sc, B=65536) == UNSUPPORTED

    auc = dict(prob=P, auc=P, S1=5, B=2, stream=None)
    f = "te_curve_auc_f64"
    assert tuple(auc) == _lib.PARAMS[f]
    assert [status(lib, f, auc, prob=None), status(lib, f, auc, auc=None), status(lib, f, auc, S1=1), status(lib, f, auc, B=0)] == [INVALID] * 4
    assert status(lib, f, auc, B=65536) == UNSUPPORTED


def test_ops_refuse_cpu_tensors_and_wrong_dtypes():
    from transformer_explainability_amd import TeError, ops
    data, vis = images(2, 3, 8, 8), relevance(2, 64)
    ranks = curves().reference_ranks(vis)
    prob = torch.zeros((5, 2), dtype=torch.float64)
    calls = [lambda: ops.gaussian_blur(data), lambda: ops.pixel_ranks(vis),
             lambda: ops.curve_inputs(data, ranks, 16, 0, 5, "deletion", fill=[0.0] * 3),
             lambda: ops.curve_scores(torch.zeros(10, 4), torch.zeros(2, dtype=torch.int64), prob, 0),
             lambda: ops.curve_auc(prob),
             lambda: ops.gaussian_blur(data.double()), lambda: ops.pixel_ranks(vis.half()),
             lambda: ops.curve_inputs(data, ranks.long(), 16, 0, 5, "deletion", fill=[0.0] * 3),
             lambda: ops.curve_scores(torch.zeros(10, 4).half(), torch.zeros(2, dtype=torch.int64), prob, 0),
             lambda: ops.curve_auc(prob.float())]
    for call in calls:
        with pytest.raises(TeError):
            call()


# ------------------------------------------------------------------------------------------------ the evaluator
def literal_curves(model, data, vis, target, step, mode, substrate, klen, nsig, dtype):
    """One image at a time, straight from the definitions: -> (scores [S+1,B], auc [B])"""
    c = curves()
    B, C, H, W = data.shape
    HW = H * W
    S = -(-HW // step)
    z = c.normalise(data, MEAN, STD)
    if substrate == "blur":
        sub = c.reference_blur(data, klen, nsig, MEAN, STD).float()
    else:
        sub = torch.tensor(c.substrate_fill(substrate, C, MEAN, STD)).reshape(1, C, 1, 1).expand(B, C, H, W)
    scores = torch.zeros((S + 1, B), dtype=torch.float64)
    for b in range(B):
        order = torch.sort(vis[b].reshape(-1), descending=True, stable=True).indices
        for i in range(S + 1):
            k = min(i * step, HW)
            start, finish = (z[b], sub[b]) if mode == "deletion" else (sub[b], z[b])
            x = start.clone().reshape(C, HW)
            x[:, order[:k]] = finish.reshape(C, HW)[:, order[:k]]
            logits = model(x.reshape(1, C, H, W).to(dtype)).double()
            scores[i, b] = torch.softmax(logits[0], -1)[target[b]]
    auc = torch.stack([torch.trapezoid(scores[:, b], dx=1.0 / S) for b in range(B)])
    return scores, auc


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_evaluator_on_cpu_tensors_equals_a_literal_loop(dtype):
    c = curves()
    B, H, W, step = 3, 16, 16, 37                                                # 256 = 6 * 37 + 34: the last step is short
    data, vis = images(B, 3, H, W, seed=1), relevance(B, H * W, seed=1).reshape(B, 1, H, W)
    vis[1, 0, 3] = vis[1, 0, 2]                                                  # a tied row of pixels
    target = torch.tensor([0, 2, 1])
    model = Stub(dtype)
    ev = c.CurveEvaluator(model, step=step, mean=MEAN, std=STD, max_forward_batch=7)      # chunks of 2 steps
    ev.update(data, vis, target)
    assert len(model.seen) == 2 * 4 and all(x.shape[0] <= 7 and x.dtype == dtype for x in model.seen)
    arrs = ev.arrays()
    assert sorted(arrs) == ["deletion_auc.npy", "deletion_scores.npy", "insertion_auc.npy", "insertion_scores.npy"]
    for mode, substrate in (("deletion", "zero"), ("insertion", "blur")):
        scores, auc = literal_curves(Stub(dtype), data, vis, target, step, mode, substrate, 11, 5.0, dtype)
        assert arrs[f"{mode}_scores.npy"].shape == (8, B) and arrs[f"{mode}_auc.npy"].shape == (B,)
        assert np.abs(arrs[f"{mode}_scores.npy"] - scores.numpy()).max() <= 16 * 2.0 ** -53
        assert np.abs(arrs[f"{mode}_auc.npy"] - auc.numpy()).max() <= 16 * 2.0 ** -53
    summary = ev.summary()
    assert summary == {m + "_auc": float(arrs[m + "_auc.npy"].mean()) for m in ("deletion", "insertion")}
    # a second batch is appended
    ev.update(data[:2], vis[:2], target[:2])
    again = ev.arrays()
    assert again["deletion_scores.npy"].shape == (8, 5) and again["insertion_auc.npy"].shape == (5,)
    assert np.array_equal(again["deletion_scores.npy"][:, 3:], arrs["deletion_scores.npy"][:, :2])


def test_evaluator_other_substrates_and_default_step():
    c = curves()
    data, vis, target = images(2, 3, 16, 16, seed=2), relevance(2, 256, seed=2), torch.tensor([1, 1])
    ev = c.CurveEvaluator(Stub(), modes=("deletion",), substrate={"deletion": "black"}, mean=MEAN, std=STD)
    ev.update(data, vis, target)
    assert ev.arrays()["deletion_scores.npy"].shape == (257, 2)                  # step = max(1, 256 // 224) = 1
    scores, _ = literal_curves(Stub(), data, vis, target, 1, "deletion", "black", 11, 5.0, torch.float32)
    assert np.abs(ev.arrays()["deletion_scores.npy"] - scores.numpy()).max() <= 16 * 2.0 ** -53
    with pytest.raises(ValueError):
        c.CurveEvaluator(Stub(), modes=("removal",))
    with pytest.raises(ValueError):
        c.CurveEvaluator(Stub(), klen=10)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
def test_evaluator_refuses_other_classifier_dtypes(dtype):
    from transformer_explainability_amd import TeError
    with pytest.raises(TeError):
        curves().CurveEvaluator(Stub(dtype))


def test_save_writes_the_four_files(tmp_path):
    c = curves()
    ev = c.CurveEvaluator(Stub(), step=50, mean=MEAN, std=STD)
    ev.update(images(3, 3, 16, 16), relevance(3, 256), torch.tensor([0, 1, 2]))
    ev.update(images(2, 3, 16, 16, seed=5), relevance(2, 256, seed=5), torch.tensor([2, 0]))
    arrs = ev.save(str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["deletion_auc.npy", "deletion_scores.npy", "insertion_auc.npy",
                                                     "insertion_scores.npy"]
    for mode in ("deletion", "insertion"):
        scores, auc = np.load(tmp_path / "out" / f"{mode}_scores.npy"), np.load(tmp_path / "out" / f"{mode}_auc.npy")
        assert scores.shape == (7, 5) and auc.shape == (5,) and scores.dtype == np.float64      # S = ceil(256 / 50) = 6
        assert np.array_equal(scores, arrs[f"{mode}_scores.npy"]) and np.array_equal(auc, arrs[f"{mode}_auc.npy"])
        assert ((scores > 0) & (scores < 1)).all()
