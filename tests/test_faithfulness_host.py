"""CPU: the restatements of faithfulness.py (the subsets, the perturbed images, the weighted sums, the scores), the evaluator
on a stub whose numbers are known in closed form, and the host side of the new entry points: declared, bound, refused."""
import math
import os
import re

import numpy as np
import pytest
import torch

from faithfulness_inputs import BALANCE_CASES, BALANCE_IDS, BALANCE_SEEDS, LinearScore, images, inputs, token_maps
from host_util import lib, same_bits, status  # noqa: F401

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fb():
    from transformer_explainability_amd import faithfulness
    return faithfulness


# ------------------------------------------------------------------------------------------------ subsets
def test_subset_keys_follow_the_counter_layout():
    """cell c: word c & 3 of philox(0x80000000 | c >> 2, d, low32(id), high32(id); seed), the cell index in the low half"""
    F = fb()
    from transformer_explainability_amd.robustness import philox4x32
    seed, id0, d0 = 0x0123456789abcdef, (1 << 32) - 1, 7
    keys = F.subset_keys(2, 10, 3, seed, id0=id0, d0=d0)
    assert keys.shape == (2, 3, 10) and keys.dtype == np.uint64
    for b, j, c in ((0, 0, 0), (1, 2, 9), (1, 1, 5), (0, 2, 3)):
        sid = id0 + b
        w = philox4x32([0x80000000 | (c >> 2), d0 + j, sid & 0xffffffff, sid >> 32], [seed & 0xffffffff, seed >> 32])
        assert int(keys[b, j, c]) == (int(w[c & 3]) << 32) | c
    # apart from the noise stream: the same (group, draw, id, seed) without the top bit gives other words
    from transformer_explainability_amd.robustness import noise_words
    assert not np.array_equal(noise_words(1, 8, 1, seed).reshape(8), (F.subset_keys(1, 8, 1, seed)[0, 0] >> np.uint64(32)))


@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 15, 196, 4096])
def test_subsets_have_k_cells_and_chunk_and_batch_do_not_matter(G):
    F = fb()
    seed, id0 = 0x9e3779b97f4a7c15, (1 << 32) - 2                        # the ids cross 2^32: the high counter word is used
    for k in sorted({1, max(1, G // 4), max(1, G - 1), G}):
        full = F.reference_subsets(3, G, k, 4, seed, id0=id0)
        assert full.shape == (3, 4, G) and full.dtype == np.uint8 and set(np.unique(full)) <= {0, 1}
        assert (full.sum(2) == k).all()
        if k == G:
            assert full.all()
        # chunks of the draws are slices of the full call
        assert np.array_equal(F.reference_subsets(3, G, k, 2, seed, id0=id0, d0=0), full[:, :2])
        assert np.array_equal(F.reference_subsets(3, G, k, 1, seed, id0=id0, d0=3), full[:, 3:])
        # a batch at id0 equals its samples run alone at id0 + b
        for b in range(3):
            assert np.array_equal(F.reference_subsets(1, G, k, 4, seed, id0=id0 + b), full[b:b + 1]), b
    if G >= 15:
        full = F.reference_subsets(3, G, max(1, G // 4), 4, seed, id0=id0)
        assert not np.array_equal(full[0], full[1]) and not np.array_equal(full[:, 0], full[:, 1])
        # the high word of the id is part of the counter: id and id + 2^32 differ
        assert not np.array_equal(F.reference_subsets(1, G, max(1, G // 4), 4, seed, id0=5),
                                  F.reference_subsets(1, G, max(1, G // 4), 4, seed, id0=5 + (1 << 32)))
        assert not np.array_equal(F.reference_subsets(1, G, max(1, G // 4), 4, seed), F.reference_subsets(1, G, max(1, G // 4), 4, seed + 1))


def test_subsets_refuse():
    F = fb()
    for bad in (dict(k=0), dict(k=17), dict(G=4097), dict(n_draws=0), dict(d0=-1), dict(d0=(1 << 32) - 1, n_draws=2), dict(B=0)):
        args = dict(B=2, G=16, k=4, n_draws=2, seed=0)
        args.update(bad)
        with pytest.raises(ValueError):
            F.reference_subsets(**args)


@pytest.mark.parametrize("G,k,D", BALANCE_CASES)
def test_every_cell_is_chosen_about_equally_often(G, k, D):
    """Over D draws the inclusion count of a cell is a sum of D Bernoulli(k / G) variables: mean D k / G, variance
    D (k / G)(1 - k / G).  Every cell within 5 sigma, for every seed and id of the table; no draw has a tie among its 32-bit
    words (the index in the low half would break it, but the stream should not need that)."""
    F = fb()
    sigma = math.sqrt(D * (k / G) * (1 - k / G))
    worst = 0.0
    for seed in BALANCE_SEEDS:
        for sid in BALANCE_IDS:
            member = F.reference_subsets(1, G, k, D, seed, id0=sid)[0]
            assert (member.sum(1) == k).all()
            dev = np.abs(member.sum(0).astype(np.float64) - D * k / G).max() / sigma
            worst = max(worst, dev)
            words = np.sort(F.subset_keys(1, G, D, seed, id0=sid)[0] >> np.uint64(32), axis=1)
            assert (np.diff(words.astype(np.int64), axis=1) != 0).all()
    print(f"balance G {G} k {k} D {D}: worst deviation {worst:.2f} sigma")
    assert worst <= 5.0


# ------------------------------------------------------------------------------------------------ the perturbed images, the sums
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_reference_subset_inputs_switches_whole_cells(out_dtype):
    F = fb()
    x = images(2, 3, 6, 9, seed=1)
    sub = images(2, 3, 6, 9, seed=2)
    attr = token_maps(2, 6, seed=3)
    out, member, attr_sum = F.reference_subset_inputs(x, 2, (2, 3), seed=5, id0=7, n_draws=3, substrate=sub, attr=attr,
                                                      out_dtype=out_dtype)
    assert out.shape == (2, 3, 3, 6, 9) and out.dtype == out_dtype and member.shape == (2, 3, 6) and attr_sum.shape == (2, 3)
    assert np.array_equal(member.numpy(), F.reference_subsets(2, 6, 2, 3, 5, id0=7))
    for b in range(2):
        for j in range(3):
            want = x[b].clone()
            total = 0.0
            for c in range(6):
                if member[b, j, c]:
                    r, q = divmod(c, 3)
                    want[:, 3 * r:3 * r + 3, 3 * q:3 * q + 3] = sub[b, :, 3 * r:3 * r + 3, 3 * q:3 * q + 3]
                    total += float(attr[b, c])
            assert same_bits(out[b, j], want.to(out_dtype))
            assert abs(float(attr_sum[b, j]) - total) <= 8 * U * float(attr[b].abs().sum())
    filled, m2, none = F.reference_subset_inputs(x, 2, (2, 3), seed=5, id0=7, n_draws=3, fill=[0.25, -1.0, 2.0], out_dtype=out_dtype)
    assert none is None and torch.equal(m2, member)
    pixels = member.reshape(2, 3, 1, 2, 3).bool().repeat_interleave(3, 3).repeat_interleave(3, 4).expand(2, 3, 3, 6, 9)
    want = torch.tensor([0.25, -1.0, 2.0]).reshape(1, 1, 3, 1, 1).expand(2, 3, 3, 6, 9)
    assert same_bits(filled[pixels], want[pixels].to(out_dtype)) and same_bits(filled[~pixels], x[:, None].expand(2, 3, 3, 6, 9)[~pixels].to(out_dtype))
    # a substrate equal to x: copies
    same, _, _ = F.reference_subset_inputs(x, 6, (2, 3), seed=5, substrate=x, out_dtype=out_dtype)
    assert same_bits(same[:, 0], x.to(out_dtype))
    for bad in (dict(substrate=None), dict(fill=[0.0] * 3), dict(grid=(4, 3)), dict(grid=(2, 9)), dict(out_dtype=torch.float16), dict(k=7)):
        args = dict(x=x, k=2, grid=(2, 3), seed=0, substrate=sub)
        args.update(bad)
        with pytest.raises(ValueError):
            F.reference_subset_inputs(**args)


def test_reference_dot_is_the_two_sums():
    F = fb()
    x, y, w = inputs(2, 12, seed=1), inputs(2, 36, seed=2).reshape(2, 3, 12), inputs(2, 4, seed=3)
    got = F.reference_dot(x, y, w)
    assert got.shape == (2, 3, 2) and got.dtype == torch.float64
    for b in range(2):
        for d in range(3):
            df = [float(x[b, e]) - float(y[b, d, e]) for e in range(12)]
            assert float(got[b, d, 0]) == pytest.approx(sum(df[e] * float(w[b, e % 4]) for e in range(12)), rel=1e-14, abs=1e-14)
            assert float(got[b, d, 1]) == pytest.approx(sum(v * v for v in df), rel=1e-14)
    assert same_bits(F.reference_dot(x, x[:, None], w), torch.zeros(2, 1, 2, dtype=torch.float64))
    from transformer_explainability_amd.robustness import reference_distance
    assert torch.allclose(got[..., 1], reference_distance(x, y)[..., 0], rtol=1e-15)
    with pytest.raises(ValueError):
        F.reference_dot(x, y, inputs(2, 5))


# ------------------------------------------------------------------------------------------------ the scores
def test_scores_against_a_loop_and_scipy():
    from scipy.stats import pearsonr
    F = fb()
    g = torch.Generator().manual_seed(3)
    B, D = 4, 9
    ip, attr = (torch.randn((B, D), generator=g, dtype=torch.float64) for _ in range(2))
    delta = 0.7 * ip + 0.3 * attr + 0.1 * torch.randn((B, D), generator=g, dtype=torch.float64)
    got = F.scores_from_sums(ip, delta, attr)
    assert set(got) == set(F.SCORE_NAMES) and all(v.shape == (B,) and v.dtype == torch.float64 for v in got.values())
    for b in range(B):
        i, d, a = (t[b].tolist() for t in (ip, delta, attr))
        inf = sum((u - v) ** 2 for u, v in zip(i, d)) / D
        beta = sum(u * v for u, v in zip(i, d)) / sum(u * u for u in i)
        inf_n = sum((beta * u - v) ** 2 for u, v in zip(i, d)) / D
        assert float(got["infidelity"][b]) == pytest.approx(inf, rel=1e-13)
        assert float(got["beta"][b]) == pytest.approx(beta, rel=1e-13)
        assert float(got["infidelity_norm"][b]) == pytest.approx(inf_n, rel=1e-12)
        assert float(got["infidelity_norm"][b]) <= float(got["infidelity"][b]) * (1 + 1e-12)      # beta is the least-squares scale
        assert float(got["faith_corr"][b]) == pytest.approx(pearsonr(a, d)[0], rel=1e-12)
    # Pearson is invariant under a positive affine map of either side and flips with the sign
    again = F.scores_from_sums(ip, 3.0 * delta + 2.0, -0.5 * attr + 1.0)
    assert torch.allclose(again["faith_corr"], -got["faith_corr"], rtol=1e-12)


def test_scores_of_the_degenerate_rows():
    F = fb()
    one = F.scores_from_sums(torch.tensor([[2.0]], dtype=torch.float64), torch.tensor([[0.5]], dtype=torch.float64),
                             torch.tensor([[1.0]], dtype=torch.float64))
    assert float(one["infidelity"]) == 2.25 and float(one["beta"]) == 0.25 and float(one["infidelity_norm"]) == 0.0
    assert math.isnan(float(one["faith_corr"]))                          # D = 1
    ip = torch.tensor([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [1.0, -1.0, 2.0]], dtype=torch.float64)
    delta = torch.tensor([[0.5, 0.5, 0.5], [1.0, 2.0, 4.0], [1.0, -1.0, 2.0]], dtype=torch.float64)
    attr = torch.tensor([[1.0, 2.0, 3.0], [2.0, 2.0, 2.0], [1.0, -1.0, 2.0]], dtype=torch.float64)
    got = F.scores_from_sums(ip, delta, attr)
    assert math.isnan(float(got["faith_corr"][0]))                       # a constant drop
    assert math.isnan(float(got["faith_corr"][1]))                       # a constant attribution sum
    assert float(got["beta"][1]) == 1.0 and float(got["infidelity"][1]) == 7.0 == float(got["infidelity_norm"][1])      # ip = 0
    assert abs(float(got["faith_corr"][2]) - 1.0) <= 4 * U and float(got["infidelity"][2]) == 0.0 and float(got["beta"][2]) == 1.0
    none = F.scores_from_sums(ip, delta)                                 # noise mode: no attribution sums
    assert bool(torch.isnan(none["faith_corr"]).all()) and torch.equal(none["infidelity"], got["infidelity"])


# ------------------------------------------------------------------------------------------------ the evaluator on CPU tensors
@pytest.mark.parametrize("perturbation", ["subset", "noise"])
def test_evaluator_linear_score_has_no_infidelity(perturbation):
    """f(x) = sum_e heat[e mod m] x_e in fp64 and the map whose pixel-level form is heat: ip = sum (x - x') heat and delta =
    f(x) - f(x') are the same number evaluated two ways.

    Derivation.  T = sum_e |heat_e| (|x_e| + |x'_e|) bounds the magnitudes of the terms of all three sums (ip's, f(x)'s,
    f(x')'s).  A sum of n products in fp64, in any order, is within (n + 1) u of the sum of the magnitudes of its terms
    (Higham, section 4.2, with the product's own rounding); the subtraction f(x) - f(x') rounds once more.  So |ip - delta|
    <= (3 (n + 1) + 1) u T <= E = 4 (n + 1) u T per draw, infidelity <= E^2, and with beta - 1 = sum ip (delta - ip) / sum ip^2,
    |beta - 1| <= sqrt(D) E / |ip|_2 by Cauchy-Schwarz, plus 4 u for the quotient's own roundings."""
    F = fb()
    B, C, g, p, D = 3, 3, 3, 2, 6
    x = images(B, C, g * p, g * p, seed=5)
    stub = LinearScore(token_maps(B, g * g, seed=6), p)
    ev = F.FaithfulnessEvaluator(stub, perturbation=perturbation, n_draws=D, subset_size=4, baseline="black", radius=0.1,
                                 output="logit", seed=2, draws_per_pass=4, keep_last=True)
    ev.update(x)
    assert stub.calls == [B * 4] * 3                                     # the reference pass, two passes of 4 draws (2 dropped)
    a, kept = ev.arrays(), ev.last
    assert set(a) == set(F.SCORE_NAMES) and kept["copies"].shape == (B, D, C, g * p, g * p)
    heat = stub.heat.reshape(B, 1, 1, -1).abs()
    T = (heat * (x.double().reshape(B, 1, C, -1).abs() + kept["copies"].double().reshape(B, D, C, -1).abs())).sum((2, 3))
    E = 4 * (C * g * g * p * p + 1) * U * T.max(1).values
    assert float(kept["ip"].abs().min()) > 0
    print(f"stub {perturbation}: infidelity {a['infidelity']}, bound {(E ** 2).tolist()}; beta - 1 {a['beta'] - 1}")
    assert (a["infidelity"] <= (E ** 2).numpy()).all() and (a["infidelity_norm"] <= (E ** 2).numpy() * (1 + 1e-9)).all()
    assert (np.abs(a["beta"] - 1) <= (math.sqrt(D) * E / kept["ip"].norm(dim=1)).numpy() + 4 * U).all()
    if perturbation == "subset":
        want, member, attr_sum = F.reference_subset_inputs(x, 4, g, seed=2, n_draws=D, fill=[-1.0] * 3, attr=stub.maps)
        assert same_bits(kept["copies"], want) and torch.equal(kept["member"], member) and same_bits(kept["attr_sum"], attr_sum)
    else:
        from transformer_explainability_amd.robustness import reference_noise
        assert same_bits(kept["copies"], reference_noise(x, D, 0.1, seed=2)) and kept["member"] is None
        assert np.isnan(a["faith_corr"]).all()


def test_evaluator_zero_substrate_gives_correlation_one():
    """p = 1 and x = 1 everywhere, the zero substrate: f(x) - f(x') = C sum over the subset of the map = C attr_sum, so the
    two sides of the correlation are proportional.

    Derivation.  delta_d = C a_d + e_d with |e_d| <= E = 4 (n + 1) u T as in the test above (T = 2 C sum |map| here).  The
    correlation is the cosine between the centred vectors; a perturbation of relative size r = sqrt(D) E / |centred C a|_2
    turns the angle by at most asin(r), so cos >= 1 - r^2; the evaluation of the correlation itself (two centred sums of D
    terms, two roots, a product and a quotient) stays within 4 (D + 4) u."""
    F = fb()
    B, C, g, D = 3, 3, 4, 8
    x = torch.ones(B, C, g, g)
    stub = LinearScore(token_maps(B, g * g, seed=8), 1)
    ev = F.FaithfulnessEvaluator(stub, perturbation="subset", n_draws=D, baseline="zero", output="logit", seed=4,
                                 draws_per_pass=3, keep_last=True)
    ev.update(x)
    a, kept = ev.arrays(), ev.last
    assert kept["member"].sum(2).unique().tolist() == [4]                # subset_size None: max(1, G // 4)
    E = 4 * (C * g * g + 1) * U * 2 * C * stub.maps.double().abs().sum(1)
    ca = C * (kept["attr_sum"] - kept["attr_sum"].mean(1, keepdim=True))
    r = math.sqrt(D) * E / ca.norm(dim=1)
    print(f"stub zero substrate: 1 - faith_corr {1 - a['faith_corr']}, bound {(r ** 2 + 4 * (D + 4) * U).tolist()}")
    assert (a["faith_corr"] <= 1.0).all() and (1 - a["faith_corr"] <= (r ** 2 + 4 * (D + 4) * U).numpy()).all()
    assert (a["infidelity"] <= (E ** 2).numpy()).all()


def test_evaluator_ids_run_on_and_an_unchanged_image_drops_nothing():
    F = fb()
    B, C, g, p, D = 4, 3, 2, 2, 5
    x = images(B, C, g * p, g * p, seed=9)
    m = token_maps(B, g * g, seed=10)
    kept = []
    ev = F.FaithfulnessEvaluator(LinearScore(m[:2], p), n_draws=D, subset_size=1, baseline="zero", seed=3, draws_per_pass=2,
                                 keep_last=True)
    for lo in (0, 2):
        ev.lrp = LinearScore(m[lo:lo + 2], p)
        ev.update(x[lo:lo + 2])
        kept.append((ev.last["copies"], ev.last["member"]))
    assert ev.last["id0"] == 2 and ev.summary()["samples"] == 4
    want, member, _ = F.reference_subset_inputs(x, 1, g, seed=3, n_draws=D, fill=[0.0] * 3)
    assert same_bits(torch.cat([c for c, _ in kept], 0), want) and torch.equal(torch.cat([mm for _, mm in kept], 0), member)
    # radius 0: the copies are the image, the drop and the product are exactly 0
    zero = F.FaithfulnessEvaluator(LinearScore(m, p), perturbation="noise", n_draws=3, radius=0.0, draws_per_pass=2, keep_last=True)
    zero.update(x)
    assert same_bits(zero.last["delta"], torch.zeros(B, 3, dtype=torch.float64)) and zero.arrays()["infidelity"].tolist() == [0.0] * B
    assert zero.arrays()["beta"].tolist() == [1.0] * B
    # "prob" runs the fp64 softmax of curves.py; given classes stay fixed
    prob = F.FaithfulnessEvaluator(LinearScore(m, p), n_draws=3, baseline=(0.25, 0.5, 0.75), output="prob", keep_last=True)
    classes = prob.update(x, index=[1, 0, 1, 0])
    assert classes.reshape(-1).tolist() == [1, 0, 1, 0] and bool((prob.last["delta"].abs() <= 1).all())


def test_evaluator_refuses_token_ids_and_bad_arguments():
    F = fb()
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.robustness import SensitivityEvaluator
    stub = LinearScore(token_maps(2, 4), 2)
    ev = F.FaithfulnessEvaluator(stub)
    ids = torch.zeros((2, 16), dtype=torch.int64)
    with pytest.raises(TeError, match="discrete") as mine:
        ev.update(ids)
    with pytest.raises(TeError) as theirs:
        SensitivityEvaluator(stub).update(ids)
    assert str(mine.value) == str(theirs.value)
    with pytest.raises(TeError, match="float32"):
        ev.update(torch.zeros((2, 3, 4, 4), dtype=torch.float64))
    with pytest.raises(TeError, match="square patch grid"):
        F.FaithfulnessEvaluator(LinearScore(token_maps(2, 4), 2)).update(torch.zeros(2, 3, 4, 6))
    with pytest.raises(ValueError, match="subset_size"):
        F.FaithfulnessEvaluator(stub, subset_size=5).update(torch.zeros(2, 3, 4, 4))
    for bad in (dict(n_draws=0), dict(radius=-1.0), dict(radius=float("nan")), dict(draws_per_pass=0), dict(subset_size=0),
                dict(perturbation="gauss"), dict(output="margin"), dict(baseline="white"), dict(klen=10)):
        with pytest.raises(ValueError):
            F.FaithfulnessEvaluator(stub, **bad)


# ------------------------------------------------------------------------------------------------ the entry points, no device
ENTRIES = ("te_subset_inputs_f32", "te_subset_inputs_bf16", "te_perturbation_dot_f32", "te_perturbation_dot_bf16")


def test_entry_points_are_declared_exported_and_bound(lib):
    import transformer_explainability_amd as te
    from transformer_explainability_amd import _cabi, _lib, faithfulness, ops
    with open(os.path.join(ROOT, "include", "te_relprop.h")) as f:
        header = f.read()
    section = header.index("---- faithfulness")
    assert header.index("---- robustness and complexity") < section < header.index("---- bf16 operands")
    for name in ENTRIES:
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, header)) == 1 and header.index(name + "(") > section
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == (18 if "subset" in name else 9), name
    assert lib.te_version() >= 705 and _lib.MIN_LIB_VERSION == 800 and _lib.TE_SUBSET_MAX_CELLS == 4096
    assert hasattr(_cabi, "CTYPES")                                      # bound from the header, not from a table kept by hand
    with open(os.path.join(ROOT, "transformer-explainability_amd", "ops.py")) as f:
        assert "argtypes" not in f.read()
    assert callable(ops.subset_inputs) and callable(ops.perturbation_dot)
    assert te.faithfulness is faithfulness and "faithfulness.py" in te.__doc__
    assert callable(faithfulness.FaithfulnessEvaluator) and "te_faithful.hip" in __import__("transformer_explainability_amd.build", fromlist=["SOURCES"]).SOURCES


def test_new_entry_points_refuse_on_the_host(lib):
    """P is a fake non-null, 16-byte-aligned address that the host never dereferences: every call returns before any HIP call."""
    P = 4096
    sub = dict(x=P, substrate=P, fill=None, attr=P, out=P, member=P, attr_sum=P, B=2, C=3, g_h=4, g_w=4, p=2, k=4, d0=0, n_d=3,
               seed=1, id0=0, stream=None)
    for f in ENTRIES[:2]:
        assert [status(lib, f, sub, x=None), status(lib, f, sub, out=None), status(lib, f, sub, member=None),
                status(lib, f, sub, substrate=None), status(lib, f, sub, attr_sum=None), status(lib, f, sub, B=0),
                status(lib, f, sub, C=0), status(lib, f, sub, g_h=0), status(lib, f, sub, g_w=-1), status(lib, f, sub, p=0),
                status(lib, f, sub, n_d=0), status(lib, f, sub, d0=-1)] == [-1] * 12
        assert [status(lib, f, sub, k=0), status(lib, f, sub, k=17), status(lib, f, sub, k=-3)] == [-1] * 3
        assert [status(lib, f, sub, d0=(1 << 32) - 2), status(lib, f, sub, d0=1 << 32, n_d=1)] == [-1, -1]
        assert [status(lib, f, sub, g_h=17, g_w=241), status(lib, f, sub, g_h=1, g_w=4097), status(lib, f, sub, g_h=4097, g_w=1),
                status(lib, f, sub, B=65536), status(lib, f, sub, p=1 << 20), status(lib, f, sub, C=1 << 40),
                status(lib, f, sub, substrate=None, fill=P, C=5)] == [-3] * 7      # G = 4097 three ways; C H W beyond 2^31 - 1
    dot = dict(x=P, y=P, w=P, sums=P, B=2, D=3, n=96, m=32, stream=None)
    for f in ENTRIES[2:]:
        assert [status(lib, f, dot, x=None), status(lib, f, dot, y=None), status(lib, f, dot, w=None), status(lib, f, dot, sums=None),
                status(lib, f, dot, B=0), status(lib, f, dot, D=0), status(lib, f, dot, n=-1), status(lib, f, dot, m=0)] == [-1] * 8
        assert [status(lib, f, dot, m=36), status(lib, f, dot, m=192)] == [-1, -1]      # n % m != 0
        assert [status(lib, f, dot, B=65536), status(lib, f, dot, n=1 << 31, m=1 << 31), status(lib, f, dot, D=1 << 31)] == [-3] * 3


def test_ops_refuse_before_any_device_call():
    from transformer_explainability_amd import TeError, ops
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(TeError, match="MI355X"):
        ops.subset_inputs(x, 2, 4, 0, fill=[0.0] * 3)
    with pytest.raises(TeError, match="MI355X"):
        ops.perturbation_dot(x.reshape(2, -1), x.reshape(2, 1, -1), x[:, 0].reshape(2, -1))
    with pytest.raises(TeError, match="float32"):
        ops.subset_inputs(x.double(), 2, 4, 0, fill=[0.0] * 3)
    with pytest.raises(TeError, match="out_dtype"):
        ops.subset_inputs(x, 2, 4, 0, fill=[0.0] * 3, out_dtype=torch.float16)
    with pytest.raises(TeError, match="float32"):
        ops.perturbation_dot(x.reshape(2, -1).to(torch.bfloat16), x.reshape(2, 1, -1), x[:, 0].reshape(2, -1))


def test_philox_is_defined_once_in_a_header():
    """The house rule of csrc/te_common.h: te_robust.hip and te_faithful.hip run one definition of the generator and of the
    bf16 rounding."""
    from test_csrc_shared import _function, _sources, definitions
    sources = _sources()
    for name in ("philox4x32_10", "bf16_bits"):
        found = definitions(sources, _function(name))
        assert len(found) == 1 and found[0][1] == 1 and found[0][0].endswith(".h"), (name, found)
    assert "philox4x32_10(" in sources["te_robust.hip"] and "philox4x32_10(" in sources["te_faithful.hip"]
    for constant in ("0xD2511F53", "0xCD9E8D57"):
        assert [n for n, text in sources.items() if constant in text] == ["te_common.h"]
