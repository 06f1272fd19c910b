"""CPU: the restatement of the robustness / complexity protocol (robustness.py) against independent definitions -- Philox's
known answers, the noise's range, moments and reproducibility, Gini against the brute-force mean difference, entropy against
scipy -- the evaluator on CPU tensors with a stub generator, and the host-side refusals of the new entry points."""
import math

import numpy as np
import pytest
import torch

from host_util import lib, same_bits, status  # noqa: F401
from robustness_inputs import KNOWN_ANSWERS, LinearMaps, inputs, maps, special_rows


def rb():
    from transformer_explainability_amd import robustness
    return robustness


# ------------------------------------------------------------------------------------------------ Philox and the noise
def test_philox_known_answers():
    R = rb()
    for counter, key, want in KNOWN_ANSWERS:
        assert tuple(int(v) for v in R.philox4x32(counter, key)) == want
    # vectorised: the three at once give the three
    got = R.philox4x32(np.array([c for c, _, _ in KNOWN_ANSWERS], dtype=np.uint64), np.array([k for _, k, _ in KNOWN_ANSWERS], dtype=np.uint64))
    assert got.dtype == np.uint32 and [tuple(int(v) for v in row) for row in got] == [w for _, _, w in KNOWN_ANSWERS]


def test_noise_words_follow_the_counter_layout():
    """Element e is word e & 3 of the call with counter (e >> 2, d, low32(id), high32(id)) and key (low32, high32 of seed)."""
    R = rb()
    seed, id0, d0 = 0x1234567890abcdef, (1 << 32) + 5, 7
    w = R.noise_words(2, 11, 3, seed, id0, d0)
    assert w.shape == (2, 3, 11) and w.dtype == np.uint32
    for b, j, e in [(0, 0, 0), (1, 2, 10), (0, 1, 5), (1, 0, 3)]:
        sample = id0 + b
        want = R.philox4x32((e >> 2, d0 + j, sample & 0xffffffff, sample >> 32), (seed & 0xffffffff, seed >> 32))[e & 3]
        assert int(w[b, j, e]) == int(want), (b, j, e)
    # a negative seed is its 64 bits read as unsigned
    assert np.array_equal(R.noise_words(1, 8, 1, -1), R.noise_words(1, 8, 1, (1 << 64) - 1))


@pytest.mark.parametrize("radius", [0.02, 0.5, 3.0])
def test_noise_stays_in_the_ball(radius):
    """|y - x| <= radius (1 + 2^-23) + ulp: |s| <= 1, the product rounds once (relative 2^-24 <= 2^-23), the sum rounds once
    (half an ulp of y <= one ulp)."""
    R = rb()
    x = inputs(3, 1001, seed=1)
    y = R.reference_noise(x, 4, radius, seed=3)
    assert y.shape == (3, 4, 1001) and y.dtype == torch.float32
    r32 = float(np.float32(radius))
    ulp = torch.from_numpy(np.spacing(np.abs(y.numpy()))).double()
    err = (y.double() - x.double()[:, None]).abs()
    assert bool((err <= r32 * (1 + 2.0 ** -23) + ulp).all()), float((err - ulp).max())
    assert float(err.max()) > 0.9 * r32                                 # ... and fills it


def test_unit_noise_is_exact_and_has_the_moments_of_a_uniform():
    """s = 2u - 1 is exact in fp32; over 10^6 words its mean is within 5 sigma of 0 and its variance within 5 sigma of 1/3
    (sigma of the mean = sqrt(1/3 / N); of the variance = sqrt((1/5 - 1/9) / N): the fourth moment of U(-1, 1) is 1/5)."""
    R = rb()
    N = 1000000
    w = R.noise_words(1, N, 1, seed=11).reshape(-1)
    s = R.unit_noise(w)
    assert s.dtype == np.float32
    exact = 2.0 * ((w >> 8).astype(np.float64) * 2.0 ** -24) - 1.0
    assert np.array_equal(s.astype(np.float64), exact)
    assert s.min() >= -1.0 and s.max() <= 1.0 - 2.0 ** -23
    mean, var = float(exact.mean()), float(exact.var())
    assert abs(mean) <= 5 * math.sqrt(1 / 3 / N), mean
    assert abs(var - 1 / 3) <= 5 * math.sqrt((1 / 5 - 1 / 9) / N), var


def test_noise_is_reproducible_and_depends_on_draw_id_and_seed():
    R = rb()
    x = inputs(3, 257, seed=2)
    base = R.reference_noise(x, 4, 0.1, seed=5, id0=10)
    assert same_bits(base, R.reference_noise(x, 4, 0.1, seed=5, id0=10))
    assert not same_bits(base, R.reference_noise(x, 4, 0.1, seed=6, id0=10))
    assert not same_bits(base, R.reference_noise(x, 4, 0.1, seed=5, id0=11))
    assert not same_bits(base[:, 0], base[:, 1])                        # two draws of a sample differ
    assert not same_bits(base[0] - x[0], base[1] - x[1])                # two samples draw different noise
    # a batch equals its samples run alone at their ids
    for b in range(3):
        assert same_bits(base[b:b + 1], R.reference_noise(x[b:b + 1], 4, 0.1, seed=5, id0=10 + b)), b
    # sample id 11 is sample id 11, wherever in a batch it stands
    assert same_bits(base[1], R.reference_noise(x[1:2], 4, 0.1, seed=5, id0=11)[0])
    # a chunk (d0, n_d) is a slice of the full call
    assert same_bits(base[:, :2], R.reference_noise(x, 2, 0.1, seed=5, id0=10, d0=0))
    assert same_bits(base[:, 3:], R.reference_noise(x, 1, 0.1, seed=5, id0=10, d0=3))
    # radius 0: exact copies; bf16: the fp32 value rounded once
    assert same_bits(R.reference_noise(x, 2, 0.0, seed=5), x[:, None].expand(3, 2, 257).contiguous())
    assert same_bits(R.reference_noise(x, 4, 0.1, seed=5, id0=10, out_dtype=torch.bfloat16), base.to(torch.bfloat16))
    # the shape of an image is kept
    img = x[:, :256].reshape(3, 1, 16, 16)
    assert same_bits(R.reference_noise(img, 2, 0.1, seed=5).reshape(3, 2, 256), R.reference_noise(x[:, :256].contiguous(), 2, 0.1, seed=5))


def test_the_torch_and_numpy_expressions_of_the_noise_agree():
    """x + s * radius, every operation rounded once to fp32: numpy's expression gives torch's bits."""
    R = rb()
    x = inputs(2, 513, seed=3)
    s = R.unit_noise(R.noise_words(2, 513, 3, seed=9))
    want = x.numpy()[:, None, :] + s * np.float32(0.07)
    assert want.dtype == np.float32
    assert same_bits(R.reference_noise(x, 3, 0.07, seed=9), torch.from_numpy(want))


@pytest.mark.parametrize("bad", [dict(radius=-0.1), dict(radius=float("nan")), dict(radius=float("inf")), dict(n_draws=0),
                                 dict(d0=-1), dict(d0=(1 << 32) - 1, n_draws=2), dict(out_dtype=torch.float16)])
def test_reference_noise_refuses(bad):
    R = rb()
    args = dict(n_draws=2, radius=0.1, seed=0)
    args.update(bad)
    with pytest.raises(ValueError):
        R.reference_noise(inputs(1, 8), **args)


# ------------------------------------------------------------------------------------------------ distance
def test_reference_distance_is_the_three_sums():
    R = rb()
    a = maps(2, 197, seed=1)
    b = torch.stack([a, -a, torch.zeros_like(a)], 1)
    b[1, 2, 5] = 3.0
    s = R.reference_distance(a, b)
    assert s.shape == (2, 3, 3) and s.dtype == torch.float64
    a2 = (a.double() ** 2).sum(1)
    assert torch.equal(s[:, 0, 0], torch.zeros(2, dtype=torch.float64)) and torch.equal(s[:, 0, 1], s[:, 0, 2])
    torch.testing.assert_close(s[:, 1, 0], 4 * a2, rtol=1e-14, atol=0)
    torch.testing.assert_close(s[0, 2], torch.stack([a2[0], a2[0], torch.zeros((), dtype=torch.float64)]), rtol=1e-14, atol=0)
    assert float(s[1, 2, 2]) == 9.0
    # bf16 copies are upcast exactly
    bb = b.to(torch.bfloat16)
    assert torch.equal(R.reference_distance(a, bb), R.reference_distance(a, bb.float()))


# ------------------------------------------------------------------------------------------------ complexity
def brute_gini(v):
    """sum_i sum_j |v_i - v_j| / (2 n S): the relative mean absolute difference, in fp64."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    return np.abs(v[:, None] - v[None, :]).sum() / (2 * len(v) * v.sum())


@pytest.mark.parametrize("n", [1, 2, 3, 64, 197, 300])
def test_gini_equals_the_mean_absolute_difference(n):
    R = rb()
    m = maps(4, n, seed=n)
    m[3] = torch.round(m[3] * 2) / 2                                    # a row of ties
    if not bool((m != 0).any(1).all()):
        m[:, 0] = 1.0
    out, _ = R.reference_complexity(m)
    for b in range(4):
        want = brute_gini(m[b].numpy())
        assert abs(float(out[b, 0]) - want) <= 4 * (n + 3) * 2.0 ** -53, (b, float(out[b, 0]), want)


@pytest.mark.parametrize("n", [1, 2, 65, 196, 1025])
def test_entropy_equals_scipy(n):
    import scipy.stats
    R = rb()
    m = maps(3, n, seed=n + 1)
    m[:, 0] = 0.5
    out, counts = R.reference_complexity(m)
    for b in range(3):
        v = np.abs(m[b].numpy().astype(np.float64))
        np.testing.assert_allclose(float(out[b, 1]), scipy.stats.entropy(v), rtol=1e-12, atol=1e-15)
        assert int(counts[b, 1]) == int((v > 0).sum())
        assert int(counts[b, 0]) == int((v > 1e-5 * v.max()).sum())


def test_complexity_of_the_special_rows():
    R = rb()
    n = 197
    rows = special_rows(n)
    out, counts = R.reference_complexity(rows, eps=1e-5)
    assert out.dtype == torch.float64 and counts.dtype == torch.int64 and out.shape == (6, 2) and counts.shape == (6, 2)
    # the zero map and the NaN row: NaN, NaN, 0, 0 -- and the neighbours are unaffected
    for b in (0, 4):
        assert bool(torch.isnan(out[b]).all()) and counts[b].tolist() == [0, 0]
    alone = [R.reference_complexity(rows[b:b + 1]) for b in range(6)]
    for b in (1, 2, 3, 5):
        assert same_bits(out[b], alone[b][0][0]) and torch.equal(counts[b], alone[b][1][0]), b
    # one-hot: Gini (n - 1) / n, entropy 0, one value
    assert abs(float(out[1, 0]) - (n - 1) / n) <= 2.0 ** -50 and float(out[1, 1]) == 0.0 and counts[1].tolist() == [1, 1]
    # constant: Gini 0, entropy ln n, all values
    assert abs(float(out[2, 0])) <= (n + 3) * 2.0 ** -53 and abs(float(out[2, 1]) - math.log(n)) <= 1e-13
    assert counts[2].tolist() == [n, n]
    # ties: the brute-force value; the order inside a tie does not matter
    assert abs(float(out[3, 0]) - brute_gini(rows[3].numpy())) <= 4 * (n + 3) * 2.0 ** -53
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
    assert abs(float(R.reference_complexity(rows[3:4][:, perm])[0][0, 0]) - float(out[3, 0])) <= 4 * (n + 3) * 2.0 ** -53
    # the threshold: eps = 0.6 of the maximum 2.0 leaves only the values above 1.2
    _, c = R.reference_complexity(rows[3:4], eps=0.6)
    assert int(c[0, 0]) == int((rows[3].abs() > 1.2).sum()) and int(c[0, 1]) == int((rows[3] != 0).sum())
    with pytest.raises(ValueError):
        R.reference_complexity(rows, eps=-1.0)


# ------------------------------------------------------------------------------------------------ the evaluator on CPU tensors
def test_evaluator_radius_zero_gives_zero_sensitivity():
    R = rb()
    ev = R.SensitivityEvaluator(LinearMaps(4.0), n_draws=4, radius=0.0, seed=1, draws_per_pass=3)
    ev.update(inputs(3, 48, seed=1).reshape(3, 3, 4, 4))
    a = ev.arrays()
    assert a["max_sens"].tolist() == [0.0] * 3 and a["avg_sens"].tolist() == [0.0] * 3
    assert bool(np.isnan(a["lipschitz"]).all())                         # no copy moved: no pair remains
    one = R.SensitivityEvaluator(LinearMaps(4.0), n_draws=3, radius=0.0, draws_per_pass=1)
    one.update(inputs(2, 48, seed=1).reshape(2, 3, 4, 4))
    assert one.lrp.calls == [2, 2, 2, 2]                                # one draw per pass: the clean batch is its own reference
    assert ev.lrp.calls == [3, 9, 9, 9]                                 # the clean batch, the reference pass, two passes of 3 draws


def test_evaluator_linear_maps_have_the_known_lipschitz_constant():
    """map = 4 x (exact in fp32): every map difference is 4 times the input difference, term by term and sum by sum (a power
    of two), so lipschitz = 4 up to the two square roots and the division, and sens[b,d] = |dx| / |x|."""
    R = rb()
    x = inputs(5, 48, seed=2).reshape(5, 3, 4, 4)
    ev = R.SensitivityEvaluator(LinearMaps(4.0), n_draws=6, radius=0.05, seed=3, draws_per_pass=4, keep_last=True)
    kept = []
    for part in (x[:2], x[2:]):
        ev.update(part)
        kept.append(ev.last["copies"])
    a = ev.arrays()
    assert set(a) == set(R.SCORE_NAMES) and all(v.shape == (5,) for v in a.values())
    np.testing.assert_allclose(a["lipschitz"], 4.0, rtol=4 * 2.0 ** -53, atol=0)
    copies = R.reference_noise(x, 6, 0.05, seed=3)                      # ids run on across the updates: 0, 1 then 2, 3, 4
    assert same_bits(torch.cat(kept, 0), copies) and ev.last["id0"] == 2
    dx = (copies.double() - x.double()[:, None]).flatten(2).norm(dim=2)
    sens = (dx / x.double().flatten(1).norm(dim=1)[:, None]).numpy()
    np.testing.assert_allclose(a["max_sens"], sens.max(1), rtol=1e-13)
    np.testing.assert_allclose(a["avg_sens"], sens.mean(1), rtol=1e-13)
    # complexity of the clean maps, and the summary
    out, counts = R.reference_complexity(4.0 * x.flatten(1))
    assert np.array_equal(a["gini"], out[:, 0].numpy()) and np.array_equal(a["entropy"], out[:, 1].numpy())
    assert np.array_equal(a["n_eff"], counts[:, 0].numpy())
    s = ev.summary()
    assert s["samples"] == 5 and abs(s["lipschitz"] - 4.0) < 1e-14 and s["gini"] == pytest.approx(float(out[:, 0].mean()))
    # one batch of five gives the same numbers as two and three: a dataset's noise does not depend on the batch size
    ev1 = R.SensitivityEvaluator(LinearMaps(4.0), n_draws=6, radius=0.05, seed=3)
    ev1.update(x)
    for name, v in ev1.arrays().items():
        assert np.array_equal(v, a[name]), name


def test_evaluator_zero_map_norm_and_given_classes():
    """captum's rule: a clean map of norm 0 divides by 1.  ``index`` fixes the classes."""
    R = rb()
    stub = LinearMaps(2.0)
    ev = R.SensitivityEvaluator(stub, n_draws=2, radius=0.1, seed=0)
    x = torch.zeros(2, 3, 4, 4)
    classes = ev.update(x, index=[3, 5])
    assert classes.reshape(-1).tolist() == [3, 5]
    a = ev.arrays()
    copies = R.reference_noise(x, 2, 0.1, seed=0)
    np.testing.assert_allclose(a["max_sens"], (2.0 * copies.double()).flatten(2).norm(dim=2).max(1).values.numpy(), rtol=1e-13)
    assert bool(np.isnan(a["gini"]).all()) and a["n_eff"].tolist() == [0, 0]


def test_evaluator_refuses_token_ids_and_bad_arguments():
    R = rb()
    from transformer_explainability_amd import TeError
    ev = R.SensitivityEvaluator(LinearMaps())
    with pytest.raises(TeError, match="discrete"):
        ev.update(torch.zeros((2, 16), dtype=torch.int64))
    with pytest.raises(TeError, match="float32"):
        ev.update(torch.zeros((2, 3, 4, 4), dtype=torch.float64))
    for bad in (dict(n_draws=0), dict(radius=-1.0), dict(radius=float("nan")), dict(draws_per_pass=0), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            R.SensitivityEvaluator(LinearMaps(), **bad)


# ------------------------------------------------------------------------------------------------ the entry points, no device
def test_new_entry_points_refuse_on_the_host(lib):
    """P is a fake non-null, 16-byte-aligned address that the host never dereferences: every call returns before any HIP call."""
    P = 4096
    noise = dict(x=P, out=P, B=2, n=100, d0=0, n_d=3, radius=0.02, seed=1, id0=0, stream=None)
    for f in ("te_noise_inputs_f32", "te_noise_inputs_bf16"):
        assert [status(lib, f, noise, x=None), status(lib, f, noise, out=None), status(lib, f, noise, B=0),
                status(lib, f, noise, n=0), status(lib, f, noise, n_d=0), status(lib, f, noise, d0=-1)] == [-1] * 6
        assert [status(lib, f, noise, radius=-0.5), status(lib, f, noise, radius=float("nan")),
                status(lib, f, noise, radius=float("inf"))] == [-1] * 3
        assert [status(lib, f, noise, d0=(1 << 32) - 2), status(lib, f, noise, d0=1 << 32, n_d=1)] == [-1, -1]
        assert [status(lib, f, noise, n=1 << 31), status(lib, f, noise, B=65536)] == [-3, -3]
    dist = dict(a=P, b=P, sums=P, B=2, D=3, n=100, stream=None)
    for f in ("te_map_distance_f32", "te_map_distance_bf16"):
        assert [status(lib, f, dist, a=None), status(lib, f, dist, b=None), status(lib, f, dist, sums=None),
                status(lib, f, dist, B=0), status(lib, f, dist, D=0), status(lib, f, dist, n=-1)] == [-1] * 6
        assert status(lib, f, dist, B=65536) == -3
    ws_bytes = lib.te_map_complexity_workspace_bytes(2, 100)
    assert ws_bytes >= 2 * 2 * 100 * 8
    cx = dict(maps=P, out=P, counts=P, B=2, n=100, eps=1e-5, ws=P, ws_bytes=ws_bytes, stream=None)
    f = "te_map_complexity_f32"
    assert [status(lib, f, cx, maps=None), status(lib, f, cx, out=None), status(lib, f, cx, counts=None), status(lib, f, cx, B=0),
            status(lib, f, cx, n=0), status(lib, f, cx, eps=-1.0), status(lib, f, cx, eps=float("nan")),
            status(lib, f, cx, eps=float("inf")), status(lib, f, cx, ws=P + 4)] == [-1] * 9
    assert [status(lib, f, cx, n=(1 << 20) + 1), status(lib, f, cx, B=65536)] == [-3, -3]
    assert [status(lib, f, cx, ws=None), status(lib, f, cx, ws_bytes=ws_bytes - 256)] == [-2, -2]
    assert [lib.te_map_complexity_workspace_bytes(*s) for s in [(0, 4), (4, 0), (65536, 4), (4, (1 << 20) + 1)]] == [0] * 4
    assert lib.te_map_complexity_workspace_bytes(65535, 1 << 20) == 65535 * 2 * (1 << 20) * 8


def test_ops_refuse_before_any_device_call():
    from transformer_explainability_amd import TeError, ops
    x = torch.zeros(2, 8)
    with pytest.raises(TeError, match="MI355X"):
        ops.noise_inputs(x, 2, 0.1, 0)
    with pytest.raises(TeError, match="MI355X"):
        ops.map_distance(x, x[:, None])
    with pytest.raises(TeError, match="MI355X"):
        ops.map_complexity(x)
    with pytest.raises(TeError, match="float32"):
        ops.noise_inputs(x.double(), 2, 0.1, 0)
    with pytest.raises(TeError, match="out_dtype"):
        ops.noise_inputs(x, 2, 0.1, 0, out_dtype=torch.float16)
    with pytest.raises(TeError, match="float32"):
        ops.map_complexity(x.to(torch.bfloat16))
