"""-m gpu: the robustness / complexity kernels (csrc/te_robust.hip) against the restatements of robustness.py on the same seeded
inputs.  The noisy copies must be equal bit for bit; the distance sums, Gini and the entropy are held to the rounding bounds
derived at their tests (each test prints what it measured before it asserts)."""
import math

import numpy as np
import pytest
import torch

from gpu_util import dev, odd_offset_view
from host_util import same_bits
from robustness_inputs import inputs, maps, noisy_maps, special_rows

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BF = torch.bfloat16


def te():
    from transformer_explainability_amd import ops, robustness
    return ops, robustness


# ------------------------------------------------------------------------------------------------ noise
def device_noise(x, n_draws, radius, seed, id0=0, d0=0, out_dtype=torch.float32):
    ops, _ = te()
    out = ops.noise_inputs(x.to(dev()), n_draws, radius, seed, id0=id0, d0=d0, out_dtype=out_dtype)
    torch.cuda.synchronize()
    assert out.dtype == out_dtype and out.shape == (x.shape[0], n_draws) + tuple(x.shape[1:])
    return out.cpu()


@pytest.mark.parametrize("out_dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1025, 3072])
def test_noise_bits_equal_the_restatement(n, out_dtype):
    _, R = te()
    seed, id0, radius = 0x9e3779b97f4a7c15, (1 << 32) - 2, 0.02           # the ids cross 2^32: the high counter word is used
    x = inputs(3, n, seed=n)
    want = R.reference_noise(x, 4, radius, seed, id0=id0, out_dtype=out_dtype)
    full = device_noise(x, 4, radius, seed, id0=id0, out_dtype=out_dtype)
    assert same_bits(full, want)
    assert not same_bits(full[:, 0], full[:, 1])
    # chunks of the draws are slices of the full call
    assert same_bits(device_noise(x, 2, radius, seed, id0=id0, d0=0, out_dtype=out_dtype), full[:, :2])
    assert same_bits(device_noise(x, 1, radius, seed, id0=id0, d0=3, out_dtype=out_dtype), full[:, 3:])
    # a batch at id0 equals its samples run alone at id0 + b
    for b in range(3):
        assert same_bits(device_noise(x[b:b + 1], 4, radius, seed, id0=id0 + b, out_dtype=out_dtype), full[b:b + 1]), b
    # radius 0: copies, bit for bit
    assert same_bits(device_noise(x, 2, 0.0, seed, out_dtype=out_dtype), x[:, None].expand(3, 2, n).to(out_dtype).contiguous())


@pytest.mark.parametrize("out_dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [5, 64, 1025, 3072])
def test_noise_on_views_off_the_16_byte_boundary(n, out_dtype):
    """x and out start one element past a 16-byte boundary: the element-wise form gives the bits of the 16-byte form."""
    ops, R = te()
    x = inputs(3, n, seed=n + 7)
    want = R.reference_noise(x, 3, 0.1, seed=5, id0=9, out_dtype=out_dtype)
    xv = odd_offset_view(x)
    out = odd_offset_view(want, dtype=out_dtype)
    for xs, os_ in ((xv, out), (x.to(dev()), out), (xv, torch.empty_like(want, device=dev()))):
        os_.zero_()
        got = ops._noise_inputs_into(xs, os_, 0.1, 5, id0=9)
        torch.cuda.synchronize()
        assert got.data_ptr() == os_.data_ptr() and same_bits(got.cpu(), want)


@pytest.mark.parametrize("out_dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_noise_of_a_vit_input(out_dtype):
    """n = 3 x 224 x 224 = 150528, an image-shaped x: the shape the evaluator runs."""
    _, R = te()
    x = inputs(3, 150528, seed=1).reshape(3, 3, 224, 224)
    want = R.reference_noise(x, 4, 0.02, seed=1, id0=5, out_dtype=out_dtype)
    got = device_noise(x, 4, 0.02, seed=1, id0=5, out_dtype=out_dtype)
    assert got.shape == (3, 4, 3, 224, 224) and same_bits(got, want)
    assert same_bits(device_noise(x, 1, 0.02, seed=1, id0=5, d0=3, out_dtype=out_dtype), got[:, 3:])


def test_noise_refusals_on_device_tensors():
    ops, _ = te()
    from transformer_explainability_amd import TeError
    x = inputs(2, 8).to(dev())
    for bad in (dict(radius=-0.1), dict(radius=float("nan")), dict(radius=float("inf")), dict(n_draws=0), dict(d0=-1),
                dict(d0=(1 << 32) - 1, n_draws=2), dict(seed=1 << 64), dict(id0=-(1 << 63) - 1)):
        args = dict(n_draws=2, radius=0.1, seed=0)
        args.update(bad)
        with pytest.raises(TeError, match="noise_inputs"):
            ops.noise_inputs(x, **args)
    with pytest.raises(TeError, match="dense"):
        ops._noise_inputs_into(x, torch.empty((2, 3, 9), device=dev()), 0.1, 0)
    with pytest.raises(TeError, match="map_distance"):
        ops.map_distance(x, torch.zeros((2, 3, 9), device=dev()))
    with pytest.raises(TeError, match="eps"):
        ops.map_complexity(x, eps=-1.0)
    # the last draw and the largest seed and id are accepted
    got = ops.noise_inputs(x, 1, 0.1, (1 << 64) - 1, id0=(1 << 64) - 1, d0=(1 << 32) - 1)
    torch.cuda.synchronize()
    _, R = te()
    assert same_bits(got.cpu(), R.reference_noise(x.cpu(), 1, 0.1, -1, id0=(1 << 64) - 1, d0=(1 << 32) - 1))


# ------------------------------------------------------------------------------------------------ distance
def device_distance(a, b):
    ops, _ = te()
    s = ops.map_distance(a.to(dev()), b.to(dev()))
    torch.cuda.synchronize()
    assert s.dtype == torch.float64 and s.shape == (b.shape[0], b.shape[1], 3)
    return s.cpu()


@pytest.mark.parametrize("n", [1, 2, 196, 197, 255, 256, 257, 4097, 150528])
def test_distance_sums_within_the_rounding_bound(n):
    """|got - want| <= 2 (n + 2) 2^-53 want for each of the three sums.

    Derivation.  Both sides form every term in fp64 from the same exact upcasts: the difference (where there is one), one
    rounding for the square -- identical on both sides.  The terms are non-negative, so a sum of n terms in ANY order has a
    relative error of at most (n - 1) u beside the term's own rounding (Higham, Accuracy and Stability, section 4.2): at most
    (n + 2) u on either side, twice that between two evaluations."""
    _, R = te()
    bound = 2 * (n + 2) * U
    for D in (1, 3):
        for dtype in (torch.float32, BF):
            a = maps(3, n, seed=n + D)
            b = noisy_maps(a, D, seed=n).to(dtype)
            b[1, 0] = a[1].to(dtype)                                    # one pair without a difference (fp32) or nearly so
            got, want = device_distance(a, b), R.reference_distance(a, b)
            rel = ((got - want).abs() / want.clamp_min(1e-300)).max()
            print(f"distance n {n} D {D} {dtype}: max rel err {float(rel):.3e}, bound {bound:.3e}")
            assert bool(((got - want).abs() <= bound * want).all()), (n, D, dtype, float(rel))
            if dtype == torch.float32:
                assert float(got[1, 0, 0]) == 0.0 and float(got[1, 0, 1]) == float(got[1, 0, 2])      # a == b: exactly zero
            # a batch equals its samples, bit for bit
            for s in range(3):
                assert same_bits(device_distance(a[s:s + 1], b[s:s + 1]), got[s:s + 1]), (n, D, dtype, s)


@pytest.mark.parametrize("n", [3, 197, 256])
def test_distance_of_zero_maps_and_views(n):
    ops, R = te()
    a = maps(2, n, seed=n)
    zero = torch.zeros(2, 2, n)
    got = device_distance(torch.zeros(2, n), zero)
    assert same_bits(got, torch.zeros(2, 2, 3, dtype=torch.float64))
    got = device_distance(a, zero)                                      # b = 0: the distance is the norm of a
    assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 2], torch.zeros(2, 2, dtype=torch.float64))
    # views off the 16-byte boundary: the element-wise loads give the bits of the 16-byte loads
    b = noisy_maps(a, 2, seed=n)
    want = device_distance(a, b)
    for bt in (b, b.to(BF)):
        ref = device_distance(a, bt)
        for av, bv in ((odd_offset_view(a), odd_offset_view(bt)), (a.to(dev()), odd_offset_view(bt)), (odd_offset_view(a), bt.to(dev()))):
            s = ops.map_distance(av, bv)
            torch.cuda.synchronize()
            assert same_bits(s.cpu(), ref)
    assert not same_bits(want, device_distance(a, b.to(BF)))


# ------------------------------------------------------------------------------------------------ complexity
def device_complexity(m, eps=1e-5):
    ops, _ = te()
    out, counts = ops.map_complexity(m.to(dev()), eps)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and counts.dtype == torch.int64 and out.shape == (m.shape[0], 2) == counts.shape
    return out.cpu(), counts.cpu()


def assert_complexity_within_bound(m, eps=1e-5, what=""):
    """counts equal; |gini - want| <= 2 (n + 3) 2^-53; |entropy - want| <= 4 (n + 4) 2^-53 max(1, ln n); NaN where want is.

    Derivation, Gini.  Every product (2k - n - 1) v_(k) is exact in fp64 (21 + 24 bits) and |2k - n - 1| < n, so the
    numerator is a sum of n exact terms of magnitude below n S in all: an error of at most (n - 1) u n S in any order,
    (n - 1) u after the division by n S; S itself is a sum of n non-negative exact terms, relative error (n - 1) u, and
    |gini| < 1; n S rounds once and the division once.  At most (n + 2) u + O(n^2 u^2) on either side before that division --
    (n + 3) u with it -- and twice that between two evaluations.
    Derivation, entropy.  Per term: p = v / S rounds once and inherits the relative error of S; ln is within 1 ulp on either
    side (the device's and torch's documented bound) and its argument's relative error e moves ln p by e absolutely, p ln p by
    p e; the product rounds once.  Summed over the terms, whose magnitudes add to H <= ln n: (n + 3) u H from S, the
    roundings and the order of the sum, plus (n - 1) u sum p = (n - 1) u from the argument of the logarithm: at most
    2 (n + 4) u max(1, ln n) on either side, twice that between the two."""
    _, R = te()
    n = m[0].numel()
    got, got_counts = device_complexity(m, eps)
    want, want_counts = R.reference_complexity(m, eps)
    assert torch.equal(got_counts, want_counts), (what, got_counts, want_counts)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    err = torch.nan_to_num((got - want).abs())
    b_gini, b_ent = 2 * (n + 3) * U, 4 * (n + 4) * U * max(1.0, math.log(n))
    print(f"complexity {what or tuple(m.shape)}: gini err {float(err[:, 0].max()):.3e} (bound {b_gini:.3e}), "
          f"entropy err {float(err[:, 1].max()):.3e} (bound {b_ent:.3e})")
    assert float(err[:, 0].max()) <= b_gini and float(err[:, 1].max()) <= b_ent, (what, err.max(0).values.tolist())
    return got, got_counts


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 196, 1025, 4097, 50176])
def test_complexity_within_the_rounding_bound(n):
    m = maps(3, n, seed=n)
    m[:, 0] = 0.5                                                       # no zero map by chance at n = 1, 2
    got, counts = assert_complexity_within_bound(m, what=f"n {n}")
    assert bool((got[:, 0] >= 0).all()) and bool((got[:, 0] < 1).all())
    assert_complexity_within_bound(m, eps=0.25, what=f"n {n} eps 0.25")
    for b in range(3):                                                  # a batch equals its samples, bit for bit
        alone, alone_counts = device_complexity(m[b:b + 1])
        assert same_bits(alone, got[b:b + 1]) and torch.equal(alone_counts, counts[b:b + 1]), b


@pytest.mark.parametrize("n", [7, 197, 1025])
def test_complexity_of_the_special_rows(n):
    rows = special_rows(n)
    got, counts = assert_complexity_within_bound(rows, what=f"special rows n {n}")
    for b in (0, 4):                                                    # the zero map, the NaN row
        assert bool(torch.isnan(got[b]).all()) and counts[b].tolist() == [0, 0]
    assert abs(float(got[1, 0]) - (n - 1) / n) <= 4 * U and float(got[1, 1]) == 0.0 and counts[1].tolist() == [1, 1]
    assert float(got[2, 0]) == 0.0 and counts[2].tolist() == [n, n]     # a constant: the weights 2k - n - 1 cancel exactly
    assert abs(float(got[2, 1]) - math.log(n)) <= 4 * (n + 4) * U * math.log(n)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
    again, again_counts = device_complexity(rows[:, perm])              # ties, in another order
    assert abs(float(again[3, 0]) - float(got[3, 0])) <= 2 * (n + 3) * U and torch.equal(again_counts, counts)
    for b in range(6):                                                  # the neighbours of the NaN row are unaffected
        alone, alone_counts = device_complexity(rows[b:b + 1])
        assert same_bits(alone, got[b:b + 1]) and torch.equal(alone_counts, counts[b:b + 1]), b


# ------------------------------------------------------------------------------------------------ graph capture
def test_captured_calls_replay_equal_eager():
    """Noise, distance and complexity on one stream under one capture; two replays on different inputs equal eager: no call
    reads back, synchronises or issues a memset node."""
    ops, _ = te()
    from transformer_explainability_amd.generators import GraphedCall

    def fn(x, m):
        copies = ops.noise_inputs(x, 3, 0.05, 7, id0=2)
        c16 = ops.noise_inputs(x, 2, 0.05, 7, id0=2, d0=1, out_dtype=BF)
        d = ops.map_distance(x, copies)
        d16 = ops.map_distance(x, c16)
        out, counts = ops.map_complexity(m)
        return torch.cat([copies.double().flatten(), c16.double().flatten(), d.flatten(), d16.flatten(), out.flatten(),
                          counts.double().flatten()])

    args = [(inputs(2, 1025, seed=s).to(dev()), maps(2, 197, seed=s).to(dev())) for s in (1, 2)]
    want = []
    for a in args:
        out = fn(*a)
        torch.cuda.synchronize()
        want.append(out.clone())
    assert not torch.equal(want[0], want[1])
    call = GraphedCall(fn, args[0])
    for i in (1, 0):
        got = call(*args[i])
        torch.cuda.synchronize()
        assert same_bits(got, want[i]), i


# ------------------------------------------------------------------------------------------------ the evaluator
def small_vit(dtype):
    from transformer_explainability_amd import vit
    torch.manual_seed(0)
    m = vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=16,
                              qkv_bias=True).eval()
    return m.to(dev()).to(dtype)


def small_vit_evaluator(dtype):
    """(run(seed, radius) -> an evaluator after one update of B = 3 images, four draws in passes of two; the images)"""
    _, R = te()
    from transformer_explainability_amd.generators import LRP
    lrp = LRP(small_vit(dtype))
    x = inputs(3, 3 * 64 * 64, seed=4).reshape(3, 3, 64, 64).to(dev())

    def run(seed, radius=0.05, draws_per_pass=2):
        ev = R.SensitivityEvaluator(lrp, n_draws=4, radius=radius, seed=seed, draws_per_pass=draws_per_pass, keep_last=True)
        ev.update(x)
        torch.cuda.synchronize()
        return ev
    return run, x


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_evaluator_on_a_small_vit(dtype):
    """B = 3, four draws in passes of two.  The per-sample numbers equal reference_scores / reference_complexity applied to
    the device's own maps and inputs within the bounds of the sums they are made of: a score is a quotient of square roots
    of two sums, each within 2 (n + 2) u of its restatement -- half of that after the root, the two halves add in the
    quotient, and the roots, the quotient and the mean add a few u: 2 (n_map + n_input + 4) u + 8 u covers every score."""
    _, R = te()
    run, x = small_vit_evaluator(dtype)
    ev = run(seed=1)
    got, kept = ev.arrays(), ev.last
    n_map, n_in = kept["map0"].shape[1], 3 * 64 * 64
    assert kept["maps"].shape == (3, 4, n_map) and kept["copies"].shape == (3, 4, 3, 64, 64) and kept["copies"].dtype == dtype
    assert same_bits(kept["x0"].cpu(), x.to(dtype).float().cpu())       # the input the model saw, upcast exactly
    assert same_bits(kept["copies"].cpu(), R.reference_noise(kept["x0"].cpu(), 4, 0.05, seed=1, out_dtype=dtype))
    assert kept["ref"].shape == kept["maps"].shape                      # the clean map every copy's map is compared with
    want = R.reference_scores(kept["map0"].cpu(), kept["maps"].cpu(), kept["x0"].cpu(), kept["copies"].cpu(), ref=kept["ref"].cpu())
    tol = 2 * (n_map + n_in + 4) * U + 8 * U
    for name in ("max_sens", "avg_sens", "lipschitz"):
        w = want[name].numpy()
        rel = np.abs(got[name] - w) / np.abs(w)
        print(f"evaluator {dtype} {name}: {got[name]}, max rel err {rel.max():.3e}, bound {tol:.3e}")
        assert np.isfinite(w).all() and (w > 0).all() and (rel <= tol).all(), (name, got[name], w)
    out, counts = R.reference_complexity(kept["map0"].cpu())
    assert np.array_equal(got["n_eff"], counts[:, 0].numpy())
    assert (np.abs(got["gini"] - out[:, 0].numpy()) <= 2 * (n_map + 3) * U).all()
    assert (np.abs(got["entropy"] - out[:, 1].numpy()) <= 4 * (n_map + 4) * U * max(1.0, math.log(n_map))).all()
    assert ev.summary()["samples"] == 3

    # the same seed: the same bits; another seed: other numbers
    again = run(seed=1).arrays()
    assert all(np.array_equal(again[k], got[k]) for k in got)
    other = run(seed=2).arrays()
    assert not np.array_equal(other["max_sens"], got["max_sens"]) and np.array_equal(other["gini"], got["gini"])


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_evaluator_radius_zero_copies_have_the_clean_map(dtype):
    """radius = 0: the copies are the clean inputs bit for bit, so every copy's map is the clean map bit for bit and
    max_sens == 0.  That needs the two maps to come from launches of the same shapes: a sample's map is NOT the same bits in
    a batch of 3 and in a batch of 6 (the stock convolution of the patch embedding picks its kernel by problem size; measured
    here on the fp32 model: maps up to 1.5e-3 relative apart), which is why the evaluator compares a pass of copies with a
    reference pass of the clean images in the same shape.  Asserted: with two draws per pass, every copy's map equals the
    clean map of its row of the reference pass; with one draw per pass, where the clean batch is its own reference, every
    copy's map equals the clean batch's map."""
    run, x = small_vit_evaluator(dtype)
    for draws_per_pass in (2, 1):
        ev0 = run(seed=1, radius=0.0, draws_per_pass=draws_per_pass)
        k0 = ev0.last
        n_map = k0["map0"].shape[1]
        assert same_bits(k0["copies"].cpu(), x.to(dtype)[:, None].expand(3, 4, 3, 64, 64).contiguous().cpu())
        apart = ((k0["ref"] - k0["map0"][:, None]).abs() / k0["map0"][:, None].abs().clamp_min(1e-30)).max()
        print(f"evaluator {dtype} radius 0, {draws_per_pass} draws per pass: reference maps against the clean batch's maps, "
              f"max rel difference {float(apart):.3e}; max_sens {ev0.arrays()['max_sens']}")
        assert same_bits(k0["maps"].cpu(), k0["ref"].cpu())
        if draws_per_pass == 1:
            assert same_bits(k0["maps"].cpu(), k0["map0"][:, None].expand(3, 4, n_map).contiguous().cpu())
        a0 = ev0.arrays()
        assert a0["max_sens"].tolist() == [0.0] * 3 and a0["avg_sens"].tolist() == [0.0] * 3 and np.isnan(a0["lipschitz"]).all()


def test_evaluator_refuses_token_ids_on_the_device():
    _, R = te()
    from transformer_explainability_amd import TeError
    ev = R.SensitivityEvaluator(object())
    with pytest.raises(TeError, match="discrete"):
        ev.update(torch.zeros((2, 16), dtype=torch.int64, device=dev()))
