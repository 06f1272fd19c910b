"""-m gpu: the faithfulness kernels (csrc/te_faithful.hip) against the restatements of faithfulness.py on the same seeded
inputs.  The perturbed images and the membership must be equal bit for bit; the attribution sums and the weighted sums are
held to the rounding bounds stated at their tests (each test prints what it measured before it asserts)."""
import functools

import numpy as np
import pytest
import torch

from faithfulness_inputs import images, inputs, token_maps
from gpu_util import dev, odd_offset_view
from host_util import same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BF = torch.bfloat16
DTYPES = pytest.mark.parametrize("out_dtype", [torch.float32, BF], ids=["f32", "bf16"])


def te():
    from transformer_explainability_amd import faithfulness, ops
    return ops, faithfulness


# ------------------------------------------------------------------------------------------------ subset inputs
def device_subsets(x, k, grid, seed, **kw):
    ops, _ = te()
    kw = {name: (v.to(dev()) if torch.is_tensor(v) else v) for name, v in kw.items()}
    out, member, attr_sum = ops.subset_inputs(x.to(dev()), k, grid, seed, **kw)
    torch.cuda.synchronize()
    n_d = kw.get("n_draws", 1)
    g_h, g_w = (grid, grid) if isinstance(grid, int) else grid
    assert out.dtype == kw.get("out_dtype", torch.float32) and out.shape == (x.shape[0], n_d) + tuple(x.shape[1:])
    assert member.dtype == torch.uint8 and member.shape == (x.shape[0], n_d, g_h * g_w)
    assert (attr_sum is None) == (kw.get("attr") is None)
    return out.cpu(), member.cpu(), None if attr_sum is None else attr_sum.cpu()


def assert_equals_the_restatement(x, k, grid, seed, what, **kw):
    """out and member bit for bit; attr_sum within 2 G u sum |attr| (both sides add the same exact fp64 upcasts, at most G of
    them, in different orders: (G - 1) u sum |attr| each, Higham section 4.2)"""
    _, F = te()
    got = device_subsets(x, k, grid, seed, **kw)
    want = F.reference_subset_inputs(x, k, grid, seed, **kw)
    assert same_bits(got[0], want[0]), what
    assert torch.equal(got[1], want[1]) and got[1].sum(2).unique().tolist() == [k], what
    if want[2] is not None:
        G = got[1].shape[2]
        bound = 2 * G * U * kw["attr"].double().abs().sum(1, keepdim=True)
        err = (got[2] - want[2]).abs()
        assert got[2].dtype == torch.float64 and bool((err <= bound).all()), (what, float(err.max()), float(bound.min()))
        return float((err / bound).max())
    return 0.0


GRIDS = [((1, 1), (1, 2, 3, 4, 8, 16)), ((1, 2), (1, 2, 3, 4, 8, 16)), ((1, 3), (1, 2, 3, 4, 8, 16)), ((2, 2), (1, 2, 3, 4, 8, 16)),
         ((1, 5), (1, 2, 3, 4, 8, 16)), ((3, 5), (1, 2, 3, 4, 8, 16)), ((14, 14), (1, 8)), ((64, 64), (1,))]


@DTYPES
@pytest.mark.parametrize("grid,ps", GRIDS, ids=["%dx%d" % g for g, _ in GRIDS])
def test_subset_inputs_bits_equal_the_restatement(grid, ps, out_dtype):
    """Every grid of the table, p through the element-wise form (1, 2, 3; bf16 also 4) and the 16-byte form, one and three
    channels, k = 1, G - 1 and G, a substrate tensor and the constants, ids that cross 2^32 (the high counter word)."""
    G = grid[0] * grid[1]
    seed, id0 = 0x9e3779b97f4a7c15, (1 << 32) - 2
    worst = 0.0
    for p in ps:
        for C in (1, 3):
            x = images(3, C, grid[0] * p, grid[1] * p, seed=p + C)
            sub = images(3, C, grid[0] * p, grid[1] * p, seed=100 + p + C)
            attr = token_maps(3, G, seed=p)
            for k in sorted({1, max(1, G - 1), G}):
                base = dict(id0=id0, d0=1, n_draws=3, out_dtype=out_dtype)
                worst = max(worst, assert_equals_the_restatement(x, k, grid, seed, (grid, p, C, k, "substrate"), substrate=sub,
                                                                 attr=attr, **base))
                assert_equals_the_restatement(x, k, grid, seed, (grid, p, C, k, "fill"), fill=[0.25, -1.5, 2.0][:C], **base)
    print(f"subset_inputs {grid} {out_dtype}: worst attr_sum error {worst:.3f} of the bound 2 G u sum |attr|")


@DTYPES
@pytest.mark.parametrize("grid,p", [((3, 5), 3), ((3, 5), 8), ((14, 14), 16), ((64, 64), 1)], ids=["3x5p3", "3x5p8", "14x14p16", "64x64p1"])
def test_subset_inputs_chunks_batches_and_views(grid, p, out_dtype):
    ops, F = te()
    G = grid[0] * grid[1]
    seed, id0, k = 11, (1 << 32) - 1, max(1, G // 4)
    x = images(3, 3, grid[0] * p, grid[1] * p, seed=p)
    sub = images(3, 3, grid[0] * p, grid[1] * p, seed=p + 1)
    attr = token_maps(3, G, seed=p + 2)
    kw = dict(substrate=sub, attr=attr, out_dtype=out_dtype)
    full = device_subsets(x, k, grid, seed, id0=id0, n_draws=4, **kw)
    want = F.reference_subset_inputs(x, k, grid, seed, id0=id0, n_draws=4, **kw)
    assert same_bits(full[0], want[0]) and torch.equal(full[1], want[1])
    assert not torch.equal(full[1][:, 0], full[1][:, 1]) and not torch.equal(full[1][0], full[1][1])
    # chunks of the draws are slices of the full call, attr_sum included: its order is fixed by G alone
    for d0, n_d in ((0, 2), (3, 1)):
        part = device_subsets(x, k, grid, seed, id0=id0, d0=d0, n_draws=n_d, **kw)
        assert all(same_bits(a, b[:, d0:d0 + n_d]) for a, b in zip(part, full)), d0
    # a batch at id0 equals its samples run alone at id0 + b
    for b in range(3):
        alone = device_subsets(x[b:b + 1], k, grid, seed, id0=id0 + b, n_draws=4, substrate=sub[b:b + 1], attr=attr[b:b + 1],
                               out_dtype=out_dtype)
        assert all(same_bits(a, f[b:b + 1]) for a, f in zip(alone, full)), b
    # a substrate equal to x: copies, bit for bit
    same = device_subsets(x, k, grid, seed, n_draws=2, substrate=x, out_dtype=out_dtype)
    assert same_bits(same[0], x[:, None].expand(3, 2, *x.shape[1:]).to(out_dtype).contiguous())
    # x, the substrate and out one element past a 16-byte boundary: the element-wise form gives the bits of the 16-byte form
    xv, sv = odd_offset_view(x), odd_offset_view(sub)
    out = odd_offset_view(want[0], dtype=out_dtype)
    for xs, ss, os_ in ((xv, sv, out), (x.to(dev()), sub.to(dev()), out), (xv, sub.to(dev()), torch.empty_like(want[0], device=dev())),
                        (x.to(dev()), sv, torch.empty_like(want[0], device=dev()))):
        os_.zero_()
        got, member, attr_sum = ops._subset_inputs_into(xs, os_, k, grid, seed, id0=id0, substrate=ss, attr=attr.to(dev()))
        torch.cuda.synchronize()
        assert got.data_ptr() == os_.data_ptr() and same_bits(got.cpu(), full[0]) and same_bits(member.cpu(), full[1])
        assert same_bits(attr_sum.cpu(), full[2])


def test_subset_inputs_refusals_on_device_tensors():
    ops, F = te()
    from transformer_explainability_amd import TeError
    x = images(2, 3, 8, 8).to(dev())
    for bad in (dict(k=0), dict(k=17), dict(grid=3), dict(grid=(2, 4)), dict(n_draws=0), dict(d0=-1), dict(d0=(1 << 32) - 1, n_draws=2),
                dict(seed=1 << 64), dict(id0=-(1 << 63) - 1), dict(fill=None), dict(fill=[0.0] * 2), dict(substrate=x),
                dict(fill=None, substrate=x[:, :2]), dict(attr=x[:, 0, 0]), dict(out_dtype=torch.float16)):
        args = dict(k=4, grid=4, seed=0, fill=[0.0] * 3)
        args.update(bad)
        with pytest.raises(TeError, match="subset_inputs"):
            ops.subset_inputs(x, **args)
    with pytest.raises(TeError, match="4096 cells"):
        ops.subset_inputs(torch.zeros(1, 1, 17, 241, device=dev()), 1, (17, 241), 0, fill=[0.0])
    with pytest.raises(TeError, match="perturbation_dot"):
        ops.perturbation_dot(x.reshape(2, -1), x.reshape(2, 1, -1), x[:, 0, :5].reshape(2, -1))
    # the last draw and the largest seed and id are accepted
    got = ops.subset_inputs(x, 4, 4, (1 << 64) - 1, id0=(1 << 64) - 1, d0=(1 << 32) - 1, fill=[0.0] * 3)
    torch.cuda.synchronize()
    want = F.reference_subset_inputs(x.cpu(), 4, 4, -1, id0=(1 << 64) - 1, d0=(1 << 32) - 1, fill=[0.0] * 3)
    assert same_bits(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


# ------------------------------------------------------------------------------------------------ perturbation dot
def device_dot(x, y, w):
    ops, _ = te()
    s = ops.perturbation_dot(x.to(dev()), y.to(dev()), w.to(dev()))
    torch.cuda.synchronize()
    assert s.dtype == torch.float64 and s.shape == (y.shape[0], y.shape[1], 2)
    return s.cpu()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1023, 1025, 3072])
def test_dot_sums_within_the_rounding_bound(n):
    """|got - want| <= 2 (n + 2) 2^-53 sum |term| for both sums: either side is an fp64 sum of the same n terms -- each formed
    from the same exact upcasts with the same roundings (one for the difference, one for the product) -- in its own order, so
    each is within (n - 1) u sum |term| of the exact sum of those terms (Higham, section 4.2)."""
    ops, F = te()
    from transformer_explainability_amd.robustness import reference_distance
    for m in sorted({n, n // 3} if n % 3 == 0 else {n}):
        for D in (1, 3):
            for dtype in (torch.float32, BF):
                x = inputs(3, n, seed=n + D)
                y = (x[:, None, :] + 0.1 * inputs(3, D * n, seed=n + m).reshape(3, D, n)).to(dtype)
                w = inputs(3, m, seed=m + 7)
                got, want = device_dot(x, y, w), F.reference_dot(x, y, w)
                bound = 2 * (n + 2) * U * F.reference_dot(x, y, w, magnitude=True)
                err = (got - want).abs()
                print(f"dot n {n} m {m} D {D} {dtype}: max err / bound {float((err / bound).max()):.3e}")
                assert bool((err <= bound).all()), (n, m, D, dtype, float((err / bound).max()))
                # a batch equals its samples, bit for bit
                for s in range(3):
                    assert same_bits(device_dot(x[s:s + 1], y[s:s + 1], w[s:s + 1]), got[s:s + 1]), (n, m, D, dtype, s)
                # the second sum has the bits of map_distance's first: the same terms in the same order
                dist = ops.map_distance(x.to(dev()), y.to(dev()))
                torch.cuda.synchronize()
                assert same_bits(got[..., 1], dist.cpu()[..., 0]), (n, m, D, dtype)
                assert bool((dist.cpu()[..., 0] - reference_distance(x, y)[..., 0]).abs().max() <= float(bound[..., 1].max()))
    # y = x: exactly 0
    x = inputs(3, n, seed=n)
    assert same_bits(device_dot(x, x[:, None].expand(3, 2, n).contiguous(), inputs(3, n, seed=1)),
                     torch.zeros(3, 2, 2, dtype=torch.float64))


@pytest.mark.parametrize("n,m", [(5, 5), (64, 64), (1025, 1025), (3072, 1024), (96, 32)])
def test_dot_on_views_off_the_16_byte_boundary(n, m):
    """the element-wise loads give the bits of the 16-byte loads"""
    ops, _ = te()
    x, w = inputs(2, n, seed=n), inputs(2, m, seed=m + 1)
    y = x[:, None, :] + 0.1 * inputs(2, 2 * n, seed=3).reshape(2, 2, n)
    for yt in (y, y.to(BF)):
        ref = device_dot(x, yt, w)
        for xv, yv, wv in ((odd_offset_view(x), odd_offset_view(yt), odd_offset_view(w)), (x.to(dev()), odd_offset_view(yt), w.to(dev())),
                           (odd_offset_view(x), yt.to(dev()), w.to(dev())), (x.to(dev()), yt.to(dev()), odd_offset_view(w))):
            s = ops.perturbation_dot(xv, yv, wv)
            torch.cuda.synchronize()
            assert same_bits(s.cpu(), ref)


# ------------------------------------------------------------------------------------------------ graph capture
def test_captured_calls_replay_equal_eager():
    """Both ops on one stream under one capture; two replays on different inputs equal eager: no call reads back,
    synchronises or issues a memset node."""
    ops, _ = te()
    from transformer_explainability_amd.generators import GraphedCall

    def fn(x, sub, attr, w):
        out, member, attr_sum = ops.subset_inputs(x, 5, (3, 5), 7, id0=2, n_draws=3, substrate=sub, attr=attr)
        o16, m16, _ = ops.subset_inputs(x, 2, (3, 5), 7, id0=2, d0=1, n_draws=2, fill=[0.5, -0.5, 0.0], out_dtype=BF)
        d = ops.perturbation_dot(x, out, w)
        d16 = ops.perturbation_dot(x, o16, w)
        return torch.cat([out.double().flatten(), member.double().flatten(), attr_sum.flatten(), o16.double().flatten(),
                          m16.double().flatten(), d.flatten(), d16.flatten()])

    args = [(images(2, 3, 24, 40, seed=s).to(dev()), images(2, 3, 24, 40, seed=s + 10).to(dev()), token_maps(2, 15, seed=s).to(dev()),
             inputs(2, 24 * 40, seed=s).to(dev())) for s in (1, 2)]
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
@functools.lru_cache(maxsize=None)
def small_vit_lrp(dtype):
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP
    torch.manual_seed(0)
    m = vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=16,
                              qkv_bias=True).eval()
    return LRP(m.to(dev()).to(dtype))


def evaluator(dtype, perturbation, **kw):
    """B = 4 images of 64 x 64 (a 4 x 4 grid of 16 x 16 patches), five draws in passes of two"""
    _, F = te()
    args = dict(perturbation=perturbation, n_draws=5, subset_size=4, baseline="black", radius=0.05, seed=1, draws_per_pass=2,
                keep_last=True)
    args.update(kw)
    return F.FaithfulnessEvaluator(small_vit_lrp(dtype), **args), images(4, 3, 64, 64, seed=4).to(dev())


@pytest.mark.parametrize("output", ["prob", "logit"])
@pytest.mark.parametrize("perturbation", ["subset", "noise"])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_evaluator_on_a_small_vit(dtype, perturbation, output):
    """The copies and the membership equal the CPU path's bit for bit (the restatements on the input the model saw); two
    updates of two images make the copies of one update of four; the product sums are within the dot kernel's bound of
    reference_dot on the device's own tensors, and the scores are scores_from_sums of what was kept."""
    _, F = te()
    from transformer_explainability_amd.robustness import reference_noise
    ev, x = evaluator(dtype, perturbation, output=output)
    ev.update(x)
    torch.cuda.synchronize()
    kept, got = ev.last, ev.arrays()
    x0 = kept["x0"].cpu()
    assert same_bits(x0, x.to(dtype).float().cpu()) and kept["copies"].dtype == dtype and kept["copies"].shape == (4, 5, 3, 64, 64)
    if perturbation == "subset":
        want, member, attr_sum = F.reference_subset_inputs(x0, 4, 4, seed=1, n_draws=5, fill=[-1.0] * 3, attr=kept["map0"].cpu(),
                                                           out_dtype=dtype)
        assert same_bits(kept["copies"].cpu(), want) and torch.equal(kept["member"].cpu(), member)
        assert bool(((kept["attr_sum"].cpu() - attr_sum).abs() <= 2 * 16 * U * kept["map0"].cpu().double().abs().sum(1, keepdim=True)).all())
    else:
        assert same_bits(kept["copies"].cpu(), reference_noise(x0, 5, 0.05, seed=1, out_dtype=dtype)) and kept["member"] is None
    n = 3 * 64 * 64
    heat = kept["heat"].cpu().reshape(4, -1)
    want_ip = F.reference_dot(x0, kept["copies"].cpu().reshape(4, 5, n), heat)[..., 0]
    bound = 2 * (n + 2) * U * F.reference_dot(x0, kept["copies"].cpu().reshape(4, 5, n), heat, magnitude=True)[..., 0]
    err = (kept["ip"].cpu() - want_ip).abs()
    print(f"evaluator {dtype} {perturbation} {output}: ip err / bound {float((err / bound).max()):.3e}; {got}")
    assert bool((err <= bound).all()) and bool(torch.isfinite(kept["delta"]).all()) and float(kept["delta"].abs().max()) > 0
    want = F.scores_from_sums(kept["ip"].cpu(), kept["delta"].cpu(), None if kept["attr_sum"] is None else kept["attr_sum"].cpu())
    # (fp64 torch here and there: five-term sums in two orders; beta's and the correlation's sums may cancel, and a
    # cancelling sum loses its condition number -- 1e-9 leaves room for one of 1e6)
    for name in F.SCORE_NAMES:
        np.testing.assert_allclose(got[name], want[name].numpy(), rtol=1e-9, atol=0, equal_nan=True)
    assert np.isfinite(got["infidelity"]).all() and (got["infidelity_norm"] <= got["infidelity"] * (1 + 1e-12)).all()
    assert np.isnan(got["faith_corr"]).all() == (perturbation == "noise") and ev.summary()["samples"] == 4

    # two updates of two images: the copies of one update of four (sample ids run on)
    two, _ = evaluator(dtype, perturbation, output=output)
    parts = []
    for lo in (0, 2):
        two.update(x[lo:lo + 2])
        parts.append((two.last["copies"], two.last["member"]))
    torch.cuda.synchronize()
    assert two.last["id0"] == 2 and same_bits(torch.cat([c for c, _ in parts], 0).cpu(), kept["copies"].cpu())
    if perturbation == "subset":
        assert torch.equal(torch.cat([m for _, m in parts], 0).cpu(), kept["member"].cpu())


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
def test_evaluator_unchanged_copies_drop_nothing(dtype):
    """radius = 0, and k = G patches of a substrate equal to the image (pixel value 1 everywhere: 1 in the normalised space
    of mean 0.5 and std 0.5, too): the copies are the clean images bit for bit, the reference pass has the shape of a pass of
    copies, so the drop is exactly 0 and so is the infidelity; beta is 1 by its rule."""
    ev, x = evaluator(dtype, "noise", radius=0.0)
    ev.update(x)
    torch.cuda.synchronize()
    a = ev.arrays()
    assert same_bits(ev.last["copies"].cpu(), x.to(dtype)[:, None].expand(4, 5, 3, 64, 64).contiguous().cpu())
    assert same_bits(ev.last["delta"].cpu(), torch.zeros(4, 5, dtype=torch.float64))
    assert a["infidelity"].tolist() == [0.0] * 4 == a["infidelity_norm"].tolist() and a["beta"].tolist() == [1.0] * 4
    ev, _ = evaluator(dtype, "subset", subset_size=16, baseline=(1.0, 1.0, 1.0))
    ones = torch.ones_like(x)
    ev.update(ones)
    torch.cuda.synchronize()
    assert same_bits(ev.last["copies"].cpu(), ones.to(dtype)[:, None].expand(4, 5, 3, 64, 64).contiguous().cpu())
    assert ev.last["member"].all()
    assert same_bits(ev.last["delta"].cpu(), torch.zeros(4, 5, dtype=torch.float64)) and ev.arrays()["infidelity"].tolist() == [0.0] * 4
    assert np.isnan(ev.arrays()["faith_corr"]).all()                     # the drop is 0 in every draw: a constant side


def test_evaluator_refuses_token_ids_on_the_device():
    _, F = te()
    from transformer_explainability_amd import TeError
    ev = F.FaithfulnessEvaluator(object())
    with pytest.raises(TeError, match="discrete"):
        ev.update(torch.zeros((2, 16), dtype=torch.int64, device=dev()))
