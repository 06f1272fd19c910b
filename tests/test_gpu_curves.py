"""-m gpu: the deletion / insertion curve kernels (csrc/te_curves.hip) against the torch restatements of curves.py on CPU copies
of the same seeded inputs.  Ranks and step images must be equal bit for bit; the blur, the scores and the AUC are held to the
rounding bounds derived at their tests (each test prints what it measured before it asserts)."""
import numpy as np
import pytest
import torch

from curves_inputs import MEAN, STD, Stub, images, logits as make_logits, relevance, special_rows, tie_example, upsampled_map
from gpu_util import dev, odd_offset_view
from host_util import same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TILE = 32                                  # csrc/te_curves.hip: kTile, the blur's outputs per tile side


def te():
    from transformer_explainability_amd import curves, ops
    return ops, curves


# ------------------------------------------------------------------------------------------------ rank
def device_ranks(vis):
    ops, _ = te()
    r = ops.pixel_ranks(vis.to(dev()))
    torch.cuda.synchronize()
    assert r.dtype == torch.int32 and r.shape == (vis.shape[0], vis[0].numel())
    return r.cpu()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 50176])
def test_ranks_equal_the_stable_sort(n):
    _, curves = te()
    vis = relevance(3, n, seed=n)
    assert torch.equal(device_ranks(vis), curves.reference_ranks(vis))


@pytest.mark.parametrize("n", [12, 1025, 4097])
def test_ranks_of_ties_zeros_infinities_and_sorted_rows(n):
    _, curves = te()
    vis = tie_example() if n == 12 else special_rows(n)
    got = device_ranks(vis)
    assert torch.equal(got, curves.reference_ranks(vis))
    if n != 12:
        assert got[0].tolist() == list(range(n))                                 # a constant row: rank == index
        assert got[3].tolist() == list(range(n))                                 # already descending
        # a batch equals its samples run alone
        for b in range(vis.shape[0]):
            assert torch.equal(device_ranks(vis[b:b + 1])[0], got[b]), b


def test_ranks_of_an_upsampled_patch_map():
    _, curves = te()
    vis = upsampled_map(B=2)
    assert vis.shape == (2, 224 * 224) and torch.unique(vis[0]).numel() < vis.shape[1]      # the replicated borders tie
    assert torch.equal(device_ranks(vis), curves.reference_ranks(vis))


# ------------------------------------------------------------------------------------------------ blur
def device_blur(data, klen, nsig=5.0, mean=MEAN, std=STD, view=False):
    ops, _ = te()
    d = odd_offset_view(data) if view else data.to(dev())
    out = ops.gaussian_blur(d, klen, nsig, mean, std)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == data.shape
    return out.cpu()


def assert_blur_within_bound(data, klen, nsig=5.0, mean=MEAN, std=STD, view=False, what=""):
    """|got - blur_fp64(z)| <= gamma_m blur_fp64(|z|), m = 2 klen + 4, gamma_m = m 2^-24 / (1 - m 2^-24), at EVERY element.

    Derivation.  The restatement takes the same fp32 z and the same fp32 taps, so only the sums differ.  The horizontal pass is
    a chain of klen FMAs from a zero accumulator: klen roundings, |h_fp32 - h| <= gamma_klen sum_j t_j |z_j| (Higham, Accuracy
    and Stability, section 3.1; 2^-24 is the unit roundoff of fp32).  The vertical pass is the same chain over h_fp32:
    |got - v| <= ((1 + gamma_klen)^2 - 1) sum_i t_i sum_j t_j |z_ij| <= gamma_{2 klen} blur(|z|).  The four further roundings cover
    the restatement itself: its 2-D kernel rounds t_i t_j once in fp64 and sums in fp64, orders of magnitude below one fp32
    rounding each.  Zero padding adds exact zeros on both sides."""
    _, curves = te()
    got = device_blur(data, klen, nsig, mean, std, view).double()
    want = curves.reference_blur(data, klen, nsig, mean, std)
    scale = curves.reference_blur(data, klen, nsig, mean, std, magnitude=True)
    m = 2 * klen + 4
    gamma = m * 2.0 ** -24 / (1 - m * 2.0 ** -24)
    err = (got - want).abs()
    worst = float((err / scale.clamp_min(1e-300)).max())
    print(f"blur {what or tuple(data.shape)} klen {klen}: max err / blur(|z|) = {worst:.3e}, bound {gamma:.3e}")
    assert bool((err <= gamma * scale).all()), (what, worst, gamma)
    return got


@pytest.mark.parametrize("shape,klen", [
    ((2, 3, 7, 9), 11),                                                          # the kernel is wider than the image; W % 4 != 0
    ((1, 1, 16, 16), 11),
    ((1, 2, TILE - 1, TILE + 1), 11), ((1, 2, TILE, TILE), 11), ((1, 2, TILE + 1, TILE - 1), 11),
    ((2, 1, 2 * TILE, 2 * TILE + 4), 11), ((1, 1, 2 * TILE + 1, 2 * TILE - 4), 3),
    ((1, 3, 20, 30), 3), ((1, 1, 40, 44), 1), ((1, 1, 40, 44), 31), ((1, 1, 35, 37), 31), ((1, 1, 33, 36), 63),
])
def test_blur_within_the_rounding_bound(shape, klen):
    C = shape[1]
    assert_blur_within_bound(images(*shape, seed=klen), klen, mean=MEAN[:C], std=STD[:C])


def test_blur_of_a_view_at_an_odd_element_offset():
    data = images(2, 3, 36, 40, seed=9)
    got = assert_blur_within_bound(data, 11, view=True, what="odd offset")
    assert same_bits(got.float(), device_blur(data, 11))                         # the element-wise form gives the same bits


def test_blur_of_an_impulse_is_the_outer_product_of_the_taps():
    _, curves = te()
    for klen, nsig in ((11, 5.0), (3, 0.8), (31, 5.0)):
        r = klen // 2
        data = torch.zeros(1, 1, 70, 72)
        y, x = 33, 31                                                            # its footprint crosses tile seams
        data[0, 0, y, x] = 1.0
        got = device_blur(data, klen, nsig, None, None)
        t = torch.from_numpy(curves.gaussian_taps(klen, nsig).astype(np.float32))
        want = torch.zeros_like(data)
        want[0, 0, y - r:y + r + 1, x - r:x + r + 1] = t[:, None] * t[None, :]   # one rounding per element, as the one FMA
        assert same_bits(got, want), klen


def test_blur_of_a_constant_image_is_the_constant_inside():
    c, klen = 0.7, 11
    data = torch.full((1, 1, 48, 52), c)
    got = assert_blur_within_bound(data, klen, mean=None, std=None, what="constant")
    r = klen // 2
    m = 2 * klen + 4
    gamma = m * 2.0 ** -24 / (1 - m * 2.0 ** -24)
    inside = got[0, 0, r:-r, r:-r]
    # (the fp32 taps sum to 1 within 2^-25 each way, their square within 2^-24: inside gamma_m)
    assert float((inside - float(np.float32(c))).abs().max()) <= gamma * c


def test_blur_batch_equals_samples_and_tile_position_does_not_matter():
    data = images(3, 2, 37, 41, seed=4)
    whole = device_blur(data, 11, mean=MEAN[:2], std=STD[:2])
    for b in range(3):
        assert same_bits(device_blur(data[b:b + 1], 11, mean=MEAN[:2], std=STD[:2])[0], whole[b]), b
    # the same image at two places of a zero canvas (zero in normalised space: mean / std = None)
    img = images(1, 1, 20, 24, seed=5)
    out = []
    for (y, x) in ((6, 8), (29, 27)):
        canvas = torch.zeros(1, 1, 70, 72)
        canvas[0, 0, y:y + 20, x:x + 24] = img[0, 0]
        blurred = device_blur(canvas, 11, 5.0, None, None)
        out.append(blurred[0, 0, y - 5:y + 25, x - 5:x + 29].clone())              # the image and the reach of the kernel
    assert same_bits(out[0], out[1])


# ------------------------------------------------------------------------------------------------ compose
def compose_case(H, W, step, s0, n_s, mode, use_tensor, out_dtype, view=False, B=2, C=3, seed=0):
    ops, curves = te()
    data, vis = images(B, C, H, W, seed=seed), relevance(B, H * W, seed=seed)
    vis[0, : min(5, H * W)] = vis[0, 0]                                           # ties
    ranks = curves.reference_ranks(vis)
    sub = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 11)) if use_tensor else None
    fill = None if use_tensor else [0.25, -1.5, 0.0, 2.0][:C]
    want = curves.reference_inputs(data, ranks, step, s0, n_s, mode, substrate=sub, fill=fill, mean=MEAN[:C], std=STD[:C],
                                   out_dtype=out_dtype)
    put = odd_offset_view if view else (lambda t: t.to(dev()))
    got = ops.curve_inputs(put(data), put(ranks), step, s0, n_s, mode, substrate=None if sub is None else put(sub), fill=fill,
                           mean=MEAN[:C], std=STD[:C], out_dtype=out_dtype)
    torch.cuda.synchronize()
    assert same_bits(got, want), (H, W, step, s0, n_s, mode, use_tensor, out_dtype, view)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,step", [(7, 9, 10), (8, 8, 16), (25, 40, 300), (32, 32, 100)])      # HW = 63, 64, 1000, 1024
def test_step_images_equal_the_restatement(H, W, step, out_dtype):
    S = -(-(H * W) // step)
    for mode, use_tensor in (("deletion", True), ("insertion", False), ("deletion", False), ("insertion", True)):
        compose_case(H, W, step, 0, S + 1, mode, use_tensor, out_dtype)          # all images, the last one with k = HW
        compose_case(H, W, step, S, 1, mode, use_tensor, out_dtype, seed=1)      # the last image alone
        compose_case(H, W, step, 1, S - 1, mode, use_tensor, out_dtype, seed=2)  # s0 != 0
    compose_case(H, W, step, 1, S, "insertion", True, out_dtype, view=True, seed=3)      # unaligned views: element-wise


@pytest.mark.parametrize("out_dtype,B", [(torch.float32, 21), (torch.bfloat16, 41)], ids=["f32", "bf16"])
def test_step_images_when_one_thread_walks_all_steps(out_dtype, B):
    """224 x 224 with enough samples that the batch alone fills the chip: the launch keeps all images of the call in one thread
    (bx * B >= 1024 blocks), the other grid split of the kernel."""
    compose_case(224, 224, 20000, 1, 3, "deletion", True, out_dtype, B=B, C=1, seed=6)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_deletion_to_black_is_the_shipped_perturbation_kernel(out_dtype):
    ops, curves = te()
    data, vis = images(2, 3, 25, 40, seed=7), relevance(2, 1000, seed=7)
    vis[1, 90:130] = vis[1, 3]                                                    # ties across a step boundary
    d, v = data.to(dev()), vis.to(dev())
    got = ops.curve_inputs(d, ops.pixel_ranks(v), 100, 1, 9, "deletion", fill=curves.substrate_fill("black", 3, MEAN, STD),
                           mean=MEAN, std=STD, out_dtype=out_dtype)
    want = ops.perturb(v, d, list(range(100, 1000, 100)), MEAN, STD, out_dtype=out_dtype)
    torch.cuda.synchronize()
    assert same_bits(got, want)


# ------------------------------------------------------------------------------------------------ scores / auc
def scores_bound(logits):
    """Relative bound of |p_device - p_torch| per row, first order in u = 2^-53.

    Device: p = e_t / sum_k e_k with e_k = exp(fl(x_k - m)), m the row's maximum (exact on both sides).  The subtraction rounds
    once: the argument is off by at most A u, A = max - min of the row, which moves e_k by a factor 1 + A u; the device's fp64
    exp is documented at 1 ulp = 2 u (ROCm device-library accuracy table): e_k is within (A + 2) u.  The K positive terms are
    summed with K - 1 additions in whatever order: (K - 1) u more on the sum; the division rounds once.  Together
    (A + 2) u [numerator] + (A + 2) u [terms of the sum] + (K - 1) u + u = (2 A + K + 4) u.  torch.softmax on the double logits
    runs the same expression (its vectorised exp is a 1-ulp routine as well) and owes the same amount: twice that in all."""
    x = logits.double()
    A = x.max(-1).values - x.min(-1).values
    return 2 * (2 * A + logits.shape[-1] + 4) * U


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [2, 7, 1000, 1001])
def test_scores_within_the_rounding_bound(K, dtype):
    ops, curves = te()
    B, n_s, s0, S1 = 4, 3, 1, 5
    x = make_logits(n_s * B, K, seed=K)
    for row, (first, last) in {0: (80.0, -80.0), 1: (80.0, -80.0), 4: (-80.0, 80.0), 5: (-80.0, 80.0)}.items():
        x[row, 0], x[row, K - 1] = first, last                                   # rows 0, 1, 4, 5 are samples 0, 1: targets 0 and K - 1,
                                                                                 # so p is next to 1 and next to exp(-160) at both
    x = x.to(dtype)
    target = torch.tensor([0, K - 1, K // 2, K - 1])
    prob = torch.full((S1, B), -1.0, dtype=torch.float64, device=dev())
    out = ops.curve_scores(x.to(dev()).reshape(n_s, B, K), target.to(dev()), prob, s0)
    torch.cuda.synchronize()
    assert out is prob
    got = prob.cpu()
    assert bool((got[0] == -1).all()) and bool((got[4] == -1).all())            # rows outside s0 .. s0 + n_s - 1 are not touched
    want = curves.reference_scores(x, target)
    assert torch.equal(want, torch.softmax(x.double(), -1).reshape(n_s, B, K)[:, torch.arange(B), target])
    bound = scores_bound(x).reshape(n_s, B)
    rel = (got[s0:s0 + n_s] - want).abs() / want
    print(f"scores K {K} {dtype}: max rel err {float(rel.max()):.3e}, smallest bound {float(bound.min()):.3e}; "
          f"p from {float(want.min()):.3e} to {float(want.max()):.3e}")
    assert bool((want > 0).all()) and bool((rel <= bound).all()), (rel, bound)


@pytest.mark.parametrize("S,B", [(1, 1), (2, 3), (225, 64), (1000, 257)])
def test_auc_within_the_rounding_bound(S, B):
    ops, curves = te()
    prob = torch.rand((S + 1, B), dtype=torch.float64, generator=torch.Generator().manual_seed(S))
    got = ops.curve_auc(prob.to(dev()))
    torch.cuda.synchronize()
    want = curves.reference_auc(prob)
    rel = (got.cpu() - want).abs() / want
    print(f"auc S {S}: max rel err {float(rel.max()):.3e}, bound {(S + 2) * U:.3e}")
    assert got.dtype == torch.float64 and got.shape == (B,)
    assert bool((rel <= (S + 2) * U).all())


# ------------------------------------------------------------------------------------------------ the evaluator
class Recorder(torch.nn.Module):
    """The stub behind a wrapper that keeps CPU copies of what it saw and what it answered."""

    def __init__(self, dtype):
        super().__init__()
        self.stub = Stub(dtype)

    def forward(self, x):
        return self.stub(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_evaluator_on_the_device(dtype):
    """B = 3, 16 x 16, 37 pixels per step (S = 7), chunks of two steps.  The images the classifier saw must be the restatement's
    bit for bit (given the device's blur as the substrate: the blur itself is held to its own bound above), and the scores
    must be the restatement's scores of the logits the classifier gave, within the scores bound; then the AUC within its
    bound, and a second batch is appended."""
    ops, curves = te()
    B, H, W, step = 3, 16, 16, 37
    S = 7
    data, vis = images(B, 3, H, W, seed=1), relevance(B, H * W, seed=1).reshape(B, 1, H, W)
    vis[1, 0, 3] = vis[1, 0, 2]
    target = torch.tensor([0, 2, 1])
    model = Recorder(dtype).to(dev())
    ev = curves.CurveEvaluator(model, step=step, mean=MEAN, std=STD, max_forward_batch=7)
    ev.update(data.to(dev()), vis.to(dev()), target.to(dev()))
    torch.cuda.synchronize()
    seen, said = model.stub.seen, model.stub.said
    assert len(seen) == 2 * 4 and all(x.dtype == dtype and x.shape[0] <= 6 for x in seen)
    arrs = ev.arrays()
    ranks = curves.reference_ranks(vis)
    blurred = ops.gaussian_blur(data.to(dev()), 11, 5.0, MEAN, STD).cpu()
    for m, (mode, sub) in enumerate((("deletion", dict(fill=[0.0] * 3)), ("insertion", dict(substrate=blurred)))):
        want_x = curves.reference_inputs(data, ranks, step, 0, S + 1, mode, mean=MEAN, std=STD, out_dtype=dtype, **sub)
        got_x = torch.cat([x.cpu() for x in seen[4 * m:4 * m + 4]], 0).reshape(S + 1, B, 3, H, W)
        assert same_bits(got_x, want_x), mode
        logits = torch.cat([y.cpu() for y in said[4 * m:4 * m + 4]], 0)
        want = curves.reference_scores(logits, target)
        got = torch.from_numpy(arrs[f"{mode}_scores.npy"])
        assert got.shape == (S + 1, B) and got.dtype == torch.float64
        rel = (got - want).abs() / want
        bound = scores_bound(logits).reshape(S + 1, B)
        print(f"evaluator {mode} {dtype}: scores max rel err {float(rel.max()):.3e}, smallest bound {float(bound.min()):.3e}")
        assert bool((rel <= bound).all()), mode
        auc, want_auc = torch.from_numpy(arrs[f"{mode}_auc.npy"]), curves.reference_auc(got)
        assert bool(((auc - want_auc).abs() <= (S + 2) * U * want_auc).all()), mode
    ev.update(data[:2].to(dev()), vis[:2].to(dev()), target[:2].to(dev()))
    again = ev.arrays()
    assert again["deletion_scores.npy"].shape == (S + 1, 5) and again["insertion_auc.npy"].shape == (5,)
    assert np.array_equal(again["insertion_scores.npy"][:, :3], arrs["insertion_scores.npy"])
    assert np.array_equal(again["insertion_scores.npy"][:, 3:], arrs["insertion_scores.npy"][:, :2])      # batch-independent


def test_captured_calls_replay_equal_eager():
    """Rank, blur, compose and scores on one stream under one capture; two replays on different inputs equal eager: no call
    reads back, synchronises or issues a memset node."""
    ops, _ = te()
    from transformer_explainability_amd.generators import GraphedCall
    B, H, W, step = 2, 20, 24, 100
    S = 5

    def fn(data, vis, target):
        ranks = ops.pixel_ranks(vis)
        blurred = ops.gaussian_blur(data, 11, 5.0, MEAN, STD)
        x = ops.curve_inputs(data, ranks, step, 0, S + 1, "insertion", substrate=blurred, mean=MEAN, std=STD)
        prob = torch.empty((S + 1, B), dtype=torch.float64, device=data.device)
        ops.curve_scores(x.mean((3, 4)), target, prob, 0)
        return torch.cat([ranks.double().flatten(), blurred.double().flatten(), x.double().flatten(), prob.flatten(),
                          ops.curve_auc(prob)])

    inputs = [(images(B, 3, H, W, seed=s).to(dev()), relevance(B, H * W, seed=s).to(dev()),
               torch.tensor([s % 3, 2 - s % 3]).to(dev())) for s in (1, 2)]
    want = []
    for args in inputs:
        out = fn(*args)
        torch.cuda.synchronize()
        want.append(out.clone())
    assert not torch.equal(want[0], want[1])
    call = GraphedCall(fn, inputs[0])
    for i in (1, 0):
        got = call(*inputs[i])
        torch.cuda.synchronize()
        assert same_bits(got, want[i]), i
