"""-m gpu: ops.map_similarity (te_map_similarity_f32: the rank kernel and the reduce kernel) against sanity.map_similarity on CPU
copies.  The integer rank sums must be equal exactly; the Spearman columns within 4 ulp of fp64 (one sqrt pair, one multiply and
one divide on two implementations; the test prints the largest distance it saw); Pearson within 8 n 2^-53 and SSIM within 1e-9
absolute, the bounds of the CPU suite.  Then the properties of the header: a batch equals its samples, a NaN sample leaves its
neighbours alone, the workspace's place and content do not matter, the refusals launch nothing, a HIP graph captures the call."""
import numpy as np
import pytest
import torch

from gpu_util import dev
from host_util import bits
from mapsim_inputs import FAMILIES, family, images

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def ulps(got, want):
    """Distance in units of the last place of the larger magnitude (NaN positions must agree and count 0)."""
    g, w = got.double().numpy(), want.double().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(w)), (g, w)
    ok = ~np.isnan(g)
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(g[ok] - w[ok]) / np.spacing(np.maximum(np.abs(g[ok]), np.abs(w[ok])))))


def run(a, b, shape=None, data_range=1.0):
    from transformer_explainability_amd import ops
    sums, sim = ops.map_similarity(a.to(dev()), b.to(dev()), shape=shape, data_range=data_range)
    torch.cuda.synchronize()
    return sums.cpu(), sim.cpu()


def assert_matches(a, b, shape=None, what=""):
    from transformer_explainability_amd import sanity
    got_sums, got = run(a, b, shape)
    want_sums, want = sanity.map_similarity(a, b, shape)
    n = a[0].numel()
    assert got_sums.dtype == torch.int64 and got_sums.shape == (a.shape[0], 2, 3) and got.dtype == torch.float64
    assert torch.equal(got_sums, want_sums), (what, got_sums, want_sums)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, got, want)
    rho = ulps(got[:, 1:3], want[:, 1:3])
    assert rho <= 4, (what, rho)
    g, w = torch.nan_to_num(got), torch.nan_to_num(want)
    pearson, ssim = float((g[:, 0] - w[:, 0]).abs().max()), float((g[:, 3] - w[:, 3]).abs().max())
    assert pearson <= 8 * n * EPS, (what, pearson)
    assert ssim <= 1e-9, (what, ssim)
    return rho, pearson, ssim


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 196, 255, 256, 257, 1024, 1025, 4096, 4097])
def test_kernel_against_the_restatement(n):
    worst = [0.0, 0.0]
    for kind in FAMILIES:
        a, b = family(kind, n)
        rho, pearson, _ = assert_matches(a, b, what=(kind, n))
        worst = [max(worst[0], rho), max(worst[1], pearson)]
    print(f"n = {n}: spearman within {worst[0]:.1f} ulp, pearson within {worst[1]:.2e} (bound {8 * n * EPS:.2e})")


@pytest.mark.parametrize("H,W", [(7, 7), (8, 7), (14, 14), (15, 17)])
def test_ssim_sizes(H, W):
    a, b = images(H, W, B=3)
    _, _, ssim = assert_matches(a, b, what=(H, W))                       # 3-D maps
    assert_matches(a.flatten(1), b.flatten(1), shape=(H, W), what=(H, W, "shape="))
    assert_matches(a * 3.0, b * 3.0, what=(H, W, "range"))               # values outside [0, 1] change nothing structural
    from transformer_explainability_amd import sanity
    got = run(a * 255.0, b * 255.0, data_range=255.0)[1][:, 3]
    assert float((got - sanity.ssim(a * 255.0, b * 255.0, 255.0)).abs().max()) <= 1e-9
    assert torch.isnan(run(a.flatten(1), b.flatten(1))[1][:, 3]).all()   # no shape: no SSIM
    print(f"ssim {H}x{W}: max |kernel - torch| = {ssim:.3e}")


def test_image_sized_maps_with_ssim():
    a, b = images(224, 224, B=2)
    a[1] = (a[1] * 4).round() / 4                                        # the second pair with heavy ties
    print("224 x 224: spearman ulp, pearson, ssim =", assert_matches(a, b, what="224"))


def test_largest_n():
    n = 1 << 20
    g = torch.Generator().manual_seed(20)
    a = torch.randn((1, n), generator=g)
    b = (a + torch.randn((1, n), generator=g)).round(decimals=2)         # ties on one side
    print("n = 2^20: spearman ulp, pearson, ssim =", assert_matches(a, b, what="2^20"))


def test_batch_equals_samples_and_nan_leaves_neighbours_alone():
    for n, shape in ((65, None), (4097, None), (15 * 17, (15, 17))):
        a, b = family("ties", n, B=3, seed=1)
        a[0], b[2] = family("distinct", n, B=1, seed=2)[0][0], family("zeros", n, B=1, seed=3)[1][0]
        sums, sim = run(a, b, shape)
        for i in range(3):
            s1, m1 = run(a[i:i + 1], b[i:i + 1], shape)
            assert torch.equal(s1[0], sums[i]) and torch.equal(bits(m1[0]), bits(sim[i])), (n, i)
        a2 = a.clone()
        a2[1, n // 2] = float("nan")
        sums2, sim2 = run(a2, b, shape)
        assert torch.isnan(sim2[1]).all() and not sums2[1].any()
        for i in (0, 2):
            assert torch.equal(sums2[i], sums[i]) and torch.equal(bits(sim2[i]), bits(sim[i])), (n, i)


def raw_call(a, b, ws, shape=None, data_range=1.0):
    """The C ABI with a workspace of the caller's: (status, rank_sums, sim)."""
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    B, n = a.shape[0], a[0].numel()
    sums = torch.full((B, 2, 3), -7, dtype=torch.int64, device=dev())
    sim = torch.full((B, 4), -7.0, dtype=torch.float64, device=dev())
    H, W = shape or (0, 0)
    rc = lib.te_map_similarity_f32(a.data_ptr(), b.data_ptr(), sums.data_ptr(), sim.data_ptr(), B, n, H, W,
                                   _lib.TE_MAPSIM_SSIM if shape else 0, data_range, ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, sums.cpu(), sim.cpu()


def test_workspace_place_and_content_do_not_matter():
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    n, shape = 15 * 17, (15, 17)
    a, b = (t.to(dev()) for t in family("ties", n, B=3, seed=4))
    need = lib.te_map_similarity_workspace_bytes(3, n)
    want = run(a, b, shape)
    for offset, fill in ((0, 0), (8, 0xff), (264, 0x5a)):
        buf = torch.full((need + 512,), fill, dtype=torch.uint8, device=dev())
        rc, sums, sim = raw_call(a, b, buf[offset:offset + need], shape)
        assert rc == 0 and torch.equal(sums, want[0]) and torch.equal(bits(sim), bits(want[1])), (offset, fill)
        assert bool((buf[offset + need:] == fill).all()) and bool((buf[:offset] == fill).all())      # nothing written outside


def test_refusals_launch_nothing():
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    a, b = (t.to(dev()) for t in family("distinct", 64))
    need = lib.te_map_similarity_workspace_bytes(3, 64)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev())
    rc, sums, sim = raw_call(a, b, ws[:need - 256])
    assert rc == _lib.TE_ERR_WORKSPACE and bool((sums == -7).all()) and bool((sim == -7).all())      # outputs untouched
    st = torch.cuda.current_stream().cuda_stream
    big = (1 << 20) + 1
    assert lib.te_map_similarity_f32(a.data_ptr(), b.data_ptr(), ws.data_ptr(), ws.data_ptr(), 1, big, 0, 0, 0, 1.0, ws.data_ptr(),
                                     ws.numel(), st) == _lib.TE_ERR_UNSUPPORTED
    assert lib.te_map_similarity_f32(a.data_ptr(), b.data_ptr(), ws.data_ptr(), ws.data_ptr(), 3, 64, 8, 9, _lib.TE_MAPSIM_SSIM, 1.0,
                                     ws.data_ptr(), ws.numel(), st) == _lib.TE_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert not ws.any()


def test_packed_buffer_and_contiguity():
    from transformer_explainability_amd import ops
    a, b = (t.to(dev()) for t in images(14, 14, B=3))
    sums, sim, flat = ops.map_similarity_packed(a, b)
    torch.cuda.synchronize()
    assert flat.dtype == torch.int64 and flat.shape == (30,)
    host = flat.cpu()
    assert torch.equal(host[:18].view(3, 2, 3), sums.cpu()) and torch.equal(host[18:], bits(sim).flatten())
    wide = torch.zeros((3, 14, 20), device=dev())
    wide[:, :, 3:17] = a                                                 # a strided view is made contiguous
    got = ops.map_similarity(wide[:, :, 3:17], b)
    assert torch.equal(got[0], sums) and torch.equal(bits(got[1]), bits(sim))


def test_captured_call_replays_equal_eager():
    """One capture, two replays on different inputs: the call allocates from the graph's pool, launches two kernels and reads
    nothing back."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import GraphedCall
    pairs = [tuple(t.to(dev()) for t in images(15, 17, B=3, seed=s)) for s in (1, 2)]
    pairs[1][0][1, 3, 3] = float("nan")
    want = []
    for a, b in pairs:
        flat = ops.map_similarity_packed(a, b)[2]
        torch.cuda.synchronize()
        want.append(flat.clone())
    assert not torch.equal(want[0], want[1])
    call = GraphedCall(lambda a, b: ops.map_similarity_packed(a, b)[2], pairs[0])
    for i in (1, 0):
        got = call(*pairs[i])
        torch.cuda.synchronize()
        assert torch.equal(got, want[i]), i
