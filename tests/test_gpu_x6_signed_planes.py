"""The Linear rule's Z-pass on the SIGNED operand planes of X (TE_X6_X_PLANES_SIGNED: |X| is formed while the planes are
staged) against the same call on the planes of |X|, the producers with a NULL |X| plane buffer, and the model path with
ops.X6_SIGNED_PLANES on and off: everything bit for bit.  Plus the identity the kernel relies on, on the CPU."""
import numpy as np
import pytest
import torch

from gpu_util import dev, rnd

gpu = pytest.mark.gpu

# (T, in_f, out_f): ragged 32-row blocks and ragged tiles in every geometry.  The last shape is the smallest one whose feature
# counts divide into the 256 x 256 geometry (out_f % 256 == 0 and in_f % 128 == 0): at the other three TE_X6_TILE_256 falls
# back to 128 x 256 tiles, and the 256 x 256 instantiation of the signed Z-pass would not run.
SHAPES = [(394, 128, 128), (197, 192, 256), (1000, 256, 384), (300, 128, 256)]
ROWS_PER_SAMPLE = {394: 197, 197: 197, 1000: 250, 300: 100}


def _rule_operands(T, in_f, out_f, seed):
    """Mixed signs, +0 and -0, exact bf16 values (zero low planes) of both signs, all-zero rows (of either zero), and one
    (row, feature) pair whose products are all negative: the halves of Z cancel and the kernel takes its exact fallback."""
    X = rnd((T, in_f), seed)
    W = rnd((out_f, in_f), seed + 1, 0.03)
    b = rnd((out_f,), seed + 2, 0.1)
    R = rnd((T, out_f), seed + 3, 1e-3)
    X[0, :8], X[0, 8:16] = 0.0, -0.0
    X[1], X[5] = 0.0, -0.0
    X[3] = X[3].bfloat16().float()
    X[4, ::2] = X[4, ::2].bfloat16().float()
    X[2] = X[2].abs() + 0.01
    W[4] = -W[4].abs() - 0.001
    X[T - 1, 1::3] = 0.0
    X, W, b, R = (t.to(dev()) for t in (X, W, b, R))
    Y = torch.nn.functional.linear(X, W, b)
    return X, W, b, R, Y


@gpu
@pytest.mark.parametrize("T,in_f,out_f", SHAPES)
def test_rule_on_signed_planes_equals_rule_on_abs_planes(T, in_f, out_f):
    from transformer_explainability_amd import ops
    lib = ops._lib.load()
    X, W, b, R, Y = _rule_operands(T, in_f, out_f, 700 + T)
    assert bool((X[2] > 0).all()) and bool((W[4] < 0).all())
    wp = ops.x6_weight_planes(W)
    st = torch.cuda.current_stream().cuda_stream
    nb = lib.te_linear_x6_planes_bytes(T, in_f)
    xs = torch.empty(nb, dtype=torch.uint8, device=dev())
    xa = torch.empty(nb, dtype=torch.uint8, device=dev())
    assert lib.te_linear_x6_split_matrix_f32(X.data_ptr(), T, in_f, 0, xs.data_ptr(), nb, st) == 0
    assert lib.te_linear_x6_split_abs_f32(X.data_ptr(), T, in_f, xa.data_ptr(), nb, st) == 0
    assert not torch.equal(xs, xa)
    rps = ROWS_PER_SAMPLE[T]
    rs = (0.5 + torch.arange(T // rps, dtype=torch.float32)).to(dev())
    ws_bytes = lib.te_linear_relprop_x6_workspace_bytes(T, in_f, out_f)

    def run(planes, flags, r_scale):
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev())
        out = torch.full((T, in_f), float("nan"), dtype=torch.float32, device=dev())
        rc = lib.te_linear_relprop_x6_f32(R.data_ptr(), r_scale.data_ptr() if r_scale is not None else None, 1, rps, X.data_ptr(),
                                          W.data_ptr(), wp.data_ptr(), planes.data_ptr() if planes is not None else None,
                                          Y.data_ptr(), b.data_ptr(), out.data_ptr(), T, in_f, out_f, flags, None, ws.data_ptr(),
                                          ws.numel(), st)
        assert rc == 0, (hex(flags), rc)
        assert lib.te_linear_relprop_x6_check(ws.data_ptr(), T, in_f, out_f, st) == 0, hex(flags)
        return out

    first = None
    for pin in (ops._lib.TE_X6_TILE_128, ops._lib.TE_X6_TILE_256, ops._lib.TE_X6_TILE_128x128):
        for grid in (0, ops.TE_X6_TEST_SMALL_GRID):
            for r_scale in (None, rs):
                want = run(xa, pin | grid, r_scale)
                got = run(xs, pin | grid | ops.TE_X6_X_PLANES_SIGNED, r_scale)
                assert torch.isfinite(want).all()
                assert torch.equal(got, want), (pin, grid, r_scale is not None)
                if r_scale is None:           # (and every geometry and grid gives the same bits)
                    first = want if first is None else first
                    assert torch.equal(want, first), (pin, grid)
    # x_planes = NULL: the call splits X itself -- into signed planes when the flag is set
    assert torch.equal(run(None, ops.TE_X6_X_PLANES_SIGNED, None), first)
    assert torch.equal(run(None, 0, None), first)
    # the cancelling pair went through the fallback and the rule still carries relevance there
    assert bool((first[2] != 0).any())


@gpu
def test_unknown_flag_bits_are_still_refused():
    from transformer_explainability_amd import _lib, ops
    lib = ops._lib.load()
    T, in_f, out_f = SHAPES[0]
    X, W, b, R, Y = _rule_operands(T, in_f, out_f, 690)
    wp = ops.x6_weight_planes(W)
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.full((lib.te_linear_relprop_x6_workspace_bytes(T, in_f, out_f),), 0x5a, dtype=torch.uint8, device=dev())
    out = torch.full((T, in_f), 7.0, dtype=torch.float32, device=dev())
    for fl in (ops.TE_X6_X_PLANES_SIGNED << 1, ops.TE_X6_X_PLANES_SIGNED | 0x100):
        rc = lib.te_linear_relprop_x6_f32(R.data_ptr(), None, 0, 1, X.data_ptr(), W.data_ptr(), wp.data_ptr(), None, Y.data_ptr(),
                                          b.data_ptr(), out.data_ptr(), T, in_f, out_f, fl, None, ws.data_ptr(), ws.numel(), st)
        assert rc == _lib.TE_ERR_INVALID_ARG, hex(fl)
    # the plain product has no use for the flag
    wg = ops.x6_matrix_planes(W, False)
    gws = torch.empty(lib.te_gemm_x6_workspace_bytes(T, in_f, out_f), dtype=torch.uint8, device=dev())
    o2 = torch.empty((T, out_f), dtype=torch.float32, device=dev())
    assert lib.te_gemm_x6_f32(X.data_ptr(), None, wg.data_ptr(), b.data_ptr(), o2.data_ptr(), T, in_f, out_f,
                              ops.TE_X6_X_PLANES_SIGNED, None, gws.data_ptr(), gws.numel(), st) == _lib.TE_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert bool((ws == 0x5a).all()) and bool((out == 7.0).all())


@gpu
def test_gelu_forward_without_abs_planes():
    """te_gelu_forward_x6_planes_f32 with planes_abs = NULL: y and the signed planes are those of the dual call."""
    from transformer_explainability_amd import ops
    lib = ops._lib.load()
    T, K = 70, 128
    x = rnd((T, K), 710, 2.0).to(dev())
    x[0, :4], x[1] = 0.0, -0.0
    st = torch.cuda.current_stream().cuda_stream
    nb = lib.te_linear_x6_planes_bytes(T, K)
    res = []
    for with_abs in (True, False):
        y = torch.full((T, K), float("nan"), dtype=torch.float32, device=dev())
        xs = torch.full((nb,), 0x5a, dtype=torch.uint8, device=dev())
        xa = torch.full((nb,), 0x5a, dtype=torch.uint8, device=dev())
        assert lib.te_gelu_forward_x6_planes_f32(x.data_ptr(), y.data_ptr(), T, K, xs.data_ptr(),
                                                 xa.data_ptr() if with_abs else None, nb, st) == 0
        res.append((y, xs, xa))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][0], ops.gelu_forward(x))
    assert bool((res[1][2] == 0x5a).all()) and not bool((res[0][2] == 0x5a).all())
    # the host wrapper: (y, planes, None)
    y, xs, xa = ops.gelu_forward_planes(x, False)
    assert xa is None and torch.equal(y, res[0][0]) and torch.equal(xs[:nb], res[0][1])


@gpu
@pytest.mark.parametrize("N", [17, 197])
def test_attention_forward_without_abs_planes(N):
    """te_attention_forward_f32 with out_planes and a NULL |out| plane buffer: out, attn, z_qk and the signed planes of the dual call."""
    from transformer_explainability_amd import ops
    B, H = 2, 2
    qkv = rnd((B, N, 3 * H * 64), 720 + N).to(dev())
    assert ops.attention_forward_planes_supported(qkv, H)
    out, attn, zqk, xs, xa = ops.attention_forward(qkv, H, 0.125, planes=True)
    out1, attn1, zqk1, xs1, xa1 = ops.attention_forward(qkv, H, 0.125, planes=True, planes_abs=False)
    torch.cuda.synchronize()
    assert xa is not None and xa1 is None
    nb = ops._lib.load().te_linear_x6_planes_bytes(B * N, H * 64)
    for a, b in ((out, out1), (attn, attn1), (zqk, zqk1), (xs[:nb], xs1[:nb])):
        assert torch.equal(a, b)
    assert torch.isfinite(out).all()


def _w128_model():
    from transformer_explainability_amd import vit
    torch.manual_seed(0)
    return vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=16,
                                 qkv_bias=True).eval().to(dev())


@gpu
@pytest.mark.parametrize("batch", [3, 16])
def test_model_maps_do_not_depend_on_the_switch(batch):
    """Two-block ViT, embedding 128, two heads, 17 tokens: generate_LRP with ops.X6_SIGNED_PLANES on and off gives byte-equal
    maps, and replayed as a GraphedCall it equals eager.  Batch 3 is below the 256 rows from which the x6 forward products
    engage (the switch must then change nothing at all); at batch 16 (272 rows) every Linear hands planes to its rule, and the
    kind the rule received is counted."""
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import ops, rules
    from transformer_explainability_amd.generators import LRP, GraphedCall
    model = _w128_model()
    x = seeded_randn((batch, 3, 64, 64), 31).to(dev())
    index = (torch.arange(batch, device=dev()) * 5) % 16
    linears = [m for m in model.modules() if isinstance(m, rules.Linear)]
    saved = (ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6, ops.X6_SIGNED_PLANES, ops.take_x_abs_planes)
    kinds = []

    def counting(cache, X, T, K):
        planes = saved[4](cache, X, T, K)
        if planes is not None:
            kinds.append(ops.planes_are_signed(planes))
        return planes

    try:
        ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6 = True, "all", True
        ops.take_x_abs_planes = counting
        maps, taken = {}, {}
        for signed in (True, False):
            ops.X6_SIGNED_PLANES = signed
            del kinds[:]
            lrp = LRP(model)
            maps[signed] = lrp.generate_LRP(x, index=index, start_layer=0).clone()
            lrp.check()
            taken[signed] = list(kinds)
            assert all("x_abs_planes" not in rules.x6_cache(m) and "x_planes_from_producer" not in rules.x6_cache(m)
                       for m in linears)
        assert torch.isfinite(maps[True]).all()
        assert maps[True].cpu().numpy().tobytes() == maps[False].cpu().numpy().tobytes()
        assert len(taken[True]) == len(taken[False]) and all(taken[True]) and not any(taken[False])
        if batch * 17 >= 256:
            assert len(taken[True]) > 0
        ops.X6_SIGNED_PLANES = True
        lrp = LRP(model)
        call = GraphedCall(lambda t: lrp.generate_LRP(t, index=index, start_layer=0), (x,))
        got = call(x)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == maps[True].cpu().numpy().tobytes()
        lrp.check()
    finally:
        ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6, ops.X6_SIGNED_PLANES, ops.take_x_abs_planes = saved


# ------------------------------------------------------------------------------------------------ CPU
def _bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even) as fp32: the rounding of v_cvt_pk_bf16_f32 on finite values."""
    u = x.view(np.uint32)
    u = (u + (((u >> 16) & 1) + 0x7fff)) & np.uint32(0xffff0000)
    return u.view(np.float32)


def _split3(x):
    """x = p0 + p1 + p2 exactly, every part a bf16 (tests/diagnostics/bf16_split_probe.py: split3), here on numpy."""
    p0 = _bf16_rne(x)
    r = x - p0
    p1 = _bf16_rne(r)
    p2 = _bf16_rne(r - p1)
    return p0, p1, p2


def _bits(p):
    return (p.view(np.uint32) >> 16).astype(np.uint16)


def test_sign_fixed_planes_decode_to_the_planes_of_abs():
    """Clearing plane 0's sign and flipping the low planes where it was set turns split3(x) into split3(|x|), up to the sign
    of a zero low plane (x - x = +0 whatever the sign of x; the flip is unmasked): what the signed Z-pass relies on."""
    rng = np.random.default_rng(17)
    n = 1 << 21
    parts = [rng.standard_normal(n).astype(np.float32),
             (rng.standard_normal(n) * np.exp2(rng.integers(-60, 60, n))).astype(np.float32),
             rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)]      # any bit pattern
    special = np.array([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 3.0e-39, -3.0e-39, 1.0 + 2.0 ** -8, -(1.0 + 2.0 ** -8),
                        1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 1.0 + 2.0 ** -16, -(1.0 + 2.0 ** -16), 65280.0, -65280.0], np.float32)
    exact = _bf16_rne(parts[0][:4096].copy())                  # exact bf16 values of both signs: zero low planes
    x = np.concatenate(parts + [special, exact])
    x = x[np.isfinite(x) & (np.abs(x) < 3.0e38)]               # (the split is defined on finite values below the bf16 overflow)
    assert x.size > 4_000_000
    with np.errstate(over="ignore"):
        signed = [_bits(p) for p in _split3(x)]
        want = [_bits(p) for p in _split3(np.abs(x))]
    m = signed[0] & np.uint16(0x8000)
    fixed = [signed[0] & np.uint16(0x7fff), signed[1] ^ m, signed[2] ^ m]
    assert np.array_equal(fixed[0], want[0])
    for q in (1, 2):
        same = fixed[q] == want[q]
        both_zero = ((fixed[q] | want[q]) & np.uint16(0x7fff)) == 0
        assert bool(np.all(same | both_zero)), q
        assert bool(np.all(want[q][both_zero & ~same] == 0))       # |x|'s zero residual is +0; only the fixed one may be -0
    assert int(np.count_nonzero(fixed[1] != want[1])) > 0        # (the -0 case occurs: negative exact bf16 values)
