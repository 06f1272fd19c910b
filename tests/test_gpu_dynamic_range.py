"""`-m gpu`: the relprop rules and the LayerNorm / GELU producers on operands whose independent problems -- rows of a Linear
layer, (b,h) slices and query rows of the attention rules, samples of an Add -- differ by up to 2^-40 in magnitude
(tests/dynamic_range_inputs.py), every problem weighed by its OWN magnitude (gpu_util.check_groups) at the bar its rule
already has: 2e-5 Linear, 3e-5 attention rules, 5e-6 LayerNorm backward.  gpu_util.check scales every error by the maximum
of the whole tensor and every other operand of the suite is a unit-scale Gaussian, so a kernel that zeroes, flushes or
mis-rounds what lies below 1e-5 of the tensor's maximum passes there.  tests/test_dynamic_range_host.py shows on the CPU that the fp32
oracle meets a quarter of each bar on these inputs and that three mutants of it fail here while passing there."""
import functools
import hashlib

import pytest
import torch
import torch.nn.functional as F

import dynamic_range_inputs as D
from gpu_util import check_groups, dev, record
from oracle import relprop_oracle as O

pytestmark = pytest.mark.gpu

LINEAR_TOL, ATTN_TOL, LN_FWD_TOL, LN_BWD_TOL = 2e-5, 3e-5, 3e-6, 5e-6
ELEMENT_TOL = 2.0 ** -20       # Add / Clone, element-wise: at most eight fp32 roundings between operands and output
GELU_ULP = 4
GELU_BWD_ULP = 412 + 1      # measured distance to torch's fp32 kernel plus one ulp (test_gelu_per_element_in_ulp)


@pytest.fixture(autouse=True)
def _flags():
    from transformer_explainability_amd import ops
    was = (ops.FORCE_SIMPLE, ops.USE_LINEAR_X6, ops.X6_CHECK)
    yield
    ops.FORCE_SIMPLE, ops.USE_LINEAR_X6, ops.X6_CHECK = was


# ------------------------------------------------------------------------------------------------ Linear
@functools.lru_cache(maxsize=None)
def _linear_refs(case, T, in_f, out_f, alpha, variant):
    c = D.linear_case(case, T, in_f, out_f)
    return (O.linear_relprop(c["R"], c["X"], c["W"], alpha, variant),
            O.linear_relprop(c["R"].double(), c["X"].double(), c["W"].double(), alpha, variant))


def _homogeneous(rule, Rd, base, tag):
    """rule(2^-k R) == 2^-k rule(R), bit for bit (powers of two: both sides are exact scalings of the same roundings)."""
    for k in D.HOMOGENEITY_K:
        s = float(D.pow2(-k))
        scaled = rule(Rd * s)
        assert torch.equal(scaled, base * s), (tag, k, float((scaled - base * s).abs().max()), float((base * s).abs().max()))


@pytest.mark.parametrize("alpha", [1.0, 2.0], ids=["alpha1", "alpha2"])
@pytest.mark.parametrize("case", D.LINEAR_CASES)
@pytest.mark.parametrize("T,in_f,out_f", D.LINEAR_FWD_SHAPES, ids=["fp32-mfma", "x6-128", "x6-256"])
def test_linear_forward_output_per_row(T, in_f, out_f, case, alpha):
    """Variant ours with the cached forward output Y (rocBLAS on the device, as the model produces it): the fp32-MFMA
    Z-pass from Y (te_linear.hip K1f), the x6 Z-pass (te_linear_x6.hip, 128-wide and 256 x 256 tiles) and, with alpha = 2,
    the general x6 entry point whose inhibitor half takes Z' from the same product (MODE_ZI).  Every row within 2e-5 of its
    own maximum; all-zero rows exactly zero; homogeneous in R bit for bit; both paths agree per row; no x6 hand-over lost.
    Before the fallback criterion knew of the bias (te_common.h: kCancelBiasTol) the small rows of X in x_scaled / xr_scaled
    were off by 11-74 % of their own maximum (172 % in MODE_ZI) and bias_scaled reached 2.4e-5
    (profiles/zbias_parent_per_row.log); with it the worst row of any case is at 4.9e-6.
    (140, 256, 192) is no x6 shape: both settings of the flag run the fp32-MFMA kernels there.)"""
    from transformer_explainability_amd import ops
    c = D.linear_case(case, T, in_f, out_f)
    ref32, ref64 = _linear_refs(case, T, in_f, out_f, alpha, "ours")
    Xd, Wd, bd, Rd = (c[k].to(dev()) for k in ("X", "W", "bias", "R"))
    Y = F.linear(Xd, Wd, bd)
    lib = ops._lib.load()
    x6_shape = bool(lib.te_linear_relprop_x6_supported(T, in_f, out_f) if alpha == 1.0 else
                    lib.te_linear_relprop_x6_general_supported(T, in_f, out_f, 0))
    assert x6_shape == (out_f != 192)
    ops.X6_CHECK = True
    ops.x6_raise_if_failed()
    got = {}
    for x6 in (False, True):
        ops.USE_LINEAR_X6 = x6
        cache = {}
        rule = lambda r: ops.linear_relprop(r, Xd, Wd, alpha=alpha, variant="ours", Y=Y, bias=bd, cache=cache)  # noqa: E731
        got[x6] = rule(Rd)
        assert ("x6_planes" in cache) == (x6 and x6_shape)                     # the kernels meant ran
        tag = f"dr.linear_fwd.{case}.a{alpha:g}.({T},{in_f},{out_f}).{'x6' if x6 else 'fp32'}"
        check_groups(tag, got[x6], ref32, ref64, -1, LINEAR_TOL)
        _homogeneous(rule, Rd, got[x6], tag)
        ops.x6_raise_if_failed()                                               # (X6_CHECK: te_linear_relprop_x6_check ran too)
    check_groups(f"dr.linear_fwd.{case}.a{alpha:g}.({T},{in_f},{out_f}).x6_vs_fp32", got[True], got[False], got[False].double(),
                 -1, LINEAR_TOL)


@pytest.mark.parametrize("simple", [False, True], ids=["two-product", "simple"])
@pytest.mark.parametrize("case", ["r_scaled", "x_scaled"])
@pytest.mark.parametrize("T,in_f,out_f", D.LINEAR_NOY_SHAPES)
def test_linear_without_forward_output_per_row(T, in_f, out_f, case, simple):
    """Variant lrp without Y: the two-product fp32-MFMA kernels and the one-thread-per-output kernels ((7, 10, 2) is an odd
    shape: the simple kernels either way)."""
    from transformer_explainability_amd import ops
    c = D.linear_case(case, T, in_f, out_f)
    ref32, ref64 = _linear_refs(case, T, in_f, out_f, 1.0, "lrp")
    Xd, Wd, Rd = (c[k].to(dev()) for k in ("X", "W", "R"))
    ops.USE_LINEAR_X6, ops.FORCE_SIMPLE = False, simple
    rule = lambda r: ops.linear_relprop(r, Xd, Wd, alpha=1.0, variant="lrp")  # noqa: E731
    got = rule(Rd)
    tag = f"dr.linear_lrp.{case}.({T},{in_f},{out_f}).{'simple' if simple else 'tiled'}"
    check_groups(tag, got, ref32, ref64, -1, LINEAR_TOL)
    _homogeneous(rule, Rd, got, tag)


@pytest.mark.parametrize("case", ["r_scaled", "x_scaled"])
def test_linear_bf16_operands_per_row(case):
    """linear_relprop_bf16 (bf16 X and W, fp32 relevance) against the fp64 oracle on the exactly widened operands, per row at
    the bar of the fp32 rule (tests/test_gpu_bf16_rules.py: 'the tolerance of the fp32 test of the same rule')."""
    from transformer_explainability_amd import ops
    T, in_f, out_f = D.LINEAR_BF16_SHAPE
    assert ops.linear_bf16_route(T, in_f, out_f) == "bf16"
    c = D.linear_case(case, T, in_f, out_f)
    Xb, Wb = c["X"].bfloat16(), c["W"].bfloat16()
    ref32 = O.linear_relprop(c["R"], Xb.float(), Wb.float())
    ref64 = O.linear_relprop(c["R"].double(), Xb.double(), Wb.double())
    got = ops.linear_relprop(c["R"].to(dev()), Xb.to(dev()), Wb.to(dev()), cache={})
    check_groups(f"dr.linear_bf16.{case}.({T},{in_f},{out_f})", got, ref32, ref64, -1, LINEAR_TOL)


@pytest.mark.parametrize("case", ["r_scaled", "x_scaled"])
def test_linear_f64_per_element(case):
    """linear_relprop_f64 on the same cases in double, at the bar of tests/test_gpu_f64.py: |got - oracle| <= 2 x the a-priori
    rounding bound of EVERY element (finer than per row), zero rows exactly zero."""
    from f64_util import linear_bound, ratio_to_bound
    from transformer_explainability_amd import ops
    T, in_f, out_f = D.LINEAR_F64_SHAPE
    c = {k: v.double() for k, v in D.linear_case(case, T, in_f, out_f).items()}
    ref, bound = O.linear_relprop(c["R"], c["X"], c["W"]), linear_bound(c["R"], c["X"], c["W"])
    got = ops.linear_relprop(c["R"].to(dev()), c["X"].to(dev()), c["W"].to(dev())).cpu()
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    r = ratio_to_bound(got, ref, bound)
    record(f"dr.linear_f64.{case}.({T},{in_f},{out_f})", err_over_bound=r)
    assert r <= 2.0, r
    assert not got[ref.abs().amax(-1) == 0].any()
    check_groups(f"dr.linear_f64.{case}.({T},{in_f},{out_f}).rows", got, ref, ref, -1, 1e-12)


# Unit-scale operands on which the bias term of the fallback criterion (te_common.h: kCancelBiasTol) cannot fire: the
# outputs must be, bit for bit, those of the kernels before that term existed.  The digests below were recorded from the
# parent commit's build on an MI355X.  Every operand is a seeded CPU draw; X and W are kept to multiples of 2^-8 and 2^-12
# so that Y = X W^T + b is exact in double whatever the summation order and its fp32 rounding is the same on every host.
UNIT_SCALE_DIGESTS = {
    # (T, in_f, out_f, alpha, x6): sha256 of the output's bytes
    (140, 256, 192, 1.0, False): "74beb7642a9054c294dc1f0eeb28b4b5db7ffeb2741b44730ec9fe0aec8eaddb",
    (140, 256, 192, 1.0, True): "74beb7642a9054c294dc1f0eeb28b4b5db7ffeb2741b44730ec9fe0aec8eaddb",
    (140, 256, 192, 2.0, False): "5daffac7bce71ac3ab0a67769660cdae4de3bd2550f7f0f966d53c3bcf1dad68",
    (140, 256, 192, 2.0, True): "5daffac7bce71ac3ab0a67769660cdae4de3bd2550f7f0f966d53c3bcf1dad68",
    (140, 256, 256, 1.0, False): "370d2c6c161dd1a992e85de8fc13a140ff3c538f87d83727f7e137dd2c0631a6",
    (140, 256, 256, 1.0, True): "0a825c901e3305c41fb6b1e864002b3878e33d009b14bf68c56eb9cc0444e848",
    (140, 256, 256, 2.0, False): "717ee960c1fd5d89db22b76429f2e47d023541867697200cce4264fafa6900f5",
    (140, 256, 256, 2.0, True): "c21950cfccc08f3613db9a1c500199b2a7e6f1dc30ae5c2e1acec6dd8650bf47",
    (300, 768, 768, 1.0, False): "01ea10afac648a370456eac7ab759e89699dce6fca4ae1e0229a5f55504f09d1",
    (300, 768, 768, 1.0, True): "c6bf0aca2181d05f7044585258b9f1ec6e934e76a59c0026c96e44899b786379",
    (300, 768, 768, 2.0, False): "0d84130a685ea777825087c34fd200cb14174d7517b35f2d61dea9eb1cc1470b",
    (300, 768, 768, 2.0, True): "afccf0150c47c3f11bdd219161ec5cc376655693a0168b2bfd596d160f83f1cb",
}


def _unit_scale_case(T, in_f, out_f):
    X = (D.rnd((T, in_f), 910) * 256.0).round() / 256.0
    W = (D.rnd((out_f, in_f), 911, 0.05) * 4096.0).round() / 4096.0
    R, bias = D.rnd((T, out_f), 912, 0.01), D.rnd((out_f,), 913, 0.3)
    Y = (X.double() @ W.double().t() + bias.double()).float()
    return X, W, R, bias, Y


def unit_scale_digests(ops):
    """{(T, in_f, out_f, alpha, x6): digest} of the forward-output rule on the unit-scale case (also run from the script that
    recorded UNIT_SCALE_DIGESTS on the parent commit's build)."""
    out = {}
    for T, in_f, out_f in D.LINEAR_FWD_SHAPES:
        X, W, R, bias, Y = _unit_scale_case(T, in_f, out_f)
        Xd, Wd, Rd, bd, Yd = (t.to(dev()) for t in (X, W, R, bias, Y))
        for alpha in (1.0, 2.0):
            for x6 in (False, True):
                ops.USE_LINEAR_X6 = x6
                got = ops.linear_relprop(Rd, Xd, Wd, alpha=alpha, variant="ours", Y=Yd, bias=bd, cache={})
                out[(T, in_f, out_f, alpha, x6)] = hashlib.sha256(got.cpu().contiguous().numpy().tobytes()).hexdigest()
    return out


def test_linear_unit_scale_outputs_keep_their_bits():
    from transformer_explainability_amd import ops
    for T, in_f, out_f in D.LINEAR_FWD_SHAPES:
        X, W, R, bias, Y = _unit_scale_case(T, in_f, out_f)
        X, W = X.double(), W.double()
        z = X.clamp(min=0) @ W.clamp(min=0).t() + X.clamp(max=0) @ W.clamp(max=0).t()             # Z  >= 0
        zi = -(X.clamp(min=0) @ W.clamp(max=0).t() + X.clamp(max=0) @ W.clamp(min=0).t())         # -Z' >= 0
        # twice the threshold: the bias term is nowhere near firing, for Z and for the inhibitor's Z'
        assert (z > 2.0 ** -3 * bias.abs().double()).all() and (zi > 2.0 ** -3 * bias.abs().double()).all()
    got = unit_scale_digests(ops)
    record("dr.linear_unit_scale_digests", digests={str(k): v for k, v in got.items()})
    assert got == UNIT_SCALE_DIGESTS, {k: v for k, v in got.items() if UNIT_SCALE_DIGESTS.get(k) != v}


# ------------------------------------------------------------------------------------------------ attention rules
ATTN_GROUPS = {"cam_attn": -1, "cam_q": -1, "cam_v": (-2, -1), "cam_k": (-2, -1)}


@pytest.mark.parametrize("case", D.ATTN_CASES)
@pytest.mark.parametrize("B,H,N,Dh", D.ATTN_SHAPES)
def test_attention_rules_per_row_and_per_head(B, H, N, Dh, case):
    """AV and QK rule, tiled and simple kernels, positive operands in the fused qkv layout, forward products handed in as
    the model does: cam_attn and cam_q per query row, cam_v and cam_k per (b,h), 3e-5 of the group's own maximum; groups
    without relevance exactly zero; homogeneous in R bit for bit.  The QK rule is judged on the relevance the device AV
    rule produced (its own input), as in test_gpu_rules.py."""
    from transformer_explainability_amd import ops
    c = D.attention_case(case, B, H, N, Dh)
    q, k, v, attn = D.attention_operands(c["qkv"], B, H, N, Dh)
    d = dev()
    qd, kd, vd = c["qkv"].to(d).view(B, N, 3, H, Dh).permute(2, 0, 3, 1, 4)      # read in place from the fused activation
    attn_d = attn.to(d)
    Rd = c["R"].to(d)
    z_av, z_qk = attn_d @ vd, qd @ kd.transpose(-1, -2)
    zc_av, zc_qk = z_av.cpu(), z_qk.cpu()
    a32, v32 = O.einsum_av_relprop(c["R"], attn, v, zc_av)
    a64, v64 = O.einsum_av_relprop(c["R"].double(), attn.double(), v.double(), zc_av.double())
    for simple in (False, True):
        ops.FORCE_SIMPLE = simple
        tag = f"dr.attn.{case}.({B},{H},{N},{Dh}).{'simple' if simple else 'tiled'}"
        cam1, cam_v = ops.matmul_relprop_av(Rd, attn_d, vd, out_scale=0.5, z=z_av)
        cam_q, cam_k = ops.matmul_relprop_qk(cam1, qd, kd, out_scale=0.5, z=z_qk)
        cam1_c = cam1.cpu()
        q32, k32 = O.einsum_qk_relprop(cam1_c, q, k, zc_qk)
        q64, k64 = O.einsum_qk_relprop(cam1_c.double(), q.double(), k.double(), zc_qk.double())
        refs = {"cam_attn": (cam1, a32, a64), "cam_v": (cam_v, v32, v64), "cam_q": (cam_q, q32, q64), "cam_k": (cam_k, k32, k64)}
        for name, (got, r32, r64) in refs.items():
            check_groups(f"{tag}.{name}", got, r32 * 0.5, r64 * 0.5, ATTN_GROUPS[name], ATTN_TOL)
        for kk in D.HOMOGENEITY_K:
            s = float(D.pow2(-kk))
            c1s, cvs = ops.matmul_relprop_av(Rd * s, attn_d, vd, out_scale=0.5, z=z_av)
            cqs, cks = ops.matmul_relprop_qk(cam1 * s, qd, kd, out_scale=0.5, z=z_qk)
            for name, scaled, base in (("cam_attn", c1s, cam1), ("cam_v", cvs, cam_v), ("cam_q", cqs, cam_q), ("cam_k", cks, cam_k)):
                assert torch.equal(scaled, base * s), (tag, name, kk, float((scaled - base * s).abs().max()),
                                                       float((base * s).abs().max()))


# ------------------------------------------------------------------------------------------------ Add, Clone
def _within(tag, got, ref32, ref64):
    worst, zeros_ok = D.elementwise_excess(got, ref64, ELEMENT_TOL)
    record(tag, worst_rel_over_2m20=worst, oracle32_rel_over_2m20=D.elementwise_excess(ref32, ref64, ELEMENT_TOL)[0])
    assert zeros_ok and worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("shape", D.ADD_SHAPES)
def test_add_and_clone_per_element(shape):
    """Samples at 2^0 ... 2^-40: |got - ref64| <= 2^-20 |ref64| on every non-zero element of the fp64 oracle (operands to
    output are at most eight fp32 roundings: the sum, + 1e-9, the quotient, the product, and four in the rescaling factor,
    whose per-sample sums the kernels keep in double) -- Add ours (two-pass and deferred), Add lrp, Clone of 2 and 3."""
    from transformer_explainability_amd import ops
    c = D.add_case(shape)
    d64 = {k: t.double() for k, t in c.items()}
    g = {k: t.to(dev()) for k, t in c.items()}
    for variant in ("ours", "lrp"):
        a, b = ops.add_relprop(g["R"], g["X0"], g["X1"], variant=variant)
        a32, b32 = O.add_relprop(c["R"], c["X0"], c["X1"], variant)
        a64, b64 = O.add_relprop(d64["R"], d64["X0"], d64["X1"], variant)
        _within(f"dr.add_{variant}{shape}.a", a, a32, a64)
        _within(f"dr.add_{variant}{shape}.b", b, b32, b64)
        if variant == "ours":
            da, db = ops.add_relprop(g["R"], g["X0"], g["X1"], variant="ours", deferred=True)
            _within(f"dr.add_deferred{shape}.a", da.materialise(), a32, a64)
            _within(f"dr.add_deferred{shape}.b", db.materialise(), b32, b64)
    for names in (("R", "R2"), ("R", "R2", "R3")):
        got = ops.clone_relprop([g[n] for n in names], g["X0"])
        _within(f"dr.clone{len(names)}{shape}", got, O.clone_relprop([c[n] for n in names], c["X0"]),
                O.clone_relprop([d64[n] for n in names], d64["X0"]))


def test_add_broadcast_mask_per_element():
    from transformer_explainability_amd import ops
    B, H, N = D.ADD_MASK_SHAPE
    c = D.add_mask_case(B, H, N)
    a, b = ops.add_relprop(c["R"].to(dev()), c["X0"].to(dev()), c["mask"].to(dev()))
    a32, b32 = O.add_relprop(c["R"], c["X0"], c["mask"])
    a64, b64 = O.add_relprop(c["R"].double(), c["X0"].double(), c["mask"].double())
    _within(f"dr.add_mask({B},{H},{N}).a", a, a32, a64)
    _within(f"dr.add_mask({B},{H},{N}).b", b, b32, b64)
    da, db = ops.add_relprop(c["R"].to(dev()), c["X0"].to(dev()), c["mask"].to(dev()), deferred=True)
    _within(f"dr.add_mask_deferred({B},{H},{N}).a", da.materialise(), a32, a64)
    _within(f"dr.add_mask_deferred({B},{H},{N}).b", db, b32, b64)


# ------------------------------------------------------------------------------------------------ LayerNorm, GELU
def _row_stats(t, ref64):
    return (t.detach().cpu().double() - ref64).abs().amax(-1), ref64.abs().amax(-1)


@pytest.mark.parametrize("C", D.LN_WIDTHS)
def test_layernorm_per_row(C):
    """Nine rows with mean / std up to 2^12 and scales 2^-14 ... 2^10 (variance far below to far above eps); C = 1028 and 1540
    run the half-empty NV = 6 and NV = 8 instantiations.  Forward against F.layer_norm in double, backward against its autograd
    in double, per row: err_row <= 2 x (the stock fp32 kernel's err_row) + tol x scale_row -- tests/test_gpu_producers.py's
    bars (3e-6 forward, 5e-6 backward) with the row's own maximum in place of the tensor's; the forward bound also allows
    2 ulp of the row's fp32 mean (below)."""
    from transformer_explainability_amd import ops
    c = D.layernorm_case(C)
    d = dev()
    x, w, b, dy = (c[k].to(d) for k in ("x", "w", "b", "dy"))
    assert ops.layernorm_supported(x)
    y, mean, rstd = ops.layernorm_forward(x, w, b, 1e-6)
    dx = ops.layernorm_backward(dy, x, w, mean, rstd)
    xr = x.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (C,), w, b, 1e-6)
    (dxr,) = torch.autograd.grad(yr, xr, dy)
    x64 = c["x"].double().requires_grad_(True)
    y64 = F.layer_norm(x64, (C,), c["w"].double(), c["b"].double(), 1e-6)
    (dx64,) = torch.autograd.grad(y64, x64, c["dy"].double())
    y64 = y64.detach()
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    x64d = c["x"].double()
    mean64, rstd64 = x64d.mean(-1), (x64d.var(-1, unbiased=False) + 1e-6).rsqrt()
    # forward only: a mean kept in fp32 is off by up to half an ulp however it is summed, and a pairwise sum of C terms of
    # one sign by a few more; 2 ulp of the mean (4 x 2^-24 |mean|) reach the output times rstd |w|.  With |mean| = 4096 std
    # this is what decides the row (1e-4 of its maximum, for the stock kernel too), and which of two correct kernels has the
    # luckier rounding of the mean is not a defect of the other.
    mean_floor = 4.0 * 2.0 ** -24 * mean64.abs() * rstd64 * float(c["w"].abs().max())
    for name, got, stock, ref, tol, floor in (("fwd", y, yr.detach(), y64, LN_FWD_TOL, mean_floor),
                                              ("bwd", dx, dxr, dx64, LN_BWD_TOL, torch.zeros_like(mean_floor))):
        err, scale = _row_stats(got, ref)
        err_stock, _ = _row_stats(stock, ref)
        bound = 2.0 * err_stock + tol * scale + floor
        excess = err / bound
        record(f"dr.layernorm.{name}(C={C})", worst_ratio=float((err / scale).max()), stock_worst_ratio=float((err_stock / scale).max()),
               worst_over_bound=float(excess.max()), worst_row=int(excess.argmax()))
        assert (err <= bound).all(), (name, C, (err / scale).tolist(), (err_stock / scale).tolist())


def test_gelu_per_element_in_ulp():
    """x on [-9, 9], the negative tail where |gelu(x)| < 1e-5 included, element by element against torch's fp32 kernel (a
    whole-tensor metric sees nothing below 1e-6 x 9).
    Forward: within 4 ulp of torch's value (measured on the MI355X: 0 -- the same bits, 10618 tail elements included).
    Backward: 4 ulp of torch's value does not hold, and cannot for any fp32 evaluation of dy (cdf + x pdf): the two terms
    cancel at gelu's minimum, x = -0.7518, where the result is far smaller than either and its ulp with it.  Measured: 412
    ulp of torch's value at x = -0.75142 (value 1.4e-4 for dy = 1.3), so the bound on that figure is 413 ulp; what the
    kernel can be held to there is asserted next to it: within 4 ulp of the LARGER of the two terms (measured: 2.0)."""
    from transformer_explainability_amd import ops
    c = D.gelu_case()
    x, dy = c["x"].to(dev()), c["dy"].to(dev())
    xr = x.clone().requires_grad_(True)
    yr = F.gelu(xr)
    (dxr,) = torch.autograd.grad(yr, xr, dy)
    y, dx = ops.gelu_forward(x), ops.gelu_backward(dy, x)
    for name, got, ref in (("fwd", y, yr.detach()), ("bwd", dx, dxr)):
        assert torch.isfinite(got).all()
        dist = D.ulp_distance(got, ref)
        worst = int(dist.argmax())
        record(f"dr.gelu.{name}", max_ulp=int(dist.max()), at_x=float(c["x"][worst]), torch_value=float(ref.cpu()[worst]),
               tail_elements=int((ref.abs() < 1e-5).sum()))
        if name == "bwd":
            x64, dy64 = c["x"].double(), c["dy"].double()
            cdf, xpdf = 0.5 * (1 + torch.erf(x64 / 2 ** 0.5)), x64 * torch.exp(-0.5 * x64 * x64) / (2 * torch.pi) ** 0.5
            term = dy64.abs() * torch.maximum(cdf.abs(), xpdf.abs())
            ulp_term = torch.exp2(torch.floor(torch.log2(term.clamp_min(2.0 ** -126))) - 23)
            in_term_ulp = (got.cpu().double() - ref.cpu().double()).abs() / ulp_term
            record("dr.gelu.bwd.term_ulp", max_term_ulp=float(in_term_ulp.max()), at_x=float(c["x"][int(in_term_ulp.argmax())]))
            assert float(in_term_ulp.max()) <= GELU_ULP, (float(in_term_ulp.max()), float(c["x"][int(in_term_ulp.argmax())]))
        bound = GELU_ULP if name == "fwd" else GELU_BWD_ULP
        assert int(dist.max()) <= bound, (name, int(dist.max()), float(c["x"][worst]), float(ref.cpu()[worst]))
