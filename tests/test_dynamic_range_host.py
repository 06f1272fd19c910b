"""CPU side of the dynamic-range tests (tests/dynamic_range_inputs.py, gpu_util.check_groups; the kernels are judged in
tests/test_gpu_dynamic_range.py):

  * the inputs are fair: on every case the GPU tests use, the plain fp32 oracle meets ONE QUARTER of the bar the kernels
    are held to, per independent problem, against the fp64 oracle;
  * the per-group check bites where the whole-tensor check is blind: three mutants of the fp32 oracle fail check_groups
    while passing gpu_util.check at the old bar;
  * the fp32 oracle is homogeneous in R bit for bit on these inputs (so no value leaves the normal range in it)."""
import pytest
import torch
import torch.nn.functional as F

import dynamic_range_inputs as D
import gpu_util
from gpu_util import check, check_groups
from oracle import relprop_oracle as O

LINEAR_TOL, ATTN_TOL = 2e-5, 3e-5
ELEMENT_TOL = 2.0 ** -20        # Add / Clone: at most eight fp32 roundings between operands and output


@pytest.fixture(autouse=True)
def _no_report(monkeypatch):
    monkeypatch.setattr(gpu_util, "record", lambda *a, **k: None)      # the parity report belongs to the device runs


def _lin64(c, alpha=1.0, variant="ours"):
    return O.linear_relprop(c["R"].double(), c["X"].double(), c["W"].double(), alpha, variant)


# ------------------------------------------------------------------------------------------------ check_groups itself
def test_check_groups_judges_every_group_and_exact_zeros():
    ref = torch.tensor([[1.0, -2.0], [1e-12, 3e-12], [0.0, 0.0]], dtype=torch.float64)
    ok = ref.float()
    s = check_groups("t", ok, ok, ref, -1, 1e-6)
    assert s["groups"] == 3 and s["live_groups"] == 2 and s["worst_ratio"] <= 1e-7
    bad = ok.clone()
    bad[1, 1] = 0.0                              # 3e-12 against a tensor maximum of 2: invisible to check() ...
    check("t", bad, ok, 1e-6)
    with pytest.raises(AssertionError):          # ... and an error of 100 % of its own row
        check_groups("t", bad, ok, ref, -1, 1e-6)
    dirty = ok.clone()
    dirty[2, 0] = 1e-30                          # a group the reference leaves exactly zero
    with pytest.raises(AssertionError):
        check_groups("t", dirty, ok, ref, -1, 1e-6)
    nan = ok.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        check_groups("t", nan, ok, ref, -1, 1e-6)
    # several reduced dims: one group per leading index
    r3 = torch.arange(1.0, 25.0, dtype=torch.float64).view(2, 3, 4)
    assert check_groups("t", r3.float(), r3.float(), r3, (1, 2), 1e-6)["groups"] == 2


def test_inputs_are_finite_normal_and_powers_of_two_scaled():
    tiny = torch.finfo(torch.float32).tiny
    for shape in D.LINEAR_FWD_SHAPES + D.LINEAR_NOY_SHAPES:
        for case in D.LINEAR_CASES:
            for t in D.linear_case(case, *shape).values():
                assert torch.isfinite(t).all() and not ((t != 0) & (t.abs() < tiny * 2.0 ** 60)).any(), (shape, case)
    c, base = D.linear_case("r_scaled", 140, 256, 192), D.rnd((140, 192), 502, 0.01)
    ratio = c["R"][16:32] / base[16:32]
    assert torch.equal(ratio, torch.full_like(ratio, 2.0 ** -8))
    assert not c["R"][5].any() and c["R"][6].any()
    x = D.linear_case("x_scaled", 140, 256, 192)["X"]
    scaled = (x[:, 0] / D.rnd((140, 256), 500)[:, 0]) != 1.0          # (column 0 is no outlier channel)
    assert 8 <= int(scaled.sum()) <= 140 // 8 + 1                     # at most 1/8 of the rows (plus the zero row)
    assert int((D.linear_case("cls_only", 300, 768, 768)["R"].abs().amax(-1) > 0).sum()) == 3


# ------------------------------------------------------------------------------------------------ Linear
@pytest.mark.parametrize("case", D.LINEAR_CASES)
@pytest.mark.parametrize("T,in_f,out_f", D.LINEAR_FWD_SHAPES)
def test_linear_cases_are_fair(T, in_f, out_f, case):
    c = D.linear_case(case, T, in_f, out_f)
    for alpha in (1.0, 2.0):
        ref32 = O.linear_relprop(c["R"], c["X"], c["W"], alpha)
        check_groups(f"host.linear.{case}", ref32, ref32, _lin64(c, alpha), -1, LINEAR_TOL / 4)


@pytest.mark.parametrize("case", ["r_scaled", "x_scaled"])
@pytest.mark.parametrize("T,in_f,out_f", D.LINEAR_NOY_SHAPES)
def test_linear_lrp_cases_are_fair(T, in_f, out_f, case):
    c = D.linear_case(case, T, in_f, out_f)
    ref32 = O.linear_relprop(c["R"], c["X"], c["W"], 1.0, "lrp")
    check_groups(f"host.linear_lrp.{case}", ref32, ref32, _lin64(c, 1.0, "lrp"), -1, LINEAR_TOL / 4)


@pytest.mark.parametrize("case", ["r_scaled", "x_scaled"])
def test_linear_bf16_operand_cases_are_fair(case):
    c = D.linear_case(case, *D.LINEAR_BF16_SHAPE)
    c["X"], c["W"] = c["X"].bfloat16().float(), c["W"].bfloat16().float()      # what a bf16 model holds, widened exactly
    ref32 = O.linear_relprop(c["R"], c["X"], c["W"])
    check_groups(f"host.linear_bf16.{case}", ref32, ref32, _lin64(c), -1, LINEAR_TOL / 4)


def _zero_small_rows(out):
    """Mutant 1: a kernel that flushes every row below 1e-5 of the tensor's maximum."""
    m = out.clone()
    rows = m.abs().amax(-1)
    m[rows < 1e-5 * rows.max()] = 0.0
    return m


def _two_planes(t):
    """Mutant 2: an operand kept as two bf16 planes (truncating split) instead of three: 16 significand bits."""
    hi = (t.view(torch.int32) & -65536).view(torch.float32)
    lo = ((t - hi).view(torch.int32) & -65536).view(torch.float32)
    return hi + lo


def forward_output_rule(c, bias_tol):
    """fp32 emulation of the one-product Z-pass, Z = ((Y - b) + |X||W|^T) / 2 with the exact positive-part sum where
    Z <= 2^-7 |X||W|^T -- and, with bias_tol, also where Z <= bias_tol |b_j|.  Returns (out, share of elements that fell back)."""
    R, X, W, b = c["R"], c["X"], c["W"], c["bias"]
    a = X.abs() @ W.abs().t()
    z = 0.5 * ((F.linear(X, W, b) - b) + a)
    px, nx, pw, nw = X.clamp(min=0), X.clamp(max=0), W.clamp(min=0), W.clamp(max=0)
    cancel = ~(z > 2.0 ** -7 * a)
    if bias_tol:
        cancel |= ~(z > bias_tol * b.abs())
    z = torch.where(cancel, px @ pw.t() + nx @ nw.t(), z)
    S = O.safe_divide(R, z)
    return px * (S @ pw) + nx * (S @ nw), float(cancel.float().mean())


def _mutant_fails_groups_only(name, mutant, ref32, ref64):
    check(name, mutant, ref32, LINEAR_TOL)                        # the suite's metric before this file: blind
    with pytest.raises(AssertionError):
        check_groups(name, mutant, ref32, ref64, -1, LINEAR_TOL)


@pytest.mark.parametrize("T,in_f,out_f", D.LINEAR_FWD_SHAPES)
def test_linear_mutants_pass_the_old_check_and_fail_the_grouped_one(T, in_f, out_f):
    c = D.linear_case("r_scaled", T, in_f, out_f)
    ref32, ref64 = O.linear_relprop(c["R"], c["X"], c["W"]), _lin64(c)
    _mutant_fails_groups_only("mutant.zeroed_rows", _zero_small_rows(ref32), ref32, ref64)
    for case in ("x_scaled", "xr_scaled"):
        c = D.linear_case(case, T, in_f, out_f)
        ref32, ref64 = O.linear_relprop(c["R"], c["X"], c["W"]), _lin64(c)
        two = O.linear_relprop(_two_planes(c["R"]), _two_planes(c["X"]), _two_planes(c["W"]))
        _mutant_fails_groups_only("mutant.two_planes", two, ref32, ref64)
    # Z from the forward output with the cancellation criterion alone: wrong on every small row of X.  Where those rows
    # carry as much relevance as the others (x_scaled) even the whole-tensor metric sees it -- no test scaled a row of X --
    # and where they carry little (xr_scaled) only the grouped check does.
    c = D.linear_case("x_scaled", T, in_f, out_f)
    ref32, ref64 = O.linear_relprop(c["R"], c["X"], c["W"]), _lin64(c)
    old, _ = forward_output_rule(c, None)
    with pytest.raises(AssertionError):
        check_groups("mutant.forward_z", old, ref32, ref64, -1, LINEAR_TOL)
    c = D.linear_case("xr_scaled", T, in_f, out_f)
    ref32, ref64 = O.linear_relprop(c["R"], c["X"], c["W"]), _lin64(c)
    old, _ = forward_output_rule(c, None)
    _mutant_fails_groups_only("mutant.forward_z", old, ref32, ref64)


@pytest.mark.parametrize("case", D.LINEAR_CASES)
@pytest.mark.parametrize("T,in_f,out_f", D.LINEAR_FWD_SHAPES)
def test_forward_output_rule_with_the_bias_term_is_fair(T, in_f, out_f, case):
    """The criterion the kernels use (te_common.h: te_z_cancels, kCancelBiasTol = 2^-4) brings the emulation back to a
    quarter of the bar on every case, the small rows of X and the outlier bias elements included."""
    c = D.linear_case(case, T, in_f, out_f)
    ref32, ref64 = O.linear_relprop(c["R"], c["X"], c["W"]), _lin64(c)
    new, share = forward_output_rule(c, 2.0 ** -4)
    check_groups(f"host.forward_z.{case}", new, ref32, ref64, -1, LINEAR_TOL / 4)
    if case in ("r_scaled", "cls_only"):          # unit-scale X and bias: the new term never fires
        assert share == forward_output_rule(c, None)[1] == 0.0


@pytest.mark.parametrize("case", D.LINEAR_CASES)
@pytest.mark.parametrize("T,in_f,out_f", D.LINEAR_FWD_SHAPES[:2] + D.LINEAR_NOY_SHAPES[1:])
def test_linear_oracle_is_homogeneous_bitwise(T, in_f, out_f, case):
    c = D.linear_case(case, T, in_f, out_f)
    for variant, alpha in (("ours", 1.0), ("ours", 2.0), ("lrp", 1.0)):
        base = O.linear_relprop(c["R"], c["X"], c["W"], alpha, variant)
        for k in D.HOMOGENEITY_K:
            s = D.pow2(-k)
            assert torch.equal(O.linear_relprop(c["R"] * s, c["X"], c["W"], alpha, variant), base * s), (variant, alpha, k)


# ------------------------------------------------------------------------------------------------ attention rules
def _attention_oracles(case, B, H, N, Dh, dtype):
    c = D.attention_case(case, B, H, N, Dh)
    q, k, v, attn = D.attention_operands(c["qkv"], B, H, N, Dh)
    z_av, z_qk = attn @ v, q @ k.transpose(-1, -2)                 # the forward products are operands of the rule
    t = lambda x: x.to(dtype)                                      # noqa: E731
    a, cv = O.einsum_av_relprop(t(c["R"]), t(attn), t(v), t(z_av))
    cam1 = (O.einsum_av_relprop(c["R"], attn, v, z_av)[0] * 0.5)   # the QK rule's input: the fp32 AV result, halved
    cq, ck = O.einsum_qk_relprop(t(cam1), t(q), t(k), t(z_qk))
    return {"cam_attn": a, "cam_v": cv, "cam_q": cq, "cam_k": ck}, (c, q, k, v, attn, z_av, z_qk, cam1)


ATTN_GROUPS = {"cam_attn": -1, "cam_q": -1, "cam_v": (-2, -1), "cam_k": (-2, -1)}


@pytest.mark.parametrize("case", D.ATTN_CASES)
@pytest.mark.parametrize("B,H,N,Dh", D.ATTN_SHAPES)
def test_attention_cases_are_fair_and_homogeneous(B, H, N, Dh, case):
    r32, (c, q, k, v, attn, z_av, z_qk, cam1) = _attention_oracles(case, B, H, N, Dh, torch.float32)
    r64, _ = _attention_oracles(case, B, H, N, Dh, torch.float64)
    for name, dims in ATTN_GROUPS.items():
        check_groups(f"host.attn.{case}.{name}", r32[name], r32[name], r64[name], dims, ATTN_TOL / 4)
    for kk in D.HOMOGENEITY_K:
        s = D.pow2(-kk)
        a, cv = O.einsum_av_relprop(c["R"] * s, attn, v, z_av)
        cq, ck = O.einsum_qk_relprop(cam1 * s, q, k, z_qk)
        assert torch.equal(a, r32["cam_attn"] * s) and torch.equal(cv, r32["cam_v"] * s), kk
        assert torch.equal(cq, r32["cam_q"] * s) and torch.equal(ck, r32["cam_k"] * s), kk
    if case == "head_scaled" and B * H >= 4:       # (heads at 2^-24 and below exist) a rule that loses the small heads passes the whole-tensor metric
        m = r32["cam_v"].clone()
        heads = m.abs().amax((-2, -1), keepdim=True)
        m = torch.where(heads < 1e-5 * heads.max(), torch.zeros_like(m), m)
        check("mutant.attn", m, r32["cam_v"], ATTN_TOL)
        with pytest.raises(AssertionError):
            check_groups("mutant.attn", m, r32["cam_v"], r64["cam_v"], (-2, -1), ATTN_TOL)


# ------------------------------------------------------------------------------------------------ Add, Clone
def _within(got, ref64, rel):
    worst, zeros_ok = D.elementwise_excess(got, ref64, rel)
    assert zeros_ok and worst <= 1.0, worst


@pytest.mark.parametrize("shape", D.ADD_SHAPES)
def test_add_and_clone_oracle_within_half_the_elementwise_bound(shape):
    c = D.add_case(shape)
    d = {k: v.double() for k, v in c.items()}
    for variant in ("ours", "lrp"):
        a, b = O.add_relprop(c["R"], c["X0"], c["X1"], variant)
        a64, b64 = O.add_relprop(d["R"], d["X0"], d["X1"], variant)
        _within(a, a64, ELEMENT_TOL / 2)
        _within(b, b64, ELEMENT_TOL / 2)
    for names in (("R", "R2"), ("R", "R2", "R3")):
        _within(O.clone_relprop([c[n] for n in names], c["X0"]), O.clone_relprop([d[n] for n in names], d["X0"]),
                ELEMENT_TOL / 2)
    # a rule that drops the small samples: invisible to the whole-tensor metric, 100 % element-wise
    a, _ = O.add_relprop(c["R"], c["X0"], c["X1"])
    a64, _ = O.add_relprop(d["R"], d["X0"], d["X1"])
    m = a.clone()
    m[1:] = 0.0
    check("mutant.add", m, a, 2e-5)
    assert D.elementwise_excess(m, a64, ELEMENT_TOL)[0] > 1.0


def test_add_mask_oracle_within_half_the_elementwise_bound():
    c = D.add_mask_case(*D.ADD_MASK_SHAPE)
    a, b = O.add_relprop(c["R"], c["X0"], c["mask"])
    a64, b64 = O.add_relprop(c["R"].double(), c["X0"].double(), c["mask"].double())
    _within(a, a64, ELEMENT_TOL / 2)
    _within(b, b64, ELEMENT_TOL / 2)
    assert not b64.any()                            # masked keys carry no relevance: the mask's share is exactly zero


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 1e-6, -3.0])
    b = torch.tensor([1.0 + 2.0 ** -23, -1.0 - 2.0 ** -22, -0.0, 1e-6, -3.0])
    assert D.ulp_distance(a, b).tolist() == [1, 2, 0, 0, 0]
    assert int(D.ulp_distance(torch.tensor([2.0 ** -149]), torch.tensor([-2.0 ** -149]))) == 2
