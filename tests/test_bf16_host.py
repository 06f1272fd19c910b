"""Host-side checks of the bf16 relprop path (no GPU needed): the C ABI declares, exports and binds the bf16 entry
points, the route functions say which kernels a shape takes, and the dtype / rule refusals are TeErrors."""
import pytest
import torch

BF16_SYMBOLS = ["te_linear_relprop_bf16", "te_linear_relprop_bf16_supported", "te_linear_relprop_bf16_workspace_bytes",
                "te_linear_bf16_weight_planes_bytes", "te_linear_bf16_prepare_weights", "te_matmul_relprop_av_bf16",
                "te_matmul_relprop_qk_bf16", "te_matmul_relprop_bf16_supported",
                "te_matmul_relprop_av_bf16_workspace_bytes", "te_matmul_relprop_qk_bf16_workspace_bytes",
                "te_add_relprop_bf16", "te_add_relprop_deferred_bf16", "te_clone_relprop_bf16",
                "te_clone_relprop_scaled_bf16", "te_index_select_relprop_bf16", "te_gradcam_headmean_bf16"]


from host_util import lib  # noqa: E402,F401


def test_bf16_entry_points_bound(lib):
    from transformer_explainability_amd import _lib
    for name in BF16_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def test_bf16_routes(lib):
    from transformer_explainability_amd import ops
    for T, i, o in ((1, 768, 2304), (12608, 768, 3072), (12608, 3072, 768), (1154, 1024, 4096), (7, 4096, 1024)):
        assert ops.linear_bf16_route(T, i, o) == "bf16", (T, i, o)
    for T, i, o in ((64, 768, 1000), (34, 64, 192), (34, 256, 64)):
        assert ops.linear_bf16_route(T, i, o) == "fp32-upcast", (T, i, o)
    for N in (16, 197, 198, 199, 577, 640):
        assert ops.attention_bf16_route(N, 64) == "bf16"
    assert ops.attention_bf16_route(17, 16) == "fp32-upcast"


def test_bf16_workspaces_and_validation(lib):
    assert lib.te_linear_relprop_bf16_workspace_bytes(197, 768, 3072) >= 3 * 197 * 3072 * 2
    assert lib.te_linear_bf16_weight_planes_bytes(768, 3072) >= 4 * 768 * 3072 * 2
    assert lib.te_matmul_relprop_av_bf16_workspace_bytes(64, 12, 197, 64) >= 3 * 64 * 12 * 197 * 64 * 2
    assert lib.te_matmul_relprop_qk_bf16_workspace_bytes(64, 12, 197, 64) >= 3 * 64 * 12 * 197 * 197 * 2
    # null pointers / unsupported shapes are refused on the host, before any HIP call
    assert lib.te_linear_relprop_bf16(None, 768, None, 0, 1, None, 768, None, None, 4, 768, 768, None, 0, None) == -1
    assert lib.te_matmul_relprop_av_bf16(None, 0, 0, 0, None, None, 0, 0, 0, None, 0, 0, 0, None, None, 0, 0, 0,
                                         1, 1, 8, 64, 1.0, 0, None, 0, None) == -1


def test_bf16_refusals_on_the_host():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    with pytest.raises(TeError, match="bfloat16"):
        ops._prep(torch.zeros(4, dtype=torch.float16))
    with pytest.raises(TeError, match="alpha"):
        ops._bf16_rule("ours", 2.0)
    with pytest.raises(TeError, match="variant"):
        ops._bf16_rule("lrp", 1.0)
    with pytest.raises(TeError, match="CPU"):
        ops.linear_relprop_bf16(torch.zeros(2, 4), torch.zeros(2, 8, dtype=torch.bfloat16),
                                torch.zeros(4, 8, dtype=torch.bfloat16))


def test_one_hot_seed_is_fp32_for_bf16_logits():
    from transformer_explainability_amd.generators import _one_hot
    logits = torch.tensor([[0.1, 2.0, -1.0], [3.0, 0.0, 1.0]], dtype=torch.bfloat16)
    oh = _one_hot(logits, None)
    assert oh.dtype == torch.float32
    assert torch.equal(oh, torch.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]))
    assert _one_hot(logits.float(), None).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ fair inputs
def _fp32_oracle_share(fn32, fn64, tol):
    """max |fp32 oracle - fp64 oracle| / max |fp64 oracle| per output, which must stay within tol / 4."""
    import bf16_rule_inputs as I
    out32, out64 = fn32(), fn64()
    if torch.is_tensor(out32):
        out32, out64 = (out32,), (out64,)
    worst = max(I.rel_to_max(a, b) for a, b in zip(out32, out64))
    assert worst <= tol / 4, (worst, tol)
    return worst


def test_rule_test_inputs_leave_the_tolerance_to_the_kernels():
    """The inputs of test_gpu_bf16_rules.py (zeros, -0.0, exact cancellation, seeds, shapes) must not eat the tolerance
    those tests grant the kernels against the fp64 oracle: the plain fp32 oracle on the same inputs stays within a quarter
    of it, for every Add, Clone and head-mean input the device tests build.  (The second-trip head-mean case is compared
    with the fp32 oracle itself on the device, so it has no share to check.)"""
    import bf16_rule_inputs as I
    from oracle import relprop_oracle as O
    worst = {"add": 0.0, "clone": 0.0, "headmean": 0.0}
    add_cases = sorted({(shape, shared) for shape, _ in I.ADD_CASES for shared in (False, True)})
    for shape, shared in add_cases + [(I.ADD_MODEL_SHAPE, False)]:
        R, X0, X1 = I.add_inputs(shape, shared)
        assert X0.dtype == X1.dtype == torch.bfloat16 and R.dtype == torch.float32
        z = X0.float() + X1.float()
        frac = float(((z == 0) & (X0.float() != 0)).float().mean())
        assert 0.01 < frac < 0.12 or z.numel() < 100, (shape, shared, frac)      # cancellation is really there
        w = _fp32_oracle_share(lambda: O.add_relprop(R, X0.float(), X1.float()),
                               lambda: O.add_relprop(R.double(), X0.double(), X1.double()), I.ADD_TOL)
        worst["add"] = max(worst["add"], w)
    for shape, _ in I.CLONE_CASES:
        for num in (2, 3):
            Rs, X = I.clone_inputs(shape, num)
            fac = I.clone_factors(shape[0])
            variants = [Rs]
            for pos in I.clone_deferred_positions(num):          # the materialised operands of the scaled form
                variants.append([r * fac[:, I.clone_factor_column(j, pos)].view(-1, 1, 1) if j in pos else r
                                 for j, r in enumerate(Rs)])
            for rs in variants:
                w = _fp32_oracle_share(lambda: O.clone_relprop(rs, X.float()),
                                       lambda: O.clone_relprop([r.double() for r in rs], X.double()), I.CLONE_TOL)
                worst["clone"] = max(worst["clone"], w)
    for B, H, N, _ in I.HEADMEAN_CASES:
        g, c = I.headmean_inputs(B, H, N)
        w = _fp32_oracle_share(lambda: O.gradcam_headmean(g.float(), c),
                               lambda: O.gradcam_headmean(g.double(), c.double()), I.HEADMEAN_TOL)
        worst["headmean"] = max(worst["headmean"], w)
    print("fp32 oracle vs fp64 oracle, relative to the tensor maximum:", worst)
