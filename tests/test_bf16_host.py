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


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib
    return _lib.load()


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
