"""Host-side checks of the bf16 evaluation pipeline (no GPU needed): te_perturb_bf16 and te_attn_headmean_bf16 are declared,
exported and bound, their argument checks answer before any device call, the Python wrappers refuse what has no kernel
with a TeError, and the sweep refuses the lrp rule library on a bf16 model before anything reaches the store."""
import ctypes

import pytest
import torch

from host_util import header_args, lib  # noqa: F401

BF = torch.bfloat16
NEW_SYMBOLS = ["te_perturb_bf16", "te_attn_headmean_bf16"]
CFG = dict(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=10, qkv_bias=True)


def test_entry_points_declared_exported_bound(lib):
    from transformer_explainability_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == header_args(name), name
    # the bf16-output form takes te_perturb_f32's arguments
    assert _lib.SIGNATURES["te_perturb_bf16"] == _lib.SIGNATURES["te_perturb_f32"]
    assert header_args("te_perturb_bf16") == header_args("te_perturb_f32")


def test_perturb_bf16_validates_on_the_host(lib):
    """Argument checks return before any HIP call (the pointers below are never dereferenced)."""
    p = ctypes.c_void_p(256)
    ks = (ctypes.c_int64 * 3)(0, 5, 9)
    ws = lib.te_perturb_workspace_bytes(2, 3)
    assert ws > 0
    for f in (lib.te_perturb_bf16, lib.te_perturb_f32):            # one front end: the same answers
        assert f(None, p, p, 2, 3, 64, ks, 3, None, None, p, ws, None) == -1
        assert f(p, None, p, 2, 3, 64, ks, 3, None, None, p, ws, None) == -1
        assert f(p, p, None, 2, 3, 64, ks, 3, None, None, p, ws, None) == -1
        assert f(p, p, p, 2, 3, 64, None, 3, None, None, p, ws, None) == -1
        assert f(p, p, p, 0, 3, 64, ks, 3, None, None, p, ws, None) == -1
        assert f(p, p, p, 2, 3, 0, ks, 3, None, None, p, ws, None) == -1
        assert f(p, p, p, 2, 3, 64, ks, 0, None, None, p, ws, None) == -1          # n_steps <= 0
        assert f(p, p, p, 2, 3, 64, ks, -2, None, None, p, ws, None) == -1
        assert f(p, p, p, 2, 5, 64, ks, 3, None, None, p, ws, None) == -3          # > TE_PERTURB_MAX_CHANNELS
        assert f(p, p, p, 2, 3, 64, ks, 17, None, None, p, 1 << 20, None) == -3    # > TE_PERTURB_MAX_STEPS
        assert f(p, p, p, 2, 3, 64, ks, 3, None, None, None, ws, None) == -2
        assert f(p, p, p, 2, 3, 64, ks, 3, None, None, p, 8, None) == -2


def test_attn_headmean_bf16_validates_on_the_host(lib):
    p = ctypes.c_void_p(256)
    f = lib.te_attn_headmean_bf16
    assert f(None, 12 * 49, 49, p, 2, 12, 7, 0, None) == -1
    assert f(p, 12 * 49, 49, None, 2, 12, 7, 0, None) == -1
    assert f(p, 12 * 49, 49, p, 0, 12, 7, 0, None) == -1
    assert f(p, 12 * 49, 49, p, 2, 0, 7, 0, None) == -1
    assert f(p, 12 * 49, 49, p, 2, 12, 0, 0, None) == -1                           # N <= 0
    assert f(p, 12 * 49, 49, p, 2, 12, -3, 0, None) == -1
    assert f(p, 12 * 49, 49, p, 2, 12, 7, 4, None) == -1                           # unknown flag bit
    assert f(p, 49, 49, p, 70000, 1, 7, 0, None) == -3                             # the grid's batch limit


def test_wrappers_refuse_without_a_kernel():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    vis, data = torch.zeros(2, 64), torch.zeros(2, 3, 8, 8)
    with pytest.raises(TeError, match="out_dtype"):
        ops.perturb(vis, data, [0, 5], out_dtype=torch.float16)
    with pytest.raises(TeError, match="CPU"):
        ops.perturb(vis, data, [0, 5], out_dtype=BF)
    with pytest.raises(TeError, match="CPU"):
        ops.perturb(vis, data, [0, 5])
    with pytest.raises(TeError, match="CPU"):
        ops.attn_headmean(torch.zeros(2, 4, 8, 8, dtype=BF))
    with pytest.raises(TeError, match="bfloat16"):
        ops.attn_headmean(torch.zeros(2, 4, 8, 8))                                 # fp32 keeps its torch expression
    with pytest.raises(TeError, match="bfloat16"):
        ops.attn_headmean(torch.zeros(2, 4, 8, 8, dtype=torch.float16))
    for word in ("bfloat16", "alpha", "variant"):
        assert word in ops.DTYPES_MSG


def test_evaluator_takes_the_classifier_dtype_once():
    from transformer_explainability_amd import vit
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.perturbation import PerturbationEvaluator
    model = vit.VisionTransformer(**CFG).eval()
    assert PerturbationEvaluator(model, 4, image_pixels=32 * 32).input_dtype == torch.float32
    assert PerturbationEvaluator(model.to(BF), 4, image_pixels=32 * 32).input_dtype == BF
    with pytest.raises(TeError, match="bfloat16"):
        PerturbationEvaluator(model.to(torch.float16), 4, image_pixels=32 * 32)


@pytest.mark.parametrize("method", ["full_lrp", "lrp_last_layer"])
def test_sweep_refuses_the_lrp_library_on_bf16_and_leaves_the_store_empty(method, tmp_path):
    from transformer_explainability_amd import rules_lrp, vit
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import LRP
    from transformer_explainability_amd.sweep import ResultsStore, SaliencySweep
    torch.manual_seed(0)
    orig = vit.make_vit_module(rules_lrp)["VisionTransformer"](**CFG).eval().to(BF)
    sw = SaliencySweep(method, orig_lrp=LRP(orig))
    g = torch.Generator().manual_seed(1)
    batches = [(torch.rand((3, 3, 32, 32), generator=g), torch.tensor([1, 2, 3]))]
    store = ResultsStore(str(tmp_path), 3, (3, 32, 32), (1, 32, 32), backend="npy")
    with pytest.raises(TeError, match="variant"):
        sw.run(batches, store)
    assert store.count == 0
    store.close()


def test_sweep_casts_the_batch_to_the_model_dtype():
    """explain() hands the generator a batch in its model's dtype (a bf16 patch embedding refuses fp32 images)."""
    from transformer_explainability_amd.sweep import SaliencySweep

    class Gen:
        def __init__(self, dtype):
            self.model = torch.nn.Linear(2, 2).to(dtype)
            self.seen = None

        def generate_LRP(self, data, **kw):
            self.seen = data.dtype
            return torch.rand(data.shape[0], 16)

    from oracle_backend import oracle_ops
    for dtype in (BF, torch.float32):
        gen = Gen(dtype)
        with oracle_ops():
            heat = SaliencySweep("transformer_attribution", lrp=gen).explain(torch.rand(2, 3, 32, 32))
        assert gen.seen == dtype and heat.dtype == torch.float32 and heat.shape == (2, 1, 32, 32)
