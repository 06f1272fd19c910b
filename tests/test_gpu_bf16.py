"""bf16 models on the MI355X: the relprop rules read the model's own bf16 tensors (csrc/te_bf16.hip, the bf16 forms of
csrc/te_elementwise.hip) and evaluate the reference's algorithm in fp32 on them.  Checked against the fp64 oracle on the
same cache (oracle.model_cache.vit_cache_from_model upcasts every cached tensor exactly), rule by rule against the fp32
kernels on the same upcast operands, for determinism, and for not disturbing fp32 models in the same process."""
import pytest
import torch

from gpu_util import (cache64, d as _d, dev, map_stats, record, rms as _rms, vit_b16_bf16,  # noqa: F401
                      vit_cache_from_model)
from host_util import one_hot
from oracle import relprop_oracle as O
from oracle.model_cache import sliced_relprop_state
from oracle.ref_harness import seeded_randn, synthetic_init

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _vit(factory, seed=0, **kw):
    from transformer_explainability_amd import vit
    model = getattr(vit, factory)(**kw).eval()
    synthetic_init(model, seed)
    return model.to(dev()).to(BF)


# ------------------------------------------------------------------------------------------------ end to end
def _oracle_maps(model, oh, i, B, num_heads, start_layers):
    with sliced_relprop_state(model, i, B):
        cache = cache64(vit_cache_from_model(model))
    res = O.vit_relprop(oh[i:i + 1].double().cpu(), cache, num_heads=num_heads, start_layer=0)
    grads = [b["attn_grad"] for b in cache["blocks"]]
    return {sl: O.vit_attribution_tail(grads, res["attn_cams"], sl) for sl in start_layers}


def test_bf16_vit_b16_batch8_vs_oracle(vit_b16_bf16):
    """The first call fails on a tree without bf16 relprop kernels (TeError: fp32-only)."""
    from transformer_explainability_amd.generators import LRP
    model = vit_b16_bf16
    B = 8
    x = seeded_randn((B, 3, 224, 224), 3).to(dev()).to(BF)
    lrp = LRP(model)
    maps0 = lrp.generate_LRP(x, method="transformer_attribution", start_layer=0)
    assert maps0.dtype == torch.float32 and maps0.shape == (B, 196) and torch.isfinite(maps0).all()
    oh = one_hot(model.head.Y)
    maps1 = model.relprop(oh, method="transformer_attribution", start_layer=1, alpha=1)
    worst = {0: 0.0, 1: 0.0}
    for i in range(B):
        ref = _oracle_maps(model, oh, i, B, 12, (0, 1))
        for sl, got in ((0, maps0), (1, maps1)):
            s = map_stats(got[i:i + 1], ref[sl])
            record(f"bf16.vit_b16_b8.map_sl{sl}.{i}", **s)
            assert s["normalised_max_abs"] <= 1e-4, (i, sl, s)
            assert s["rel_linf"] <= 3e-4, (i, sl, s)
            worst[sl] = max(worst[sl], s["rel_linf"])
    record("bf16.vit_b16_b8.summary", worst_rel_sl0=worst[0], worst_rel_sl1=worst[1])


def test_bf16_determinism_and_batch_equals_samples(vit_b16_bf16):
    from transformer_explainability_amd.generators import LRP
    model = vit_b16_bf16
    B = 4
    x = seeded_randn((B, 3, 224, 224), 5).to(dev()).to(BF)
    lrp = LRP(model)
    a = lrp.generate_LRP(x, start_layer=1).clone()
    b = lrp.generate_LRP(x, start_layer=1).clone()
    assert torch.equal(a, b)
    oh = one_hot(model.head.Y)
    for i in range(B):
        with sliced_relprop_state(model, i, B):
            one = model.relprop(oh[i:i + 1], method="transformer_attribution", start_layer=1, alpha=1)
        assert torch.equal(one, a[i:i + 1]), i


def test_bf16_generator_options_and_methods(vit_b16_bf16):
    """overlap_backward / prune give the plain call's bits; the other methods give a finite map or raise TeError."""
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import LRP, Baselines
    model = vit_b16_bf16
    x = seeded_randn((2, 3, 224, 224), 7).to(dev()).to(BF)
    plain = LRP(model).generate_LRP(x, start_layer=1).clone()
    for kw in ({"overlap_backward": True}, {"prune": True}):
        got = LRP(model, **kw).generate_LRP(x, start_layer=1)
        torch.cuda.synchronize()
        assert torch.equal(got, plain), kw
    for method in ("rollout", "last_layer", "last_layer_attn", "second_layer", "full"):
        try:
            out = LRP(model).generate_LRP(x, method=method)
        except TeError:
            continue
        assert out is not None and torch.isfinite(out.float()).all(), method
    for call in (lambda: Baselines(model).generate_cam_attn(x), lambda: Baselines(model).generate_rollout(x)):
        try:
            out = call()
        except TeError:
            continue
        assert torch.isfinite(out.float()).all()


def test_bf16_vit_l16_384_vs_oracle():
    from transformer_explainability_amd.generators import LRP
    model = _vit("vit_large_patch16_224", seed=1, img_size=384)
    B = 2
    x = seeded_randn((B, 3, 384, 384), 11).to(dev()).to(BF)
    maps = LRP(model).generate_LRP(x, start_layer=1)
    assert maps.shape == (B, 576) and maps.dtype == torch.float32
    oh = one_hot(model.head.Y)
    ref = _oracle_maps(model, oh, 1, B, 16, (1,))[1]
    s = map_stats(maps[1:2], ref)
    record("bf16.vit_l16_384.map_sl1.1", **s)
    assert s["normalised_max_abs"] <= 1e-4 and s["rel_linf"] <= 3e-4, s
    del model
    torch.cuda.empty_cache()


def test_bf16_vit_tiny_fallback_route(golden_vit_tiny):
    """Head dim 16 and 64-wide layers: every GEMM-shaped rule takes the fp32-upcast route; same-cache oracle parity."""
    from transformer_explainability_amd import ops, vit
    from transformer_explainability_amd.generators import LRP
    g = golden_vit_tiny
    model = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=10,
                                  qkv_bias=True).eval()
    model.load_state_dict({k[6:]: v for k, v in g.items() if k.startswith("state.")})
    model.to(dev()).to(BF)
    assert ops.linear_bf16_route(34, 64, 192) == "fp32-upcast" and ops.attention_bf16_route(17, 16) == "fp32-upcast"
    x = g["x"].to(dev()).to(BF)
    maps = LRP(model).generate_LRP(x, start_layer=0)
    oh = one_hot(model.head.Y)
    for i in range(2):
        ref = _oracle_maps(model, oh, i, 2, 4, (0,))[0]
        s = map_stats(maps[i:i + 1], ref)
        record(f"bf16.vit_tiny.map_sl0.{i}", **s)
        assert s["normalised_max_abs"] <= 1e-4 and s["rel_linf"] <= 3e-4, s


def test_bf16_no_spill_over_and_refusals():
    from transformer_explainability_amd import ops, vit
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import LRP

    def small(dtype):
        torch.manual_seed(0)
        m = vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=16,
                                  qkv_bias=True).eval()
        return m.to(dev()).to(dtype)
    x = seeded_randn((2, 3, 64, 64), 2).to(dev())
    m32 = small(torch.float32)
    before = LRP(m32).generate_LRP(x).clone()
    LRP(small(BF)).generate_LRP(x.to(BF))
    LRP(_vit("vit_base_patch16_224", seed=2)).generate_LRP(seeded_randn((1, 3, 224, 224), 4).to(dev()).to(BF))
    after = LRP(m32).generate_LRP(x)
    assert torch.equal(before, after)
    with pytest.raises(TeError, match="bfloat16"):
        LRP(small(torch.float16)).generate_LRP(x.half())
    X = torch.randn(4, 256, device=dev()).to(BF)
    W = torch.randn(128, 256, device=dev()).to(BF)
    R = torch.randn(4, 128, device=dev())
    with pytest.raises(TeError, match="alpha"):
        ops.linear_relprop(R, X, W, alpha=2.0)
    with pytest.raises(TeError, match="variant"):
        ops.linear_relprop(R, X, W, variant="lrp")
    with pytest.raises(TeError):
        ops.linear_relprop(R.to(BF), X, W)          # bf16 relevance


# ------------------------------------------------------------------------------------------------ rules vs fp64
def _signed_bf16(shape, seed, zero_frac=0.1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    t[torch.rand(shape, generator=g) < zero_frac] = 0.0
    return t.to(BF)


@pytest.mark.parametrize("T,in_f,out_f", [(1, 768, 2304), (197, 768, 3072), (197, 3072, 768), (203, 1024, 4096),
                                          (197, 1024, 3072)])
def test_bf16_linear_rule_vs_fp64(T, in_f, out_f):
    from transformer_explainability_amd import ops
    assert ops.linear_bf16_route(T, in_f, out_f) == "bf16"
    X = _signed_bf16((T, in_f), 1)
    if T > 2:
        X[T // 2] = 0.0                           # a row with Z = 0: safe_divide gives 0
    W = _signed_bf16((out_f, in_f), 2, zero_frac=0.02, scale=0.02)
    R = torch.randn(T, out_f, generator=torch.Generator().manual_seed(3))
    Xd, Wd, Rd = X.to(dev()), W.to(dev()), R.to(dev())
    cache = {}
    got = ops.linear_relprop(Rd, Xd, Wd, cache=cache)
    assert "bf16_planes" in cache and got.dtype == torch.float32
    f32 = ops.linear_relprop(Rd, Xd.float(), Wd.float())
    ref = O.linear_relprop(R.double(), X.double(), W.double())
    e_bf, e_32 = _rms(got, ref), _rms(f32, ref)
    record(f"bf16.linear.{T}x{in_f}x{out_f}", rms_bf16=e_bf, rms_f32=e_32, ref_rms=float(ref.pow(2).mean().sqrt()))
    assert torch.isfinite(got).all() and e_bf <= 1.1 * e_32 + 1e-12, (e_bf, e_32)
    if T > 2:
        assert float(got[T // 2].abs().max()) == 0.0
    # a second call reuses the cached planes and gives the same bits
    assert torch.equal(ops.linear_relprop(Rd, Xd, Wd, cache=cache), got)
    # per-sample factor (Deferred relevance): same as the materialised relevance, bit for bit
    fac = torch.full((1, 2), 0.75, device=dev())
    gd = ops.linear_relprop(ops.Deferred(Rd.reshape(1, T, out_f), fac[:, 0]), Xd.reshape(1, T, in_f), Wd, cache=cache)
    assert torch.equal(gd.reshape(T, in_f), ops.linear_relprop(Rd * 0.75, Xd, Wd, cache=cache))


def test_bf16_linear_strided_rows_and_upcast_route():
    """cls rows of a [B,N,C] activation are read in place; an untiled shape (1000 classes) takes the fp32-upcast route
    and gives the fp32 kernel's bits on the upcast operands."""
    from transformer_explainability_amd import ops
    B, N, C, O_ = 3, 197, 768, 3072
    X = _signed_bf16((B, N, C), 5).to(dev())
    W = _signed_bf16((O_, C), 6, scale=0.02).to(dev())
    R = torch.randn(B, 1, O_, device=dev())
    got = ops.linear_relprop(R, X[:, :1], W)
    ref = ops.linear_relprop(R, X[:, :1].contiguous(), W)
    assert torch.equal(got, ref)
    assert ops.linear_bf16_route(4, 768, 1000) == "fp32-upcast"
    Wh = _signed_bf16((1000, 768), 7, scale=0.02).to(dev())
    Xh = _signed_bf16((4, 768), 8).to(dev())
    Rh = torch.randn(4, 1000, device=dev())
    assert torch.equal(ops.linear_relprop(Rh, Xh, Wh), ops.linear_relprop(Rh, Xh.float(), Wh.float()))


def _norm_rms(got, ref, den):
    """rms of the error relative to the componentwise condition bound |gate| (|S| |B|) of each output (fp64): with a
    signed Z the raw error is dominated by the few outputs whose S = R / Z is huge, for every fp32 evaluation alike."""
    d = _d(den)
    m = d > 0
    return float((((_d(got) - _d(ref)) / d.clamp_min(1e-300))[m] ** 2).mean().sqrt())


@pytest.mark.parametrize("N", [16, 197, 198, 199, 577, 640])
@pytest.mark.parametrize("with_z", [True, False])
def test_bf16_attention_rules_vs_fp64(N, with_z):
    from transformer_explainability_amd import ops
    B, H, D = (2, 2, 64) if N < 500 else (1, 2, 64)
    C = H * D
    g = torch.Generator().manual_seed(N)
    qkv = (torch.randn(B, N, 3 * C, generator=g)).to(BF).to(dev())
    q, k, v = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)          # strided views of the fused activation
    attn = torch.softmax(torch.randn(B, H, N, N, generator=g) * 2, -1).to(BF).to(dev())
    z_av = torch.matmul(attn, v) if with_z else None
    z_qk = torch.matmul(q, k.transpose(-1, -2)) if with_z else None
    R_av = torch.randn(B, H, N, D, generator=g).to(dev())
    R_qk = torch.randn(B, H, N, N, generator=g).to(dev())
    fac = torch.tensor([[1.5, 0.0], [0.25, 0.0]], device=dev())[:B]
    up = lambda t: None if t is None else t.float()                    # noqa: E731
    for name, fn, args, zz in (
            ("av", ops.matmul_relprop_av, (R_av, attn, v), z_av),
            ("qk", ops.matmul_relprop_qk, (R_qk, q, k), z_qk),
            ("qk_scaled", ops.matmul_relprop_qk, (ops.Deferred(R_qk, fac[:, 0]), q, k), z_qk)):
        got = fn(*args, out_scale=0.5, z=zz)
        f32 = fn(args[0], up(args[1]), up(args[2]), out_scale=0.5, z=up(zz))
        R64 = _d(args[0].materialise() if isinstance(args[0], ops.Deferred) else args[0])
        a64, b64 = _d(args[1]), _d(args[2])
        o = O.einsum_av_relprop if name == "av" else O.einsum_qk_relprop
        z64 = _d(zz) if zz is not None else (a64 @ b64 if name == "av" else a64 @ b64.transpose(-1, -2))
        ref = o(R64, a64, b64, z64)
        den = o(R64.abs(), a64.abs(), b64.abs(), z64.abs())
        for j in range(2):
            e_bf, e_32 = _norm_rms(got[j], ref[j] * 0.5, den[j] * 0.5), _norm_rms(f32[j], ref[j] * 0.5, den[j] * 0.5)
            record(f"bf16.attn.{name}.N{N}.z{int(with_z)}.{j}", rms_bf16=e_bf, rms_f32=e_32)
            assert torch.isfinite(got[j]).all()
            # with the forward product given both kernels divide by the same Z: the products decide (the x6 criterion);
            # a recomputed Z is each kernel's own summation of a mixed-sign sum, so S itself differs there
            bound = 1.1 if with_z else 4.0
            assert e_bf <= bound * e_32 + 1e-12, (name, j, e_bf, e_32)
