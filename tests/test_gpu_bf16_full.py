"""method="full" on a bf16 ViT on the MI355X: the z^B rule of the patch embedding on bf16 operands (csrc/te_conv_bf16.hip).

The rule recomputes conv(X, W) from the model's own bf16 tensors on bf16 MFMAs and never divides by the layer's cached
bf16 output.  Checked against the fp64 oracle next to the fp32 kernel on the exact upcast operands (the criterion of
test_bf16_linear_rule_vs_fp64), for exact zeros and conservation, for determinism (batch == samples, strided and
unaligned relevance views, plane reuse and rebuild), on the fp32-upcast route, and through the model.

Every test fails on a tree without the rule: ops.conv2d_zb_relprop refuses bf16 tensors with a TeError."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import (cache64, d as _d, dev, map_stats, record, rms as _rms, vit_b16_bf16,  # noqa: F401
                      vit_cache_from_model)
from host_util import one_hot
from oracle import relprop_oracle as O
from oracle.model_cache import sliced_relprop_state
from oracle.ref_harness import seeded_randn, synthetic_init

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
T147 = (3, 112, 112, 16, 256)          # T = 147: two row tiles, tiles holding rows of three samples, two column tiles


def _inputs(B, H, W, p, E, seed=0):
    """CPU tensors: X, W bf16 (W: randn * 0.02 with 2 % zeros), a nonzero bf16 bias, R fp32 token-major [B, P, E] with one
    patch's row zeroed, and that patch (sample, py, px)."""
    g = torch.Generator().manual_seed(1000 * seed + E + H + p)
    X = torch.randn(B, 3, H, W, generator=g).to(BF)
    Wt = torch.randn(E, 3, p, p, generator=g) * 0.02
    Wt[torch.rand(Wt.shape, generator=g) < 0.02] = 0.0
    bias = (torch.randn(E, generator=g) * 0.1 + 0.3).to(BF)
    Hp, Wp = H // p, W // p
    R = torch.randn(B, Hp * Wp, E, generator=g)
    zb, zt = B // 2, (Hp * Wp) // 2
    R[zb, zt] = 0.0
    return X, Wt.to(BF), bias, R, (zb, zt // Wp, zt % Wp)


def _as_conv_output(R, Hp, Wp):
    """token-major [B, P, E] -> the [B, E, Hp, Wp] VIEW PatchEmbed.relprop builds (no copy)"""
    return R.unflatten(1, (Hp, Wp)).permute(0, 3, 1, 2)


def _rule_f32(Rv, Xd, Wd, p):
    """the fp32 kernel on the exact upcast operands, Y = their fp32 convolution on the device"""
    from transformer_explainability_amd import ops
    Xf, Wf = Xd.float(), Wd.float()
    return ops.conv2d_zb_relprop(Rv, Xf, Wf, F.conv2d(Xf, Wf, stride=p))


# ------------------------------------------------------------------------------------------------ rule vs fp64
@pytest.mark.parametrize("B,H,W,p,E", [(1, 16, 16, 16, 128), (2, 32, 48, 16, 128), T147, (2, 32, 64, 32, 128)])
def test_bf16_conv_zb_rule_vs_fp64(B, H, W, p, E):
    from transformer_explainability_amd import ops
    assert ops.conv_bf16_route(3, E, p) == "bf16"
    X, Wt, bias, R, (zb, zy, zx) = _inputs(B, H, W, p, E)
    Hp, Wp = H // p, W // p
    Xd, Wd, bd, Rd = X.to(dev()), Wt.to(dev()), bias.to(dev()), R.to(dev())
    Rv = _as_conv_output(Rd, Hp, Wp)
    Y16 = F.conv2d(Xd, Wd, bd, stride=p)                   # what a bf16 layer caches: must play no part
    cache = {}
    got = ops.conv2d_zb_relprop(Rv, Xd, Wd, Y16, bd, cache=cache)
    assert got.dtype == torch.float32 and got.shape == X.shape and "conv_bf16_planes" in cache
    # neither the cached output nor the bias is read
    assert torch.equal(ops.conv2d_zb_relprop(Rv, Xd, Wd, None, None, cache=cache), got)
    f32 = _rule_f32(Rv, Xd, Wd, p)
    R64 = _as_conv_output(R.double(), Hp, Wp)
    ref = O.conv2d_zb_relprop(R64, X.double(), Wt.double(), p)
    e_bf, e_32 = _rms(got, ref), _rms(f32, ref)
    record(f"bf16.conv_zb.{B}x{H}x{W}.p{p}.E{E}", rms_bf16=e_bf, rms_f32=e_32, ratio=e_bf / max(e_32, 1e-300),
           ref_rms=float(ref.pow(2).mean().sqrt()))
    print(f"conv_zb bf16 {B}x{H}x{W} p{p} E{E}: rms_bf16 {e_bf:.3e} rms_f32 {e_32:.3e} ratio {e_bf / max(e_32, 1e-300):.3f}")
    assert torch.isfinite(got).all() and e_bf <= 1.1 * e_32 + 1e-12, (e_bf, e_32)
    # the zeroed patch gives exactly zero pixels
    assert float(got[zb, :, zy * p:(zy + 1) * p, zx * p:(zx + 1) * p].abs().max()) == 0.0
    # conservation per sample (up to the 1e-9 of the denominator): a dropped or doubled patch breaks it at order 1 / P
    g64 = _d(got)
    for b in range(B):
        lhs, rhs = float(g64[b].sum()), float(R[b].double().sum())
        assert abs(lhs - rhs) <= 1e-5 * float(g64[b].abs().sum()), (b, lhs, rhs)


# ------------------------------------------------------------------------------------------------ bits
@pytest.fixture(scope="module")
def t147():
    B, H, W, p, E = T147
    X, Wt, bias, R, _ = _inputs(B, H, W, p, E, seed=1)
    from transformer_explainability_amd import ops
    Xd, Wd, Rd = X.to(dev()), Wt.to(dev()), R.to(dev())
    cache = {}
    got = ops.conv2d_zb_relprop(_as_conv_output(Rd, H // p, W // p), Xd, Wd, None, cache=cache)
    return dict(X=Xd, W=Wd, R=Rd, got=got, cache=cache, Hp=H // p, Wp=W // p, p=p, E=E, B=B)


def test_bf16_conv_zb_repeat_and_plane_reuse(t147):
    from transformer_explainability_amd import ops
    s = t147
    planes = s["cache"]["conv_bf16_planes"][2]
    again = ops.conv2d_zb_relprop(_as_conv_output(s["R"], s["Hp"], s["Wp"]), s["X"], s["W"], None, cache=s["cache"])
    assert torch.equal(again, s["got"])
    assert s["cache"]["conv_bf16_planes"][2] is planes                     # built once per weight version
    assert torch.equal(ops.conv2d_zb_relprop(_as_conv_output(s["R"], s["Hp"], s["Wp"]), s["X"], s["W"], None), s["got"])


def test_bf16_conv_zb_batch_equals_samples(t147):
    from transformer_explainability_amd import ops
    s = t147
    for i in range(s["B"]):
        one = ops.conv2d_zb_relprop(_as_conv_output(s["R"][i:i + 1], s["Hp"], s["Wp"]), s["X"][i:i + 1], s["W"], None,
                                    cache=s["cache"])
        assert torch.equal(one, s["got"][i:i + 1]), i


def test_bf16_conv_zb_strided_and_unaligned_relevance(t147):
    from transformer_explainability_amd import ops
    s = t147
    B, P, E = s["R"].shape
    # cam[:, 1:] of a [B, P + 1, E] tensor, as VisionTransformer.relprop hands it over: consumed in place
    cam = torch.full((B, P + 1, E), 7.0, device=dev())
    cam[:, 1:] = s["R"]
    view = cam[:, 1:]
    assert not view.is_contiguous()
    assert torch.equal(ops.conv2d_zb_relprop(_as_conv_output(view, s["Hp"], s["Wp"]), s["X"], s["W"], None,
                                             cache=s["cache"]), s["got"])
    # a base that is only 4-byte aligned
    buf = torch.empty(B * P * E + 1, device=dev())
    off = buf[1:].view(B, P, E)
    off.copy_(s["R"])
    assert off.data_ptr() % 16 == 4
    assert torch.equal(ops.conv2d_zb_relprop(_as_conv_output(off, s["Hp"], s["Wp"]), s["X"], s["W"], None,
                                             cache=s["cache"]), s["got"])


def test_bf16_conv_zb_weight_replacement_rebuilds_planes(t147):
    from transformer_explainability_amd import ops, rules
    s = t147
    p, E = s["p"], s["E"]
    Rv = _as_conv_output(s["R"], s["Hp"], s["Wp"])
    conv = rules.Conv2d(3, E, kernel_size=p, stride=p).to(dev()).to(BF).eval()
    with torch.no_grad():
        conv.weight.copy_(s["W"])
        conv(s["X"])
    assert torch.equal(conv.relprop(Rv, alpha=1), s["got"])
    planes = rules.x6_cache(conv)["conv_bf16_planes"][2]
    assert torch.equal(conv.relprop(Rv, alpha=1), s["got"]) and rules.x6_cache(conv)["conv_bf16_planes"][2] is planes
    # load_state_dict drops the planes
    W2 = _inputs(*T147, seed=2)[1].to(dev())
    want2 = ops.conv2d_zb_relprop(Rv, s["X"], W2, None)
    assert not torch.equal(want2, s["got"])
    state = {k: v.clone() for k, v in conv.state_dict().items()}
    state["weight"] = W2
    conv.load_state_dict(state)
    assert not rules.x6_cache(conv)
    assert torch.equal(conv.relprop(Rv, alpha=1), want2)
    # an edit autograd does not see (.data) needs ops.x6_invalidate, which reaches the layer through the model
    W3 = _inputs(*T147, seed=3)[1].to(dev())
    want3 = ops.conv2d_zb_relprop(Rv, s["X"], W3, None)
    conv.weight.data.copy_(W3)
    assert ops.x6_invalidate(torch.nn.Sequential(conv)) == 1
    assert torch.equal(conv.relprop(Rv, alpha=1), want3)


def test_bf16_conv_zb_refusals():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    X, Wt, _, R, _ = _inputs(1, 16, 16, 16, 128)
    Xd, Wd, Rv = X.to(dev()), Wt.to(dev()), _as_conv_output(R.to(dev()), 1, 1)
    with pytest.raises(TeError, match="bfloat16"):
        ops.conv2d_zb_relprop(Rv.to(BF), Xd, Wd, None)             # bf16 relevance
    with pytest.raises(TeError, match="bfloat16"):
        ops.conv2d_zb_relprop(Rv, Xd, Wd.float(), None)            # mixed operands
    with pytest.raises(TeError, match="CPU"):
        ops.conv2d_zb_relprop(Rv, X, Wd, None)


# ------------------------------------------------------------------------------------------------ upcast route
@pytest.mark.parametrize("B,H,W,p,E", [(2, 32, 32, 8, 64), (2, 28, 28, 14, 128)])
def test_bf16_conv_zb_upcast_route(B, H, W, p, E):
    """A geometry the bf16 kernel does not tile runs the fp32 kernel on exact fp32 copies with their fp32 convolution
    as Y -- never the layer's bf16 output."""
    from transformer_explainability_amd import ops
    assert ops.conv_bf16_route(3, E, p) == "fp32-upcast"
    X, Wt, bias, R, _ = _inputs(B, H, W, p, E)
    Xd, Wd, bd = X.to(dev()), Wt.to(dev()), bias.to(dev())
    Rv = _as_conv_output(R.to(dev()), H // p, W // p)
    got = ops.conv2d_zb_relprop(Rv, Xd, Wd, F.conv2d(Xd, Wd, bd, stride=p), bd)
    assert got.dtype == torch.float32 and torch.equal(got, _rule_f32(Rv, Xd, Wd, p))


# ------------------------------------------------------------------------------------------------ model
TAIL_KEYS = ("pos_add_x0", "pos_embed", "patch_x", "patch_w")


def test_bf16_full_tail_vs_oracle(vit_b16_bf16):
    """Position-embedding Add, class token dropped, z^B rule, channel sum -- on a seeded relevance, against the fp64
    oracle on the exact upcast cache."""
    model = vit_b16_bf16
    x = seeded_randn((3, 3, 224, 224), 11).to(dev()).to(BF)
    with torch.no_grad():
        model(x)
    cam = seeded_randn((3, 197, 768), 12)
    c, _ = model.add.relprop(cam.to(dev()), alpha=1)
    got = model.patch_embed.relprop(c[:, 1:], alpha=1).sum(dim=1)
    assert got.dtype == torch.float32 and got.shape == (3, 224, 224) and torch.isfinite(got).all()
    cache = cache64(vit_cache_from_model(model), TAIL_KEYS)
    ref = O.vit_full_tail(cam.double(), cache)
    s = map_stats(got, ref)
    record("bf16.vit_b16.full_tail", **s)
    print("bf16 full tail vs fp64 oracle:", s)
    assert s["normalised_max_abs"] <= 1e-4, s


def test_bf16_full_whole_call(vit_b16_bf16):
    from transformer_explainability_amd.generators import LRP
    model = vit_b16_bf16
    B = 3
    x = seeded_randn((B, 3, 224, 224), 13).to(dev()).to(BF)
    full = LRP(model).generate_LRP(x, method="full").clone()
    assert full.dtype == torch.float32 and full.shape == (B, 224, 224) and torch.isfinite(full).all()
    oh = one_hot(model.head.Y)
    for i in range(B):
        with sliced_relprop_state(model, i, B):
            one = model.relprop(oh[i:i + 1], method="full", alpha=1)
        assert torch.equal(one[0], full[i]), i
    # distance to the fp64 oracle over the whole chain, one sample: recorded, not asserted (the chain above the tail is
    # existing code with its own tests)
    with sliced_relprop_state(model, 0, B):
        cache = cache64(vit_cache_from_model(model))
    res = O.vit_relprop(oh[:1].double().cpu(), cache, num_heads=12)
    s = map_stats(full[:1], O.vit_full_tail(res["cam"], cache))
    record("bf16.vit_b16.full.whole_chain.0", **s)
    print("bf16 method=full vs fp64 oracle, whole chain, sample 0:", s)
    assert torch.equal(LRP(model, overlap_backward=True).generate_LRP(x, method="full"), full)


def test_bf16_full_does_not_disturb_fp32_models(vit_b16_bf16):
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP
    m32 = vit.vit_base_patch16_224().eval()
    synthetic_init(m32, 1)
    m32.to(dev())
    x = seeded_randn((2, 3, 224, 224), 17).to(dev())
    before = LRP(m32).generate_LRP(x, method="full").clone()
    assert before.dtype == torch.float32 and torch.isfinite(before).all()
    out16 = LRP(vit_b16_bf16).generate_LRP(x.to(BF), method="full")
    assert torch.isfinite(out16).all()
    assert torch.equal(LRP(m32).generate_LRP(x, method="full"), before)
