"""AttnLRP at pixel level on the MI355X (csrc/te_attnlrp_patch.hip, Conv2d.attnlrp, generate_attnlrp(method="full")).

Rule: every pixel against the fp64 evaluation of the rule on A = ops.alrp_damp(G, y) (bit-tested in test_gpu_attnlrp.py)
within the any-order bound of an E-term fp32 fma chain plus the final rounding,
    |out - ref64| <= sum_c |X_c| 1.01 E 2^-24 sum_e |A_e W_e| + 1.001 2^-24 |ref64| + 2^-149,
derived, not measured.  The tiled kernel equals the one-thread-per-pixel kernel bit for bit (the k order and the patch
addressing), a sample alone equals the sample in the batch, misaligned views give the same bits, and the bf16 entry gives the
f32 entry's bits on exact copies.

Models: the yardstick is the pixel restatement (tests/attnlrp_pixel_ref.py) in fp64; the kernel chain stays within 2 x the
per-sample relative L2 error of the fp32 restatement.  The errors go to attnlrp_pixel_parity.json next to the parity report
(committed as profiles/attnlrp_pixel_parity.json).  With the convolution's bias zeroed and eps = 0 the pixels of a patch sum to
the token call's relevance within the two calls' rounding bounds on the model's own operands.

Every test calls ops.alrp_patch_relevance or passes method= to generate_attnlrp: neither exists without the feature."""
import copy
import json
import os

import pytest
import torch

import attnlrp_pixel_ref as pix
from gpu_util import REPORT, dev, odd_offset_view, rnd
from host_util import same_bits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16 = torch.bfloat16
PARITY = os.path.join(os.path.dirname(REPORT), "attnlrp_pixel_parity.json")
_parity = {}

SPECIAL_Y = [0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0, 1e-6, -1e-6]      # as test_gpu_attnlrp.py plants them

# (B, C, H, W, E, p).  Tiled: 64-token tiles, 64 pixel columns, e in chunks of 32 -- one token (a tile with 63 empty rows), B P =
# 48, 12 and 8 (one partly filled tile), B P = 80 (a whole tile and a partly filled one; C = 2, E = one chunk), p p = 64 / 256 /
# 1024 (1, 4, 16 column tiles), H != W.  Simple: p p not a multiple of 64; E not a multiple of 32; C = 1.
TILED = [(1, 3, 8, 8, 128, 8), (3, 3, 32, 32, 128, 8), (2, 3, 32, 48, 256, 16), (2, 3, 64, 32, 128, 32), (5, 2, 32, 32, 32, 8)]
SIMPLE = [(2, 3, 28, 28, 96, 14), (2, 1, 12, 12, 5, 4)]
# (the tiled kernel does not claim an E that is no multiple of its e step: (2,3,16,16,130,8) is on the simple route)
SIMPLE_ONLY_E = (2, 3, 16, 16, 130, 8)


def _case(shape, seed=0, plant_corners=False):
    """-> G, x0 [B,P+1,E], X [B,C,H,W], W [E,C,p,p] on the device; special values planted in the patch rows of x0"""
    B, C, H, Wd, E, p = shape
    P = (H // p) * (Wd // p)
    G, x0 = rnd((B, P + 1, E), seed + 1) * 2.0, rnd((B, P + 1, E), seed + 2)
    flat = x0[:, 1:].reshape(-1).clone()
    perm = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(seed + 3))[:len(SPECIAL_Y)]
    flat[perm] = torch.tensor(SPECIAL_Y)[:len(perm)]
    x0[:, 1:] = flat.view(B, P, E)
    X, W = rnd((B, C, H, Wd), seed + 4), rnd((E, C, p, p), seed + 5, 0.1)
    if plant_corners:      # one distinct large value per patch corner: a transposed (i, j) or a wrong hp / wp stride cannot cancel
        n = 0
        for b in range(B):
            for hp in range(H // p):
                for wp in range(Wd // p):
                    for (i, j) in ((0, 0), (0, p - 1), (p - 1, 0), (p - 1, p - 1)):
                        n += 1
                        X[b, n % C, hp * p + i, wp * p + j] = 100.0 + 7.0 * n
    return tuple(t.to(dev()) for t in (G, x0, X, W))


def _to_image(acc, B, C, H, Wd, p):
    """[B, P, C p p] (token-major, columns (c, i, j)) -> [B, C, H, W]"""
    return acc.view(B, H // p, Wd // p, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, Wd)


def _ref_and_bound(G, x0, X, W, eps):
    """fp64 on the host: the rule on A = ops.alrp_damp(G, y), and the issue's per-pixel bound"""
    from transformer_explainability_amd import ops
    B, C, H, Wd = X.shape
    E, p = W.shape[0], W.shape[2]
    A = ops.alrp_damp(G[:, 1:].contiguous(), x0[:, 1:].contiguous(), eps).double().cpu()      # [B,P,E]
    X64, W64 = X.double().cpu(), W.double().cpu().view(E, -1)
    acc, mag = A @ W64, A.abs() @ W64.abs()
    ref = (X64 * _to_image(acc, B, C, H, Wd, p)).sum(1)
    bound = (X64.abs() * _to_image(mag, B, C, H, Wd, p)).sum(1) * (1.01 * E * U) + 1.001 * U * ref.abs() + 2.0 ** -149
    return ref, bound


def _assert_within_bound(got, G, x0, X, W, eps, tag):
    ref, bound = _ref_and_bound(G, x0, X, W, eps)
    err = (got.double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print(f"{tag}: worst |out - ref64| / bound = {worst:.3e}, max |ref64| = {float(ref.abs().max()):.3e}")
    assert got.dtype == torch.float32 and got.shape == ref.shape and torch.isfinite(got).all()
    assert bool((err <= bound).all()), (tag, worst)
    assert float(ref.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("shape", TILED + SIMPLE + [SIMPLE_ONLY_E], ids=str)
def test_rule_within_the_rounding_bound(shape, eps):
    from transformer_explainability_amd import ops
    B, C, H, Wd, E, p = shape
    assert ops.alrp_patch_route(C, E, p) == ("tiled" if shape in TILED else "simple")
    G, x0, X, W = _case(shape, seed=sum(shape))
    got = ops.alrp_patch_relevance(G, x0, X, W, eps)
    _assert_within_bound(got, G, x0, X, W, eps, f"rule{shape} eps={eps}")
    if shape in SIMPLE:      # forcing the simple kernel on its own route changes nothing
        assert same_bits(ops.alrp_patch_relevance(G, x0, X, W, eps, simple=True), got)


@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("shape", TILED, ids=str)
def test_tiled_equals_simple_bit_for_bit(shape, eps):
    from transformer_explainability_amd import ops
    G, x0, X, W = _case(shape, seed=11 + sum(shape), plant_corners=True)
    tiled = ops.alrp_patch_relevance(G, x0, X, W, eps)
    simple = ops.alrp_patch_relevance(G, x0, X, W, eps, simple=True)
    assert torch.isfinite(tiled).all() and float(tiled.abs().max()) > 1.0
    assert same_bits(tiled, simple), float((tiled - simple).abs().max())
    _assert_within_bound(tiled, G, x0, X, W, eps, f"corners{shape} eps={eps}")


@pytest.mark.parametrize("shape", [(3, 3, 32, 32, 128, 8), (2, 3, 32, 48, 256, 16), (2, 3, 28, 28, 96, 14)], ids=str)
def test_a_sample_alone_and_misaligned_views_give_the_batch_bits(shape):
    from transformer_explainability_amd import ops
    B = shape[0]
    G, x0, X, W = _case(shape, seed=23)
    batch = ops.alrp_patch_relevance(G, x0, X, W)
    for b in range(B):
        assert same_bits(ops.alrp_patch_relevance(G[b:b + 1], x0[b:b + 1], X[b:b + 1], W), batch[b:b + 1]), b
    # every operand one element past a 16-byte boundary (the single-element staging), then one at a time
    views = [odd_offset_view(t) for t in (G, x0, X, W)]
    assert all(v.data_ptr() % 16 == 4 for v in views)
    assert same_bits(ops.alrp_patch_relevance(*views), batch)
    for i in range(4):
        args = [G, x0, X, W]
        args[i] = views[i]
        assert same_bits(ops.alrp_patch_relevance(*args), batch), i
    # a batch stride that is not the dense one: the rows are read in place
    wide = torch.zeros((B, G.shape[1] + 2, G.shape[2]), device=dev())
    wide[:, :G.shape[1]] = G
    assert same_bits(ops.alrp_patch_relevance(wide[:, :G.shape[1]], x0, X, W), batch)


@pytest.mark.parametrize("shape", [(3, 3, 32, 32, 128, 8), (2, 3, 32, 48, 256, 16)], ids=str)
def test_bf16_entry_is_the_f32_entry_on_exact_copies(shape):
    from transformer_explainability_amd import TeError, ops
    G, x0, X, W = _case(shape, seed=29)
    x0h, Xh, Wh = x0.to(BF16), X.to(BF16), W.to(BF16)
    for simple in (False, True):
        got = ops.alrp_patch_relevance(G, x0h, Xh, Wh, 1e-6, simple=simple)
        want = ops.alrp_patch_relevance(G, x0h.float(), Xh.float(), Wh.float(), 1e-6, simple=simple)
        assert got.dtype == torch.float32 and same_bits(got, want), simple
    assert same_bits(ops.alrp_patch_relevance(G, odd_offset_view(x0h), odd_offset_view(Xh), odd_offset_view(Wh), 1e-6), want)
    _assert_within_bound(want, G, x0h.float(), Xh.float(), Wh.float(), 1e-6, f"bf16{shape}")
    with pytest.raises(TeError, match="torch.bfloat16"):
        ops.alrp_patch_relevance(G, x0h, X, Wh)
    with pytest.raises(TeError, match="torch.bfloat16"):
        ops.alrp_patch_relevance(G.to(BF16), x0h, Xh, Wh)


# ------------------------------------------------------------------------------------------------ models
def _record(tag, **kw):
    _parity[tag] = kw
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        json.dump(_parity, f, indent=1, sort_keys=True)


def _rel_l2(got, want):
    """per-sample ||got - want|| / ||want|| in fp64"""
    got, want = got.detach().double().flatten(1), want.detach().double().flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)


def _assert_within_twice(tag, got, R32, R64):
    e_chain, e_ref = _rel_l2(got, R64), _rel_l2(R32, R64)
    _record(tag, kernel_chain_rel_l2=e_chain.tolist(), fp32_restatement_rel_l2=e_ref.tolist(), ratio=(e_chain / e_ref).tolist())
    print(f"{tag}: chain {e_chain.tolist()} fp32 restatement {e_ref.tolist()}")
    assert torch.isfinite(got).all() and got.dtype == torch.float32
    assert bool((e_chain <= 2.0 * e_ref).all()), (tag, e_chain.tolist(), e_ref.tolist())


def _tiny_vit(seed=3):
    """the vit128 construction of test_gpu_attnlrp.py: img 32, patch 8, dim 128, depth 2, 2 heads"""
    from transformer_explainability_amd import vit
    torch.manual_seed(seed)
    model = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2, num_classes=10,
                                  qkv_bias=True).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return model.to(dev())


@pytest.fixture(scope="module")
def vit128():
    model = _tiny_vit()
    return model, copy.deepcopy(model), copy.deepcopy(model).double(), rnd((3, 3, 32, 32), 31).to(dev())


def test_vit_tiny_pixels_against_the_restatement(vit128):
    from transformer_explainability_amd.generators import LRP
    model, m32, m64, x = vit128
    lrp = LRP(model)
    idx = torch.tensor([1, 7, 4])
    for name, index, eps in (("argmax", None, 1e-6), ("index", idx, 1e-6), ("eps0", idx, 0.0)):
        got = lrp.generate_attnlrp(x, index=index, eps=eps, method="full")
        assert got.shape == (3, 32, 32) and got.dtype == torch.float32
        cls = model.head.Y.detach().argmax(-1) if index is None else index
        _assert_within_twice(f"vit_tiny_dim128_pixels.{name}", got, pix.vit_attnlrp_pixels(m32, x, index=cls, eps=eps)[0],
                             pix.vit_attnlrp_pixels(m64, x.double(), index=cls, eps=eps)[0])
    torch.cuda.synchronize()
    lrp.check()


def test_vit_tiny_pixels_of_a_patch_sum_to_its_token(vit128):
    """bias zeroed, eps = 0.  Per token t: |sum of the patch's pixels - token call| <= the sum over the patch's pixels of the rule
    test's bound (on the model's own G, x0, X, W) + the token call's: fp64 products and sums, one rounding to fp32 --
    1.001 2^-24 |R_t| + E 2^-53 sum_e |x0 G|."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model = copy.deepcopy(vit128[0])
    x = vit128[3]
    with torch.no_grad():
        model.patch_embed.proj.bias.zero_()
    seen = {}
    inner = ops.alrp_patch_relevance

    def spy(G, x0, X, W, eps=1e-6, simple=False):
        seen.update(G=G.clone(), x0=x0.clone(), X=X.clone(), W=W.clone())
        return inner(G, x0, X, W, eps, simple)
    lrp = LRP(model)
    ops.alrp_patch_relevance = spy
    try:
        pixels = lrp.generate_attnlrp(x, eps=0.0, method="full")
    finally:
        ops.alrp_patch_relevance = inner
    tokens = lrp.generate_attnlrp(x, eps=0.0)
    assert pixels.shape == (3, 32, 32) and tokens.shape == (3, 16)
    G, x0, X, W = (seen[k] for k in ("G", "x0", "X", "W"))
    _, bound = _ref_and_bound(G, x0, X, W, 0.0)
    terms = (x0.double() * G.double()).abs().sum(-1)[:, 1:].cpu()
    tol = pix.patch_sums(bound, 8) + 1.001 * U * tokens.double().abs().cpu() + x0.shape[-1] * 2.0 ** -53 * terms
    gap = (pix.patch_sums(pixels.double().cpu(), 8) - tokens.double().cpu()).abs()
    print(f"conservation: worst gap / tolerance = {float((gap / tol).max()):.3e}, max |token| = {float(tokens.abs().max()):.3e}")
    assert float(tokens.abs().max()) > 0.0 and bool((gap <= tol).all()), float((gap / tol).max())


def test_vit_tiny_bf16_reads_the_models_own_tensors(vit128):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model = copy.deepcopy(vit128[0]).to(BF16)
    x = vit128[3].to(BF16)
    seen = {}
    inner = ops.alrp_patch_relevance

    def spy(G, x0, X, W, eps=1e-6, simple=False):
        seen.update(G=G, x0=x0, X=X, W=W, eps=eps)
        return inner(G, x0, X, W, eps, simple)
    lrp = LRP(model)
    ops.alrp_patch_relevance = spy
    try:
        got = lrp.generate_attnlrp(x, method="full")
    finally:
        ops.alrp_patch_relevance = inner
    proj = model.patch_embed.proj
    assert got.shape == (3, 32, 32) and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert seen["G"].dtype == torch.float32 and all(seen[k].dtype == BF16 for k in ("x0", "X", "W"))
    assert seen["x0"].data_ptr() == model.add.X[0].data_ptr() and seen["X"].data_ptr() == proj.X.data_ptr()
    assert seen["W"].data_ptr() == proj.weight.data_ptr() and seen["eps"] == 1e-6
    _assert_within_bound(got, seen["G"], seen["x0"].float(), seen["X"].float(), seen["W"].float(), 1e-6, "vit_tiny_bf16")
    # the token call is what it was
    assert same_bits(lrp.generate_attnlrp(x, method="tokens"), lrp.generate_attnlrp(x))
    torch.cuda.synchronize()
    lrp.check()


def test_eager_graph_replay_and_the_producer_flag_give_the_same_bits(vit128):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP, GraphedCall, _one_hot
    model, _, _, x = vit128
    lrp = LRP(model)
    eager = lrp.generate_attnlrp(x, method="full").clone()
    graphed = GraphedCall(lambda inp: lrp._attnlrp(inp, method="full"), (x,))
    assert same_bits(graphed(x).clone(), eager)
    x2 = rnd((3, 3, 32, 32), 77).to(dev())
    assert same_bits(graphed(x2).clone(), lrp.generate_attnlrp(x2, method="full"))
    assert same_bits(graphed(x).clone(), eager)
    public = GraphedCall(lambda inp: lrp.generate_attnlrp(inp, method="full"), (x,))
    assert same_bits(public(x).clone(), eager)
    torch.cuda.synchronize()
    lrp.check()
    # on the SAME caches the chain does not read the producer flag (test_gpu_attnlrp.py explains why the caches are shared)
    assert not ops.USE_FUSED_PRODUCERS
    try:
        for forward_flag in (False, True):
            ops.USE_FUSED_PRODUCERS = forward_flag
            with torch.no_grad():
                seed = _one_hot(model(x), None)
                maps = []
                for chain_flag in (False, True):
                    ops.USE_FUSED_PRODUCERS = chain_flag
                    maps.append(model.attnlrp(seed, eps=1e-6, method="full"))
            assert maps[0].shape == (3, 32, 32) and same_bits(maps[0], maps[1]), forward_flag
    finally:
        ops.USE_FUSED_PRODUCERS = False


def test_the_token_call_did_not_move(vit128):
    from transformer_explainability_amd.generators import LRP
    model, _, _, x = vit128
    for m, inp in ((model, x), (copy.deepcopy(model).to(BF16), x.to(BF16))):
        lrp = LRP(m)
        a, b = lrp.generate_attnlrp(inp), lrp.generate_attnlrp(inp, method="tokens")
        assert a.shape == (3, 16) and a.dtype == torch.float32 and same_bits(a, b)
        with torch.no_grad():
            seed = torch.zeros_like(m.head.Y, dtype=torch.float32)
            seed[:, 2] = 1.0
            assert same_bits(m.attnlrp(seed), m.attnlrp(seed, method="tokens"))
