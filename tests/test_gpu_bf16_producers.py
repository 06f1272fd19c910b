"""GPU: the fused attention producers of a bf16 model (csrc/te_attn_bf16.hip; ops.attention_forward_qkv /
attention_backward_qkv on bf16 views, ops.USE_FUSED_PRODUCERS in vit.py / bert.py).

Accuracy is measured against an fp64 evaluation of the UNROUNDED function on the same bf16 inputs; the bar is the error of the
stock bf16 PyTorch path in the same test (torch ops forward, autograd backward, on the device): max-abs and rms error
<= 2 x stock's + 1e-6 -- the producer bar of tests/test_gpu_producers.py.  Both sides are dominated by the same bf16
roundings, so a faithful kernel sits near 1.0 and has the factor as headroom.  Every figure goes to the parity report."""

import pytest
import torch

from gpu_util import bert_base_bf16, cache64, dev, record, rnd, vit_b16_bf16  # noqa: F401
from host_util import one_hot

pytestmark = pytest.mark.gpu

D = 64
SHAPES = [(2, 12, 197), (1, 16, 577), (2, 12, 512), (1, 2, 640), (3, 2, 16), (2, 3, 61), (1, 2, 198), (1, 2, 199), (2, 2, 1)]
MASKED = [(2, 12, 512), (2, 12, 197), (1, 2, 640), (2, 3, 128)]      # BERT: three tensors and a padding mask
MASK_VALUE = -9984.0          # (1 - 0) * -10000 in bf16


def _inputs(B, H, N, layout, seed=81):
    """q, k, v [B,N,C] bf16: strided thirds of one fused activation, or three tensors."""
    C = H * D
    qkv = rnd((B, N, 3 * C), seed).to(dev()).to(torch.bfloat16)
    if layout == "thirds":
        return qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    return tuple(qkv[..., i * C:(i + 1) * C].contiguous() for i in range(3))


def _mask(B, N):
    """Additive bf16 mask [B,1,1,N]: the last 64 keys of every other sample are padding."""
    m = torch.zeros(B, 1, 1, N, device=dev())
    m[0::2, ..., max(N - 64, 1):] = MASK_VALUE
    return m.to(torch.bfloat16)


def _heads(t, H):
    B, N, C = t.shape
    return t.view(B, N, H, D).permute(0, 2, 1, 3)


def _chain(q, k, v, mask, H, scale, g_out):
    """The attention block in the dtype of its operands with torch ops, and its gradients by autograd."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    z = _heads(q, H) @ _heads(k, H).transpose(-1, -2)
    s = z * scale
    if mask is not None:
        s = s + mask.to(s.dtype)
    attn = torch.softmax(s, dim=-1)
    attn.retain_grad()
    B, N, _ = q.shape
    out = (attn @ _heads(v, H)).permute(0, 2, 1, 3).reshape(B, N, H * D)
    out.backward(g_out.to(out.dtype))
    return dict(z_qk=z.detach(), attn=attn.detach(), out=out.detach(), d_attn=attn.grad, d_q=q.grad, d_k=k.grad, d_v=v.grad)


def _err(got, ref64):
    d = (got.double() - ref64).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


def _bars(tag, mine, stock, ref):
    fails = []
    for name in ("z_qk", "attn", "out", "d_attn", "d_q", "d_k", "d_v"):
        (m_max, m_rms), (s_max, s_rms) = _err(mine[name], ref[name]), _err(stock[name], ref[name])
        record(f"bf16_producer.{name}{tag}", max_abs=m_max, rms=m_rms, stock_max_abs=s_max, stock_rms=s_rms,
               ratio_max=m_max / max(s_max, 1e-30), ratio_rms=m_rms / max(s_rms, 1e-30))
        print(f"bf16_producer.{name}{tag}: max {m_max:.4e} (stock {s_max:.4e})  rms {m_rms:.4e} (stock {s_rms:.4e})")
        assert mine[name].dtype == torch.bfloat16 and bool(torch.isfinite(mine[name].float()).all()), name
        if not (m_max <= 2 * s_max + 1e-6 and m_rms <= 2 * s_rms + 1e-6):
            fails.append((name, m_max, s_max, m_rms, s_rms))
    assert not fails, fails


def _run(q, k, v, mask, H, scale, g_out, need_qk=True, want_x=False):
    from transformer_explainability_amd import ops
    out, attn, zqk, xsc = ops.attention_forward_qkv(q, k, v, H, scale, mask=mask, want_z=True, want_x=want_x)
    d_q, d_k, d_v = (torch.full_like(out, 7.0) for _ in range(3))
    d_attn = ops.attention_backward_qkv(g_out, q, k, v, attn, H, scale, d_q, d_k, d_v, need_qk=need_qk, out=out)
    return dict(z_qk=zqk, x=xsc, attn=attn, out=out, d_attn=d_attn, d_q=d_q, d_k=d_k, d_v=d_v)


def _case(B, H, N, layout, masked):
    scale = D ** -0.5
    q, k, v = _inputs(B, H, N, layout)
    mask = _mask(B, N) if masked else None
    g_out = rnd((B, N, H * D), 83).to(dev()).to(torch.bfloat16)
    mine = _run(q, k, v, mask, H, scale, g_out, want_x=masked)
    stock = _chain(q, k, v, mask, H, scale, g_out)
    ref = _chain(q.double(), k.double(), v.double(), mask, H, scale, g_out.double())
    tag = f"({B},{H},{N},{layout}{',mask' if masked else ''})"
    _bars(tag, mine, stock, ref)
    return q, k, v, mask, g_out, mine


@pytest.mark.parametrize("layout", ["thirds", "three"])
@pytest.mark.parametrize("B,H,N", SHAPES)
def test_bf16_producers_accuracy_and_exact_properties(B, H, N, layout):
    from transformer_explainability_amd import ops
    assert ops.attention_forward_bf16_supported(N, D)
    scale = D ** -0.5
    q, k, v, _, g_out, mine = _case(B, H, N, layout, masked=False)
    assert float((mine["attn"].float().sum(-1) - 1).abs().max()) < 2e-2          # rows of bf16 probabilities
    # strided and contiguous operands: the same bits
    other = _run(*_inputs(B, H, N, "three" if layout == "thirds" else "thirds"), None, H, scale, g_out)
    for name in ("z_qk", "attn", "out", "d_attn", "d_q", "d_k", "d_v"):
        assert torch.equal(other[name], mine[name]), name
    # sample i of a batch = the single-sample call, forward and backward
    for i in range(B):
        one = _run(q[i:i + 1], k[i:i + 1], v[i:i + 1], None, H, scale, g_out[i:i + 1])
        for name in ("z_qk", "attn", "out", "d_attn", "d_q", "d_k", "d_v"):
            assert torch.equal(one[name], mine[name][i:i + 1]), (name, i)
    # need_qk = 0: the same d_attn and d_v, d_q / d_k untouched
    low = _run(q, k, v, None, H, scale, g_out, need_qk=False)
    assert torch.equal(low["d_attn"], mine["d_attn"]) and torch.equal(low["d_v"], mine["d_v"])
    assert bool((low["d_q"] == 7.0).all()) and bool((low["d_k"] == 7.0).all())


@pytest.mark.parametrize("B,H,N", MASKED)
def test_bf16_producers_masked(B, H, N):
    scale = D ** -0.5
    q, k, v, mask, g_out, mine = _case(B, H, N, "three", masked=True)
    assert mine["x"].dtype == torch.bfloat16
    assert torch.equal(mine["x"], mine["z_qk"] * scale)                           # from the rounded z_qk; 2^-3: exact
    pad = (mask.view(B, N) != 0)
    assert bool(pad.any())
    attn = mine["attn"]
    assert bool(torch.isfinite(attn.float()).all())
    assert bool((attn.permute(0, 3, 1, 2)[pad] == 0).all())                       # masked keys: exactly 0
    for i in range(B):
        one = _run(q[i:i + 1], k[i:i + 1], v[i:i + 1], mask[i:i + 1], H, scale, g_out[i:i + 1], want_x=True)
        for name in ("z_qk", "x", "attn", "out", "d_attn", "d_q", "d_k", "d_v"):
            assert torch.equal(one[name], mine[name][i:i + 1]), (name, i)


def test_bf16_producers_refuse_other_shapes_and_dtypes():
    from transformer_explainability_amd import TeError, _lib, ops
    lib = _lib.load()
    assert not ops.attention_forward_bf16_supported(641, 64) and not ops.attention_forward_bf16_supported(197, 32)
    assert ops.attention_forward_bf16_supported(640, 64) and ops.attention_forward_bf16_supported(1, 64)
    for N, Dh in ((641, 64), (64, 32)):
        B, H = 1, 2
        C = H * Dh
        t = [torch.zeros(B, N, C, device=dev(), dtype=torch.bfloat16) for _ in range(8)]
        nn_ = [torch.zeros(B, H, N, N, device=dev(), dtype=torch.bfloat16) for _ in range(3)]
        st = (N * C, Dh, C)
        rc = lib.te_attention_forward_strided_bf16(t[0].data_ptr(), *st, t[1].data_ptr(), *st, t[2].data_ptr(), *st, None,
                                                   nn_[0].data_ptr(), None, nn_[1].data_ptr(), t[3].data_ptr(), *st, B, H, N, Dh,
                                                   0.125, None)
        assert rc == _lib.TE_ERR_UNSUPPORTED
        ws = torch.zeros(4096, device=dev(), dtype=torch.uint8)
        rc = lib.te_attention_backward_strided_bf16(t[3].data_ptr(), *st, t[0].data_ptr(), *st, t[1].data_ptr(), *st,
                                                    t[2].data_ptr(), *st, nn_[1].data_ptr(), nn_[2].data_ptr(), t[4].data_ptr(), *st,
                                                    t[5].data_ptr(), *st, t[6].data_ptr(), *st, B, H, N, Dh, 0.125, 1,
                                                    ws.data_ptr(), ws.numel(), None)
        assert rc == _lib.TE_ERR_UNSUPPORTED
    q, k, v = _inputs(1, 2, 16, "three")
    with pytest.raises(TeError, match="bf16 rule got a torch.float32"):
        ops.attention_forward_qkv(q, k.float(), v, 2, 0.125)
    with pytest.raises(TeError, match="float16"):
        ops.attention_forward_qkv(q.half(), k.half(), v.half(), 2, 0.125)
    with pytest.raises(TeError, match="CPU"):
        ops.attention_forward_qkv(q.cpu(), k.cpu(), v.cpu(), 2, 0.125)
    with pytest.raises(TeError, match="planes"):
        ops.attention_forward(torch.cat([q, k, v], -1), 2, 0.125, planes=True)
    # the fused-qkv wrappers: the bits of the three-view calls
    qkv = torch.cat([q, k, v], -1)
    out, attn, zqk = ops.attention_forward(qkv, 2, 0.125)
    o2, a2, z2, _ = ops.attention_forward_qkv(q, k, v, 2, 0.125)
    assert torch.equal(out, o2) and torch.equal(attn, a2) and torch.equal(zqk, z2)
    g = rnd(tuple(out.shape), 5).to(dev()).to(torch.bfloat16)
    d_attn, d_qkv = ops.attention_backward(g, qkv, attn, 2, 0.125)
    dq, dk, dv = (torch.empty_like(out) for _ in range(3))
    d2 = ops.attention_backward_qkv(g, q, k, v, attn, 2, 0.125, dq, dk, dv)
    assert torch.equal(d_attn, d2) and torch.equal(d_qkv, torch.cat([dq, dk, dv], -1))


# ------------------------------------------------------------------------------------------------ models
BF = torch.bfloat16


class _fused:
    """ops.USE_FUSED_PRODUCERS = True inside, restored on the way out."""

    def __enter__(self):
        from transformer_explainability_amd import ops
        self.was, ops.USE_FUSED_PRODUCERS = ops.USE_FUSED_PRODUCERS, True

    def __exit__(self, *exc):
        from transformer_explainability_amd import ops
        ops.USE_FUSED_PRODUCERS = self.was


@pytest.fixture(scope="module")
def vit_b16():
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import vit
    model = vit.vit_base_patch16_224().eval()
    synthetic_init(model, 0)
    return model.to(dev())


def test_bf16_vit_b16_fused_batch8_vs_oracle(vit_b16_bf16):
    """Fails on a tree without the bf16 producers at the `_fused_anchor` assertion: a bf16 block stays on stock PyTorch."""
    from gpu_util import map_stats, vit_cache_from_model
    from oracle import relprop_oracle as O
    from oracle.model_cache import sliced_relprop_state
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd.generators import LRP
    model = vit_b16_bf16
    B = 8
    x = seeded_randn((B, 3, 224, 224), 3).to(dev()).to(BF)
    with _fused():
        lrp = LRP(model)
        maps0 = lrp.generate_LRP(x, method="transformer_attribution", start_layer=0)
        assert all(b.attn._fused_anchor is not None for b in model.blocks)
        assert maps0.dtype == torch.float32 and maps0.shape == (B, 196) and bool(torch.isfinite(maps0).all())
        for blk in model.blocks:
            q, k = blk.attn.matmul1.X
            qkv = blk.attn._fused_anchor
            assert q.dtype == BF and q.untyped_storage().data_ptr() == qkv.untyped_storage().data_ptr() \
                and k.untyped_storage().data_ptr() == qkv.untyped_storage().data_ptr()       # views of the block's qkv
            assert blk.attn.matmul1.Y.dtype == BF and blk.attn.get_attn().dtype == BF \
                and blk.attn.get_attn_gradients().dtype == BF
        oh = one_hot(model.head.Y)
        maps1 = model.relprop(oh, method="transformer_attribution", start_layer=1, alpha=1)
        for i in range(B):
            with sliced_relprop_state(model, i, B):
                cache = cache64(vit_cache_from_model(model))
            res = O.vit_relprop(oh[i:i + 1].double().cpu(), cache, num_heads=12, start_layer=0)
            grads = [b["attn_grad"] for b in cache["blocks"]]
            for sl, got in ((0, maps0), (1, maps1)):
                s = map_stats(got[i:i + 1], O.vit_attribution_tail(grads, res["attn_cams"], sl))
                record(f"bf16_producer.vit_b16_b8.map_sl{sl}.{i}", **s)
                assert s["normalised_max_abs"] <= 1e-4, (i, sl, s)
                assert s["rel_linf"] <= 3e-4, (i, sl, s)


def test_bf16_vit_b16_fused_bits(vit_b16_bf16):
    """Batch = singles, GraphedLRP replay = eager, prune / overlap_backward = the plain fused call, bit for bit."""
    from oracle.model_cache import sliced_relprop_state
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd.generators import LRP, GraphedLRP
    model = vit_b16_bf16
    B = 4
    x = seeded_randn((B, 3, 224, 224), 5).to(dev()).to(BF)
    with _fused():
        lrp = LRP(model)
        plain = lrp.generate_LRP(x, start_layer=1).clone()
        assert all(b.attn._fused_anchor is not None for b in model.blocks)
        assert torch.equal(lrp.generate_LRP(x, start_layer=1), plain)
        lrp.generate_LRP(x, start_layer=1)
        oh = one_hot(model.head.Y)
        for i in range(B):                   # the rules on sample i of the batch's own cache
            with sliced_relprop_state(model, i, B):
                one = model.relprop(oh[i:i + 1], method="transformer_attribution", start_layer=1, alpha=1)
            assert torch.equal(one, plain[i:i + 1]), i
        for kw in ({"overlap_backward": True}, {"prune": True}):
            got = LRP(model, **kw).generate_LRP(x, start_layer=1)
            torch.cuda.synchronize()
            assert torch.equal(got, plain), kw
        glrp = GraphedLRP(lrp, x, method="transformer_attribution", start_layer=1)
        assert torch.equal(glrp(x), plain)
        x2 = seeded_randn((B, 3, 224, 224), 8).to(dev()).to(BF)
        assert torch.equal(glrp(x2).clone(), lrp.generate_LRP(x2, start_layer=1))


def test_bf16_fused_no_spill_over_and_unsupported_shapes_keep_stock(vit_b16, vit_b16_bf16):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP
    x = seeded_randn((2, 3, 224, 224), 9).to(dev())
    before32 = LRP(vit_b16).generate_LRP(x, start_layer=1).clone()
    before16 = LRP(vit_b16_bf16).generate_LRP(x.to(BF), start_layer=1).clone()
    assert all(b.attn._fused_anchor is None for b in vit_b16_bf16.blocks)
    with _fused():
        LRP(vit_b16_bf16).generate_LRP(x.to(BF), start_layer=1)
        # head dim 32 and 26 x 26 + 1 = 677 > 640 tokens: refused by the kernels, the blocks keep the stock route
        torch.manual_seed(0)
        for kw, size in ((dict(embed_dim=64, num_heads=2), 64), (dict(embed_dim=128, num_heads=2), 416)):
            m = vit.VisionTransformer(img_size=size, patch_size=16, depth=2, num_classes=16, qkv_bias=True, **kw).eval()
            m = m.to(dev()).to(BF)
            out = LRP(m).generate_LRP(seeded_randn((1, 3, size, size), 2).to(dev()).to(BF))
            assert bool(torch.isfinite(out).all()) and all(b.attn._fused_anchor is None for b in m.blocks), kw
    assert torch.equal(LRP(vit_b16).generate_LRP(x, start_layer=1), before32)
    assert torch.equal(LRP(vit_b16_bf16).generate_LRP(x.to(BF), start_layer=1), before16)


def test_bf16_fused_vs_stock_distance_to_fp32_maps(vit_b16_bf16):
    """Across caches (fused bf16 against stock bf16) maps are not comparable sample by sample.  What is
    comparable: the distance of each bf16 map to the map of the fp32 model with the upcast weights, min-max-normalised, over 16
    samples -- the fused path's median must be <= 2 x the stock bf16 path's median."""
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP
    m32 = vit.vit_base_patch16_224().eval()
    m32.load_state_dict({k: v.float() for k, v in vit_b16_bf16.state_dict().items()})
    m32.to(dev())
    x = seeded_randn((16, 3, 224, 224), 11).to(dev()).to(BF)

    def norm(m):
        lo, hi = m.amin(-1, keepdim=True), m.amax(-1, keepdim=True)
        return (m - lo) / (hi - lo)
    ref = norm(LRP(m32).generate_LRP(x.float(), start_layer=1).double())
    stock = norm(LRP(vit_b16_bf16).generate_LRP(x, start_layer=1).double())
    with _fused():
        fused = norm(LRP(vit_b16_bf16).generate_LRP(x, start_layer=1).double())
    d_stock = (stock - ref).abs().amax(-1)
    d_fused = (fused - ref).abs().amax(-1)
    ms, mf = float(d_stock.median()), float(d_fused.median())
    record("bf16_producer.vit_b16.distance_to_fp32_maps", stock_median=ms, fused_median=mf, stock_max=float(d_stock.max()),
           fused_max=float(d_fused.max()))
    print(f"distance to the fp32 maps: stock bf16 median {ms:.4e} max {float(d_stock.max()):.4e}; "
          f"fused bf16 median {mf:.4e} max {float(d_fused.max()):.4e}")
    assert mf <= 2 * ms, (mf, ms)


def _ids_mask(B, N, pad=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 20000, (B, N), generator=g)
    mask = torch.ones(B, N)
    mask[::2, N - pad:] = 0
    return ids.to(dev()), mask.to(dev())


def test_bf16_bert_base_512_fused_vs_oracle(bert_base_bf16):
    from gpu_util import bert_cache_from_model, map_stats, sliced_relprop_state
    from oracle import relprop_oracle as O
    from transformer_explainability_amd.generators import Generator
    model = bert_base_bf16
    B, N = 4, 512
    ids, mask = _ids_mask(B, N)
    before = Generator(model).generate_LRP(ids, mask, start_layer=0).clone()
    with _fused():
        gen = Generator(model)
        out = gen.generate_LRP(ids, mask, start_layer=0).clone()
        layers = model.bert.encoder.layer
        assert all(lay.attention.self._fused_anchor is not None for lay in layers)
        assert out.dtype == torch.float32 and out.shape == (B, N) and bool(torch.isfinite(out).all())
        assert torch.equal(gen.generate_LRP(ids, mask, start_layer=0), out)
        for lay in layers:
            sa = lay.attention.self
            assert sa.add.X[0].dtype == BF and sa.add.X[1].dtype == BF and sa.matmul1.Y.dtype == BF
            assert torch.equal(sa.add.X[0], sa.matmul1.Y * 0.125)          # the producer's x = z_qk * scale
            pad = (mask == 0)
            assert bool((sa.get_attn().permute(0, 3, 1, 2)[pad] == 0).all())
        oh = one_hot(model.classifier.Y)
        for i in (0, 1):                               # padded, unpadded
            with sliced_relprop_state(model, i, B):
                cache = cache64(bert_cache_from_model(model))
                model.relprop(oh[i:i + 1], alpha=1)
                one = gen.attribution_tail(start_layer=0)
                assert torch.equal(one, out[i:i + 1]), float((one - out[i:i + 1]).abs().max())
            ref = O.bert_relprop(oh[i:i + 1].double().cpu(), cache, num_heads=12, start_layer=0)
            s = map_stats(out[i:i + 1], ref["map"])
            record(f"bf16_producer.bert_base_512.oracle.map_sl0.{i}", **s)
            assert s["normalised_max_abs"] <= 1e-4 and s["rel_linf"] <= 3e-4, (i, s)
    # flag off again: the stock route's bits, untouched by the fused calls
    assert torch.equal(Generator(model).generate_LRP(ids, mask, start_layer=0), before)
    assert all(lay.attention.self._fused_anchor is None for lay in model.bert.encoder.layer)


def test_bf16_bert_fused_graphed_call_replays_eager(bert_base_bf16):
    from transformer_explainability_amd.generators import GraphedCall, Generator
    model = bert_base_bf16
    with _fused():
        ids, mask = _ids_mask(2, 128, pad=16, seed=3)
        gen = Generator(model)
        eager = gen.generate_LRP(ids, mask, start_layer=0).clone()
        assert all(lay.attention.self._fused_anchor is not None for lay in model.bert.encoder.layer)
        g = GraphedCall(lambda i, m: gen.generate_LRP(i, m, start_layer=0), (ids, mask))
        got = g(ids, mask).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, eager)
        ids2, mask2 = _ids_mask(2, 128, pad=40, seed=4)
        eager2 = gen.generate_LRP(ids2, mask2, start_layer=0).clone()
        assert torch.equal(g(ids2, mask2).clone(), eager2)
