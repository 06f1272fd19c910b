"""bf16 BERT on the MI355X: the broadcast-mask Add of BERT self-attention reads bf16 X0 and mask (te_add_bcast_relprop_bf16
and its deferred form) and gives the fp32 kernel's bits on exact fp32 copies of them; a bf16 BertForSequenceClassification
gets fp32 maps that match the fp64 oracle on the same cache (oracle.model_cache.bert_cache_from_model upcasts exactly).

The oracle recomputes the mask Add's first operand as z_qk / sqrt(D) in fp32: that is the bf16 forward's add.X[0] exactly
only when sqrt(D) is a power of two, hence head dims 16 and 64 below."""
import pytest
import torch

from gpu_util import (bert_base_bf16, bert_cache_from_model, cache64, dev, map_stats, record,  # noqa: F401
                      sliced_relprop_state, stats)
from host_util import one_hot
from oracle import relprop_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _bits_equal(name, got, ref):
    got, ref = got.detach(), ref.detach()
    eq = bool(torch.equal(got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)))
    record(name, bitwise_equal=eq, max_abs=float((got - ref).abs().max()))
    return eq


# ------------------------------------------------------------------------------------------------ the mask Add kernel
def _mask_add_operands(B, H, N, mask_batch, seed):
    g = torch.Generator().manual_seed(seed)
    X0 = (torch.randn(B, H, N, N, generator=g) * 3.0).to(BF)
    m = torch.zeros(mask_batch, N)
    m[:, N - max(1, N // 8):] = -9984.0            # bf16(-10000): padding
    m[:, 1:3] = -39.0                              # soft entries (attention_mask 1 - 2^-8)
    if N > 8:
        m[0, 5] = -3.0
    m = m.to(BF).reshape(mask_batch, 1, 1, N)
    R = torch.randn(B, H, N, N, generator=g)
    R[:, :, 0] = 0.0                               # all-zero relevance rows
    R[0, H - 1, N // 2] = 0.0
    if B > 2:
        R[B - 1] = 0.0                             # and a sample without relevance (factors 0)
    return R.to(dev()), X0.to(dev()), m.to(dev())


def _direct_deferred(fn, R, X0, mask2d, B, H, N):
    from transformer_explainability_amd import _lib, ops
    lib = _lib.load()
    a = torch.empty(R.shape, dtype=torch.float32, device=R.device)
    out1 = torch.empty((B, N), dtype=torch.float32, device=R.device)
    fac = torch.empty((B, 2), dtype=torch.float32, device=R.device)
    ws = ops._ws(lib.te_add_bcast_relprop_workspace_bytes(B, H, N), R)
    _lib.check(getattr(lib, fn)(R.data_ptr(), X0.data_ptr(), mask2d.data_ptr(), a.data_ptr(), out1.data_ptr(),
                                fac.data_ptr(), B, H, N, ws.data_ptr(), ws.numel(), ops._stream(R)), fn)
    return a, out1, fac


@pytest.mark.parametrize("N,H,B,mask_batch", [(24, 2, 3, 3), (197, 12, 1, 1), (512, 12, 3, 1), (1000, 2, 3, 3)])
def test_bcast_mask_add_bf16_bits_equal_f32_on_upcast_copies(N, H, B, mask_batch):
    """Fails on a tree without the bf16 mask Add (TeError: unsupported operand shapes)."""
    from transformer_explainability_amd import ops
    R, X0, mask = _mask_add_operands(B, H, N, mask_batch, seed=N + H + B)
    X0f, maskf = X0.float(), mask.float()
    tag = f"bf16.bert_mask_add.N{N}.H{H}.B{B}.m{mask_batch}"
    p16 = ops.add_relprop(R, X0, mask)
    p32 = ops.add_relprop(R, X0f, maskf)
    d16 = ops.add_relprop(R, X0, mask, deferred=True)
    d32 = ops.add_relprop(R, X0f, maskf, deferred=True)
    assert isinstance(d16[0], ops.Deferred) and p16[0].dtype == torch.float32 and p16[1].shape == (B, 1, 1, N)
    m2 = mask.reshape(mask_batch, N).expand(B, N).contiguous()
    a16, o16, f16 = _direct_deferred("te_add_bcast_relprop_deferred_bf16", R, X0, m2, B, H, N)
    a32, o32, f32 = _direct_deferred("te_add_bcast_relprop_deferred_f32", R, X0f, m2.float(), B, H, N)
    results = {
        "out0": _bits_equal(tag + ".out0", p16[0], p32[0]),
        "out1": _bits_equal(tag + ".out1", p16[1], p32[1]),
        "deferred.a": _bits_equal(tag + ".deferred.a", d16[0].t, d32[0].t),
        "deferred.fa": _bits_equal(tag + ".deferred.fa", d16[0].scale, d32[0].scale),
        "deferred.out1": _bits_equal(tag + ".deferred.out1", d16[1], d32[1]),
        "c.a": _bits_equal(tag + ".c.a", a16, a32),
        "c.out1": _bits_equal(tag + ".c.out1", o16, o32),
        "c.fac": _bits_equal(tag + ".c.fac", f16, f32),
        "a*fa==out0": _bits_equal(tag + ".a_fa_vs_out0", d16[0].materialise(), p16[0]),
        "out1 forms": _bits_equal(tag + ".out1_forms", d16[1], p16[1]),
    }
    assert all(results.values()), results
    assert torch.isfinite(p16[0]).all() and torch.isfinite(p16[1]).all()
    if B > 2:
        assert not p16[0][B - 1].any() and not p16[1][B - 1].any()
    assert not p16[0][:, :, 0].any()


def test_bcast_mask_add_bf16_vs_fp64():
    from transformer_explainability_amd import ops
    B, H, N = 3, 2, 197
    R, X0, mask = _mask_add_operands(B, H, N, 1, seed=5)
    out0, out1 = ops.add_relprop(R, X0, mask)
    ref0, ref1 = O.add_relprop(R.double().cpu(), X0.double().cpu(), mask.double().cpu())
    for name, got, ref in (("out0", out0, ref0), ("out1", out1, ref1)):
        s = stats(got, ref)
        record(f"bf16.bert_mask_add.fp64.{name}", **s)
        assert s["nonfinite"] == 0 and s["rel"] <= 1e-5, (name, s)
    from transformer_explainability_amd._lib import TeError
    with pytest.raises(TeError, match="mask"):                   # scores [B,H,N-1,N]: refused on the host
        ops.add_relprop(R[:, :, 1:], X0[:, :, 1:], mask)


# ------------------------------------------------------------------------------------------------ BERT-base, N = 512
def _ids_mask(B, N, pad=64, seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 20000, (B, N), generator=g)
    mask = torch.ones(B, N)
    mask[::2, N - pad:] = 0                        # even samples padded, odd ones not (test_config3's inputs)
    return ids.to(dev()), mask.to(dev())


def test_bf16_bert_base_512_vs_oracle(bert_base_bf16):
    from transformer_explainability_amd.generators import Generator
    model = bert_base_bf16
    B, N = 4, 512
    ids, mask = _ids_mask(B, N)
    gen = Generator(model)
    out = gen.generate_LRP(ids, mask, start_layer=0).clone()
    assert out.dtype == torch.float32 and out.shape == (B, N) and torch.isfinite(out).all()
    assert torch.equal(gen.generate_LRP(ids, mask, start_layer=0), out)
    sa = model.bert.encoder.layer[0].attention.self
    assert sa.add.X[0].dtype == BF and sa.add.X[1].dtype == BF
    oh = one_hot(model.classifier.Y)
    cam = model.relprop(oh, alpha=1)
    assert cam.dtype == torch.float32
    sums = cam.double().sum(dim=(1, 2)).cpu()
    record("bf16.bert_base_512.conservation", min=float(sums.min()), max=float(sums.max()))
    assert (sums - 1.0).abs().max() < 2e-3, sums
    for i in (0, 1):                               # padded, unpadded
        with sliced_relprop_state(model, i, B):
            cache = cache64(bert_cache_from_model(model))
            model.relprop(oh[i:i + 1], alpha=1)
            one = gen.attribution_tail(start_layer=0)
            assert torch.equal(one, out[i:i + 1]), float((one - out[i:i + 1]).abs().max())
        ref = O.bert_relprop(oh[i:i + 1].double().cpu(), cache, num_heads=12, start_layer=0)
        s = map_stats(out[i:i + 1], ref["map"])
        record(f"bf16.bert_base_512.oracle.map_sl0.{i}", **s)
        assert s["normalised_max_abs"] <= 1e-4 and s["rel_linf"] <= 3e-4, (i, s)


def test_bf16_bert_base_512_options_give_the_plain_bits(bert_base_bf16):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import Generator
    model = bert_base_bf16
    B, N = 4, 512
    ids, mask = _ids_mask(B, N, seed=2)
    plain = Generator(model).generate_LRP(ids, mask, start_layer=0).clone()
    plain11 = Generator(model).generate_LRP(ids, mask).clone()          # the reference's default start_layer = 11
    got = {}
    try:
        ops.USE_DEFERRED_ADD = False
        got["no_deferred_add"] = (Generator(model).generate_LRP(ids, mask, start_layer=0).clone(), plain)
    finally:
        ops.USE_DEFERRED_ADD = True
    try:
        model.bert.exploit_cls_sparsity = False
        got["dense_last_layer"] = (Generator(model).generate_LRP(ids, mask, start_layer=0).clone(), plain)
    finally:
        model.bert.exploit_cls_sparsity = True
    got["prune_sl11"] = (Generator(model, prune=True).generate_LRP(ids, mask).clone(), plain11)
    got["prune_sl0"] = (Generator(model, prune=True).generate_LRP(ids, mask, start_layer=0).clone(), plain)
    ov = Generator(model, overlap_backward=True).generate_LRP(ids, mask, start_layer=0)
    torch.cuda.synchronize()
    got["overlap_backward"] = (ov.clone(), plain)
    for name, (a, b) in got.items():
        assert a.dtype == torch.float32 and a.shape == (B, N) and torch.isfinite(a).all(), name
    eq = {name: _bits_equal(f"bf16.bert_base_512.{name}", a, b) for name, (a, b) in got.items()}
    assert all(eq.values()), eq


def test_bf16_bert_graphed_call_replays_eager(bert_base_bf16):
    from transformer_explainability_amd.generators import GraphedCall, Generator
    model = bert_base_bf16
    ids, mask = _ids_mask(2, 128, pad=16, seed=3)
    gen = Generator(model)
    eager = gen.generate_LRP(ids, mask, start_layer=0).clone()
    g = GraphedCall(lambda i, m: gen.generate_LRP(i, m, start_layer=0), (ids, mask))
    got = g(ids, mask).clone()
    torch.cuda.synchronize()
    assert _bits_equal("bf16.bert_base_128.graphed_vs_eager", got, eager)
    ids2, mask2 = _ids_mask(2, 128, pad=40, seed=4)
    eager2 = gen.generate_LRP(ids2, mask2, start_layer=0).clone()
    assert _bits_equal("bf16.bert_base_128.graphed_vs_eager.2", g(ids2, mask2).clone(), eager2)


# ------------------------------------------------------------------------------------------------ small models
def _oracle_check(name, model, out, oh, B, num_heads, start_layer=0):
    for i in range(B):
        with sliced_relprop_state(model, i, B):
            cache = cache64(bert_cache_from_model(model))
        ref = O.bert_relprop(oh[i:i + 1].double().cpu(), cache, num_heads=num_heads, start_layer=start_layer)
        s = map_stats(out[i:i + 1], ref["map"])
        record(f"{name}.{i}", **s)
        assert s["normalised_max_abs"] <= 1e-4 and s["rel_linf"] <= 3e-4, (name, i, s)


def test_bf16_bert_tiny_fp32_upcast_routes_vs_oracle(golden_bert_tiny):
    """Head dim 16 and 64-wide layers: every GEMM-shaped rule takes the fp32-upcast route; the mask Add is bf16."""
    from transformer_explainability_amd import bert, ops
    from transformer_explainability_amd.generators import Generator
    g = golden_bert_tiny
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=64, num_hidden_layers=3, num_attention_heads=4,
                              intermediate_size=128, max_position_embeddings=40, num_labels=2)
    model = bert.BertForSequenceClassification(cfg).eval()
    model.load_state_dict({k[6:]: v for k, v in g.items() if k.startswith("state.")})
    model.to(dev()).to(BF)
    assert ops.attention_bf16_route(24, 16) == "fp32-upcast" and ops.linear_bf16_route(48, 64, 64) == "fp32-upcast"
    ids, mask = g["input_ids"].long().to(dev()), g["attention_mask"].to(dev())
    for sl in (0, 2):
        out = Generator(model).generate_LRP(ids, mask, start_layer=sl)
        assert out.dtype == torch.float32 and out.shape == (2, 24)
        _oracle_check(f"bf16.bert_tiny.map_sl{sl}", model, out, one_hot(model.classifier.Y), 2, 4, sl)


def _soft_mask_model(dtype):
    """The model of test_bert_soft_mask_fused_equals_stock_and_oracle (head dim 64)."""
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                              intermediate_size=256, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(11)
    model = bert.BertForSequenceClassification(cfg).eval()
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return model.to(dev()).to(dtype)


def _soft_mask_inputs():
    B, N = 3, 24
    ids = torch.randint(1, 100, (B, N), generator=torch.Generator().manual_seed(12)).to(dev())
    mask = torch.ones(B, N)
    mask[:, 5:9] = 0.99609375        # 1 - 2^-8, which bf16 keeps: extended mask -39.0 (0.9997 would round to 1)
    mask[1, 20:] = 0.0
    return ids, mask.to(dev())


def test_bf16_bert_soft_mask_vs_oracle():
    from transformer_explainability_amd.generators import Generator
    model = _soft_mask_model(BF)
    ids, mask = _soft_mask_inputs()
    out = Generator(model).generate_LRP(ids, mask, start_layer=0)
    ext = model.bert.encoder.layer[0].attention.self.add.X[1]
    assert ext.dtype == BF and float(ext[0, 0, 0, 5]) == -39.0 and float(ext[1, 0, 0, 21]) == -9984.0
    _oracle_check("bf16.bert_soft_mask.map_sl0", model, out, one_hot(model.classifier.Y), 3, 2)


def test_bf16_bert_other_methods_fp16_refusal_and_fp32_untouched():
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import Generator
    ids, mask = _soft_mask_inputs()
    m32 = _soft_mask_model(torch.float32)
    before = Generator(m32).generate_LRP(ids, mask, start_layer=0).clone()
    model = _soft_mask_model(BF)
    gen = Generator(model)
    outcome = {}
    for name in ("generate_LRP_last_layer", "generate_full_lrp", "generate_attn_gradcam",
                 "generate_attn_last_layer", "generate_rollout"):
        try:
            out = getattr(gen, name)(ids, mask)
        except TeError as e:
            outcome[name] = f"TeError: {e}"
            continue
        outcome[name] = {"dtype": str(out.dtype), "shape": list(out.shape),
                         "nonfinite": int((~torch.isfinite(out.float())).sum())}
    # the reference's min-max of attn_gradcam is 0 / 0 on a sample whose clamped map is all zero (here sample 2: both heads'
    # mean gradients are negative); the fp32 model gives the same NaN row
    gc16 = gen.generate_attn_gradcam(ids, mask)
    gc32 = Generator(m32).generate_attn_gradcam(ids, mask)
    outcome["attn_gradcam_nonfinite_fp32"] = int((~torch.isfinite(gc32)).sum())
    record("bf16.bert_other_methods", **outcome)
    assert torch.equal(torch.isfinite(gc16), torch.isfinite(gc32))
    for name in ("generate_LRP_last_layer", "generate_full_lrp", "generate_attn_gradcam"):      # these run relprop
        assert isinstance(outcome[name], dict) and outcome[name]["dtype"] == "torch.float32", (name, outcome[name])
    for name, o in outcome.items():
        if name.startswith("generate_") and name != "generate_attn_gradcam":
            assert isinstance(o, str) or (o["shape"] == [3, 24] and o["nonfinite"] == 0), (name, o)
    with pytest.raises(TeError, match="bfloat16"):
        Generator(_soft_mask_model(torch.float16)).generate_LRP(ids, mask, start_layer=0)
    after = Generator(m32).generate_LRP(ids, mask, start_layer=0)
    assert _bits_equal("bf16.bert_fp32_untouched", after, before)
