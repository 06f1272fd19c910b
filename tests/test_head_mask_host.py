"""head_mask without a GPU: the mask shapes get_head_mask takes and refuses, the masked forward pass on the CPU (stock torch),
the refusals of the two new ops wrappers, Mul.relprop's remaining NotImplementedError, the host-side argument checks of the
five C entry points, and the CPU restatement (tests/head_mask_ref.py) against the oracle where no mask is involved.

On a tree without the feature: BertSelfAttention.forward raises NotImplementedError for any mask, BertModel has no
get_head_mask, ops has no mul_head_relprop / head_relevance, the library exports no te_mul_head_relprop_*."""
import inspect

import pytest
import torch

import head_mask_ref as HR
from oracle import relprop_oracle as O
from oracle.model_cache import bert_cache_from_model, vit_cache_from_model

BF = torch.bfloat16
L_, H_, B_, N_ = 2, 2, 3, 24


def _bert(dtype=torch.float32):
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=128, num_hidden_layers=L_, num_attention_heads=H_,
                              intermediate_size=256, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(11)
    model = bert.BertForSequenceClassification(cfg).eval()
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return model.to(dtype)


def _inputs():
    ids = torch.randint(1, 100, (B_, N_), generator=torch.Generator().manual_seed(12))
    mask = torch.ones(B_, N_)
    mask[1, 20:] = 0.0
    return ids, mask


def _vit():
    from transformer_explainability_amd import vit
    torch.manual_seed(0)
    model = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=4, num_classes=10,
                                  qkv_bias=True).eval()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    return model, x


# ------------------------------------------------------------------------------------------------ get_head_mask
def test_get_head_mask_shapes_and_dtype():
    model = _bert()
    gm = model.bert.get_head_mask
    assert gm(None, L_) == [None] * L_
    one = gm(torch.tensor([1.0, 0.5]), L_)
    assert one.shape == (L_, 1, H_, 1, 1) and one.dtype == torch.float32
    assert torch.equal(one[0].flatten(), torch.tensor([1.0, 0.5])) and torch.equal(one[1], one[0])
    per_layer = gm(torch.tensor([[1.0, 0.0], [-2.0, 0.5]]), L_)
    assert per_layer.shape == (L_, 1, H_, 1, 1) and float(per_layer[1, 0, 0, 0, 0]) == -2.0
    per_sample = gm(torch.arange(L_ * B_ * H_, dtype=torch.float32).view(L_, B_, H_), L_, batch_size=B_)
    assert per_sample.shape == (L_, B_, H_, 1, 1) and float(per_sample[1, 2, 1, 0, 0]) == L_ * B_ * H_ - 1
    assert gm(torch.ones(L_, 1, H_), L_, batch_size=B_).shape == (L_, 1, H_, 1, 1)
    # cast to the model's dtype, as Hugging Face does: integer and double masks on an fp32 model, any mask on a bf16 model
    assert gm(torch.tensor([1, 0]), L_).dtype == torch.float32
    assert gm(torch.tensor([1.0, 0.0], dtype=torch.float64), L_).dtype == torch.float32
    assert _bert(BF).bert.get_head_mask(torch.tensor([1.0, 0.5]), L_).dtype == BF
    assert gm([1.0, 0.0], L_).shape == (L_, 1, H_, 1, 1)                         # (anything torch.as_tensor takes)


@pytest.mark.parametrize("shape", [(), (H_ + 1,), (L_ + 1, H_), (L_, H_ + 1), (L_, B_ + 1, H_), (L_, B_, H_ + 1),
                                   (L_, 1, H_, 1, 1), (L_, B_, H_, N_, N_), (1, H_, N_, N_)])
def test_get_head_mask_refuses_other_shapes_before_the_forward_pass(shape):
    model = _bert()
    ids, mask = _inputs()
    ran = []
    handle = model.bert.embeddings.register_forward_pre_hook(lambda *a: ran.append(1))
    try:
        with pytest.raises(ValueError, match="one value per head"):
            model(input_ids=ids, attention_mask=mask, head_mask=torch.ones(shape))
    finally:
        handle.remove()
    assert not ran, "the refusal must come before anything runs"


def test_vit_get_head_mask():
    model, x = _vit()
    L, H = 2, 4
    assert model.get_head_mask(None) == [None] * L
    assert model.get_head_mask(torch.ones(H)).shape == (L, 1, H, 1, 1)
    assert model.get_head_mask(torch.ones(L, H)).shape == (L, 1, H, 1, 1)
    assert model.get_head_mask(torch.ones(L, 2, H), batch_size=2).shape == (L, 2, H, 1, 1)
    for bad in ((H + 1,), (L, 3, H), (L, H, 17, 17)):
        with pytest.raises(ValueError, match="one value per head"):
            model(x, head_mask=torch.ones(bad))


# ------------------------------------------------------------------------------------------------ the masked forward pass (CPU)
def test_bert_masked_forward_on_the_cpu():
    """Stock torch on the CPU: the forward pass no longer raises; a mask of ones changes no bit; the accessor keeps the unmasked
    probabilities; Mul and MatMul cache [P, m] and P . m; a head masked with 0 has an exactly zero attention gradient; the
    mask is rewritten by the next call."""
    model = _bert()
    ids, mask = _inputs()
    plain = model(input_ids=ids, attention_mask=mask)[0].detach().clone()
    sa0, sa1 = (lay.attention.self for lay in model.bert.encoder.layer)
    assert sa0.head_mask is None
    ones = model(input_ids=ids, attention_mask=mask, head_mask=torch.ones(H_))[0]
    assert torch.equal(ones, plain)
    hm = torch.tensor([[1.0, 0.0], [0.5, 1.0]])
    out = model(input_ids=ids, attention_mask=mask, head_mask=hm)[0]
    assert not torch.equal(out, plain)
    assert tuple(sa0.head_mask.shape) == (1, H_, 1, 1) and sa0.head_mask is not None
    P, m = sa0.mul.X
    assert torch.equal(P, sa0.get_attn().detach()) and torch.equal(m, sa0.head_mask)
    assert torch.equal(sa0.matmul2.X[0], P * m) and not sa0.matmul2.X[0][:, 1].any() and P[:, 1].any()
    assert torch.equal(sa0.matmul2.Y.detach(), torch.matmul(P * m, sa0.matmul2.X[1]))
    loss = out[torch.arange(B_), out.argmax(-1)].sum()
    g0, g1 = torch.autograd.grad(loss, [sa0.get_attn(), sa1.get_attn()])
    assert not g0[:, 1].any() and g0[:, 0].any(), "d/dP = m . d/dP': exactly zero for the head masked with 0"
    assert g1[:, 0].any() and g1[:, 1].any()
    # the next call without a mask: nothing of the mask is left
    again = model(input_ids=ids, attention_mask=mask)[0]
    assert sa0.head_mask is None and sa1.head_mask is None and torch.equal(again, plain)
    assert torch.equal(sa0.matmul2.X[0], sa0.get_attn().detach())


def test_cpu_model_with_a_mask_reaches_the_kernel_wrappers_refusal():
    """No GPU, no fallback: the forward pass runs (stock torch), the relprop chain reaches an ops wrapper and gets its TeError."""
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import Generator, LRP
    model = _bert()
    ids, mask = _inputs()
    with pytest.raises(TeError, match="CPU"):
        Generator(model).generate_LRP(ids, mask, start_layer=0, head_mask=torch.tensor([1.0, 0.0]))
    with pytest.raises(TeError, match="CPU"):
        Generator(model).generate_head_relevance(ids, mask)
    vmodel, x = _vit()
    with pytest.raises(TeError, match="CPU"):
        LRP(vmodel).generate_LRP(x, head_mask=torch.ones(4))
    blk = vmodel.blocks[0].attn
    assert tuple(blk.mul.X[1].shape) == (1, 4, 1, 1) and torch.equal(blk.matmul2.X[0], blk.get_attn().detach() * blk.mul.X[1])
    with pytest.raises(TeError, match="CPU"):
        LRP(vmodel).generate_head_relevance(x)


def test_generators_take_head_mask_last():
    from transformer_explainability_amd.generators import Generator, LRP
    names = [(LRP, n) for n in ("generate_LRP", "generate_all", "generate_head_relevance")]
    names += [(Generator, n) for n in ("generate_LRP", "generate_all", "generate_LRP_last_layer", "generate_full_lrp",
                                       "generate_attn_last_layer", "generate_rollout", "generate_attn_gradcam",
                                       "generate_head_relevance")]
    for cls, n in names:
        params = list(inspect.signature(getattr(cls, n)).parameters.values())
        assert params[-1].name == "head_mask" and params[-1].default is None, (cls.__name__, n)


# ------------------------------------------------------------------------------------------------ ops / rules refusals
def _operands(dtype_r=torch.float32, dtype_p=torch.float32, dtype_m=None):
    R = torch.zeros(2, 3, 5, 5, dtype=dtype_r)
    P = torch.ones(2, 3, 5, 5, dtype=dtype_p)
    m = torch.ones(1, 3, 1, 1, dtype=dtype_p if dtype_m is None else dtype_m)
    return R, P, m


def test_ops_refuse_host_tensors():
    from transformer_explainability_amd import ops, TeError
    for dt in (torch.float32, torch.float64):
        with pytest.raises(TeError, match="CPU"):
            ops.mul_head_relprop(*_operands(dt, dt))
        with pytest.raises(TeError, match="CPU"):
            ops.head_relevance(torch.zeros(2, 3, 5, 4, dtype=dt))
    with pytest.raises(TeError, match="CPU"):
        ops.mul_head_relprop(*_operands(torch.float32, BF))


@pytest.mark.parametrize("r,p,m", [(torch.float16, torch.float16, None), (torch.float32, torch.float16, None),
                                   (torch.float32, torch.float32, BF), (torch.float32, BF, torch.float32),
                                   (BF, BF, None), (torch.float64, torch.float32, None),
                                   (torch.float32, torch.float64, None), (torch.float32, torch.float32, torch.float64)],
                         ids=["fp16", "fp16-operand", "bf16-mask-only", "bf16-P-only", "bf16-relevance", "f64-relevance-only",
                              "f64-operand-only", "f64-mask-only"])
def test_ops_refuse_fp16_mixed_and_bf16_relevance(r, p, m):
    from transformer_explainability_amd import ops, TeError
    with pytest.raises(TeError) as e:
        ops.mul_head_relprop(*_operands(r, p, m))
    assert ops.DTYPES_MSG in str(e.value)
    for dt in (torch.float16, BF):
        with pytest.raises(TeError) as e:
            ops.head_relevance(torch.zeros(2, 3, 5, 4, dtype=dt))
        assert ops.DTYPES_MSG in str(e.value)


def test_ops_refuse_other_shapes():
    from transformer_explainability_amd import ops, TeError
    R, P, m = _operands()
    with pytest.raises(TeError, match=r"\[B,H,rows,cols\]"):
        ops.mul_head_relprop(R[0], P[0], m)
    with pytest.raises(TeError, match=r"\[B,H,rows,cols\]"):
        ops.mul_head_relprop(R, P[:, :, :4], m)
    with pytest.raises(TeError, match=r"\[B,H,N,D\]"):
        ops.head_relevance(torch.zeros(2, 15, 4))


def test_mul_relprop_off_the_head_mask_stays_off_path():
    from transformer_explainability_amd import rules, rules_lrp
    for lib in (rules, rules_lrp):
        mul = lib.Mul()
        a, b = torch.ones(2, 3, 5, 5), torch.ones(2, 3, 5, 5)
        assert torch.equal(mul([a, 2 * b]), 2 * a)
        with pytest.raises(NotImplementedError, match="off the accelerated"):
            mul.relprop(a, 1)                                 # two full tensors: not a head mask
        mul([a, torch.ones(2, 1, 1, 5)])
        with pytest.raises(NotImplementedError):
            mul.relprop(a, 1)                                 # a key mask
        mul([torch.ones(4, 5), torch.ones(5)])
        with pytest.raises(NotImplementedError):
            mul.relprop(torch.ones(4, 5), 1)
        with pytest.raises(NotImplementedError):
            lib.Mul().relprop(a, 1)                           # no forward pass, no operands
        assert lib.Mul.is_head_mask(a, torch.ones(1, 3, 1, 1)) and lib.Mul.is_head_mask(a, torch.ones(2, 3, 1, 1))
        assert not lib.Mul.is_head_mask(a, torch.ones(3, 3, 1, 1)) and not lib.Mul.is_head_mask(a, torch.ones(3))


# ------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_validate_on_the_host():
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    P = 4096                                                  # a fake non-null address: never dereferenced on the host
    for sfx in ("f32", "bf16", "f64"):
        fn = getattr(lib, "te_mul_head_relprop_" + sfx)
        ok = dict(R=P, P=P, m=P, m_sb=0, out=P, B=2, H=3, rows=5, cols=5, stream=None)
        bad = [dict(R=None), dict(P=None), dict(m=None), dict(out=None), dict(B=-1), dict(B=0), dict(H=-2), dict(rows=-1),
               dict(cols=0), dict(m_sb=-3), dict(m_sb=2)]
        assert [fn(*{**ok, **b}.values()) for b in bad] == [-1] * len(bad), sfx
    for sfx in ("f32", "f64"):
        fn = getattr(lib, "te_head_relevance_" + sfx)
        ok = dict(R=P, r_sb=24 * 128, r_sh=64, r_sn=128, out=P, B=3, H=2, N=24, D=64, stream=None)
        bad = [dict(R=None), dict(out=None), dict(B=0), dict(H=-1), dict(N=-5), dict(D=0), dict(r_sb=-1), dict(r_sh=-1),
               dict(r_sn=-1), dict(r_sn=32)]
        assert [fn(*{**ok, **b}.values()) for b in bad] == [-1] * len(bad), sfx


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_equals_the_oracle_without_a_mask_and_obeys_the_rule():
    """head_mask_ref with no masked layer is the oracle, bit for bit (BERT and ViT, CPU caches of a CPU forward pass); the Mul
    step with m = 1 returns safe_divide's R . (P != 0) pattern, and with m = 0 zeros."""
    model = _bert()
    ids, mask = _inputs()
    out = model(input_ids=ids, attention_mask=mask)[0]
    sas = [lay.attention.self for lay in model.bert.encoder.layer]
    grads = torch.autograd.grad(out[torch.arange(B_), out.argmax(-1)].sum(), [sa.get_attn() for sa in sas])
    for sa, g in zip(sas, grads):
        sa.save_attn_gradients(g)
    cache = bert_cache_from_model(model)
    oh = torch.zeros_like(out.detach()).scatter_(1, out.detach().argmax(-1, keepdim=True), 1.0)
    want = O.bert_relprop(oh, cache, num_heads=H_, start_layer=0)
    got = HR.bert_relprop(oh, cache, H_, [None] * L_, [None] * L_, start_layer=0)
    assert torch.equal(got["map"], want["map"]) and torch.equal(got["cam"], want["cam"])
    assert got["head_relevance"].shape == (B_, L_, H_) and got["head_relevance"].dtype == torch.float64

    vmodel, x = _vit()
    logits = vmodel(x)
    attns = [blk.attn.get_attn() for blk in vmodel.blocks]
    for blk, g in zip(vmodel.blocks, torch.autograd.grad(logits.max(-1).values.sum(), attns)):
        blk.attn.save_attn_gradients(g)
    vcache = vit_cache_from_model(vmodel)
    voh = torch.zeros_like(logits.detach()).scatter_(1, logits.detach().argmax(-1, keepdim=True), 1.0)
    want = O.vit_relprop(voh, vcache, num_heads=4, start_layer=0)
    got = HR.vit_relprop(voh, vcache, 4, [None] * 2, [None] * 2, start_layer=0)
    assert torch.equal(got["map"], want["map"]) and torch.equal(got["cam"], want["cam"])

    P = torch.softmax(torch.randn(1, 2, 4, 4, generator=torch.Generator().manual_seed(3)), -1)
    P[..., 0] = 0.0
    R = torch.randn(1, 2, 4, 4, generator=torch.Generator().manual_seed(4))
    assert not HR.mul_head_relprop(R, P, torch.zeros(1, 2, 1, 1)).any()
    one = HR.mul_head_relprop(R, P, torch.ones(1, 2, 1, 1))
    assert not one[..., 0].any() and torch.allclose(one[..., 1:], R[..., 1:], rtol=1e-5, atol=0)


def test_a_masked_pass_is_a_stock_forward_pass_and_restores_the_flag():
    """ops.stock_forward switches the producers off for the duration of a masked model call only (an exception included)."""
    from transformer_explainability_amd import ops
    model = _bert()
    ids, mask = _inputs()
    seen = []
    handle = model.bert.encoder.layer[0].register_forward_pre_hook(lambda *a: seen.append(ops.USE_FUSED_PRODUCERS))
    assert ops.USE_FUSED_PRODUCERS is False
    try:
        ops.USE_FUSED_PRODUCERS = True
        model(input_ids=ids, attention_mask=mask)
        model(input_ids=ids, attention_mask=mask, head_mask=torch.ones(H_))
        assert seen == [True, False] and ops.USE_FUSED_PRODUCERS is True
        with pytest.raises(ValueError):
            model(input_ids=ids, attention_mask=mask, head_mask=torch.ones(H_ + 1))
        with pytest.raises(RuntimeError), ops.stock_forward():
            raise RuntimeError("inside")
        assert ops.USE_FUSED_PRODUCERS is True
    finally:
        handle.remove()
        ops.USE_FUSED_PRODUCERS = False
