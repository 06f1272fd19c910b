"""AttnLRP, CPU: the torch restatement (tests/attnlrp_ref.py) states conserving rules -- with everything that absorbs
relevance removed (biases, beta, position embedding, eps, softmax) the token relevances of a toy ViT sum to the
class logit to 1e-12 in fp64, and each rule alone conserves a (.) G; the refusals of generate_attnlrp fire before any forward
pass; the header's AttnLRP entries are exported and bound as declared."""
import os
import re

import pytest
import torch

import attnlrp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "te_relprop.h")
F64 = torch.float64


def rnd(shape, seed, dtype=F64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def toy_vit(dtype=F64, conserving=True, seed=0):
    from transformer_explainability_amd import vit
    torch.manual_seed(seed)
    model = vit.VisionTransformer(img_size=16, patch_size=8, embed_dim=16, depth=2, num_heads=2, num_classes=5,
                                  qkv_bias=True).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))              # gamma away from 1, biases away from 0
            elif "weight" in name:
                p.mul_(10.0)                                   # activations of order one
        if conserving:
            for name, p in model.named_parameters():
                if name.endswith("bias") and not name.startswith("patch_embed"):
                    p.zero_()                                  # Linear biases and LayerNorm beta
            model.pos_embed.zero_()
            model.cls_token.normal_()                          # (a zero class token would make every logit zero)
    return model.to(dtype)


def test_chain_conserves_the_logit_when_nothing_absorbs(monkeypatch):
    """2-block toy ViT, zero biases, beta = 0, zero position embedding, eps = 0, softmax replaced by the identity:
    sum_t R[b, t] over ALL tokens (the class token included) = logit_c to 1e-12 relative in fp64, for the argmax class and
    for a given one."""
    monkeypatch.setattr(ref, "softmax", lambda s, dim: s)
    model = toy_vit()
    x = rnd((3, 3, 16, 16), 1)
    for index in (None, torch.tensor([4, 0, 2])):
        R, logits = ref.vit_attnlrp(model, x, index=index, eps=0.0, keep_cls=True)
        cls = logits.argmax(-1) if index is None else index
        want = logits.gather(1, cls.view(-1, 1)).squeeze(1)
        assert R.shape == (3, 5)                               # the class token's relevance is part of the sum
        assert float(want.abs().min()) > 1e-6
        assert float(((R.sum(1) - want) / want).abs().max()) <= 1e-12, (R.sum(1), want)
        dropped, _ = ref.vit_attnlrp(model, x, index=index, eps=0.0)
        assert torch.equal(dropped, R[:, 1:])


def test_softmax_bias_and_eps_absorb():
    """The counterpart: with the real softmax, biases and eps the same model does NOT conserve (the test above would pass
    vacuously if the restatement ignored its switches)."""
    model = toy_vit(conserving=False)
    x = rnd((3, 3, 16, 16), 1)
    R, logits = ref.vit_attnlrp(model, x, eps=1e-6, keep_cls=True)
    want = logits.max(-1).values
    assert float(((R.sum(1) - want) / want).abs().max()) > 1e-6


def _relevance(x, y, seed):
    """(sum x (.) G_x, sum y (.) G_y) for a random G_y through the autograd graph from leaf x to y"""
    G = rnd(y.shape, seed)
    (gx,) = torch.autograd.grad((y * G).sum(), x)
    return float((x.detach() * gx).sum()), float((y.detach() * G).sum())


def _close(a, b):
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (a, b)


def test_linear_rule_conserves_without_bias_and_eps():
    lin = torch.nn.Linear(7, 5, bias=False).double()
    x = rnd((4, 7), 2).requires_grad_(True)
    _close(*_relevance(x, ref.linear(x, lin, 0.0), 3))
    # the bias absorbs its share: the difference is exactly sum b (.) G_y
    lin_b = torch.nn.Linear(7, 5).double()
    y = ref.linear(x, lin_b, 0.0)
    G = rnd(y.shape, 3)
    (gx,) = torch.autograd.grad((y * G).sum(), x)
    _close(float((x.detach() * gx).sum()) + float((lin_b.bias.detach() * G).sum()), float((y.detach() * G).sum()))


def test_add_rule_conserves():
    a, b = rnd((4, 6), 4).requires_grad_(True), rnd((4, 6), 5).requires_grad_(True)
    y = ref.add(a, b, 0.0)
    G = rnd(y.shape, 6)
    ga, gb = torch.autograd.grad((y * G).sum(), (a, b))
    assert torch.equal(ga, gb)                                 # G_a = G_b = damp(G_o, o)
    _close(float((a.detach() * ga).sum() + (b.detach() * gb).sum()), float((y.detach() * G).sum()))


def test_damp_is_the_epsilon_rule():
    y = torch.tensor([0.0, -0.0, 2.0, -2.0, 1e-30, -1e-30], dtype=F64, requires_grad=True)
    G = torch.full_like(y, 3.0)
    (g,) = torch.autograd.grad((ref.damp(y, 0.5) * G).sum(), y)
    yd = y.detach()
    assert torch.equal(g, 3.0 * yd / (yd + torch.tensor([0.5, 0.5, 0.5, -0.5, 0.5, -0.5], dtype=F64)))
    (g0,) = torch.autograd.grad((ref.damp(y, 0.0) * G).sum(), y)
    assert torch.equal(g0, G)                                  # eps = 0: the identity, also at y == 0


def test_layernorm_rule_conserves_without_beta():
    norm = torch.nn.LayerNorm(9, eps=1e-6).double()
    with torch.no_grad():
        norm.weight.copy_(rnd((9,), 7))
        norm.bias.zero_()
    x = (rnd((5, 9), 8) + 0.7).requires_grad_(True)
    _close(*_relevance(x, ref.layer_norm(x, norm), 9))
    # and it is the stated formula
    G = rnd((5, 9), 9)
    (gx,) = torch.autograd.grad((ref.layer_norm(x, norm) * G).sum(), x)
    xd = x.detach()
    rstd = torch.rsqrt(xd.var(-1, unbiased=False, keepdim=True) + norm.eps)
    t = norm.weight.detach() * G
    assert float((gx - rstd * (t - t.mean(-1, keepdim=True))).abs().max()) <= 1e-14


def test_identity_rule_conserves_and_takes_the_limit_at_zero():
    x = rnd((6, 8), 10)
    x[0, :4] = torch.tensor([0.0, -0.0, 1e-20, -20.0], dtype=F64)
    x.requires_grad_(True)
    for f, slope in ((ref.gelu, 0.5), (ref.tanh, 1.0)):
        _close(*_relevance(x, f(x), 11))
        (gx,) = torch.autograd.grad(f(x).sum(), x)
        assert float(gx[0, 0]) == slope and float(gx[0, 1]) == slope and torch.isfinite(gx).all()
    assert torch.allclose(ref.gelu(x), torch.nn.functional.gelu(x.detach()), rtol=1e-15, atol=0)


def test_uniform_rule_gives_each_operand_half():
    a, b = rnd((2, 3, 5, 4), 12).requires_grad_(True), rnd((2, 3, 4, 6), 13).requires_grad_(True)
    y = ref.uniform_matmul(a, b)
    G = rnd(y.shape, 14)
    ga, gb = torch.autograd.grad((y * G).sum(), (a, b))
    total = float((y.detach() * G).sum())
    _close(float((a.detach() * ga).sum()), 0.5 * total)
    _close(float((b.detach() * gb).sum()), 0.5 * total)
    assert torch.equal(y, torch.matmul(a, b).detach()) or torch.allclose(y, torch.matmul(a, b), rtol=1e-15)


# ------------------------------------------------------------------------------------------------ refusals
def _no_forward(model):
    def forward(*a, **k):
        raise AssertionError("the forward pass ran before the refusal")
    model.forward = forward
    return model


def _toy_bert(dtype=torch.float32):
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=50, hidden_size=16, num_hidden_layers=1, num_attention_heads=2,
                              intermediate_size=32, max_position_embeddings=16, num_labels=2)
    return bert.BertForSequenceClassification(cfg).eval().to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
def test_other_dtypes_are_refused_before_the_forward_pass(dtype):
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP, Generator
    x = torch.zeros(1, 3, 16, 16, dtype=dtype)
    with pytest.raises(TeError, match=str(dtype)):
        LRP(_no_forward(toy_vit(dtype, conserving=False))).generate_attnlrp(x)
    ids, mask = torch.ones(1, 4, dtype=torch.long), torch.ones(1, 4)
    with pytest.raises(TeError, match=str(dtype)):
        Generator(_no_forward(_toy_bert(dtype))).generate_attnlrp(ids, mask)


def test_head_mask_train_mode_and_bad_eps_are_refused_before_the_forward_pass():
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP, Generator
    x = torch.zeros(1, 3, 16, 16)
    ids, mask = torch.ones(1, 4, dtype=torch.long), torch.ones(1, 4)
    lrp, gen = LRP(_no_forward(toy_vit(torch.float32))), Generator(_no_forward(_toy_bert()))
    with pytest.raises(TeError, match="head_mask"):
        lrp.generate_attnlrp(x, head_mask=torch.ones(2))
    with pytest.raises(TeError, match="head_mask"):
        gen.generate_attnlrp(ids, mask, head_mask=torch.ones(2))
    for bad in (-1e-6, float("nan"), float("inf"), "1e-6", True):
        with pytest.raises(ValueError, match="eps"):
            lrp.generate_attnlrp(x, eps=bad)
    lrp.model.train()
    gen.model.train()
    with pytest.raises(TeError, match="train mode"):
        lrp.generate_attnlrp(x)
    with pytest.raises(TeError, match="train mode"):
        gen.generate_attnlrp(ids, mask)


def test_the_chain_has_no_cpu_fallback():
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(TeError):
        LRP(toy_vit(torch.float32, conserving=False)).generate_attnlrp(torch.zeros(1, 3, 16, 16))


def test_method_tables_are_untouched():
    from transformer_explainability_amd import methods, sweep
    assert "attnlrp" not in methods.LRP_NEEDS and "attnlrp" not in methods.GENERATOR_NEEDS
    assert not any("attnlrp" in str(m).lower() for m in sweep.METHODS)


# ------------------------------------------------------------------------------------------------ header <-> library <-> binding
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(te_alrp_[a-z0-9_]+)\s*\(", src)))


def test_attnlrp_entries_declared_exported_and_bound():
    from ctypes import c_float, c_int, c_int64, c_void_p
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib, ops
    lib = _lib.load()
    names = _declared()
    assert names == ["te_alrp_act_f32", "te_alrp_damp_f32", "te_alrp_layernorm_f32", "te_alrp_row_rstd_f32",
                     "te_alrp_scale3_f32", "te_alrp_token_relevance_f32"]
    P, S = c_void_p, _lib.SIGNATURES
    for n in names:
        assert hasattr(lib, n) and n in S and S[n][0] is c_int, n
    assert sorted(n for n in S if n.startswith("te_alrp_")) == names
    assert S["te_alrp_damp_f32"][1] == [P, P, P, c_int64, c_float, P]
    assert S["te_alrp_act_f32"][1] == [P, P, P, c_int64, c_int, P]
    assert S["te_alrp_scale3_f32"][1] == [P, P, P, c_int64, c_int64, c_int64, P]
    assert S["te_alrp_row_rstd_f32"][1] == [P, P, c_int64, c_int64, c_float, P]
    assert S["te_alrp_layernorm_f32"][1] == [P, P, P, P, c_int64, c_int64, P]
    assert S["te_alrp_token_relevance_f32"][1] == [P, P, P, c_int64, c_int64, c_int64, c_int, P]
    assert _lib.PARAMS["te_alrp_token_relevance_f32"] == ("x0", "G", "out", "B", "N", "C", "skip_first", "stream")
    assert (_lib.TE_ALRP_ACT_GELU, _lib.TE_ALRP_ACT_TANH) == (0, 1) and lib.te_version() >= 707
    for name in ("alrp_damp", "alrp_act", "alrp_scale3", "alrp_row_rstd", "alrp_layernorm", "alrp_token_relevance", "alrp_linear"):
        assert callable(getattr(ops, name)), name


def test_attnlrp_entries_refuse_on_the_host():
    """Every refusal comes before a launch: fake non-null addresses are never dereferenced."""
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    A, INV, UNS = 4096, _lib.TE_ERR_INVALID_ARG, _lib.TE_ERR_UNSUPPORTED
    assert lib.te_alrp_damp_f32(None, A, A, 4, 1e-6, None) == INV and lib.te_alrp_damp_f32(A, A, A, 0, 1e-6, None) == INV
    assert [lib.te_alrp_damp_f32(A, A, A, 4, e, None) for e in (-1.0, float("nan"), float("inf"))] == [INV] * 3
    assert lib.te_alrp_damp_f32(A + 2, A, A, 4, 1e-6, None) == UNS
    assert lib.te_alrp_act_f32(A, A, A, 4, 2, None) == INV and lib.te_alrp_act_f32(A, None, A, 4, 0, None) == INV
    assert lib.te_alrp_act_f32(A, A, A + 1, 4, 0, None) == UNS
    assert lib.te_alrp_scale3_f32(A, A, None, 8, 2, 8, None) == INV and lib.te_alrp_scale3_f32(A, A, A, 4, 2, 8, None) == INV
    assert lib.te_alrp_scale3_f32(A, A + 2, A, 8, 2, 8, None) == UNS
    assert lib.te_alrp_row_rstd_f32(A, A, 0, 8, 1e-6, None) == INV and lib.te_alrp_row_rstd_f32(A, A, 2, 8, -1.0, None) == INV
    assert lib.te_alrp_layernorm_f32(A, A, None, A, 2, 8, None) == INV and lib.te_alrp_layernorm_f32(A, A, A, A, 2, 0, None) == INV
    assert lib.te_alrp_layernorm_f32(A, A + 3, A, A, 2, 8, None) == UNS
    assert lib.te_alrp_token_relevance_f32(A, A, A, 1, 1, 8, 1, None) == INV          # nothing left without the first token
    assert lib.te_alrp_token_relevance_f32(A, A, A, 1, 4, 8, 2, None) == INV
    assert lib.te_alrp_token_relevance_f32(A, A, A, 1 << 31, 4, 8, 0, None) == UNS
