"""AttnLRP on bf16 models, CPU: the same-cache restatement (tests/attnlrp_cache_ref.py) states the header's rules -- in fp64 on
an fp64 model it agrees with the autograd restatement (tests/attnlrp_ref.py) to 1e-12; the new entries are declared, exported
and bound; the route functions answer as specified; the refusals of generate_attnlrp for bf16 models fire before any forward
pass."""
import copy
import os
import re

import pytest
import torch

import attnlrp_cache_ref as cref
import attnlrp_ref as ref
from test_attnlrp_host import _no_forward, _toy_bert, toy_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "te_relprop.h")
F64 = torch.float64


def rnd(shape, seed, dtype=F64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _rel_l2(got, want):
    got, want = got.double().flatten(1), want.double().flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("index", [None, [4, 0, 2]])
@pytest.mark.parametrize("eps", [1e-6, 0.0])
def test_cache_restatement_is_the_autograd_restatement_vit(index, eps):
    """fp64 toy ViT: the explicit rules on the model's caches against attnlrp_ref's autograd on a deep copy, <= 1e-12 relative
    L2 per sample (measured: 3e-16 to 4e-16).

    Recorded, not asserted: on the caches of a BF16 toy ViT (toy_vit(torch.bfloat16, conserving=False), batch 3) this
    restatement in fp64 differs from attnlrp_ref's fp64 restatement with its own forward pass by 2.4e-3 to 1.2e-2 relative
    L2 per sample -- the forward pass's bf16 rounding, not the chain's error -- while its fp32 evaluation differs from its
    fp64 evaluation by 2.3e-7 to 3.1e-7: the scale the kernel chain on a bf16 model is held to (tests/test_gpu_attnlrp_bf16.py)."""
    model = toy_vit(F64, conserving=False)
    x = rnd((3, 3, 16, 16), 1)
    with torch.no_grad():
        logits = model(x)
    seed, idx = cref.one_hot(logits, index)
    got = cref.vit_chain(model, seed, eps, F64)
    want, _ = ref.vit_attnlrp(copy.deepcopy(model), x, index=idx, eps=eps)
    assert got.shape == want.shape == (3, 4) and got.dtype == F64
    err = _rel_l2(got, want)
    assert float(err.max()) <= 1e-12, err.tolist()


@pytest.mark.parametrize("index", [None, [1, 1, 0]])
@pytest.mark.parametrize("eps", [1e-6, 0.0])
def test_cache_restatement_is_the_autograd_restatement_bert(index, eps):
    """fp64 toy BERT (test_attnlrp_host._toy_bert's configuration), batch 3 with one padded sample, <= 1e-12 relative L2 per
    sample."""
    model = _toy_bert(F64)
    ids = torch.randint(1, 50, (3, 6), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(3, 6, dtype=F64)
    mask[1, 4:] = 0.0
    with torch.no_grad():
        logits = model(input_ids=ids, attention_mask=mask)[0]
    seed, idx = cref.one_hot(logits, index)
    got = cref.bert_chain(model, seed, eps, F64)
    want, _ = ref.bert_attnlrp(copy.deepcopy(model), ids, mask, index=idx, eps=eps)
    assert got.shape == want.shape == (3, 6) and got.dtype == F64
    err = _rel_l2(got, want)
    assert float(err.max()) <= 1e-12, err.tolist()


def test_fp32_evaluation_of_the_restatement_is_at_rounding_scale():
    """The second evaluation the model tests compare with: the same rules in fp32 on the same (here fp64 -> bf16 rounded) caches
    stay at fp32 rounding scale of the fp64 evaluation -- far below the 2e-3 the own-forward yardstick is off by."""
    model = toy_vit(torch.bfloat16, conserving=False)
    x = rnd((3, 3, 16, 16), 1).to(torch.bfloat16)
    with torch.no_grad():
        logits = model(x)
    seed, _ = cref.one_hot(logits)
    R64, R32 = cref.vit_chain(model, seed, 1e-6, F64), cref.vit_chain(model, seed, 1e-6, torch.float32)
    assert R32.dtype == torch.float32 and float(_rel_l2(R32, R64).max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ header <-> library <-> binding
NEW = ["te_attnlrp_act_bf16", "te_attnlrp_attention_bf16", "te_attnlrp_attention_bf16_supported",
       "te_attnlrp_attention_bf16_workspace_bytes", "te_attnlrp_damp_bf16", "te_attnlrp_layernorm_bf16", "te_attnlrp_linear_bf16",
       "te_attnlrp_linear_bf16_supported", "te_attnlrp_linear_bf16_workspace_bytes", "te_attnlrp_row_rstd_bf16",
       "te_attnlrp_token_relevance_bf16"]


def test_bf16_entries_declared_exported_and_bound():
    from ctypes import c_float, c_int, c_int64, c_size_t, c_void_p
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib, ops
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(te_attnlrp_[a-z0-9_]+)\s*\(", src))) == NEW
    P, I, S = c_void_p, c_int64, _lib.SIGNATURES
    assert sorted(n for n in S if n.startswith("te_attnlrp_")) == NEW
    for n in NEW:
        assert hasattr(lib, n) and S[n][0] is (c_size_t if n.endswith("_bytes") else c_int), n
    # the streaming rules: the argument lists of their _f32 entries
    for rule in ("damp", "act", "row_rstd", "layernorm", "token_relevance"):
        assert S[f"te_attnlrp_{rule}_bf16"] == S[f"te_alrp_{rule}_f32"], rule
        assert _lib.PARAMS[f"te_attnlrp_{rule}_bf16"] == _lib.PARAMS[f"te_alrp_{rule}_f32"], rule
    assert S["te_attnlrp_linear_bf16"][1] == [P, I, P, I, P, c_int, P, I, I, I, c_float, P, c_size_t, P]
    assert _lib.PARAMS["te_attnlrp_linear_bf16"] == ("G", "g_ld", "Y", "y_ld", "W", "w_transposed", "out", "T", "in_f", "out_f", "eps", "ws",
                                                     "ws_bytes", "stream")
    assert S["te_attnlrp_attention_bf16"][1] == ([P, I, I, I] * 4 + [P, c_float] + [P, I, I, I] * 3 + [I, I, I, I, P, c_size_t, P])
    assert S["te_attnlrp_linear_bf16_supported"][1] == [I, I, I] and S["te_attnlrp_attention_bf16_supported"][1] == [I, I]
    assert _lib.MIN_LIB_VERSION == 800 and lib.te_version() >= 801
    for name in ("alrp_linear_bf16_route", "alrp_attention_bf16_route", "alrp_attention_bf16", "alrp_weight_t"):
        assert callable(getattr(ops, name)), name


def test_routes_answer_as_specified():
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib, ops
    lib = _lib.load()
    assert ops.alrp_linear_bf16_route(51, 128, 384) == "bf16"
    assert ops.alrp_linear_bf16_route(51, 128, 10) == "fp32-upcast"          # the 10-class head of the tiny models
    assert ops.alrp_linear_bf16_route(1, 768, 1000) == "fp32-upcast"         # the 1000-class head
    assert ops.alrp_linear_bf16_route(1, 768, 3072) == "bf16" and ops.alrp_linear_bf16_route(51, 64, 128) == "fp32-upcast"
    assert ops.alrp_attention_bf16_route(17, 64) == "bf16"
    assert ops.alrp_attention_bf16_route(17, 48) == "fp32-upcast"
    assert ops.alrp_attention_bf16_route(1025, 64) == "fp32-upcast" and ops.alrp_attention_bf16_route(1024, 64) == "bf16"
    # where the existing bf16 rules hold, and a workspace for every shape they take
    for N, D in ((1, 64), (17, 64), (1024, 64), (1025, 64), (17, 48)):
        assert bool(lib.te_attnlrp_attention_bf16_supported(N, D)) == bool(lib.te_matmul_relprop_bf16_supported(N, D))
    assert lib.te_attnlrp_linear_bf16_workspace_bytes(51, 128, 384) >= 3 * 2 * 51 * 384
    assert lib.te_attnlrp_attention_bf16_workspace_bytes(2, 2, 17, 64) >= 2 * 2 * (6 * 17 * 64 + 10 * 17 * 17)


def test_bf16_entries_refuse_on_the_host():
    """The refusals of the _f32 entries, before any launch (fake non-null addresses are never dereferenced); a bf16 pointer
    needs 2-byte alignment only."""
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    A, INV, UNS, WS = 4096, _lib.TE_ERR_INVALID_ARG, _lib.TE_ERR_UNSUPPORTED, _lib.TE_ERR_WORKSPACE
    assert lib.te_attnlrp_damp_bf16(None, A, A, 4, 1e-6, None) == INV and lib.te_attnlrp_damp_bf16(A, A, A, 0, 1e-6, None) == INV
    assert [lib.te_attnlrp_damp_bf16(A, A, A, 4, e, None) for e in (-1.0, float("nan"), float("inf"))] == [INV] * 3
    assert lib.te_attnlrp_damp_bf16(A + 2, A, A, 4, 1e-6, None) == UNS and lib.te_attnlrp_damp_bf16(A, A + 1, A, 4, 1e-6, None) == UNS
    assert lib.te_attnlrp_act_bf16(A, A, A, 4, 2, None) == INV and lib.te_attnlrp_act_bf16(A, A + 1, A, 4, 0, None) == UNS
    assert lib.te_attnlrp_row_rstd_bf16(A, A, 0, 8, 1e-6, None) == INV and lib.te_attnlrp_row_rstd_bf16(A, A, 2, 8, -1.0, None) == INV
    assert lib.te_attnlrp_row_rstd_bf16(A + 1, A, 2, 8, 1e-6, None) == UNS
    assert lib.te_attnlrp_layernorm_bf16(A, A, None, A, 2, 8, None) == INV and lib.te_attnlrp_layernorm_bf16(A, A + 1, A, A, 2, 8, None) == UNS
    assert lib.te_attnlrp_token_relevance_bf16(A, A, A, 1, 1, 8, 1, None) == INV
    assert lib.te_attnlrp_token_relevance_bf16(A + 1, A, A, 1, 4, 8, 0, None) == UNS
    lin = lambda *a: lib.te_attnlrp_linear_bf16(*a[:5], 0, *a[5:], None)      # noqa: E731
    assert lin(A, 128, A, 128, A, A, 4, 128, 128, 1e-6, None, 0) == WS and lin(A, 128, A, 128, A, A, 4, 128, 128, 1e-6, A, 16) == WS
    assert lin(A, 64, A, 128, A, A, 4, 128, 128, 1e-6, A, 1 << 20) == INV and lin(A, 128, None, 128, A, A, 4, 128, 128, 1e-6, A, 1 << 20) == INV
    assert lin(A, 128, A, 256, A, A, 4, 128, 256, 1e-6, A, 1 << 20) == INV      # g_ld < out_f
    assert lin(A, 192, A, 192, A, A, 4, 128, 192, 1e-6, A, 1 << 20) == UNS and lin(A, 128, A, 128, A, A, 4, 64, 128, 1e-6, A, 1 << 20) == UNS
    s = (17 * 128, 64, 128)
    att = lambda N, D, ws, nb: lib.te_attnlrp_attention_bf16(A, *s, A, *s, A, *s, A, *s, A, 0.125, A, *s, A, *s, A, *s, 1, 2, N, D,      # noqa: E731
                                                          ws, nb, None)
    assert att(17, 48, A, 1 << 20) == UNS and att(1025, 64, A, 1 << 30) == UNS and att(17, 64, None, 0) == WS and att(17, 64, A, 16) == WS


# ------------------------------------------------------------------------------------------------ refusals
def test_mixed_bf16_and_fp32_is_refused_before_the_forward_pass():
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP, Generator
    both = r"(?s)(torch\.bfloat16.*torch\.float32|torch\.float32.*torch\.bfloat16)"
    with pytest.raises(TeError, match=both):                   # a bf16 model, fp32 images
        LRP(_no_forward(toy_vit(torch.bfloat16, conserving=False))).generate_attnlrp(torch.zeros(1, 3, 16, 16))
    with pytest.raises(TeError, match=both):                   # the reverse
        LRP(_no_forward(toy_vit(torch.float32, conserving=False))).generate_attnlrp(torch.zeros(1, 3, 16, 16, dtype=torch.bfloat16))
    mixed = toy_vit(torch.bfloat16, conserving=False)
    mixed.head.float()                                         # one layer left in fp32
    with pytest.raises(TeError, match=both):
        LRP(_no_forward(mixed)).generate_attnlrp(torch.zeros(1, 3, 16, 16, dtype=torch.bfloat16))
    bert = _toy_bert(torch.bfloat16)
    bert.classifier.float()
    ids, mask = torch.ones(1, 4, dtype=torch.long), torch.ones(1, 4)
    with pytest.raises(TeError, match=both):
        Generator(_no_forward(bert)).generate_attnlrp(ids, mask)


def test_bf16_on_the_host_is_refused_before_the_forward_pass():
    """There is no host chain: a bf16 model or input that is not on a GPU is turned away with a message that names the dtype
    -- whatever the dtype of BERT's attention_mask, which a bf16 model casts itself."""
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP, Generator
    with pytest.raises(TeError, match=r"torch\.bfloat16.*GPU"):
        LRP(_no_forward(toy_vit(torch.bfloat16, conserving=False))).generate_attnlrp(torch.zeros(1, 3, 16, 16, dtype=torch.bfloat16))
    ids = torch.ones(1, 4, dtype=torch.long)
    for mask in (torch.ones(1, 4), torch.ones(1, 4, dtype=torch.bfloat16), torch.ones(1, 4, dtype=torch.long)):
        with pytest.raises(TeError, match=r"torch\.bfloat16.*GPU"):
            Generator(_no_forward(_toy_bert(torch.bfloat16))).generate_attnlrp(ids, mask)


def test_fp16_is_still_refused_and_fp32_is_untouched():
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP, Generator, _refuse_attnlrp
    with pytest.raises(TeError, match=r"torch\.float16"):
        LRP(_no_forward(toy_vit(torch.float16, conserving=False))).generate_attnlrp(torch.zeros(1, 3, 16, 16, dtype=torch.float16))
    with pytest.raises(TeError, match=r"torch\.float16"):      # a bf16 model with fp16 images: the dtype that has no chain is named
        LRP(_no_forward(toy_vit(torch.bfloat16, conserving=False))).generate_attnlrp(torch.zeros(1, 3, 16, 16, dtype=torch.float16))
    ids = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(TeError, match=r"torch\.float64"):      # an fp32 BERT keeps refusing a mask of another float dtype
        Generator(_no_forward(_toy_bert())).generate_attnlrp(ids, torch.ones(1, 4, dtype=torch.float64))
    # an fp32 model with fp32 inputs passes every refusal, on the host too (its chain then asks for the GPU itself)
    _refuse_attnlrp(toy_vit(torch.float32, conserving=False), 1e-6, None, torch.zeros(1, 3, 16, 16))
    _refuse_attnlrp(_toy_bert(), 1e-6, None, ids, cast=(torch.ones(1, 4),))
