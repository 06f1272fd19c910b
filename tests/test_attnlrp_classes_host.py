"""AttnLRP with a class axis, CPU (te_relprop.h, "AttnLRP, a class axis"): the te_alrpk_* entries are declared, exported and
bound as the header says and refuse on the host before any launch; generate_attnlrp_classes raises its refusals before the
forward pass; the method tables do not know the method; and the linearity in the seed the feature rests on holds on the fp64
torch restatement (tests/attnlrp_ref.py through tests/attnlrp_seed_ref.py)."""
import os
import re

import pytest
import torch

import attnlrp_ref as ref
import attnlrp_seed_ref as sref
from test_attnlrp_host import _no_forward, _toy_bert, rnd, toy_vit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "te_relprop.h")
NEW = ["te_alrpk_act_bf16", "te_alrpk_act_f32", "te_alrpk_damp_bf16", "te_alrpk_damp_f32", "te_alrpk_layernorm_bf16",
       "te_alrpk_layernorm_f32", "te_alrpk_token_relevance_bf16", "te_alrpk_token_relevance_f32"]


# ------------------------------------------------------------------------------------------------ header <-> library <-> binding
def test_class_entries_declared_exported_and_bound():
    from ctypes import c_float, c_int, c_int64, c_void_p
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(te_alrpk_[a-z0-9_]+)\s*\(", src))) == NEW
    P, I, S = c_void_p, c_int64, _lib.SIGNATURES
    assert sorted(n for n in S if n.startswith("te_alrpk_")) == NEW
    for n in NEW:
        assert hasattr(lib, n) and S[n][0] is c_int, n
    assert S["te_alrpk_damp_f32"][1] == [P, P, P, I, I, c_float, P]
    assert S["te_alrpk_act_f32"][1] == [P, P, P, I, I, c_int, P]
    assert S["te_alrpk_layernorm_f32"][1] == [P, P, P, P, I, I, I, P]
    assert S["te_alrpk_token_relevance_f32"][1] == [P, P, P, I, I, I, I, c_int, P]
    assert _lib.PARAMS["te_alrpk_damp_f32"] == ("G", "Y", "out", "K", "n", "eps", "stream")
    assert _lib.PARAMS["te_alrpk_layernorm_f32"] == ("G", "gamma", "rstd", "out", "K", "rows", "C", "stream")
    assert _lib.PARAMS["te_alrpk_token_relevance_f32"] == ("x0", "G", "out", "K", "B", "N", "C", "skip_first", "stream")
    for rule in ("damp", "act", "layernorm", "token_relevance"):
        # the class entry is its parent with K in front of the sizes; the bf16 entry is the f32 entry
        assert S[f"te_alrpk_{rule}_bf16"] == S[f"te_alrpk_{rule}_f32"], rule
        assert _lib.PARAMS[f"te_alrpk_{rule}_bf16"] == _lib.PARAMS[f"te_alrpk_{rule}_f32"], rule
        parent, child = list(_lib.PARAMS[f"te_alrp_{rule}_f32"]), list(_lib.PARAMS[f"te_alrpk_{rule}_f32"])
        child.remove("K")
        assert child == parent, rule
    # (MIN_LIB_VERSION stays where the C-ABI tests pin it: no existing argument list changed)
    assert lib.te_version() >= 803 and _lib.MIN_LIB_VERSION == 800


def test_class_entries_refuse_on_the_host():
    """Every refusal comes before a launch: fake non-null addresses are never dereferenced."""
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    A, INV, UNS = 4096, _lib.TE_ERR_INVALID_ARG, _lib.TE_ERR_UNSUPPORTED
    BIG = 1 << 31
    for sfx, odd in (("f32", 2), ("bf16", 1)):      # `odd`: an operand address off its element's boundary
        damp, act = getattr(lib, "te_alrpk_damp_" + sfx), getattr(lib, "te_alrpk_act_" + sfx)
        ln, tok = getattr(lib, "te_alrpk_layernorm_" + sfx), getattr(lib, "te_alrpk_token_relevance_" + sfx)
        # null pointers, K <= 0, sizes <= 0
        assert [damp(*p, 2, 4, 1e-6, None) for p in ((None, A, A), (A, None, A), (A, A, None))] == [INV] * 3
        assert damp(A, A, A, 0, 4, 1e-6, None) == INV and damp(A, A, A, -1, 4, 1e-6, None) == INV
        assert damp(A, A, A, 2, 0, 1e-6, None) == INV
        assert [damp(A, A, A, 2, 4, e, None) for e in (-1.0, float("nan"), float("inf"))] == [INV] * 3
        assert damp(A + 2, A, A, 2, 4, 1e-6, None) == UNS and damp(A, A + odd, A, 2, 4, 1e-6, None) == UNS
        assert damp(A, A, A + 1, 2, 4, 1e-6, None) == UNS
        assert damp(A, A, A, BIG, 4, 1e-6, None) == UNS and damp(A, A, A, 2, 1 << 42, 1e-6, None) == UNS
        assert act(A, A, A, 2, 4, 2, None) == INV and act(A, A, A, 2, 4, -1, None) == INV
        assert act(A, None, A, 2, 4, 0, None) == INV and act(A, A, A, 0, 4, 0, None) == INV and act(A, A, A, 2, 0, 1, None) == INV
        assert act(A, A + odd, A, 2, 4, 0, None) == UNS and act(A + 1, A, A, 2, 4, 0, None) == UNS
        assert act(A, A, A, 2, 1 << 42, 0, None) == UNS
        assert [ln(*p, 2, 2, 8, None) for p in ((None, A, A, A), (A, None, A, A), (A, A, None, A), (A, A, A, None))] == [INV] * 4
        assert [ln(A, A, A, A, *s, None) for s in ((0, 2, 8), (2, 0, 8), (2, 2, 0), (-3, 2, 8))] == [INV] * 4
        assert ln(A, A + odd, A, A, 2, 2, 8, None) == UNS and ln(A, A, A + 2, A, 2, 2, 8, None) == UNS
        assert ln(A + 3, A, A, A, 2, 2, 8, None) == UNS and ln(A, A, A, A + 2, 2, 2, 8, None) == UNS
        assert ln(A, A, A, A, 2, 1 << 34, 8, None) == UNS and ln(A, A, A, A, 2, 2, BIG, None) == UNS
        assert ln(A, A, A, A, BIG, 2, 8, None) == UNS
        assert [tok(*p, 2, 1, 4, 8, 0, None) for p in ((None, A, A), (A, None, A), (A, A, None))] == [INV] * 3
        assert [tok(A, A, A, *s, 0, None) for s in ((0, 1, 4, 8), (2, 0, 4, 8), (2, 1, 0, 8), (2, 1, 4, 0))] == [INV] * 4
        assert tok(A, A, A, 2, 1, 1, 8, 1, None) == INV          # nothing left without the first token
        assert tok(A, A, A, 2, 1, 4, 8, 2, None) == INV and tok(A, A, A, 2, 1, 4, 8, -1, None) == INV
        assert tok(A + odd, A, A, 2, 1, 4, 8, 0, None) == UNS and tok(A, A + 2, A, 2, 1, 4, 8, 0, None) == UNS
        assert tok(A, A, A + 2, 2, 1, 4, 8, 0, None) == UNS
        assert tok(A, A, A, 2, BIG, 4, 8, 0, None) == UNS and tok(A, A, A, 2, 1, 4, BIG, 0, None) == UNS
        assert tok(A, A, A, BIG, 1, 4, 8, 0, None) == UNS


# ------------------------------------------------------------------------------------------------ refusals of the public calls
def _calls():
    from transformer_explainability_amd.generators import LRP, Generator
    x = torch.zeros(2, 3, 16, 16)
    ids, mask = torch.ones(2, 4, dtype=torch.long), torch.ones(2, 4)
    lrp, gen = LRP(_no_forward(toy_vit(torch.float32, conserving=False))), Generator(_no_forward(_toy_bert()))
    return ((lambda **kw: lrp.generate_attnlrp_classes(x, **kw), lrp.model, 5),
            (lambda **kw: gen.generate_attnlrp_classes(ids, mask, **kw), gen.model, 2))


def test_bad_requests_are_refused_before_the_forward_pass():
    from transformer_explainability_amd import TeError
    for call, model, C in _calls():
        # exactly one of classes / topk / seeds
        with pytest.raises(ValueError, match="exactly one"):
            call()
        with pytest.raises(ValueError, match="exactly one"):
            call(classes=[0, 1], topk=2)
        for k in (0, C + 1, 1.5, True):
            with pytest.raises(ValueError, match="topk"):
                call(topk=k)
        with pytest.raises(ValueError, match="classes"):
            call(classes=[[0, C], [1, 0]])                     # out of range in host data
        with pytest.raises(ValueError, match="classes"):
            call(classes=[[0], [1], [0]])                      # three rows, a batch of two
        with pytest.raises(TeError, match="float32"):
            call(seeds=torch.zeros(2, C, dtype=torch.float64))
        with pytest.raises(ValueError, match="seeds"):
            call(seeds=torch.zeros(2, C + 1))
        with pytest.raises(ValueError, match="seeds"):
            call(seeds=[[0.0] * C] * 2)
        for bad in (0, -1, 1.5, True, "2"):
            with pytest.raises(ValueError, match="chunk"):
                call(topk=1, chunk=bad)
        for bad in (-1e-6, float("nan"), float("inf"), "1e-6", True):
            with pytest.raises(ValueError, match="eps"):
                call(topk=1, eps=bad)
        with pytest.raises(TypeError, match="head_mask"):      # not an argument of the new calls
            call(topk=1, head_mask=torch.ones(2))
        model.train()
        with pytest.raises(TeError, match="train mode"):
            call(topk=1)
        model.eval()
    vit_call = _calls()[0][0]
    for bad in ("transformer_attribution", "pixels", None):
        with pytest.raises(ValueError, match="method"):
            vit_call(topk=1, method=bad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64])
def test_other_dtypes_are_refused_before_the_forward_pass(dtype):
    """(bf16 here: a bf16 model on the host -- the chain on bf16 operands runs in the HIP kernels only)"""
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP, Generator
    x = torch.zeros(1, 3, 16, 16, dtype=dtype)
    with pytest.raises(TeError, match="GPU" if dtype == torch.bfloat16 else str(dtype)):
        LRP(_no_forward(toy_vit(dtype, conserving=False))).generate_attnlrp_classes(x, topk=2)
    ids, mask = torch.ones(1, 4, dtype=torch.long), torch.ones(1, 4)
    with pytest.raises(TeError, match="GPU" if dtype == torch.bfloat16 else str(dtype)):
        Generator(_no_forward(_toy_bert(dtype))).generate_attnlrp_classes(ids, mask, topk=2)


def test_method_tables_are_untouched():
    from transformer_explainability_amd import methods, sweep
    for name in ("attnlrp", "attnlrp_classes"):
        assert name not in methods.LRP_NEEDS and name not in methods.GENERATOR_NEEDS
        assert name not in methods.BASELINE_METHODS and name not in methods.SINGLE_CALL_PRUNED
    assert not any("attnlrp" in str(m).lower() for m in sweep.METHODS)


# ------------------------------------------------------------------------------------------------ linearity in the seed
def _onehot(B, C, cls):
    s = torch.zeros(B, C, dtype=torch.float64)
    s.scatter_(1, torch.as_tensor(cls).view(B, 1), 1.0)
    return s


def _assert_linear(R_diff, R_c, R_d):
    """R(onehot(c) - onehot(c')) = R(c) - R(c'): both sides are fp64 evaluations of sums whose terms have the magnitude of
    the two maps, so they agree to fp64 rounding of |R(c)| + |R(c')| -- 1e-12 of that magnitude leaves four digits for the
    depth of the chain."""
    scale = (R_c.abs() + R_d.abs()).amax(dim=-1, keepdim=True)
    assert float(scale.min()) > 0
    err = (R_diff - (R_c - R_d)).abs()
    assert bool((err <= 1e-12 * scale).all()), float((err / scale).max())
    assert float((R_c - R_d).abs().max()) > 1e-6 * float(scale.max())      # the two maps do differ


def test_the_restated_chain_is_linear_in_the_seed_vit():
    model = toy_vit(conserving=False)
    x = rnd((3, 3, 16, 16), 1)
    c, d = [4, 0, 2], [1, 3, 1]
    R_c, logits = ref.vit_attnlrp(model, x, index=torch.tensor(c))
    R_d, _ = ref.vit_attnlrp(model, x, index=torch.tensor(d))
    # a one-hot seed through the seeded restatement is the indexed one
    same, _ = sref.vit_attnlrp_seed(model, x, _onehot(3, 5, c))
    assert torch.equal(same, R_c)
    R_diff, _ = sref.vit_attnlrp_seed(model, x, _onehot(3, 5, c) - _onehot(3, 5, d))
    _assert_linear(R_diff, R_c, R_d)
    # and a general combination
    w = rnd((3, 5), 2)
    R_w, _ = sref.vit_attnlrp_seed(model, x, w)
    parts = [ref.vit_attnlrp(model, x, index=torch.full((3,), j))[0] for j in range(5)]
    want = sum(w[:, j:j + 1] * parts[j] for j in range(5))
    scale = sum((w[:, j:j + 1] * parts[j]).abs() for j in range(5)).amax(dim=-1, keepdim=True)
    assert bool(((R_w - want).abs() <= 1e-12 * scale).all())


def test_the_restated_chain_is_linear_in_the_seed_bert():
    model = _toy_bert(torch.float64)
    ids = torch.randint(1, 50, (3, 6), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(3, 6, dtype=torch.float64)
    mask[1, 4:] = 0.0
    R_1, _ = ref.bert_attnlrp(model, ids, mask, index=torch.tensor([1, 1, 1]))
    R_0, _ = ref.bert_attnlrp(model, ids, mask, index=torch.tensor([0, 0, 0]))
    R_diff, _ = sref.bert_attnlrp_seed(model, ids, mask, _onehot(3, 2, [1, 1, 1]) - _onehot(3, 2, [0, 0, 0]))
    _assert_linear(R_diff, R_1, R_0)
