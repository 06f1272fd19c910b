"""Host-side checks of bf16 BERT (no GPU needed): the forward runs in the parameters' dtype with the extended mask built
the way transformers 3.5.1 builds it, every rule module caches bf16 operands, the broadcast-mask Add's bf16 entry points
are declared, exported and bound, and the refusals are TeErrors."""
import ctypes
import os
import re

import pytest
import torch

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["te_add_bcast_relprop_bf16", "te_add_bcast_relprop_deferred_bf16"]


from host_util import lib  # noqa: E402,F401


def _small_bert(dtype=BF, rules=None, seed=0):
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                              intermediate_size=128, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(seed)
    cls = bert.BertForSequenceClassification if rules is None else \
        bert.make_bert_module(rules)["BertForSequenceClassification"]
    return cls(cfg).eval().to(dtype)


def _inputs(B=2, N=24):
    ids = torch.randint(1, 100, (B, N), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(B, N)
    mask[1, N - 6:] = 0.0                 # padding
    mask[0, 3] = 0.99609375               # 1 - 2^-8: bf16 keeps it, the extended mask is -39.0625 -> bf16 -39.0
    return ids, mask


def _operands(model):
    for name, mod in model.named_modules():
        X = getattr(mod, "X", None)
        if X is None:
            continue
        for x in (X if isinstance(X, list) else [X]):
            yield name, x


def test_bf16_bert_forward_caches_bf16_operands():
    """A bf16 BERT used to fail here: the fp32 extended mask promoted scores + mask to fp32 and matmul2 got fp32
    probabilities with bf16 v (RuntimeError)."""
    model = _small_bert()
    ids, mask = _inputs()
    logits = model(ids, attention_mask=mask)[0]
    assert logits.dtype == BF and logits.shape == (2, 2) and torch.isfinite(logits.float()).all()
    ops_seen = list(_operands(model))
    assert len(ops_seen) > 30
    assert [(n, x.dtype) for n, x in ops_seen if x.dtype != BF] == []
    for lay in model.bert.encoder.layer:
        sa = lay.attention.self
        assert sa.get_attn().dtype == BF and sa.matmul2.Y.dtype == BF


def test_bf16_extended_mask_values():
    model = _small_bert()
    ids, mask = _inputs()
    model(ids, attention_mask=mask)
    for lay in model.bert.encoder.layer:
        ext = lay.attention.self.add.X[1]
        assert ext.dtype == BF and ext.shape == (2, 1, 1, 24)
        assert float(ext[0, 0, 0, 3]) == -39.0
        assert float(ext[1, 0, 0, 20]) == -9984.0          # bf16(-10000)
        hard = torch.cat([ext[0, 0, 0, :3], ext[0, 0, 0, 4:], ext[1, 0, 0]])
        assert set(hard.float().unique().tolist()) <= {0.0, -9984.0}
        assert (hard == -9984.0).sum() == 6
    # no mask given: all ones, extended mask zero in bf16
    model(ids)
    ext = model.bert.encoder.layer[0].attention.self.add.X[1]
    assert ext.dtype == BF and not ext.any()


def test_fp32_extended_mask_is_bitwise_unchanged():
    model = _small_bert(torch.float32)
    ids, mask = _inputs()
    for m in (mask, mask.long(), mask.bool()):
        model(ids, attention_mask=m)
        ext = model.bert.encoder.layer[0].attention.self.add.X[1]
        want = (1.0 - m[:, None, None, :].float()) * -10000.0
        assert ext.dtype == torch.float32
        assert torch.equal(ext.view(torch.int32), want.view(torch.int32))


def test_fp16_bert_forward_runs_and_relprop_refuses():
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import Generator
    model = _small_bert(torch.float16)
    ids, mask = _inputs()
    logits = model(ids, attention_mask=mask)[0]
    assert logits.dtype == torch.float16
    assert model.bert.encoder.layer[0].attention.self.add.X[1].dtype == torch.float16
    with pytest.raises(TeError, match="bfloat16"):
        Generator(model).generate_LRP(ids, mask, start_layer=0)


def test_bcast_mask_entry_points_declared_exported_bound(lib):
    from transformer_explainability_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "te_relprop.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert _lib.SIGNATURES["te_add_bcast_relprop_bf16"][1] == _lib.SIGNATURES["te_add_bcast_relprop_f32"][1]
    assert _lib.SIGNATURES["te_add_bcast_relprop_deferred_bf16"][1] == \
        _lib.SIGNATURES["te_add_bcast_relprop_deferred_f32"][1]


def test_bcast_mask_entry_points_validate_on_the_host(lib):
    """Argument checks return before any HIP call (the pointers below are never dereferenced)."""
    p = ctypes.c_void_p(256)
    ws = lib.te_add_bcast_relprop_workspace_bytes(2, 12, 512)
    assert ws > 0
    # null pointers / sizes
    assert lib.te_add_bcast_relprop_bf16(None, p, p, p, p, 2, 12, 512, 0, p, ws, None) == -1
    assert lib.te_add_bcast_relprop_bf16(p, p, p, p, p, 0, 12, 512, 0, p, ws, None) == -1
    assert lib.te_add_bcast_relprop_deferred_bf16(p, p, None, p, p, p, 2, 12, 512, p, ws, None) == -1
    # unknown variant: invalid; the lrp variant: not implemented on bf16 operands (it is on fp32)
    assert lib.te_add_bcast_relprop_bf16(p, p, p, p, p, 2, 12, 512, 7, p, ws, None) == -1
    assert lib.te_add_bcast_relprop_bf16(p, p, p, p, p, 2, 12, 512, 1, p, ws, None) == -3
    # the N <= 2048 limit of the _f32 forms
    big = lib.te_add_bcast_relprop_workspace_bytes(1, 1, 2049)
    assert lib.te_add_bcast_relprop_bf16(p, p, p, p, p, 1, 1, 2049, 0, p, big, None) == -3
    assert lib.te_add_bcast_relprop_deferred_bf16(p, p, p, p, p, p, 1, 1, 2049, p, big, None) == -3
    assert lib.te_add_bcast_relprop_deferred_bf16(p, p, p, p, p, p, 70000, 1, 8, p, 1 << 40, None) == -3
    # workspace
    assert lib.te_add_bcast_relprop_bf16(p, p, p, p, p, 2, 12, 512, 0, None, ws, None) == -2
    assert lib.te_add_bcast_relprop_deferred_bf16(p, p, p, p, p, p, 2, 12, 512, p, ws - 1, None) == -2


def test_bcast_mask_refusals():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    R = torch.zeros(2, 12, 16, 16)
    X0 = torch.zeros(2, 12, 16, 16, dtype=BF)
    mask = torch.zeros(2, 1, 1, 16, dtype=BF)
    with pytest.raises(TeError, match="CPU"):
        ops.add_relprop(R, X0, mask)
    with pytest.raises(TeError, match="CPU"):
        ops.add_relprop(R, X0, mask, deferred=True)
    with pytest.raises(TeError, match="variant"):
        ops.add_relprop(R, X0, mask, variant="lrp")


def test_bf16_bert_lrp_variant_and_alpha_refused():
    """The reference's BERT_orig_lrp on a bf16 model, and alpha != 1: TeError, before anything reaches the device."""
    from transformer_explainability_amd import ops, rules_lrp
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import Generator
    ids, mask = _inputs()
    model = _small_bert(rules=rules_lrp)
    with pytest.raises(TeError, match="variant"):
        Generator(model).generate_LRP(ids, mask, start_layer=0)
    model = _small_bert()
    logits = model(ids, attention_mask=mask)[0]
    oh = torch.zeros(logits.shape)
    oh[:, 0] = 1.0
    with pytest.raises(TeError, match="alpha"):
        model.relprop(oh, alpha=2)
    with pytest.raises(TeError, match="alpha"):
        ops.linear_relprop(oh, model.classifier.X, model.classifier.weight, alpha=2)


def test_bert_base_bf16_routes(lib):
    from transformer_explainability_amd import ops
    for B in (1, 4, 32):
        assert ops.linear_bf16_route(B, 768, 2) == "fp32-upcast"          # the num_labels-wide classifier
        assert ops.linear_bf16_route(B, 768, 768) == "bf16"               # pooler; last layer's cls rows
        assert ops.linear_bf16_route(B, 768, 3072) == "bf16"
        assert ops.linear_bf16_route(B, 3072, 768) == "bf16"
        T = B * 512
        for i, o in ((768, 768), (768, 3072), (3072, 768)):
            assert ops.linear_bf16_route(T, i, o) == "bf16", (T, i, o)
    assert ops.attention_bf16_route(512, 64) == "bf16"
    assert ops.attention_bf16_route(128, 64) == "bf16"
    assert ops.attention_bf16_route(24, 16) == "fp32-upcast"               # head dim 16 (the tiny golden BERT)
    for T, i, o in ((48, 64, 64), (48, 64, 128), (48, 128, 64)):
        assert ops.linear_bf16_route(T, i, o) == "fp32-upcast", (T, i, o)
