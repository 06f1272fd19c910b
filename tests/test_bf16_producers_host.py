"""Host-side checks of the bf16 attention producers (no GPU needed): the entry points of csrc/te_attn_bf16.hip are declared,
bound and exported by the cross-compiled library and validate their arguments before any HIP call; the ops wrappers refuse
CPU operands; ops.USE_FUSED_PRODUCERS changes nothing for a bf16 model on the CPU."""
import ctypes
import os
import re

import pytest
import torch

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["te_attention_bf16_supported", "te_attention_forward_strided_bf16", "te_attention_backward_strided_bf16",
               "te_attention_backward_strided_bf16_workspace_bytes"]


from host_util import lib  # noqa: E402,F401


def test_entry_points_declared_bound_and_exported(lib):
    from transformer_explainability_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "te_relprop.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in te_relprop.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} is not exported by libte_relprop.so"
    # the argument lists of the _strided_f32 entry points; the backward without the fp32 form's optional forward output `out`
    # and its three strides, which the bf16 kernels do not take
    assert _lib.SIGNATURES["te_attention_forward_strided_bf16"] == _lib.SIGNATURES["te_attention_forward_strided_f32"]
    assert _lib.PARAMS["te_attention_forward_strided_bf16"] == _lib.PARAMS["te_attention_forward_strided_f32"]
    f32 = _lib.PARAMS["te_attention_backward_strided_f32"]
    assert f32[4:8] == ("out", "o_sb", "o_sh", "o_sn")
    assert _lib.PARAMS["te_attention_backward_strided_bf16"] == f32[:4] + f32[8:]
    types = _lib.SIGNATURES["te_attention_backward_strided_f32"]
    assert _lib.SIGNATURES["te_attention_backward_strided_bf16"] == (types[0], types[1][:4] + types[1][8:])
    assert "te_attn_bf16.hip" in open(os.path.join(ROOT, "transformer-explainability_amd", "build.py")).read()


def test_supported_shapes_and_host_side_validation(lib):
    from transformer_explainability_amd import _lib, ops
    assert ops.attention_forward_bf16_supported(197, 64) and ops.attention_forward_bf16_supported(640, 64)
    assert ops.attention_forward_bf16_supported(1, 64)
    assert not ops.attention_forward_bf16_supported(641, 64) and not ops.attention_forward_bf16_supported(0, 64)
    assert not ops.attention_forward_bf16_supported(197, 32)
    assert lib.te_attention_backward_strided_bf16_workspace_bytes(64, 12, 197) >= 64 * 12 * 197 * 4
    assert lib.te_attention_backward_strided_bf16_workspace_bytes(0, 12, 197) == 0
    # null pointers, unsupported shapes and unaligned views are rejected on the host, before any HIP call
    buf = (ctypes.c_uint16 * 4096)()
    base = ctypes.addressof(buf)
    p = (base + 15) // 16 * 16
    st = (128, 64, 128)
    fwd = lambda q, N, D, sn=128: lib.te_attention_forward_strided_bf16(      # noqa: E731
        q, 128, 64, sn, p, *st, p, *st, None, None, None, p, p, *st, 1, 2, N, D, 0.125, None)
    assert fwd(None, 1, 64) == -1
    assert fwd(p, 641, 64) == _lib.TE_ERR_UNSUPPORTED
    assert fwd(p, 1, 32) == _lib.TE_ERR_UNSUPPORTED
    assert fwd(p + 2, 1, 64) == _lib.TE_ERR_UNSUPPORTED          # 16-byte loads of feature rows
    assert fwd(p, 1, 64, sn=132) == _lib.TE_ERR_UNSUPPORTED
    bwd = lambda N, D, need_qk, ws, nb: lib.te_attention_backward_strided_bf16(      # noqa: E731
        p, *st, p, *st, p, *st, p, *st, p, p, p, *st, p, *st, p, *st, 1, 2, N, D, 0.125, need_qk, ws, nb, None)
    assert bwd(641, 64, 1, p, 4096) == _lib.TE_ERR_UNSUPPORTED
    assert bwd(1, 32, 1, p, 4096) == _lib.TE_ERR_UNSUPPORTED
    assert bwd(1, 64, 1, None, 0) == -2
    assert bwd(1, 64, 1, p, 4) == -2


def test_ops_wrappers_refuse_cpu_and_mixed_operands():
    from transformer_explainability_amd import TeError, ops
    q, k, v = (torch.zeros(1, 4, 128, dtype=BF) for _ in range(3))
    with pytest.raises(TeError, match="CPU"):
        ops.attention_forward_qkv(q, k, v, 2, 0.125)
    with pytest.raises(TeError, match="CPU"):
        ops.attention_forward(torch.zeros(1, 4, 384, dtype=BF), 2, 0.125)
    attn = torch.zeros(1, 2, 4, 4, dtype=BF)
    with pytest.raises(TeError, match="CPU"):
        ops.attention_backward_qkv(q, q, k, v, attn, 2, 0.125, q.clone(), k.clone(), v.clone())
    with pytest.raises(TeError, match="CPU"):
        ops.attention_backward(q, torch.zeros(1, 4, 384, dtype=BF), attn, 2, 0.125)
    with pytest.raises(TeError, match="bf16 rule got a torch.float32"):
        ops.attention_forward_qkv(q.float(), k, v, 2, 0.125)
    with pytest.raises(TeError, match="planes"):
        ops.attention_forward(torch.zeros(1, 4, 384, dtype=BF), 2, 0.125, planes=True)


def _flag_on_off(fn):
    from transformer_explainability_amd import ops
    was = ops.USE_FUSED_PRODUCERS
    try:
        ops.USE_FUSED_PRODUCERS = False
        off = fn()
        ops.USE_FUSED_PRODUCERS = True
        on = fn()
    finally:
        ops.USE_FUSED_PRODUCERS = was
    return off, on


def test_bf16_cpu_models_ignore_the_flag():
    """The fused route is for device tensors: a bf16 model on the CPU gives the same bits with the flag on and off."""
    from transformer_explainability_amd import bert, ops, vit
    assert ops.USE_FUSED_PRODUCERS is False
    torch.manual_seed(0)
    m = vit.VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=8,
                              qkv_bias=True).eval().to(BF)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(BF)
    off, on = _flag_on_off(lambda: m(x).clone())
    assert off.dtype == BF and torch.equal(off, on)
    assert all(b.attn._fused_anchor is None for b in m.blocks)
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                              intermediate_size=128, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(0)
    b = bert.BertForSequenceClassification(cfg).eval().to(BF)
    ids = torch.randint(1, 100, (2, 24), generator=torch.Generator().manual_seed(1))
    mask = torch.ones(2, 24)
    mask[1, 18:] = 0.0
    off, on = _flag_on_off(lambda: b(ids, attention_mask=mask)[0].clone())
    assert off.dtype == BF and torch.equal(off, on)
    assert all(lay.attention.self._fused_anchor is None for lay in b.bert.encoder.layer)
