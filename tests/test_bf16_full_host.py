"""Host-side checks of the bf16 z^B rule of the patch embedding (method="full" on a bf16 ViT; no GPU needed): the C ABI
declares, exports and binds the entry points, the shape and workspace queries give the documented values, bad arguments
are refused with the right status before any HIP call, conv_bf16_route names the kernel a geometry takes, and rules.Conv2d
keeps its weight planes the way rules.Linear does."""
import copy
import pickle

import pytest
import torch

TE_ERR_INVALID_ARG, TE_ERR_WORKSPACE, TE_ERR_UNSUPPORTED = -1, -2, -3
SYMBOLS = ["te_conv2d_zb_relprop_bf16_supported", "te_conv2d_zb_relprop_bf16_workspace_bytes",
           "te_conv2d_zb_bf16_weight_planes_bytes", "te_conv2d_zb_bf16_prepare_weights", "te_conv2d_zb_relprop_bf16"]


from host_util import lib  # noqa: E402,F401


def _up(n, a=256):
    return -(-n // a) * a


def test_entry_points_bound_and_version(lib):
    from transformer_explainability_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.te_version() >= 601 and _lib.MIN_LIB_VERSION >= 601


def test_supported_shapes(lib):
    sup = lib.te_conv2d_zb_relprop_bf16_supported
    for C, E, p in ((3, 768, 16), (3, 1024, 16), (3, 128, 16), (3, 128, 32), (3, 256, 48)):
        assert sup(C, E, p) == 1, (C, E, p)
    for C, E, p in ((3, 64, 8), (3, 128, 14), (1, 128, 16), (4, 128, 16), (3, 192, 16), (3, 64, 16), (3, 128, 8),
                    (3, 0, 16), (3, 128, 0)):
        assert sup(C, E, p) == 0, (C, E, p)


def test_conv_bf16_route(lib):
    from transformer_explainability_amd import ops
    assert ops.conv_bf16_route(3, 768, 16) == "bf16"
    assert ops.conv_bf16_route(3, 128, 32) == "bf16"
    assert ops.conv_bf16_route(3, 64, 8) == "fp32-upcast"
    assert ops.conv_bf16_route(3, 128, 14) == "fp32-upcast"
    assert ops.conv_bf16_route(1, 128, 16) == "fp32-upcast"


def test_workspace_and_plane_sizes(lib):
    ws = lib.te_conv2d_zb_relprop_bf16_workspace_bytes
    # three bf16 planes of S [T, E] and the per-sample min / max, each rounded up to 256 bytes
    assert ws(64, 3, 224, 224, 768, 16) == _up(3 * 64 * 196 * 768 * 2) + _up(64 * 2 * 4) == 57803264
    assert ws(1, 3, 16, 16, 128, 16) == _up(3 * 128 * 2) + 256 == 1024
    assert ws(2, 3, 32, 48, 128, 16) == _up(3 * 12 * 128 * 2) + 256
    for bad in ((0, 3, 224, 224, 768, 16), (2, 3, 224, 230, 768, 16), (2, 3, 220, 224, 768, 16), (2, 3, 224, 224, 0, 16),
                (2, 3, 224, 224, 768, 0)):
        assert ws(*bad) == 0, bad
    planes = lib.te_conv2d_zb_bf16_weight_planes_bytes
    # W+^T and W-^T [K, E] in bf16, then the two fp32 channel sums
    assert planes(3, 768, 16) == 2 * 768 * 768 * 2 + _up(768 * 2 * 4) == 2365440
    assert planes(3, 128, 32) == 2 * 3072 * 128 * 2 + 1024
    assert planes(3, 0, 16) == 0


def test_arguments_are_validated_before_any_hip_call(lib):
    """No device is touched: the pointers are made-up (aligned, non-null) addresses and every call must return first."""
    rule = lib.te_conv2d_zb_relprop_bf16
    P_, big = 0x10000, 1 << 40
    B, C, H, W, E, p = 2, 3, 32, 48, 128, 16
    PE = (H // p) * (W // p) * E
    good = dict(R=P_, r_bs=PE, X=P_, Wt=P_, planes=P_, out=P_, B=B, C=C, H=H, W=W, E=E, p=p, ws=P_, ws_bytes=big)

    def call(**kw):
        a = dict(good, **kw)
        return rule(a["R"], a["r_bs"], a["X"], a["Wt"], a["planes"], a["out"], a["B"], a["C"], a["H"], a["W"], a["E"],
                    a["p"], a["ws"], a["ws_bytes"], None)

    for name in ("R", "X", "Wt", "planes", "out"):
        assert call(**{name: None}) == TE_ERR_INVALID_ARG, name
    for name in ("B", "C", "H", "W", "E", "p"):
        assert call(**{name: 0}) == TE_ERR_INVALID_ARG, name
    assert call(r_bs=PE - 1) == TE_ERR_INVALID_ARG
    assert call(X=P_ + 2) == TE_ERR_INVALID_ARG and call(Wt=P_ + 8) == TE_ERR_INVALID_ARG      # 16-byte loads
    assert call(H=40) == TE_ERR_UNSUPPORTED and call(W=40) == TE_ERR_UNSUPPORTED                # H % p, W % p
    assert call(C=1) == TE_ERR_UNSUPPORTED and call(E=64) == TE_ERR_UNSUPPORTED
    assert call(p=8, r_bs=1 << 30) == TE_ERR_UNSUPPORTED
    need = lib.te_conv2d_zb_relprop_bf16_workspace_bytes(B, C, H, W, E, p)
    assert call(ws=None) == TE_ERR_WORKSPACE
    assert call(ws_bytes=need - 1) == TE_ERR_WORKSPACE
    assert call(ws_bytes=0) == TE_ERR_WORKSPACE
    assert call(ws=P_ + 4) == TE_ERR_WORKSPACE
    prep = lib.te_conv2d_zb_bf16_prepare_weights
    assert prep(None, 3, 128, 16, P_, big, None) == TE_ERR_INVALID_ARG
    assert prep(P_, 3, 128, 16, None, big, None) == TE_ERR_INVALID_ARG
    assert prep(P_, 3, 0, 16, P_, big, None) == TE_ERR_INVALID_ARG
    assert prep(P_, 3, 128, 16, P_, lib.te_conv2d_zb_bf16_weight_planes_bytes(3, 128, 16) - 1, None) == TE_ERR_WORKSPACE


def test_refusals_on_the_host(lib):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    bf = torch.bfloat16
    R, X, W = torch.zeros(1, 128, 1, 1), torch.zeros(1, 3, 16, 16, dtype=bf), torch.zeros(128, 3, 16, 16, dtype=bf)
    with pytest.raises(TeError, match="CPU"):
        ops.conv2d_zb_relprop_bf16(R, X, W)
    with pytest.raises(TeError, match="CPU"):               # the public entry dispatches on the operand dtype
        ops.conv2d_zb_relprop(R, X, W, None)
    with pytest.raises(TeError, match="bfloat16"):          # mixed operand dtypes
        ops.conv2d_zb_relprop(R, X, W.float(), None)
    with pytest.raises(TeError, match="bfloat16"):
        ops.conv2d_zb_relprop(R, X.float(), W, None)
    with pytest.raises(TeError, match="bfloat16"):
        ops.conv2d_zb_relprop(R, X.half(), W.half(), torch.zeros(1, 128, 1, 1))  # fp16 stays refused


def test_conv2d_keeps_its_planes_like_linear(lib):
    """The weight planes are device scratch: out of pickle / deepcopy, dropped by load_state_dict, .to() and
    ops.x6_invalidate, and keyed on the weight's identity and version."""
    from transformer_explainability_amd import ops, rules
    conv = rules.Conv2d(3, 128, kernel_size=16, stride=16)
    key = ops._weight_key(conv.weight.detach())
    rules.x6_cache(conv)["conv_bf16_planes"] = (key, torch.zeros(1), torch.zeros(1))
    assert "_te_cache" not in pickle.loads(pickle.dumps(conv)).__dict__
    assert "_te_cache" not in copy.deepcopy(conv).__dict__
    assert rules.x6_cache(conv)                                  # the original keeps its own
    assert ops.x6_invalidate(conv) == 1 and not rules.x6_cache(conv)
    rules.x6_cache(conv)["conv_bf16_planes"] = (key, torch.zeros(1), torch.zeros(1))
    conv.load_state_dict(copy.deepcopy(conv.state_dict()))
    assert not rules.x6_cache(conv)
    rules.x6_cache(conv)["conv_bf16_planes"] = (key, torch.zeros(1), torch.zeros(1))
    conv.to(torch.bfloat16)
    assert not rules.x6_cache(conv)
    # an in-place edit autograd records changes the key
    k0 = ops._weight_key(conv.weight.detach())
    with torch.no_grad():
        conv.weight.mul_(2.0)
    assert ops._weight_key(conv.weight.detach()) != k0
    # a model-wide invalidation reaches the patch embedding
    seq = torch.nn.Sequential(conv, rules.Linear(4, 4))
    rules.x6_cache(conv)["conv_bf16_planes"] = (k0, torch.zeros(1), torch.zeros(1))
    assert ops.x6_invalidate(seq) == 1 and not rules.x6_cache(conv)


def test_fp32_operands_without_the_forward_output_are_refused(lib):
    """Y is optional only because bf16 operands do without it: an fp32 call that leaves it out gets a TeError."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    with pytest.raises(TeError, match="forward output"):
        ops.conv2d_zb_relprop(torch.zeros(1, 128, 1, 1), torch.zeros(1, 3, 16, 16), torch.zeros(128, 3, 16, 16), None)


def test_the_bf16_gemm_loops_share_one_definition_of_their_helpers():
    """te_bf16.hip and te_conv_bf16.hip run the same tile structure: the staging constants, the fragment read and the
    16x16x32 bf16 MFMA macro are defined once, in csrc/te_bf16_tile.h (the rule of tests/test_csrc_shared.py)."""
    import test_csrc_shared as shared
    sources = shared._sources()
    for what, pattern in [("u16x8", shared._typedef("u16x8")), ("bf", shared._function("bf")),
                          ("frag", shared._function("frag")), ("TE_MFMA16_BF16", shared._macro("TE_MFMA16_BF16")),
                          ("the 16x16x32 bf16 MFMA", r"__builtin_amdgcn_mfma_f32_16x16x32_bf16"),
                          ("kLd", r"\bint\s+kLd\b"), ("kBK", r"\bint\s+kBK\b")]:
        assert shared.definitions(sources, pattern) == [("te_bf16_tile.h", 1)], what
    for name in ("te_bf16.hip", "te_conv_bf16.hip"):
        assert '#include "te_bf16_tile.h"' in sources[name], name
