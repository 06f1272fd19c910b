"""fp64 models, host side (no GPU): the dispatch on torch.float64, the refusals (each a TeError that names the dtype, raised
before any HIP call), the host-only parts of the C ABI (workspace queries, argument validation) and the torch rollout tail."""
import pytest
import torch

from f64_util import F64, rnd64
from host_util import lib  # noqa: F401
from oracle import relprop_oracle as O


def _lin(dt_r=F64, dt_x=F64, dt_w=F64):
    return rnd64((5, 3), 1).to(dt_r), rnd64((5, 4), 2).to(dt_x), rnd64((3, 4), 3).to(dt_w)


def test_fp64_linear_on_cpu_tensors_is_refused_for_the_device_not_the_dtype():
    """Fails on a tree without the fp64 path: there the refusal is the dtype message (… got torch.float64 here)."""
    from transformer_explainability_amd import TeError, ops
    with pytest.raises(TeError, match="CPU"):
        ops.linear_relprop(*_lin())


def test_every_fp64_rule_dispatches_and_asks_for_the_device():
    from transformer_explainability_amd import TeError, ops
    B, H, N, D = 1, 2, 5, 4
    q, k, v = rnd64((B, H, N, D), 4), rnd64((B, H, N, D), 5), rnd64((B, H, N, D), 6)
    a, r_nn = rnd64((B, H, N, N), 7), rnd64((B, H, N, N), 8)
    x = rnd64((2, 5, 4), 9)
    calls = [lambda: ops.matmul_relprop_av(q, a, v), lambda: ops.matmul_relprop_qk(r_nn, q, k),
             lambda: ops.add_relprop(x, x, x), lambda: ops.add_relprop(x, x, x[:1]),
             lambda: ops.add_relprop(r_nn, a, rnd64((B, 1, 1, N), 10), deferred=True),
             lambda: ops.clone_relprop([x, x], x), lambda: ops.clone_relprop([x, x, x], x),
             lambda: ops.index_select_relprop(x[:, :1], x, 0), lambda: ops.gradcam_headmean(a, r_nn)]
    for call in calls:
        with pytest.raises(TeError, match="CPU"):
            call()


def test_fp64_refusals_name_the_dtype():
    from transformer_explainability_amd import TeError, ops
    R, X, W = _lin()
    with pytest.raises(TeError, match=r"torch\.float64.*variant"):
        ops.linear_relprop(R, X, W, variant="lrp")
    with pytest.raises(TeError, match=r"torch\.float64.*alpha"):
        ops.linear_relprop(R, X, W, alpha=2.0)
    with pytest.raises(TeError, match=r"torch\.float64.*variant"):
        ops.add_relprop(X, X, X, variant="lrp")
    with pytest.raises(TeError, match=r"torch\.float64.*variant"):
        ops.matmul_relprop_av(rnd64((1, 1, 3, 2), 1), rnd64((1, 1, 3, 3), 2), rnd64((1, 1, 3, 2), 3), variant="lrp")
    # fp64 operands with fp32 relevance, the reverse, and fp64 mixed with bf16: no narrower format inside an fp64 rule
    for dts in ((torch.float32, F64, F64), (F64, torch.float32, torch.float32), (F64, F64, torch.float32),
                (F64, torch.bfloat16, torch.bfloat16), (torch.float32, F64, torch.bfloat16)):
        with pytest.raises(TeError, match="float64") as e:
            ops.linear_relprop(*_lin(*dts))
        assert "bfloat16" in str(e.value) and str(next(d for d in dts if d != F64)) in str(e.value), str(e.value)
    x = rnd64((2, 5, 4), 9)
    with pytest.raises(TeError, match=r"torch\.float32"):
        ops.clone_relprop([x, x.float()], x)
    with pytest.raises(TeError, match=r"torch\.float32"):
        ops.add_relprop(x.float(), x, x)
    with pytest.raises(TeError, match=r"torch\.float32"):
        ops.gradcam_headmean(rnd64((1, 2, 3, 3), 1), rnd64((1, 2, 3, 3), 2).float())
    with pytest.raises(TeError, match="float64"):
        ops.conv2d_zb_relprop(rnd64((1, 4, 2, 2), 1), rnd64((1, 3, 4, 4), 2), rnd64((4, 3, 2, 2), 3), None)
    assert "bfloat16" in ops.DTYPES_MSG and "float64" in ops.DTYPES_MSG


def test_method_full_on_an_fp64_model_is_refused_before_the_forward_pass():
    from transformer_explainability_amd import TeError, vit
    from transformer_explainability_amd.generators import LRP
    model = vit.VisionTransformer(img_size=16, patch_size=8, embed_dim=16, depth=1, num_heads=2, num_classes=3).double()
    x = rnd64((1, 3, 16, 16), 1)
    with pytest.raises(TeError, match=r"method='full'.*torch\.float64"):
        LRP(model).generate_LRP(x, method="full")
    assert getattr(model.head, "X", None) is None              # no forward pass ran
    with pytest.raises(TeError, match=r"method='full'.*torch\.float64"):
        model.relprop(torch.zeros(1, 3, dtype=F64), method="full")
    with pytest.raises(TeError, match="CPU"):                  # the default method reaches the fp64 rules
        LRP(model).generate_LRP(x)


def test_fused_producers_do_not_take_fp64():
    from transformer_explainability_amd import ops, producers, rules
    x = rnd64((2, 5, 16), 1)
    old = ops.USE_FUSED_PRODUCERS
    try:
        ops.USE_FUSED_PRODUCERS = True
        assert not producers.gelu_usable(x) and not producers.usable(x)
        assert not any(producers.linear_plan(x, rules.Linear(16, 8).double().eval()))
    finally:
        ops.USE_FUSED_PRODUCERS = old


def test_f64_workspace_queries(lib):
    T, i, o = 130, 72, 40
    assert lib.te_linear_relprop_f64_workspace_bytes(T, i, o) >= 8 * T * o
    assert lib.te_linear_relprop_f64_workspace_bytes(12608, 768, 3072) >= 8 * 12608 * 3072
    assert lib.te_matmul_relprop_av_f64_workspace_bytes(2, 3, 17, 16) >= 8 * 2 * 3 * 17 * 16
    assert lib.te_matmul_relprop_qk_f64_workspace_bytes(2, 3, 17, 16) >= 8 * 2 * 3 * 17 * 17
    assert lib.te_add_relprop_f64_workspace_bytes(3, 197 * 64) >= 8 * 3 * 5
    assert lib.te_add_bcast_relprop_f64_workspace_bytes(2, 2, 24) >= 8 * 2 * (24 + 5)
    for z in ((0, 1, 1), (1, 0, 1), (1, 1, -1)):
        assert lib.te_linear_relprop_f64_workspace_bytes(*z) == 0
        assert lib.te_add_bcast_relprop_f64_workspace_bytes(*z) == 0
    assert lib.te_matmul_relprop_av_f64_workspace_bytes(1, 1, 0, 4) == 0
    assert lib.te_matmul_relprop_qk_f64_workspace_bytes(1, 0, 1, 4) == 0
    assert lib.te_add_relprop_f64_workspace_bytes(0, 5) == 0 and lib.te_add_relprop_f64_workspace_bytes(2, 0) == 0


def test_f64_argument_validation_without_device(lib):
    """NULL, non-positive sizes and short workspaces are refused on the host (no pointer is dereferenced, no HIP call)."""
    p = 0x1000                                                 # a non-NULL value the host code must not read through
    assert lib.te_linear_relprop_f64(None, 3, p, 4, p, 4, p, 5, 4, 3, p, 1 << 20, None) == -1
    assert lib.te_linear_relprop_f64(p, 3, p, 4, p, 4, p, 0, 4, 3, p, 1 << 20, None) == -1
    assert lib.te_linear_relprop_f64(p, 2, p, 4, p, 4, p, 5, 4, 3, p, 1 << 20, None) == -1      # r_ld < out_f
    assert lib.te_linear_relprop_f64(p, 3, p, 4, p, 4, p, 5, 4, 3, None, 1 << 20, None) == -2
    assert lib.te_linear_relprop_f64(p, 3, p, 4, p, 4, p, 5, 4, 3, p, 8 * 5 * 3 - 1, None) == -2
    av = [p, 1, 1, 1, p, p, 1, 1, 1, p, 1, 1, 1, p, p, 1, 1, 1, 1, 1, 3, 2, 0.5]
    assert lib.te_matmul_relprop_av_f64(*av, p, 8 * 6 - 1, None) == -2
    assert lib.te_matmul_relprop_av_f64(*([None] + av[1:]), p, 1 << 20, None) == -1
    qk = [p, p, 1, 1, 1, p, 1, 1, 1, p, p, 1, 1, 1, p, 1, 1, 1, 1, 1, 3, 2, 0.5]
    assert lib.te_matmul_relprop_qk_f64(*qk, p, 8 * 9 - 1, None) == -2
    assert lib.te_matmul_relprop_qk_f64(*(qk[:9] + [None] + qk[10:]), p, 1 << 20, None) == -1     # Z is always an operand
    assert lib.te_add_relprop_f64(p, p, p, p, p, 2, 0, 0, p, 1 << 20, None) == -1
    assert lib.te_add_relprop_f64(p, p, p, p, p, 2, 8, 8, p, 8, None) == -2
    assert lib.te_add_bcast_relprop_f64(p, p, None, 0, p, p, 2, 2, 4, p, 1 << 20, None) == -1
    assert lib.te_add_bcast_relprop_f64(p, p, p, 0, p, p, 2, 2, 4, None, 0, None) == -2
    assert lib.te_clone_relprop_f64(p, None, None, p, p, 16, None) == -1
    assert lib.te_clone_relprop_f64(p, p, None, p, p, 0, None) == -1
    assert lib.te_index_select_relprop_f64(p, p, p, 2, 3, 4, 3, None) == -1                      # index out of range
    assert lib.te_gradcam_headmean_f64(p, p, None, 1, 2, 3, None) == -1


def test_f64_entries_are_timed_like_the_others(monkeypatch):
    """Every fp64 binding brackets its C-ABI call with ops._timed (bench.py's per-kernel table)."""
    import inspect
    from transformer_explainability_amd import ops
    for name in ("linear_relprop_f64", "matmul_relprop_av_f64", "matmul_relprop_qk_f64", "add_relprop_f64",
                 "clone_relprop_f64", "index_select_relprop_f64", "gradcam_headmean_f64"):
        assert "_timed(" in inspect.getsource(getattr(ops, name)), name


@pytest.mark.parametrize("normalise,cls_fixup,row0", [(False, False, True), (True, True, True), (True, False, False)])
def test_rollout_tail_in_double_is_the_reference_expression(normalise, cls_fixup, row0):
    from transformer_explainability_amd import ops
    cams = rnd64((4, 2, 6, 6), 3).abs()
    got = ops.rollout(cams, start_layer=1, normalise=normalise, cls_fixup=cls_fixup, row0_only=row0)
    ref = O.rollout(list(cams), 1, normalise=normalise).clone()
    if cls_fixup:
        ref[:, 0, 0] = ref[:, 0].min(dim=-1).values
    ref = ref[:, 0] if row0 else ref
    assert got.dtype == F64 and torch.equal(got, ref)
