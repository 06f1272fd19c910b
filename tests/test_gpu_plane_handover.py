"""The plane hand-overs between layers (DESIGN.md "The layer's scratch dict") at the smallest shapes at which they engage:
head dim 64, >= 256 rows, features in multiples of 128.  B = 2, N = 130: T = 260 rows, ragged against the 32-row blocks."""
import pytest
import torch

from gpu_util import dev, rnd

pytestmark = pytest.mark.gpu

MAILBOXES = ("x_planes_from_producer", "x_abs_planes", "dy_planes_from_consumer")


def test_attention_block_hands_planes_to_the_projection_small():
    """vit.Attention(128, 2 heads) on the producer kernels, projection on the x6 kernels: output and proj.relprop are bitwise
    equal with the hand-over on and off (ops.X6_KEEP_ABS).  And the negative case: planes that wait for the producer's output
    are not used for another tensor -- a clone of it -- the entry is gone, and the layer's own split pass gives the same bits."""
    from transformer_explainability_amd import ops, rules, vit
    d = dev()
    torch.manual_seed(7)
    x = rnd((2, 130, 128), 121).to(d)
    R = rnd((2, 130, 128), 122, 1e-3).to(d)
    saved = (ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6, ops.X6_KEEP_ABS)
    orig = ops.attention_forward
    calls = {"planes": 0}

    def counting(*a, **k):
        calls["planes"] += int(bool(k.get("planes")))
        return orig(*a, **k)

    try:
        ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6 = True, "all", True
        blk = vit.Attention(128, num_heads=2, qkv_bias=True).to(d).eval()
        cache = rules.x6_cache(blk.proj)
        ops.attention_forward = counting
        res = {}
        for handover in (True, False):
            ops.X6_KEEP_ABS = handover
            calls["planes"] = 0
            y = blk(x)
            assert calls["planes"] == (1 if handover else 0)
            assert "x_planes_from_producer" not in cache and ("x_abs_planes" in cache) == handover
            cam = blk.proj.relprop(R, alpha=1)
            assert not any(k in cache for k in MAILBOXES)
            res[handover] = (y.detach().clone(), cam.detach().clone())
        assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
        # the producer alone, so that its planes wait in the projection's dict; they are zeroed: using them would show
        ops.X6_KEEP_ABS = True
        out, _, _ = vit._FusedAttention.apply(blk.qkv(x), 2, blk.scale, blk, cache)
        assert cache["x_planes_from_producer"][3].data_ptr() == out.data_ptr()
        cache["x_planes_from_producer"][1].zero_()
        other = out.detach().clone()
        y2 = blk.proj(other)
        assert "x_planes_from_producer" not in cache
        assert cache["x_abs_planes"][0] == ops._x_abs_key(other, 260, 128)        # split from the tensor the layer received
        assert torch.equal(y2, res[True][0])
        assert torch.equal(blk.proj.relprop(R, alpha=1), res[True][1]) and "x_abs_planes" not in cache
    finally:
        ops.attention_forward = orig
        ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6, ops.X6_KEEP_ABS = saved


def test_mlp_block_gelu_hands_planes_to_its_neighbours_small():
    """vit.Mlp(128, 512) inside ops.gelu_backward_plane_handoff(): output, input gradient and relprop are bitwise equal with
    the GELU emitting its neighbours' operand planes (ops.X6_FUSE_GELU) and without; the plane-emitting kernels ran exactly
    when it was on, and no mailbox entry is left in either layer's dict."""
    from transformer_explainability_amd import ops, rules, vit
    d = dev()
    torch.manual_seed(8)
    mlp = vit.Mlp(128, 512).to(d).eval()
    x = rnd((2, 130, 128), 131).to(d).requires_grad_(True)
    g = rnd((2, 130, 128), 132).to(d)
    R = rnd((2, 130, 128), 133, 1e-3).to(d)
    was = (ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6, ops.X6_KEEP_ABS, ops.X6_FUSE_GELU)
    f0, b0 = ops.gelu_forward_planes, ops.gelu_backward_planes
    calls = {"fwd": 0, "bwd": 0}

    def fwd(*a):
        calls["fwd"] += 1
        return f0(*a)

    def bwd(*a):
        calls["bwd"] += 1
        return b0(*a)

    ops.gelu_forward_planes, ops.gelu_backward_planes = fwd, bwd
    try:
        ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6, ops.X6_KEEP_ABS = True, "all", True, True
        outs = []
        for fuse in (True, False):
            ops.X6_FUSE_GELU = fuse
            with ops.gelu_backward_plane_handoff():
                y = mlp(x)
            (dx,) = torch.autograd.grad(y, x, g)
            cam = mlp.relprop(R, alpha=1.0)
            outs.append((y.detach().clone(), dx.clone(), cam.clone()))
            assert calls == {"fwd": 1, "bwd": 1}                 # (ran once in the first pass, not again in the second)
            for lin in (mlp.fc1, mlp.fc2):
                assert not any(k in rules.x6_cache(lin) for k in MAILBOXES)
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        assert all(torch.isfinite(t).all() for t in outs[0])
    finally:
        ops.gelu_forward_planes, ops.gelu_backward_planes = f0, b0
        ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.USE_LINEAR_X6, ops.X6_KEEP_ABS, ops.X6_FUSE_GELU = was
