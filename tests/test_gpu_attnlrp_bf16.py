"""AttnLRP on bf16 models, on the MI355X (te_relprop.h, "AttnLRP, bf16 operands").

Streaming rules: every te_attnlrp_*_bf16 entry equals its te_alrp_*_f32 entry on ``.float()`` copies of the bf16 operand bit for
bit -- aligned bases and bases one and two elements off, special values, eps 0 and 1e-6, in place.

Linear product: with a W that has at most one non-zero (+-2^j) per column the output is G's (eps = 0) or te_attnlrp_damp_bf16's
(eps = 1e-6) bits, permuted and scaled, bit for bit; on random operands it stays within the first-order bound derived at the
test; a row alone equals the same row in a batch, strided G / Y are read in place.

Attention rule: per sample within 2 x the error of the fp32 torch expression of the same backward against its fp64 evaluation
on the upcast operands; exact at N = 1; a (b, h) alone equals the same pair in the batch.

Models: the yardstick is the same-cache restatement (tests/attnlrp_cache_ref.py) in fp64; per sample the chain's error stays
within 2 x the error of the same restatement evaluated in fp32.  Batch = samples, eager = graph replay, and the same bits
whatever ops.USE_FUSED_PRODUCERS says.  The measured ratios go to attnlrp_bf16_parity.json next to the parity report
(committed as profiles/attnlrp_bf16_parity.json).

Without the feature the model tests fail at the refusal of generate_attnlrp and the rule tests at the missing entries."""
import json
import math
import os

import pytest
import torch

import attnlrp_cache_ref as cref
from gpu_util import REPORT, dev, rnd, sliced_relprop_state
from test_gpu_attnlrp import _bert_inputs, _rel_l2, _tiny_bert, _tiny_vit, bits_equal

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
U = 2.0 ** -24
PARITY = os.path.join(os.path.dirname(REPORT), "attnlrp_bf16_parity.json")
_parity = {}


def _ratio(e, e_ref):
    """e / e_ref per sample; None where the reference's error is zero (the assertion then asks for zero)"""
    return [float(a / b) if b > 0 else None for a, b in zip(e.tolist(), e_ref.tolist())]


def _record(tag, **kw):
    _parity[tag] = kw
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        json.dump(_parity, f, indent=1, sort_keys=True)


def at_offset(t, off):
    """t's values in a dense device view that starts ``off`` elements behind a 16-byte boundary"""
    base = torch.empty(t.numel() + off, dtype=t.dtype, device=dev())
    assert base.data_ptr() % 16 == 0
    view = base[off:].view(t.shape)
    view.copy_(t)
    return view


# values a bf16 holds exactly: +-0, the nearest bf16 of +-1e-30, +-3
SPECIAL = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0]).to(BF16)
OFFSETS = (0, 1, 2)


def _operand(shape, seed, scale=1.0):
    """a bf16 operand with the special values in front (and once more, shuffled, further back)"""
    y = (rnd(shape, seed) * scale).to(BF16)
    flat = y.view(-1)
    n = flat.numel()
    flat[:min(n, 6)] = SPECIAL[:n]
    if n > 16:
        flat[9:15] = SPECIAL[torch.randperm(6, generator=torch.Generator().manual_seed(seed))]
    return y


# ------------------------------------------------------------------------------------------------ streaming rules
@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_damp_bf16_is_the_f32_entry_on_upcast_copies(n, eps):
    from transformer_explainability_amd import ops
    Y, G = _operand((n,), n + 1), rnd((n,), n + 2) * 4.0
    want = ops.alrp_damp(G.to(dev()), Y.to(dev()).float(), eps)
    assert torch.isfinite(want).all()
    for g_off in (0, 1):
        for y_off in OFFSETS:
            Gv, Yv = at_offset(G, g_off), at_offset(Y, y_off)
            assert Yv.dtype == BF16 and Yv.data_ptr() % 16 == 2 * y_off
            assert bits_equal(ops.alrp_damp(Gv, Yv, eps), want), (g_off, y_off)
            assert bits_equal(ops.alrp_damp(Gv, Yv, eps, out=at_offset(torch.zeros(n), g_off)), want), (g_off, y_off)
            assert ops.alrp_damp(Gv, Yv, eps, out=Gv) is Gv and bits_equal(Gv, want), (g_off, y_off)      # in place


@pytest.mark.parametrize("kind", ["gelu", "tanh"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_act_bf16_is_the_f32_entry_on_upcast_copies(n, kind):
    from transformer_explainability_amd import ops
    x, G = _operand((n,), n + 3, 3.0), rnd((n,), n + 4) * 2.0
    if n > 16:
        x[15:17] = torch.tensor([20.0, -20.0]).to(BF16)
    want = ops.alrp_act(G.to(dev()), x.to(dev()).float(), kind)
    assert torch.isfinite(want).all()
    if n >= 2:
        assert bits_equal(want[:2], (G[:2] * (0.5 if kind == "gelu" else 1.0)).to(dev()))      # f'(0) at x == +-0
    for g_off in (0, 1):
        for x_off in OFFSETS:
            Gv, xv = at_offset(G, g_off), at_offset(x, x_off)
            assert bits_equal(ops.alrp_act(Gv, xv, kind), want), (g_off, x_off)
            assert ops.alrp_act(Gv, xv, kind, out=Gv) is Gv and bits_equal(Gv, want), (g_off, x_off)


@pytest.mark.parametrize("C", [1, 64, 100, 768])
@pytest.mark.parametrize("rows", [1, 3, 197])
def test_row_rstd_and_layernorm_bf16_are_the_f32_entries_on_upcast_copies(rows, C):
    from transformer_explainability_amd import ops
    x = _operand((rows, C), rows + C, 2.0)
    gamma = (1.0 + 0.3 * rnd((C,), C + 5)).to(BF16)
    G = rnd((rows, C), rows + C + 6)
    xf, gf, Gd = x.to(dev()).float(), gamma.to(dev()).float(), G.to(dev())
    rstd = ops.alrp_row_rstd(xf, 1e-6)
    want = ops.alrp_layernorm(Gd, gf, rstd)
    assert torch.isfinite(rstd).all() and torch.isfinite(want).all()
    for eps in (0.0, 1e-6):                                    # (eps = 0 with C == 1: 1 / sqrt(0) = inf in both)
        want_rstd = ops.alrp_row_rstd(xf, eps)
        for off in OFFSETS:
            assert bits_equal(ops.alrp_row_rstd(at_offset(x, off), eps), want_rstd), (eps, off)
    for off in OFFSETS:
        for g_off in (0, 1):
            Gv = at_offset(G, g_off)
            assert bits_equal(ops.alrp_layernorm(Gv, at_offset(gamma, off), rstd), want), (off, g_off)
            assert ops.alrp_layernorm(Gv, at_offset(gamma, off), rstd, out=Gv) is Gv and bits_equal(Gv, want), (off, g_off)
    r = rows // 2                                              # a row alone, as a view into the batch
    xd = x.to(dev())
    assert bits_equal(ops.alrp_row_rstd(xd[r:r + 1], 1e-6), rstd[r:r + 1])


@pytest.mark.parametrize("B,N,C", [(1, 2, 1), (3, 17, 100), (2, 197, 768)])
@pytest.mark.parametrize("skip_first", [True, False])
def test_token_relevance_bf16_is_the_f32_entry_on_upcast_copies(B, N, C, skip_first):
    from transformer_explainability_amd import ops
    x0, G = _operand((B, N, C), B + N), rnd((B, N, C), B + N + C)
    want = ops.alrp_token_relevance(x0.to(dev()).float(), G.to(dev()), skip_first=skip_first)
    for off in OFFSETS:
        for g_off in (0, 2):
            got = ops.alrp_token_relevance(at_offset(x0, off), at_offset(G, g_off), skip_first=skip_first)
            assert got.shape == (B, N - int(skip_first)) and bits_equal(got, want), (off, g_off)
    xd, Gd = x0.to(dev()), G.to(dev())
    for b in range(B):                                         # a sample alone: a view into the batch
        assert bits_equal(ops.alrp_token_relevance(xd[b:b + 1], Gd[b:b + 1], skip_first=skip_first), want[b:b + 1]), b


# ------------------------------------------------------------------------------------------------ the Linear product
LINEAR_SHAPES = [(1, 128, 128), (51, 128, 384), (129, 256, 128), (130, 384, 512)]


def _linear_case(T, in_f, out_f, seed):
    G = (rnd((T, out_f), seed) * 2.0).to(dev())
    Y = _operand((T, out_f), seed + 1).to(dev())
    return G, Y


@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("T,in_f,out_f", LINEAR_SHAPES)
def test_linear_product_moves_bits_exactly(T, in_f, out_f, eps):
    """Column i of W holds one non-zero, +-2^j at row pi(i): out[t][i] = A[t][pi(i)] (+-2^j), exact in every step of the sum --
    the three planes of A[t][pi(i)] times the weight add up to it in fp32 without rounding (smallest first: p2, p2 + p1 = the
    residual of the first rounding, then the value itself), every other term is an exact zero.  A dropped plane, a wrong plane
    order, a wrong stride or a transposition error changes bits."""
    from transformer_explainability_amd import ops
    assert ops.alrp_linear_bf16_route(T, in_f, out_f) == "bf16"
    g = torch.Generator().manual_seed(T + in_f + out_f)
    pi = torch.randint(0, out_f, (in_f,), generator=g)
    pi[:min(in_f, out_f)] = torch.randperm(out_f, generator=g)[:min(in_f, out_f)]      # every row of W used where there is room
    w = torch.ldexp(torch.where(torch.rand(in_f, generator=g) < 0.5, -1.0, 1.0), torch.randint(-3, 4, (in_f,), generator=g))
    W = torch.zeros(out_f, in_f)
    W[pi, torch.arange(in_f)] = w
    G, Y = _linear_case(T, in_f, out_f, 5)
    A = G if eps == 0.0 else ops.alrp_damp(G, Y, eps)
    want = A[:, pi.to(dev())] * w.to(dev()) + 0.0             # (+ 0.0: a sum that starts at +0 never ends at -0)
    assert torch.isfinite(want).all()
    got = ops.alrp_linear(G, W.to(BF16).to(dev()), None, Y=Y, eps=eps)
    assert got.shape == (T, in_f) and got.dtype == torch.float32
    assert bits_equal(got, want)


@pytest.mark.parametrize("T,in_f,out_f", LINEAR_SHAPES)
def test_linear_product_within_the_first_order_bound(T, in_f, out_f):
    """Against the fp64 evaluation of damp and product on the exact operands, eps = 1e-6: A = fl(fl(G Y) / fl(Y + eps sgn Y))
    carries three roundings (3 u relative, first order); its planes and every plane x weight product are exact; an output is
    the fp32 sum of 3 out_f exact terms in one accumulator, of which the two lower planes of an element are below 2^-8 and
    2^-16 of it -- to first order at most out_f + 1 additions that matter, each off by u times a partial sum that
    sum_o |A||W| bounds:  |err| <= (3 + out_f + 1) u S, S = sum_o |A||W|; stated as (out_f + 8) u S, the rest room for the
    second-order terms."""
    from transformer_explainability_amd import ops
    eps = 1e-6
    G, Y = _linear_case(T, in_f, out_f, 7)
    Y = torch.where(Y == 0, torch.ones_like(Y), Y)             # order one: the specials are the exactness test's business
    Y = torch.where(Y.float().abs() < 1e-3, torch.ones_like(Y), Y)
    W = rnd((out_f, in_f), 9).to(BF16).to(dev())
    got = ops.alrp_linear(G, W, None, Y=Y, eps=eps)
    G64, Y64, W64 = G.double(), Y.double(), W.double()
    A64 = G64 * Y64 / (Y64 + eps * torch.where(Y64 >= 0, 1.0, -1.0))
    want = A64 @ W64
    bound = (out_f + 8) * U * (A64.abs() @ W64.abs())
    err = (got.double() - want).abs()
    worst = float((err / bound).max())
    # record, not assert: the fp32 chain's route on upcast copies (damp, then te_gemm_x6_f32 / the stock GEMM)
    up = ops.alrp_linear(ops.alrp_damp(G, Y.float(), eps), W.float())
    rms = lambda t: float(((t.double() - want) ** 2).mean().sqrt())      # noqa: E731
    _record(f"linear.{T}x{in_f}x{out_f}", worst_err_over_bound=worst, rms_err_bf16_route=rms(got), rms_err_fp32_upcast_route=rms(up),
            rms_ratio=rms(got) / rms(up))
    print(f"linear {T}x{in_f}x{out_f}: worst err / bound {worst:.3f}, rms {rms(got):.3e} (fp32 route on upcast copies {rms(up):.3e})")
    assert torch.isfinite(got).all() and bool((err <= bound).all()), worst


@pytest.mark.parametrize("T,in_f,out_f", LINEAR_SHAPES)
def test_linear_product_rows_are_independent_and_strided_operands_are_read_in_place(T, in_f, out_f):
    from transformer_explainability_amd import ops
    eps = 1e-6
    G, Y = _linear_case(T, in_f, out_f, 11)
    W = rnd((out_f, in_f), 13).to(BF16).to(dev())
    batch = ops.alrp_linear(G, W, None, Y=Y, eps=eps)
    # the two weight-side layouts (W in place / the cached W^T) run the same products in the same order
    cache = {}
    for flag in (False, True, True):                           # (the third call takes W^T from the cache)
        ops.ALRP_WEIGHT_T, was = flag, ops.ALRP_WEIGHT_T
        try:
            assert bits_equal(ops.alrp_linear(G, W, cache, Y=Y, eps=eps), batch), flag
        finally:
            ops.ALRP_WEIGHT_T = was
    assert bits_equal(cache["alrp_weight_t"][1], W.t().contiguous())
    for t in sorted({0, T // 2, T - 1}):
        assert bits_equal(ops.alrp_linear(G[t:t + 1], W, None, Y=Y[t:t + 1], eps=eps), batch[t:t + 1]), t
        assert bits_equal(ops.alrp_linear(G[t:t + 1].clone(), W, None, Y=Y[t:t + 1].clone(), eps=eps), batch[t:t + 1]), t
    # g_ld = out_f + 5 and y_ld = out_f + 3 (rows off every vector boundary), and row strides that keep the boundaries
    for pad_g, pad_y, lo_g, lo_y in ((5, 3, 1, 0), (4, 8, 4, 4)):
        Gw = torch.zeros((T, out_f + pad_g), device=dev())
        Yw = torch.zeros((T, out_f + pad_y), dtype=BF16, device=dev())
        Gs, Ys = Gw[:, lo_g:lo_g + out_f], Yw[:, lo_y:lo_y + out_f]
        Gs.copy_(G)
        Ys.copy_(Y)
        assert not Gs.is_contiguous() or T == 1
        assert bits_equal(ops.alrp_linear(Gs, W, None, Y=Ys, eps=eps), batch), (pad_g, pad_y)
    # 3-D leading dimensions keep their shape
    if T % 3 == 0:
        assert bits_equal(ops.alrp_linear(G.view(3, T // 3, out_f), W, None, Y=Y.view(3, T // 3, out_f), eps=eps),
                          batch.view(3, T // 3, in_f))


def test_linear_upcast_route_is_the_fp32_chain_on_exact_copies():
    """A shape te_attnlrp_linear_bf16 does not tile (the 10-class head; a 64-wide layer): the fp32 chain's own two calls on
    .float() copies, on the GPU."""
    from transformer_explainability_amd import ops
    for T, in_f, out_f in ((51, 128, 10), (17, 64, 192)):
        assert ops.alrp_linear_bf16_route(T, in_f, out_f) == "fp32-upcast"
        G, Y = _linear_case(T, in_f, out_f, 15)
        W = rnd((out_f, in_f), 17).to(BF16).to(dev())
        got = ops.alrp_linear(G, W, None, Y=Y, eps=1e-6)
        assert got.is_cuda and bits_equal(got, ops.alrp_linear(ops.alrp_damp(G, Y.float(), 1e-6), W.float()))


# ------------------------------------------------------------------------------------------------ the attention rule
ATT_SHAPES = [(1, 1, 1), (2, 2, 17), (1, 2, 64), (1, 2, 65), (1, 1, 197)]
D = 64


def _backward(go, q, k, v, p, scale):
    """the block's backward for d_out = go on [B,H,N,D] operands, then the uniform rule: the header's formula, the expression
    of rules.attention_attnlrp's torch branch, in the dtype of its arguments"""
    return cref.attention(go, q, k, v, p, scale)


def _attention_case(B, H, N, fused):
    C = H * D
    scale = D ** -0.5
    qkv = (rnd((B, N, 3 * C), B + H + N) * 1.5).to(BF16).to(dev())
    if fused:
        q, k, v = (qkv[..., i * C:(i + 1) * C] for i in range(3))
    else:
        q, k, v = (qkv[..., i * C:(i + 1) * C].contiguous() for i in range(3))
    heads = lambda t: t.reshape(B, N, H, D).permute(0, 2, 1, 3)      # noqa: E731
    attn = torch.softmax(torch.matmul(heads(q).float(), heads(k).float().transpose(-1, -2)) * scale, -1).to(BF16)
    G_o = rnd((B, N, C), B * H * N + 1).to(dev())
    return G_o, q, k, v, attn, scale, heads


def _run_attention(G_o, q, k, v, attn, H, scale, fused):
    from transformer_explainability_amd import ops, rules
    B, N, C = G_o.shape
    if fused:
        d = torch.full((B, N, 3 * C), float("nan"), device=dev())
        outs = tuple(d[..., i * C:(i + 1) * C] for i in range(3))
        rules.attention_attnlrp(G_o, q, k, v, attn, H, scale, *outs)
        ops.alrp_scale3(d)
    else:
        outs = tuple(torch.full((B, N, C), float("nan"), device=dev()) for _ in range(3))
        rules.attention_attnlrp(G_o, q, k, v, attn, H, scale, *outs)
        ops.alrp_scale3(*outs)
    return outs


@pytest.mark.parametrize("fused", [True, False], ids=["fused_qkv", "three_tensors"])
@pytest.mark.parametrize("B,H,N", ATT_SHAPES)
def test_attention_rule_within_twice_the_fp32_expression(B, H, N, fused):
    from transformer_explainability_amd import ops
    assert ops.alrp_attention_bf16_route(N, D) == "bf16"
    G_o, q, k, v, attn, scale, heads = _attention_case(B, H, N, fused)
    got = _run_attention(G_o, q, k, v, attn, H, scale, fused)
    cat = lambda ts: torch.cat([t.reshape(B, -1) for t in ts], 1)      # noqa: E731
    merge = lambda t: t.permute(0, 2, 1, 3).reshape(B, N, H * D)      # noqa: E731
    want = [merge(t) for t in _backward(heads(G_o).double(), heads(q).double(), heads(k).double(), heads(v).double(),
                                        attn.double(), scale)]
    ref32 = [merge(t) for t in _backward(heads(G_o), heads(q).float(), heads(k).float(), heads(v).float(), attn.float(), scale)]
    assert all(torch.isfinite(t).all() for t in got)
    e_kernel, e_ref = _rel_l2(cat(got), cat(want)), _rel_l2(cat(ref32), cat(want))
    _record(f"attention.B{B}H{H}N{N}.{'fused' if fused else 'separate'}", kernel_rel_l2=e_kernel.tolist(),
            fp32_expression_rel_l2=e_ref.tolist(), ratio=_ratio(e_kernel, e_ref))
    print(f"attention B{B} H{H} N{N} fused={fused}: kernel {e_kernel.tolist()} fp32 expression {e_ref.tolist()}")
    assert bool((e_kernel <= 2.0 * e_ref).all()), (e_kernel.tolist(), e_ref.tolist())
    if N == 1:                                                 # a lone token: p = 1, d_s = 0
        assert bits_equal(got[2], G_o * 0.5) and not got[0].any() and not got[1].any()


@pytest.mark.parametrize("B,H,N", [(2, 2, 17), (1, 2, 65)])
def test_attention_rule_a_head_alone_equals_the_head_in_the_batch(B, H, N):
    G_o, q, k, v, attn, scale, heads = _attention_case(B, H, N, True)
    batch = _run_attention(G_o, q, k, v, attn, H, scale, True)
    for b in range(B):
        for h in range(H):
            one = lambda t: t[b:b + 1, :, h * D:(h + 1) * D]      # noqa: E731
            alone = _run_attention(one(G_o).contiguous(), one(q), one(k), one(v), attn[b:b + 1, h:h + 1], 1, scale, False)
            for a, full in zip(alone, batch):
                assert bits_equal(a, one(full).contiguous()), (b, h)


def test_attention_upcast_route_is_the_fp32_rule_on_exact_copies():
    """head dim 48: te_attnlrp_attention_bf16 does not take the shape; the fp32 routes of rules.attention_attnlrp on .float()
    copies, on the GPU."""
    from transformer_explainability_amd import ops, rules
    B, H, N, Dh = 2, 2, 17, 48
    assert ops.alrp_attention_bf16_route(N, Dh) == "fp32-upcast"
    C = H * Dh
    q, k, v = ((rnd((B, N, C), 20 + i)).to(BF16).to(dev()) for i in range(3))
    attn = torch.softmax(rnd((B, H, N, N), 23), -1).to(BF16).to(dev())
    G_o = rnd((B, N, C), 24).to(dev())
    got = tuple(torch.empty((B, N, C), device=dev()) for _ in range(3))
    want = tuple(torch.empty((B, N, C), device=dev()) for _ in range(3))
    rules.attention_attnlrp(G_o, q, k, v, attn, H, Dh ** -0.5, *got)
    rules.attention_attnlrp(G_o, q.float(), k.float(), v.float(), attn.float(), H, Dh ** -0.5, *want)
    assert all(g.is_cuda and bits_equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ models
def _assert_within_twice(tag, got, R32, R64):
    e_chain, e_ref = _rel_l2(got, R64), _rel_l2(R32, R64)
    _record(tag, kernel_chain_rel_l2=e_chain.tolist(), fp32_restatement_rel_l2=e_ref.tolist(), ratio=_ratio(e_chain, e_ref))
    print(f"{tag}: chain {e_chain.tolist()} fp32 restatement {e_ref.tolist()}")
    assert torch.isfinite(got).all() and got.dtype == torch.float32
    assert bool((e_chain <= 2.0 * e_ref).all()), (tag, e_chain.tolist(), e_ref.tolist())


def _vit_cases(tag, model, x):
    """generate_attnlrp for the argmax class, a given index and eps = 0 against the restatement on the caches each call left"""
    from transformer_explainability_amd.generators import LRP
    lrp = LRP(model)
    for name, index, eps in (("argmax", None, 1e-6), ("index", torch.tensor([1, 7, 4]), 1e-6), ("eps0", torch.tensor([1, 7, 4]), 0.0)):
        got = lrp.generate_attnlrp(x, index=index, eps=eps)
        assert got.shape == (3, 16)
        idx = model.head.Y.detach().argmax(-1) if index is None else index.to(dev())
        seed, _ = cref.one_hot(model.head.Y, idx)
        _assert_within_twice(f"{tag}.{name}", got, cref.vit_chain(model, seed, eps, torch.float32),
                             cref.vit_chain(model, seed, eps, torch.float64))
    torch.cuda.synchronize()
    lrp.check()


@pytest.fixture(scope="module")
def vit128():
    """dim 128, 2 heads (D = 64), bf16: every Linear product but the head's on te_attnlrp_linear_bf16, the attention rule on
    te_attnlrp_attention_bf16, the 10-class head on the upcast route."""
    model = _tiny_vit(128, 3)[0].to(BF16)
    return model, rnd((3, 3, 32, 32), 31).to(dev()).to(BF16)


def test_vit_tiny_bf16_against_the_same_cache_restatement(vit128):
    from transformer_explainability_amd import ops
    model, x = vit128
    assert all(p.dtype == BF16 for p in model.parameters())
    assert ops.alrp_linear_bf16_route(51, 128, 384) == "bf16" and ops.alrp_linear_bf16_route(51, 512, 128) == "bf16"
    assert ops.alrp_linear_bf16_route(3, 128, 10) == "fp32-upcast" and ops.alrp_attention_bf16_route(17, 64) == "bf16"
    _vit_cases("vit_tiny_dim128_bf16", model, x)


def test_vit_tiny_bf16_head_dim_48_every_product_on_the_upcast_route():
    from transformer_explainability_amd import ops
    model = _tiny_vit(96, 4)[0].to(BF16)
    assert ops.alrp_attention_bf16_route(17, 48) == "fp32-upcast"
    assert not any(ops.alrp_linear_bf16_route(51, i, o) == "bf16" for i, o in ((96, 288), (96, 96), (96, 384), (384, 96), (96, 10)))
    _vit_cases("vit_tiny_dim96_bf16", model, rnd((3, 3, 32, 32), 41).to(dev()).to(BF16))


def test_bert_tiny_bf16_against_the_same_cache_restatement():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import Generator, _one_hot
    model = _tiny_bert()[0].to(BF16)
    ids, mask = _bert_inputs()
    gen = Generator(model)
    for name, index, eps in (("argmax", None, 1e-6), ("index", torch.tensor([1, 1, 0]), 1e-6), ("eps0", torch.tensor([1, 1, 0]), 0.0)):
        got = gen.generate_attnlrp(ids, mask, index=index, eps=eps)
        assert got.shape == (3, 12)
        idx = model.classifier.Y.detach().argmax(-1) if index is None else index.to(dev())
        seed, _ = cref.one_hot(model.classifier.Y, idx)
        _assert_within_twice(f"bert_tiny_bf16.{name}", got, cref.bert_chain(model, seed, eps, torch.float32),
                             cref.bert_chain(model, seed, eps, torch.float64))
    torch.cuda.synchronize()
    gen.check()
    # the mask in the dtypes generate_LRP takes it in
    assert bits_equal(gen.generate_attnlrp(ids, mask.to(BF16), index=index, eps=0.0), got)
    # batch = samples on the same caches, and the chain does not read the producer flag
    with torch.no_grad():
        seed = _one_hot(model(input_ids=ids, attention_mask=mask)[0], torch.tensor([1, 1, 0]))
        batch = model.attnlrp(seed)
        for i in range(3):
            with sliced_relprop_state(model, i, 3):
                assert bits_equal(model.attnlrp(seed[i:i + 1]), batch[i:i + 1]), i
        ops.USE_FUSED_PRODUCERS = True
        try:
            assert bits_equal(model.attnlrp(seed), batch)
        finally:
            ops.USE_FUSED_PRODUCERS = False


def test_bf16_chain_gives_the_same_bits_whatever_the_producer_flag_says(vit128):
    """On the SAME caches: one forward pass (under either setting of the flag) fills them, then the chain runs with
    ops.USE_FUSED_PRODUCERS off and on."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP, _one_hot
    model, x = vit128
    assert not ops.USE_FUSED_PRODUCERS
    try:
        for forward_flag in (False, True):
            ops.USE_FUSED_PRODUCERS = forward_flag
            with torch.no_grad():
                seed = _one_hot(model(x), None)
                maps = []
                for chain_flag in (False, True):
                    ops.USE_FUSED_PRODUCERS = chain_flag
                    maps.append(model.attnlrp(seed, eps=1e-6))
            assert bits_equal(maps[0], maps[1]), forward_flag
            _assert_within_twice(f"vit_tiny_dim128_bf16.forward_producers_{'on' if forward_flag else 'off'}", maps[0],
                                 cref.vit_chain(model, seed, 1e-6, torch.float32), cref.vit_chain(model, seed, 1e-6, torch.float64))
        ops.USE_FUSED_PRODUCERS = True
        lrp = LRP(model)
        got = lrp.generate_attnlrp(x)                          # the public call under the flag
        assert bits_equal(got, maps[0])
        torch.cuda.synchronize()
        lrp.check()
    finally:
        ops.USE_FUSED_PRODUCERS = False


def test_bf16_eager_and_graph_replay_give_the_same_bits(vit128):
    from transformer_explainability_amd.generators import LRP, GraphedCall
    model, x = vit128
    lrp = LRP(model)
    eager = lrp.generate_attnlrp(x).clone()
    graphed = GraphedCall(lambda inp: lrp._attnlrp(inp), (x,))
    assert bits_equal(graphed(x).clone(), eager)
    x2 = rnd((3, 3, 32, 32), 77).to(dev()).to(BF16)
    assert bits_equal(graphed(x2).clone(), lrp.generate_attnlrp(x2))
    assert bits_equal(graphed(x).clone(), eager)
    public = GraphedCall(lambda inp: lrp.generate_attnlrp(inp), (x,))
    assert bits_equal(public(x).clone(), eager)
    torch.cuda.synchronize()
    lrp.check()


def test_bf16_batch_equals_its_samples(vit128):
    """On the same caches (gpu_util.sliced_relprop_state): the kernels work per row, per token or per (b, h), the bf16 products
    do not depend on the number of rows, and the head's upcast product multiplies a one-hot row."""
    from transformer_explainability_amd.generators import _one_hot
    model, x = vit128
    with torch.no_grad():
        seed = _one_hot(model(x), None)
        batch = model.attnlrp(seed)
        for i in range(3):
            with sliced_relprop_state(model, i, 3):
                one = model.attnlrp(seed[i:i + 1])
            assert bits_equal(one, batch[i:i + 1]), i


def test_bf16_refusals_on_the_device(vit128):
    """A bf16 model with fp32 images (and the reverse) on the GPU is refused with both dtypes named; fp16 stays refused."""
    from transformer_explainability_amd import TeError
    from transformer_explainability_amd.generators import LRP
    model, x = vit128
    both = r"(?s)(torch\.bfloat16.*torch\.float32|torch\.float32.*torch\.bfloat16)"
    with pytest.raises(TeError, match=both):
        LRP(model).generate_attnlrp(x.float())
    with pytest.raises(TeError, match=r"torch\.float16"):
        LRP(model).generate_attnlrp(x.half())
    with pytest.raises(TeError, match=r"torch\.bfloat16.*GPU"):
        LRP(model).generate_attnlrp(x.cpu())
    assert math.isfinite(float(LRP(model).generate_attnlrp(x).sum()))
