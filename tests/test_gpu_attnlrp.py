"""AttnLRP on the MI355X (csrc/te_attnlrp.hip, the attnlrp chains of vit.py / bert.py, generate_attnlrp).

Kernels: damp, the identity rule (GELU) and scale3 against their torch expression on the device, bit for bit, aligned and
misaligned; the LayerNorm rule, its row statistics, the token sums and the tanh identity rule against fp64 with a-priori
bounds derived below from C and the row's sum of |terms| (u = 2^-24); a row alone equals the same row in a batch.

Models: the yardstick is the torch restatement (tests/attnlrp_ref.py) in fp64 on .double() copies; the error that counts
is the per-sample relative L2 error of the fp32 restatement (torch autograd, same device) against it, and the kernel chain
must stay within 2 x that on every sample (two fp32 evaluations of one formula in different summation orders).  Both
errors go to attnlrp_parity.json next to the parity report (gpu_util.REPORT; committed as profiles/attnlrp_parity.json).  The chain gives the same bits
whatever ops.USE_FUSED_PRODUCERS says, eager and under GraphedCall replay, and for a batch and its samples.

Every test calls generate_attnlrp, model.attnlrp or an ops.alrp_* binding: none exists without the feature."""
import copy
import json
import os

import pytest
import torch

import attnlrp_ref as ref
from gpu_util import REPORT, dev, rnd, sliced_relprop_state

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PARITY = os.path.join(os.path.dirname(REPORT), "attnlrp_parity.json")
_parity = {}


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def offset_view(t, off=1):
    """a contiguous copy of t whose storage starts `off` elements behind a 16-byte boundary"""
    base = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    assert base.data_ptr() % 16 == 0
    view = base[off:].view(t.shape)
    view.copy_(t)
    return view


SPECIAL_Y = [0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0, 1e-6, -1e-6]


# ------------------------------------------------------------------------------------------------ damp
@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_damp_is_its_torch_expression_bit_for_bit(n, eps):
    from transformer_explainability_amd import ops
    Y = rnd((n,), n + 1)
    Y[:min(n, len(SPECIAL_Y))] = torch.tensor(SPECIAL_Y[:n])
    if n > 8:
        Y[8:16] = torch.tensor(SPECIAL_Y)[torch.randperm(8, generator=torch.Generator().manual_seed(n))]
    G, Y = (rnd((n,), n + 2) * 4.0).to(dev()), Y.to(dev())
    if eps == 0.0:
        want = G.clone()                                       # eps = 0: the identity, also where Y == 0
    else:
        want = G * Y / (Y + torch.where(Y >= 0, eps, -eps))    # sgn(+-0) = +1; every op rounded on its own, in fp32
    assert want.dtype == torch.float32 and torch.isfinite(want).all()
    got = ops.alrp_damp(G, Y, eps)
    assert bits_equal(got, want)
    # misaligned views (storage offset 1): all three in one phase (vectors from the first boundary), then mixed phases
    Gv, Yv = offset_view(G), offset_view(Y)
    assert Gv.data_ptr() % 16 == 4
    assert bits_equal(ops.alrp_damp(Gv, Yv, eps, out=offset_view(torch.zeros_like(G))), want)
    assert bits_equal(ops.alrp_damp(Gv, Y, eps), want) and bits_equal(ops.alrp_damp(G, offset_view(Y, 3), eps), want)
    # in place
    Gi = G.clone()
    assert ops.alrp_damp(Gi, Y, eps, out=Gi) is Gi and bits_equal(Gi, want)


# ------------------------------------------------------------------------------------------------ identity rule
def _act_inputs(n):
    x = rnd((n,), n + 3) * 3.0
    special = [0.0, -0.0, 1e-20, -1e-20, 20.0, -20.0]
    x[:min(n, 6)] = torch.tensor(special[:n])
    return (rnd((n,), n + 4) * 2.0).to(dev()), x.to(dev())


@pytest.mark.parametrize("n", [1, 6, 7, 1027])
def test_gelu_identity_rule_is_its_torch_expression_bit_for_bit(n):
    """G (gelu(x) / x) with gelu = the package's own kernel (ops.gelu_forward), the factor 0.5 at x == +-0."""
    from transformer_explainability_amd import ops
    G, x = _act_inputs(n)
    pad = torch.zeros((n + 3) // 4 * 4, dtype=torch.float32, device=dev())      # (gelu_forward takes multiples of 4)
    pad[:n] = x
    f = ops.gelu_forward(pad)[:n]
    ratio = torch.where(x == 0, torch.full_like(x, 0.5), f / torch.where(x == 0, torch.ones_like(x), x))
    want = ratio * G
    assert torch.isfinite(want).all()
    got = ops.alrp_act(G, x, "gelu")
    assert bits_equal(got, want)
    if n >= 2:
        assert bits_equal(got[:2], G[:2] * 0.5)
    assert bits_equal(ops.alrp_act(offset_view(G), offset_view(x), "gelu", out=offset_view(torch.zeros_like(G))), want)
    assert bits_equal(ops.alrp_act(offset_view(G), x, "gelu"), want)
    Gi = G.clone()
    assert ops.alrp_act(Gi, x, "gelu", out=Gi) is Gi and bits_equal(Gi, want)


@pytest.mark.parametrize("n", [6, 1027])
def test_tanh_identity_rule_within_the_rounding_bound(n):
    """out = fl(G fl(tanhf(x) / x)): tanhf within 5 ulp (the OpenCL bound the device library conforms to), one division and
    one multiply of half an ulp each -> |out - fp64| <= 6 * 2^-23 |fp64|; exactly G at x == +-0."""
    from transformer_explainability_amd import ops
    G, x = _act_inputs(n)
    got = ops.alrp_act(G, x, "tanh")
    x64, G64 = x.double(), G.double()
    want = torch.where(x64 == 0, G64, G64 * torch.tanh(x64) / torch.where(x64 == 0, torch.ones_like(x64), x64))
    assert bits_equal(got[:2], G[:2])
    err = (got.double() - want).abs()
    assert bool((err <= 6 * 2.0 ** -23 * want.abs() * 1.001).all()), float((err / want.abs().clamp(min=1e-300)).max())
    assert bits_equal(ops.alrp_act(offset_view(G), x, "tanh"), got)


# ------------------------------------------------------------------------------------------------ scale3
@pytest.mark.parametrize("T,C", [(1, 1), (3, 5), (17, 128), (5, 96)])
def test_scale3_is_exact(T, C):
    from transformer_explainability_amd import ops
    g = rnd((2, T, 3 * C), T + C).to(dev())
    want = g.clone()
    want[..., :2 * C] *= 0.25
    want[..., 2 * C:] *= 0.5
    for make in (torch.clone, offset_view):
        fused = make(g)
        assert ops.alrp_scale3(fused) is fused and bits_equal(fused, want)
        q, k, v = (make(g[..., i * C:(i + 1) * C].contiguous()) for i in range(3))
        ops.alrp_scale3(q, k, v)
        assert bits_equal(torch.cat((q, k, v), -1), want)


# ------------------------------------------------------------------------------------------------ LayerNorm rule
def _ln_case(rows, C):
    G = rnd((rows, C), rows + C)
    G[0, 0] = 0.0
    gamma = 1.0 + 0.3 * rnd((C,), C + 5)
    x = rnd((rows, C), rows + C + 6) * 2.0 + 0.5
    return G.to(dev()), gamma.to(dev()), x.to(dev())


@pytest.mark.parametrize("C", [1, 64, 100, 768])
@pytest.mark.parametrize("rows", [1, 3, 197])
def test_layernorm_rule_and_row_rstd_within_the_rounding_bound(rows, C):
    """out_i = fl(rstd fl(t_i - m)), t_i = fl(gamma_i G_i), m = fl(fl-sum(t) / C).  With S = sum_j |gamma_j G_j|: the sum of C
    rounded terms is off by at most C u S in any order, so |m - mean| <= u S (1 + 1/C); the subtraction adds u (|t_i| + |m|) and
    the rounding of t_i u |t_i|, the last multiply u |out|:
        |out_i - fp64| <= |rstd| u (3 |gamma_i G_i| + S (1 + 3 / C))          (times 1.01 for the second-order terms).
    rstd = fl(1 / fl(sqrt(fl(v + eps)))), v = fl(fl-sum(fl(d_j^2)) / C), d_j = fl(x_j - m'), m' the mean as above, off by
    delta <= u (sum|x| + |mean|): sum (x_j - m')^2 / C = var + delta^2, every term non-negative, so v is relatively off by
    (C + 3) u, the addition, the root and the division by u each (the root halves what it is given):
        |rstd - fp64| <= rstd ((C / 2 + 4) u 1.01 + delta^2 / (2 (var + eps))).
    A row alone -- as a view into the batch, whatever its alignment, and as a copy -- equals the same row in the batch."""
    from transformer_explainability_amd import ops
    G, gamma, x = _ln_case(rows, C)
    eps = 2.0 ** -20                                           # (a float32 number: the kernel and the fp64 side add the same eps)
    rstd = ops.alrp_row_rstd(x, eps)
    assert rstd.shape == (rows,)
    x64 = x.double()
    var = x64.var(-1, unbiased=False)
    want = 1.0 / torch.sqrt(var + eps)
    delta = U * (x64.abs().sum(-1) + x64.mean(-1).abs())
    bound = want * ((C / 2 + 4) * U * 1.01 + delta ** 2 / (2 * (var + eps)))
    assert bool(((rstd.double() - want).abs() <= bound).all()), float(((rstd.double() - want).abs() / bound).max())

    got = ops.alrp_layernorm(G, gamma, rstd)
    t = gamma.double() * G.double()
    ref64 = rstd.double().unsqueeze(-1) * (t - t.mean(-1, keepdim=True))
    S = t.abs().sum(-1, keepdim=True)
    bound = rstd.double().unsqueeze(-1).abs() * U * (3 * t.abs() + S * (1 + 3 / C)) * 1.01
    err = (got.double() - ref64).abs()
    assert torch.isfinite(got).all() and bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    if C == 1:
        assert not got.any()                                   # t - mean(t) is exactly zero
    for r in sorted({0, rows // 2, rows - 1}):
        for row in (lambda a: a[r:r + 1], lambda a: a[r:r + 1].clone()):
            assert bits_equal(ops.alrp_row_rstd(row(x), eps), rstd[r:r + 1]), r
            assert bits_equal(ops.alrp_layernorm(row(G), gamma, rstd[r:r + 1]), got[r:r + 1]), r
    assert bits_equal(ops.alrp_layernorm(offset_view(G), gamma, rstd), got)
    Gi = G.clone()
    assert ops.alrp_layernorm(Gi, gamma, rstd, out=Gi) is Gi and bits_equal(Gi, got)


# ------------------------------------------------------------------------------------------------ token relevance
@pytest.mark.parametrize("B,N,C", [(1, 2, 1), (3, 17, 128), (2, 197, 768)])
@pytest.mark.parametrize("skip_first", [True, False])
def test_token_relevance_within_the_rounding_bound(B, N, C, skip_first):
    """The products are exact in fp64 and C of them are added in fp64, here and in the torch sum this is compared with: each
    is within C 2^-53 S of the exact sum, S = sum_c |x0 G|; the result is rounded to fp32 once:
        |out - fp64| <= 2 C 2^-53 S + 2^-24 |fp64|          (+ the smallest subnormal)."""
    from transformer_explainability_amd import ops
    x0, G = rnd((B, N, C), B + N).to(dev()), rnd((B, N, C), B + N + C).to(dev())
    x0[0, N - 1] = 0.0
    got = ops.alrp_token_relevance(x0, G, skip_first=skip_first)
    first = int(skip_first)
    assert got.shape == (B, N - first) and got.dtype == torch.float32
    terms = (x0.double() * G.double())[:, first:]
    want, S = terms.sum(-1), terms.abs().sum(-1)
    bound = 2 * C * 2.0 ** -53 * S + U * want.abs() * 1.001 + 2.0 ** -149
    err = (got.double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert not got[0, N - 1 - first].any()
    for b in range(B):                                         # a sample alone: a view into the batch, and an offset copy
        assert bits_equal(ops.alrp_token_relevance(x0[b:b + 1], G[b:b + 1], skip_first=skip_first), got[b:b + 1]), b
    assert bits_equal(ops.alrp_token_relevance(offset_view(x0), offset_view(G, 2), skip_first=skip_first), got)


# ------------------------------------------------------------------------------------------------ models
def _record(tag, **kw):
    _parity[tag] = kw
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        json.dump(_parity, f, indent=1, sort_keys=True)


def _rel_l2(got, want):
    """per-sample ||got - want|| / ||want|| in fp64"""
    got, want = got.detach().double().flatten(1), want.detach().double().flatten(1)
    return (got - want).norm(dim=1) / want.norm(dim=1)


def _tiny_vit(dim, seed):
    from transformer_explainability_amd import vit
    torch.manual_seed(seed)
    model = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=dim, depth=2, num_heads=2, num_classes=10,
                                  qkv_bias=True).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    model.to(dev())
    return model, copy.deepcopy(model), copy.deepcopy(model).double()


def _tiny_bert(seed=11):
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                              intermediate_size=256, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(seed)
    model = bert.BertForSequenceClassification(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    model.to(dev())
    return model, copy.deepcopy(model), copy.deepcopy(model).double()


@pytest.fixture(scope="module")
def vit128():
    """dim 128, 2 heads (D = 64): the attention rule on te_attention_backward_strided_f32, every Linear product but the head's
    on te_gemm_x6_f32.  -> (model, x, the class per sample, the fp64 yardstick, the fp32 restatement), for the argmax class."""
    model, m32, m64 = _tiny_vit(128, 3)
    x = rnd((3, 3, 32, 32), 31).to(dev())
    with torch.no_grad():
        index = model(x).argmax(-1)
    R64, _ = ref.vit_attnlrp(m64, x.double(), index=index)
    R32, _ = ref.vit_attnlrp(m32, x, index=index)
    return model, x, index, R64, R32, (m32, m64)


def _assert_within_twice(tag, got, R32, R64):
    e_chain, e_ref = _rel_l2(got, R64), _rel_l2(R32, R64)
    _record(tag, kernel_chain_rel_l2=e_chain.tolist(), fp32_restatement_rel_l2=e_ref.tolist(),
            ratio=(e_chain / e_ref).tolist())
    assert torch.isfinite(got).all() and got.dtype == torch.float32
    assert bool((e_chain <= 2.0 * e_ref).all()), (tag, e_chain.tolist(), e_ref.tolist())


def test_vit_tiny_against_the_restatement(vit128):
    from transformer_explainability_amd.generators import LRP
    model, x, index, R64, R32, (m32, m64) = vit128
    lrp = LRP(model)
    got = lrp.generate_attnlrp(x)                              # index=None: the device argmax
    torch.cuda.synchronize()
    lrp.check()
    assert got.shape == (3, 16)
    _assert_within_twice("vit_tiny_dim128.argmax", got, R32, R64)
    idx = torch.tensor([1, 7, 4])
    got = lrp.generate_attnlrp(x, index=idx)
    _assert_within_twice("vit_tiny_dim128.index", got, ref.vit_attnlrp(m32, x, index=idx)[0],
                         ref.vit_attnlrp(m64, x.double(), index=idx)[0])
    # eps = 0 is allowed: damp is the identity
    got0 = lrp.generate_attnlrp(x, index=idx, eps=0.0)
    _assert_within_twice("vit_tiny_dim128.eps0", got0, ref.vit_attnlrp(m32, x, index=idx, eps=0.0)[0],
                         ref.vit_attnlrp(m64, x.double(), index=idx, eps=0.0)[0])


def test_vit_tiny_head_dim_48_torch_attention_and_stock_products():
    """dim 96, 2 heads (D = 48): no attention producer takes the shape (the torch expression of the same backward) and
    te_gemm_x6_f32 takes none of the Linear shapes (the stock GEMM)."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model, m32, m64 = _tiny_vit(96, 4)
    assert not ops._lib.load().te_attention_strided_supported(17, 48)
    assert not any(ops.gemm_x6_supported(51, k, m) for k, m in ((288, 96), (96, 96), (384, 96), (96, 384)))
    x = rnd((3, 3, 32, 32), 41).to(dev())
    got = LRP(model).generate_attnlrp(x)
    index = model.head.Y.detach().argmax(-1)
    assert got.shape == (3, 16)
    _assert_within_twice("vit_tiny_dim96.argmax", got, ref.vit_attnlrp(m32, x, index=index)[0],
                         ref.vit_attnlrp(m64, x.double(), index=index)[0])


def _bert_inputs():
    B, N = 3, 12
    ids = torch.randint(1, 100, (B, N), generator=torch.Generator().manual_seed(12)).to(dev())
    mask = torch.ones(B, N)
    mask[1, 8:] = 0.0                                          # a padded sample
    return ids, mask.to(dev())


def test_bert_tiny_against_the_restatement():
    from transformer_explainability_amd.generators import Generator
    model, m32, m64 = _tiny_bert()
    ids, mask = _bert_inputs()
    gen = Generator(model)
    got = gen.generate_attnlrp(ids, mask)
    torch.cuda.synchronize()
    gen.check()
    index = model.classifier.Y.detach().argmax(-1)
    assert got.shape == (3, 12)
    _assert_within_twice("bert_tiny.argmax", got, ref.bert_attnlrp(m32, ids, mask, index=index)[0],
                         ref.bert_attnlrp(m64, ids, mask.double(), index=index)[0])
    idx = torch.tensor([1, 1, 0])
    _assert_within_twice("bert_tiny.index", gen.generate_attnlrp(ids, mask, index=idx),
                         ref.bert_attnlrp(m32, ids, mask, index=idx)[0], ref.bert_attnlrp(m64, ids, mask.double(), index=idx)[0])
    # batch = samples on the same caches, and the chain does not read the producer flag
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import _one_hot
    with torch.no_grad():
        seed = _one_hot(model(input_ids=ids, attention_mask=mask)[0], idx)
        batch = model.attnlrp(seed)
        for i in range(3):
            with sliced_relprop_state(model, i, 3):
                assert bits_equal(model.attnlrp(seed[i:i + 1]), batch[i:i + 1]), i
        ops.USE_FUSED_PRODUCERS = True
        try:
            assert bits_equal(model.attnlrp(seed), batch)
        finally:
            ops.USE_FUSED_PRODUCERS = False


def test_chain_gives_the_same_bits_whatever_the_producer_flag_says(vit128):
    """The caches compared are the SAME tensors: one forward pass fills them (qkv.Y with its q / k / v thirds, the attention
    probabilities, the inputs of the LayerNorms and activations, the outputs of the Linears and Adds), then the chain runs on
    them once with ops.USE_FUSED_PRODUCERS off and once with it on -- for a forward pass made under either setting.  (Two
    forward passes under different settings fill the caches with tensors that differ in rounding: those maps agree to
    rounding, not in bits, and are not compared here.)"""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP, _one_hot
    model, x, index, R64, R32, _ = vit128
    assert not ops.USE_FUSED_PRODUCERS
    try:
        for forward_flag in (False, True):
            ops.USE_FUSED_PRODUCERS = forward_flag
            with torch.no_grad():
                seed = _one_hot(model(x), index)
                maps = []
                for chain_flag in (False, True):
                    ops.USE_FUSED_PRODUCERS = chain_flag
                    maps.append(model.attnlrp(seed, eps=1e-6))
            assert bits_equal(maps[0], maps[1]), forward_flag
            _assert_within_twice(f"vit_tiny_dim128.forward_producers_{'on' if forward_flag else 'off'}", maps[0], R32, R64)
        # the public call under the flag: the forward pass is whatever the flag says, the refusals and the result shape hold
        ops.USE_FUSED_PRODUCERS = True
        got = LRP(model).generate_attnlrp(x, index=index)
        assert bits_equal(got, maps[0])
    finally:
        ops.USE_FUSED_PRODUCERS = False


def test_eager_and_graph_replay_give_the_same_bits(vit128):
    from transformer_explainability_amd.generators import LRP, GraphedCall
    model, x, index, _, _, _ = vit128
    lrp = LRP(model)
    eager = lrp.generate_attnlrp(x).clone()
    graphed = GraphedCall(lambda inp: lrp._attnlrp(inp), (x,))
    assert bits_equal(graphed(x).clone(), eager)
    x2 = rnd((3, 3, 32, 32), 77).to(dev())
    assert bits_equal(graphed(x2).clone(), lrp.generate_attnlrp(x2))
    assert bits_equal(graphed(x).clone(), eager)
    # the public call itself is capturable too (its x6 poll / post step aside during capture)
    public = GraphedCall(lambda inp: lrp.generate_attnlrp(inp), (x,))
    assert bits_equal(public(x).clone(), eager)
    torch.cuda.synchronize()
    lrp.check()


def test_batch_equals_its_samples(vit128):
    """On the same caches (gpu_util.sliced_relprop_state, the existing model tests' way): the kernels work per row, per
    token or per (b, h), te_gemm_x6_f32 does not depend on the number of rows, and the one stock product (the head's, 10
    classes) multiplies a one-hot row, whose sum has a single non-zero term."""
    from transformer_explainability_amd.generators import _one_hot
    model, x, index, _, _, _ = vit128
    with torch.no_grad():
        seed = _one_hot(model(x), index)
        batch = model.attnlrp(seed)
        for i in range(3):
            with sliced_relprop_state(model, i, 3):
                one = model.attnlrp(seed[i:i + 1])
            assert torch.equal(one, batch[i:i + 1]), i
