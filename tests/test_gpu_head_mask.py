"""head_mask on the MI355X: the Mul rule kernel bit for bit, the per-head relevance kernel, and tiny BERT / ViT models with
masked heads against the CPU restatement of the reference's relprop with the Mul rule (tests/head_mask_ref.py) on the same cache.

On a tree without the feature every test here fails: NotImplementedError from BertSelfAttention.forward, AttributeError for
ops.mul_head_relprop / ops.head_relevance / generate_head_relevance, TypeError for VisionTransformer.forward(head_mask=)."""
import copy

import pytest
import torch

import head_mask_ref as HR
from f64_util import bert_cache_f64, bits_equal, cpu64, norm_err, vit_cache_f64
from gpu_util import (bert_cache_from_model, check, dev, map_stats, record, sliced_relprop_state, vit_cache_from_model)
from host_util import one_hot

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
MASK_VALUES = (1.0, 0.0, 0.5, -2.0)
cpu32 = lambda t: t.detach().float().cpu()      # noqa: E731  (oracle.model_cache's own conversion)


def _same(a, b):
    """bit for bit, NaN positions included (attn_gradcam's 0 / 0 rows)."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)))


# ------------------------------------------------------------------------------------------------ 1. the rule kernel
RULE_SHAPES = [(1, 2, 1, 1), (2, 3, 5, 5), (1, 2, 1, 9), (3, 4, 67, 67), (1, 12, 197, 197), (1100, 64, 1, 1)]


def _rule_case(B, H, rows, cols, dtype, seed):
    """P: a softmax with some key columns forced to exact zero by a -10000 mask; R about 1e-3 randn (CPU tensors)."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, H, rows, cols, generator=g, dtype=dtype)
    key_mask = torch.zeros(cols, dtype=dtype)
    if cols > 1:
        key_mask[cols // 3::4] = -10000.0
        key_mask[0] = 0.0
    P = torch.softmax(logits + key_mask, dim=-1)
    R = 1e-3 * torch.randn(B, H, rows, cols, generator=g, dtype=dtype)
    if cols > 1:
        assert (P == 0).any() and (P != 0).any()
    return R, P


def _mask(B, H, kind, dtype):
    vals = torch.tensor(MASK_VALUES, dtype=dtype)
    if kind == "shared":
        return vals[torch.arange(H) % 4].view(1, H, 1, 1)
    return vals[(torch.arange(B).view(B, 1) + torch.arange(H).view(1, H)) % 4].view(B, H, 1, 1)      # "per_sample"


def _assert_no_subnormal_intermediate(R, P, m):
    """Host and device may differ only by flushing subnormals: the CPU evaluation must meet none (zeros are fine)."""
    from oracle.relprop_oracle import safe_divide
    tiny = torch.finfo(R.dtype).tiny
    Z = P * m
    S = safe_divide(R, Z)
    eps = torch.tensor(1e-9, dtype=R.dtype)
    den = Z + eps
    steps = {"Z": Z, "den": den, "quotient": R / torch.where(den == 0, eps, den), "S": S, "S m": S * m, "out": P * (S * m)}
    for name, t in steps.items():
        assert torch.isfinite(t).all(), name
        assert not ((t != 0) & (t.abs() < tiny)).any(), f"a subnormal in {name}: pick other inputs"


@pytest.mark.parametrize("kind", ["shared", "per_sample"])
@pytest.mark.parametrize("shape", RULE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mul_rule_kernel_bit_for_bit(shape, kind):
    """fp32 and fp64 against the CPU torch restatement, bf16 against the fp32 kernel on exact upcasts, all bit for bit: the
    rule takes no sum, the library is built without contraction and with correctly rounded division, so equality follows.
    Also: in place gives the same bits, a batch equals its samples, masked planes are exactly zero."""
    from transformer_explainability_amd import ops
    B, H, rows, cols = shape
    tag = f"head_mask.rule.{'x'.join(map(str, shape))}.{kind}"
    d = dev()
    for dtype, name in ((torch.float32, "f32"), (F64, "f64")):
        R, P = _rule_case(B, H, rows, cols, dtype, seed=sum(shape))
        m = _mask(B, H, kind, dtype)
        _assert_no_subnormal_intermediate(R, P, m)
        ref = HR.mul_head_relprop(R, P, m)
        Rd, Pd, md = R.to(d), P.to(d), m.to(d)
        got = ops.mul_head_relprop(Rd, Pd, md)
        assert got.dtype == dtype and got.data_ptr() != Rd.data_ptr()
        check(f"{tag}.{name}", got, ref, 0.0, exact=True)
        zero_planes = (m.expand(B, H, 1, 1) == 0).view(B, H)
        assert not got[zero_planes.to(d)].any() and (cols == 1 or got[~zero_planes.to(d)].any())
        # the mask in its other accepted layouts
        assert torch.equal(ops.mul_head_relprop(Rd, Pd, md.flatten(1)), got)
        if kind == "shared":
            assert torch.equal(ops.mul_head_relprop(Rd, Pd, md.flatten()), got)
        # in place
        buf = Rd.clone()
        assert ops.mul_head_relprop(buf, Pd, md, out=buf) is buf
        check(f"{tag}.{name}.in_place", buf, ref, 0.0, exact=True)
        # a batch equals its samples
        for i in sorted({0, B // 2, B - 1}):
            mi = md if md.shape[0] == 1 else md[i:i + 1]
            assert torch.equal(ops.mul_head_relprop(Rd[i:i + 1], Pd[i:i + 1], mi), got[i:i + 1]), i
        if dtype == torch.float32:
            # bf16 operands: P and m rounded to bf16 (read exactly by the kernel) against the fp32 kernel on their upcasts
            P16, m16 = Pd.to(BF), md.to(BF)
            got16 = ops.mul_head_relprop(Rd, P16, m16)
            assert got16.dtype == torch.float32
            check(f"{tag}.bf16_vs_f32_on_upcasts", got16, ops.mul_head_relprop(Rd, P16.float(), m16.float()), 0.0, exact=True)
            buf = Rd.clone()
            ops.mul_head_relprop(buf, P16, m16, out=buf)
            assert torch.equal(buf, got16)


@pytest.mark.parametrize("value", MASK_VALUES)
def test_mul_rule_kernel_uniform_masks_and_unaligned_planes(value):
    """Every head the same value; R, P and out deliberately at 4-byte-aligned addresses that differ from one another modulo 16
    (slices of larger buffers), odd planes: the head / body / tail split must not depend on how the three pointers are aligned."""
    from transformer_explainability_amd import ops
    B, H, rows, cols = 2, 3, 67, 67
    R, P = _rule_case(B, H, rows, cols, torch.float32, seed=5)
    m = torch.full((1, H, 1, 1), value)
    _assert_no_subnormal_intermediate(R, P, m)
    ref = HR.mul_head_relprop(R, P, m)
    d = dev()
    n = R.numel()

    def at(t, off):
        buf = torch.zeros(n + 8, dtype=t.dtype, device=d)
        buf[off:off + n] = t.flatten().to(d)
        return buf[off:off + n].view(t.shape)

    for r_off, p_off, o_off in ((0, 0, 0), (1, 2, 3), (3, 0, 1), (2, 2, 2)):
        Rd, Pd = at(R, r_off), at(P, p_off)
        out = at(torch.zeros_like(R), o_off)
        assert Rd.is_contiguous() and out.is_contiguous()
        got = ops.mul_head_relprop(Rd, Pd, m.to(d), out=out)
        check(f"head_mask.rule.uniform{value}.offsets{r_off}{p_off}{o_off}", got, ref, 0.0, exact=True)
        got16 = ops.mul_head_relprop(Rd, at(P.to(BF), p_off), m.to(d).to(BF))
        assert torch.equal(got16, ops.mul_head_relprop(Rd, P.to(BF).float().to(d), m.to(d)))
    if value == 0.0:
        assert not got.any()
        # a masked plane is written as zeros without reading R or P: NaN there does not reach the output
        Rn, Pn = torch.full_like(R, float("nan")).to(d), torch.full_like(P, float("nan")).to(d)
        assert not ops.mul_head_relprop(Rn, Pn, m.to(d)).any()


# ------------------------------------------------------------------------------------------------ 2. the head-relevance kernel
@pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,D", [(1, 1), (5, 3), (197, 64)])
def test_head_relevance_kernel(N, D, dtype):
    """Against R.double().sum((2, 3)) on the CPU.  Every addend is exact in fp64, so whatever the order of the N D - 1 additions
    the two sums differ by at most N D 2^-53 sum|R| per head (the a-priori bound of a recursive sum; no measured constant).
    The relevance is read in place from the [B,N,C] layout; a repeated call and the samples on their own give the same bits."""
    from transformer_explainability_amd import ops
    B, H = 3, 4
    g = torch.Generator().manual_seed(N * 100 + D)
    cam = (1e-3 * torch.randn(B, N, H * D, generator=g, dtype=dtype))
    heads = lambda t: t.view(t.shape[0], N, H, D).permute(0, 2, 1, 3)      # noqa: E731
    ref = heads(cam).double().sum(dim=(2, 3))
    bound = N * D * 2.0 ** -53 * heads(cam).double().abs().sum(dim=(2, 3))
    cd = cam.to(dev())
    view = heads(cd)
    assert not view.is_contiguous() or N == 1 or H == 1
    got = ops.head_relevance(view)
    assert got.dtype == F64 and got.shape == (B, H)
    err = (got.cpu() - ref).abs()
    record(f"head_mask.head_relevance.N{N}.D{D}.{dtype}", max_err=float(err.max()), min_bound=float(bound.min()),
           max_err_over_bound=float((err / bound).max()))
    assert (err <= bound).all(), (err, bound)
    assert bits_equal(ops.head_relevance(view), got)
    for i in range(B):
        assert bits_equal(ops.head_relevance(heads(cd[i:i + 1])), got[i:i + 1]), i
    assert bits_equal(ops.head_relevance(view.contiguous()), got)          # the order depends on (N, D) alone, not on the strides


# ------------------------------------------------------------------------------------------------ 3. tiny BERT
L_, H_, B_, N_ = 2, 2, 3, 24
LH_MASK = [[1.0, 0.0], [0.5, 1.0]]                                     # layer 0 head 1 masked out, layer 1 head 0 halved
LBH_MASK = [[[1.0, 0.0], [0.5, 1.0], [1.0, 1.0]], [[-2.0, 1.0], [1.0, 0.5], [0.0, 1.0]]]


def _bert(dtype=torch.float32):
    """The small model of tests/test_gpu_models.py (test_bert_soft_mask_fused_equals_stock_and_oracle)."""
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=128, num_hidden_layers=L_, num_attention_heads=H_,
                              intermediate_size=256, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(11)
    model = bert.BertForSequenceClassification(cfg).eval()
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return model.to(dev()).to(dtype)


def _bert_inputs():
    ids = torch.randint(1, 100, (B_, N_), generator=torch.Generator().manual_seed(12)).to(dev())
    mask = torch.ones(B_, N_)
    mask[1, 20:] = 0.0               # padding on one sample
    return ids, mask.to(dev())


@pytest.fixture(scope="module")
def bert32():
    return _bert()


def _attn(model):
    return [lay.attention.self for lay in model.bert.encoder.layer]


def _assert_map(name, got, ref, norm_tol, rel_tol):
    """tests/test_gpu_models.py::_assert_map: the project's same-cache bars through gpu_util.map_stats."""
    s = map_stats(got, ref)
    record(name, **s)
    print(name, s)
    assert torch.isfinite(got).all()
    assert s["raw_max_abs"] <= 1e-4, (name, s)
    assert s["rel_linf"] <= rel_tol, (name, s)
    assert s["normalised_max_abs"] <= norm_tol, (name, s)


def _spy_relprop(modules):
    """Record the relevance each listed rule module receives (instance attribute over the class method; undo() removes it)."""
    seen = {}

    def wrap(key, mod):
        inner = type(mod).relprop.__get__(mod)

        def relprop(R, *a, **kw):
            seen[key] = R
            return inner(R, *a, **kw)
        mod.relprop = relprop

    for key, mod in modules.items():
        wrap(key, mod)

    def undo():
        for mod in modules.values():
            del mod.relprop
    return seen, undo


@pytest.mark.parametrize("which", ["LH", "LBH"])
def test_bert_tiny_masked_vs_restatement_on_the_same_cache(bert32, which):
    """Generator.generate_LRP(start_layer=0) with masked heads against head_mask_ref on the cache of that very pass; bars:
    the tiny-BERT same-cache bars of tests/test_gpu_models.py (norm 1e-4, rel 3e-4).  Then the exact facts of a head masked
    with 0 and the per-head relevance."""
    from transformer_explainability_amd.generators import Generator
    model = bert32
    ids, mask = _bert_inputs()
    hm = torch.tensor(LH_MASK if which == "LH" else LBH_MASK)
    gen = Generator(model)
    sas = _attn(model)
    D = 128 // H_
    seen, undo = _spy_relprop({(i, n): getattr(sa, n) for i, sa in enumerate(sas) for n in ("query", "key", "value")})
    try:
        out = gen.generate_LRP(ids, mask, start_layer=0, head_mask=hm).clone()
    finally:
        undo()
    assert out.shape == (B_, N_) and out.dtype == torch.float32
    for sa in sas:
        assert sa._fused_anchor is None and tuple(sa.head_mask.shape) == ((1 if which == "LH" else B_), H_, 1, 1)
        assert torch.equal(sa.mul.X[0], sa.get_attn().detach()) and torch.equal(sa.matmul2.X[0], sa.mul.X[0] * sa.mul.X[1])
    cache = bert_cache_from_model(model)
    pm, ms = HR.masked_operands(sas, cpu32)
    ref = HR.bert_relprop(one_hot(model.classifier.Y, device="cpu"), cache, H_, pm, ms, start_layer=0)
    _assert_map(f"head_mask.bert_tiny.{which}.map_sl0", out, ref["map"], norm_tol=1e-4, rel_tol=3e-4)
    for i, sa in enumerate(sas):
        check(f"head_mask.bert_tiny.{which}.attn_cam.{i}", sa.get_attn_cam(), ref["attn_cams"][i], 3e-4)
    # exact facts about the heads masked with 0: (layer, sample or all, head)
    zeroed = [(0, slice(None), 1)] if which == "LH" else [(0, 0, 1), (1, 2, 0)]
    for lay, b, h in zeroed:
        sa = sas[lay]
        z = lambda t: not t[b, h].any()                                              # noqa: E731
        assert z(sa.get_attn_gradients()), "d/dP = m . d/dP' must be exactly zero"
        assert sa.get_attn()[b, h].any() and z(sa.get_attn_cam())
        for n in ("query", "key", "value"):
            r = seen[(lay, n)]
            assert r.shape == (B_, N_, 128) and not r[b, :, h * D:(h + 1) * D].any(), (lay, n)
            assert r[b, :, (1 - h) * D:(2 - h) * D].any()
    # per-head relevance of the same masked model: [B,L,H] fp64; a priori it equals the restatement's sums up to the same-cache
    # relative bar (3e-4) applied to each head's sum of |relevance| (the error of a sum is at most the sum of the errors)
    hr = gen.generate_head_relevance(ids, mask, head_mask=hm)
    assert hr.shape == (B_, L_, H_) and hr.dtype == F64
    c1_abs = ref["head_relevance_abs"]
    err = (hr.cpu() - ref["head_relevance"]).abs()
    record(f"head_mask.bert_tiny.{which}.head_relevance", max_err=float(err.max()), max_rel=float((err / c1_abs.clamp(min=1e-300)).max()))
    assert (err <= 3e-4 * c1_abs).all(), (err, c1_abs)
    for lay, b, h in zeroed:
        assert not hr[b, lay, h].any(), "nothing arrives at a head whose context is exactly zero"
    assert bits_equal(gen.generate_head_relevance(ids, mask, head_mask=hm), hr)
    assert all(not sa.save_head_relevance for sa in sas)
    assert torch.isfinite(hr).all()


def test_bert_tiny_options_give_the_plain_bits(bert32):
    """prune, overlap_backward, the producer flag, a HIP-graph replay and generate_all give the bits of the plain masked call;
    a call without a mask after a masked one gives the bits of a fresh unmasked call."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import GraphedCall, Generator
    model = bert32
    ids, mask = _bert_inputs()
    hm = torch.tensor(LBH_MASK, device=dev())
    fresh = Generator(model).generate_LRP(ids, mask, start_layer=0).clone()
    fresh1 = Generator(model).generate_LRP(ids, mask, start_layer=1).clone()
    plain = Generator(model).generate_LRP(ids, mask, start_layer=0, head_mask=hm).clone()
    plain1 = Generator(model).generate_LRP(ids, mask, start_layer=1, head_mask=hm).clone()
    assert not torch.equal(plain, fresh)
    got = {"prune_sl0": (Generator(model, prune=True).generate_LRP(ids, mask, start_layer=0, head_mask=hm).clone(), plain),
           "prune_sl1": (Generator(model, prune=True).generate_LRP(ids, mask, start_layer=1, head_mask=hm).clone(), plain1)}
    ov = Generator(model, overlap_backward=True).generate_LRP(ids, mask, start_layer=0, head_mask=hm)
    torch.cuda.synchronize()
    got["overlap_backward"] = (ov.clone(), plain)
    assert not ops.USE_FUSED_PRODUCERS
    try:
        ops.USE_FUSED_PRODUCERS = True
        fused = Generator(model).generate_LRP(ids, mask, start_layer=0, head_mask=hm).clone()
        assert all(sa._fused_anchor is None and sa.head_mask is not None for sa in _attn(model)), "a masked layer takes the stock branch"
    finally:
        ops.USE_FUSED_PRODUCERS = False
    got["fused_producers_flag"] = (fused, plain)
    gen = Generator(model)
    graphed = GraphedCall(lambda i, m: gen.generate_LRP(i, m, start_layer=0, head_mask=hm), (ids, mask))
    got["graphed_replay"] = (graphed(ids, mask).clone(), plain)
    torch.cuda.synchronize()
    # a call without a mask after the masked ones: no stale operands
    got["unmasked_after_masked_sl0"] = (Generator(model).generate_LRP(ids, mask, start_layer=0).clone(), fresh)
    got["unmasked_after_masked_sl1"] = (Generator(model, prune=True).generate_LRP(ids, mask, start_layer=1).clone(), fresh1)
    assert all(sa.head_mask is None for sa in _attn(model))
    eq = {}
    for name, (a, b) in got.items():
        eq[name] = _same(a, b)
        record(f"head_mask.bert_tiny.{name}", bitwise_equal=eq[name], max_abs=float((a - b).abs().max()))
    print(eq)
    assert all(eq.values()), eq


def test_bert_tiny_generate_all_with_a_mask_equals_the_single_calls(bert32):
    from transformer_explainability_amd.generators import Generator
    model = bert32
    ids, mask = _bert_inputs()
    hm = torch.tensor(LH_MASK)
    gen = Generator(model)
    single = {"LRP": gen.generate_LRP(ids, mask, start_layer=1, head_mask=hm).clone(),
              "LRP_last_layer": gen.generate_LRP_last_layer(ids, mask, head_mask=hm).clone(),
              "full_lrp": gen.generate_full_lrp(ids, mask, head_mask=hm).clone(),
              "attn_last_layer": gen.generate_attn_last_layer(ids, mask, head_mask=hm).clone(),
              "rollout": gen.generate_rollout(ids, mask, head_mask=hm).clone(),
              "attn_gradcam": gen.generate_attn_gradcam(ids, mask, head_mask=hm).clone()}
    unmasked = gen.generate_all(ids, mask, list(single), start_layer=1)
    got = gen.generate_all(ids, mask, list(single), start_layer=1, head_mask=hm)
    eq = {m: _same(got[m], single[m]) for m in single}
    assert all(eq.values()), eq
    assert not _same(got["LRP"], unmasked["LRP"]) and not _same(got["full_lrp"], unmasked["full_lrp"])


def test_bert_tiny_bf16_masked_vs_restatement_in_double():
    """A bf16 model: fp32 map against the fp64 restatement on the exactly upcast cache, per sample; the bar tests/test_gpu_bf16_bert.py
    applies to its tiny models (normalised <= 1e-4, relative <= 3e-4)."""
    from transformer_explainability_amd.generators import Generator
    model = _bert(BF)
    ids, mask = _bert_inputs()
    hm = torch.tensor(LBH_MASK)
    out = Generator(model).generate_LRP(ids, mask, start_layer=0, head_mask=hm)
    assert out.dtype == torch.float32 and out.shape == (B_, N_) and torch.isfinite(out).all()
    sas = _attn(model)
    assert all(sa.mul.X[0].dtype == BF and sa.mul.X[1].dtype == BF and sa.get_attn_cam().dtype == torch.float32 for sa in sas)
    assert not sas[0].get_attn_cam()[0, 1].any() and not sas[0].get_attn_gradients()[0, 1].any()
    oh = one_hot(model.classifier.Y, F64, device="cpu")
    for i in range(B_):
        with sliced_relprop_state(model, i, B_):
            cache = bert_cache_f64(model)
            pm, ms = HR.masked_operands(sas, cpu64)
        ref = HR.bert_relprop(oh[i:i + 1], cache, H_, pm, ms, start_layer=0)
        s = map_stats(out[i:i + 1], ref["map"])
        record(f"head_mask.bert_tiny.bf16.map_sl0.{i}", **s)
        print("bf16", i, s)
        assert s["normalised_max_abs"] <= 1e-4 and s["rel_linf"] <= 3e-4, (i, s)


def test_bert_tiny_f64_masked_vs_restatement_in_double():
    """An fp64 model under the rule of tests/test_gpu_f64.py for its model-level comparisons: e64 <= 1e-4 (normalised, in double)
    and e64 <= 2^-20 e32, e32 the fp32 path's same-cache error on the .float() copy of the same model, inputs and mask."""
    from transformer_explainability_amd.generators import Generator
    m32 = _bert()
    model = copy.deepcopy(m32).double()
    ids, mask = _bert_inputs()
    hm = torch.tensor(LBH_MASK)
    out = Generator(model).generate_LRP(ids, mask, start_layer=0, head_mask=hm)
    assert out.dtype == F64 and out.shape == (B_, N_) and torch.isfinite(out).all()
    assert all(sa.mul.X[1].dtype == F64 for sa in _attn(model))
    index = model.classifier.Y.detach().argmax(-1)

    def restated(m):
        oh = torch.zeros(m.classifier.Y.shape, dtype=F64).scatter_(1, index.cpu().view(-1, 1), 1.0)
        pm, ms = HR.masked_operands(_attn(m), cpu64)
        return HR.bert_relprop(oh, bert_cache_f64(m), H_, pm, ms, start_layer=0)["map"]

    e64 = norm_err(out, restated(model))
    out32 = Generator(m32).generate_LRP(ids, mask, index=index, start_layer=0, head_mask=hm)
    e32 = norm_err(out32, restated(m32))
    record("head_mask.bert_tiny.f64", e64=e64, e32=e32, ratio=e64 / max(e32, 1e-300))
    print("f64", e64, e32)
    assert e64 <= 1e-4, e64
    assert e64 <= 2.0 ** -20 * e32, (e64, e32)
    assert bits_equal(Generator(model).generate_LRP(ids, mask, start_layer=0, head_mask=hm), out)
    hr = Generator(model).generate_head_relevance(ids, mask, head_mask=hm)
    assert hr.dtype == F64 and not hr[0, 0, 1].any() and not hr[2, 1, 0].any()


# ------------------------------------------------------------------------------------------------ 4. tiny ViT
VL, VH = 3, 4
V_MASK = [[1.0, 0.0, 0.5, 1.0], [1.0, 1.0, 1.0, -2.0], [0.0, 1.0, 1.0, 0.5]]      # heads (0,1) and (2,0) masked out


@pytest.fixture(scope="module")
def vit_tiny():
    """The 64-wide test model (tests/test_gpu_models.py::test_vit_tiny_golden's shape), seeded."""
    from transformer_explainability_amd import vit
    torch.manual_seed(0)
    model = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=VL, num_heads=VH, num_classes=10,
                                  qkv_bias=True).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.02 * torch.randn_like(p))
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(21))
    return model.to(dev()), x.to(dev())


def test_vit_tiny_masked_vs_restatement_on_the_same_cache(vit_tiny):
    """The same-cache comparison under the tiny-ViT bars of tests/test_gpu_models.py (_assert_map: normalised 1e-3, relative 2e-3,
    raw 1e-4), the facts of the heads masked with 0, the cls-only path against the dense one, and the options."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model, x = vit_tiny
    B, D = x.shape[0], 64 // VH
    hm = torch.tensor(V_MASK)
    attns = [blk.attn for blk in model.blocks]
    fresh = LRP(model).generate_LRP(x, start_layer=0).clone()
    seen, undo = _spy_relprop({i: a.qkv for i, a in enumerate(attns)})
    try:
        out = LRP(model).generate_LRP(x, start_layer=0, head_mask=hm).clone()
    finally:
        undo()
    assert out.shape == (B, 16) and not torch.equal(out, fresh)
    cache = vit_cache_from_model(model)
    pm, ms = HR.masked_operands(attns, cpu32)
    ref = HR.vit_relprop(one_hot(model.head.Y, device="cpu"), cache, VH, pm, ms, start_layer=0)
    _assert_map("head_mask.vit_tiny.map_sl0", out, ref["map"], norm_tol=1e-3, rel_tol=2e-3)
    for i, a in enumerate(attns):
        check(f"head_mask.vit_tiny.attn_cam.{i}", a.get_attn_cam(), ref["attn_cams"][i], 2e-3)
    for lay, h in ((0, 1), (2, 0)):
        a = attns[lay]
        assert not a.get_attn_gradients()[:, h].any() and a.get_attn()[:, h].any()
        assert not a.get_attn_cam()[:, h].any() and not a.get_v_cam()[:, h].any()
        r = seen[lay].view(B, 17, 3, VH, D)
        assert not r[:, :, :, h].any() and r[:, :, :, 3 - h].any()
    # the cls-only evaluation of the last block against the dense one, and the options, bit for bit
    try:
        model.exploit_cls_sparsity = False
        dense = LRP(model).generate_LRP(x, start_layer=0, head_mask=hm).clone()
    finally:
        model.exploit_cls_sparsity = True
    got = {"dense_last_block": dense,
           "prune_sl1": LRP(model, prune=True).generate_LRP(x, start_layer=1, head_mask=hm).clone()}
    ov = LRP(model, overlap_backward=True).generate_LRP(x, start_layer=0, head_mask=hm)
    torch.cuda.synchronize()
    got["overlap_backward"] = ov.clone()
    want = {"prune_sl1": LRP(model).generate_LRP(x, start_layer=1, head_mask=hm).clone()}
    allm = LRP(model).generate_all(x, ["transformer_attribution", "rollout", "last_layer", "full"], start_layer=0, head_mask=hm)
    got["generate_all"] = allm["transformer_attribution"].clone()
    assert _same(allm["rollout"], LRP(model).generate_LRP(x, method="rollout", head_mask=hm))
    assert _same(allm["full"], LRP(model).generate_LRP(x, method="full", head_mask=hm))
    eq = {k: _same(v, want.get(k, out)) for k, v in got.items()}
    print(eq)
    assert all(eq.values()), eq
    assert all(a._fused_anchor is None for a in attns)
    assert _same(LRP(model).generate_LRP(x, start_layer=0), fresh) and all(a.head_mask is None for a in attns)
    assert not ops.USE_FUSED_PRODUCERS


def test_vit_tiny_head_relevance_is_conserved(vit_tiny):
    """generate_head_relevance: [B,L,H] fp64 whose rows sum to the relevance that entered each block's attention branch (the
    relevance proj.relprop returned, summed over tokens and channels in double on the CPU), within the sum bound of the kernel
    test: N C 2^-53 sum|R| per layer for each of the two summation orders."""
    from transformer_explainability_amd.generators import LRP
    model, x = vit_tiny
    hm = torch.tensor(V_MASK)
    attns = [blk.attn for blk in model.blocks]
    entered = {}
    handles = []
    for i, a in enumerate(attns):
        inner = a.relprop_after_proj

        def spy(cam, _i=i, _inner=inner, **kw):
            entered[_i] = cam.detach().clone()
            return _inner(cam, **kw)
        a.relprop_after_proj = spy
        handles.append(a)
    try:
        hr = LRP(model).generate_head_relevance(x, head_mask=hm)
    finally:
        for a in handles:
            del a.relprop_after_proj
    B = x.shape[0]
    assert hr.shape == (B, VL, VH) and hr.dtype == F64 and torch.isfinite(hr).all()
    assert not hr[:, 0, 1].any() and not hr[:, 2, 0].any() and hr[:, 1].all()
    for i in range(VL):
        cam = entered[i].double().cpu()
        total, mag = cam.sum(dim=(1, 2)), cam.abs().sum(dim=(1, 2))
        bound = 2 * cam[0].numel() * 2.0 ** -53 * mag
        err = (hr[:, i].sum(dim=1).cpu() - total).abs()
        record(f"head_mask.vit_tiny.conservation.{i}", max_err=float(err.max()), min_bound=float(bound.min()))
        assert (err <= bound).all(), (i, err, bound)
    # the unmasked model, and the scores of a pass are reproducible
    plain = LRP(model).generate_head_relevance(x)
    assert plain.all() and bits_equal(LRP(model).generate_head_relevance(x), plain)
    # fp64 model: same call, fp64 relevance read by the fp64 kernel
    m64 = copy.deepcopy(model).double()
    hr64 = LRP(m64).generate_head_relevance(x.double(), head_mask=hm)
    assert hr64.dtype == F64 and not hr64[:, 0, 1].any()
    cache = vit_cache_f64(m64)
    pm, ms = HR.masked_operands([blk.attn for blk in m64.blocks], cpu64)
    oh = torch.zeros(m64.head.Y.shape, dtype=F64).scatter_(1, m64.head.Y.detach().cpu().argmax(-1, keepdim=True), 1.0)
    ref = HR.vit_relprop(oh, cache, VH, pm, ms)
    # (the bar of the fp32 chain, the same-cache relative bar against each head's own magnitude: an fp64 chain can do no worse)
    err = (hr64.cpu() - ref["head_relevance"]).abs()
    record("head_mask.vit_tiny.f64.head_relevance", max_err=float(err.max()), scale=float(ref["head_relevance_abs"].max()))
    assert (err <= 2e-3 * ref["head_relevance_abs"]).all(), err
