"""fp64 models on the MI355X: every relprop rule in double (csrc/te_f64.hip) against the CPU oracle in double, with
a-priori rounding bounds (tests/f64_util.py: u = 2^-53 times contraction lengths + a small constant times the sum of the
absolute values of an output's terms; asserted as |got - oracle| <= 2 bound since both sides round in fp64), determinism and
batch = samples bit for bit, and the model-level maps of ViT / DeiT and BERT with the project's bar (min-max-normalised
max-abs <= 1e-4, in double) and the fp64 claim e64 <= 2^-20 e32 (e32: the fp32 path's same-cache error for the .float()
copy of the same model and inputs)."""
import copy

import pytest
import torch

from f64_util import (F64, U, add_bounds, bert_cache_f64, bits_equal, headmean_bound, linear_bound, matmul_rule_bounds,
                      norm_err, ratio_to_bound, rnd64, vit_cache_f64)
from gpu_util import dev, record, sliced_relprop_state
from oracle import relprop_oracle as O

pytestmark = pytest.mark.gpu


def _within(name, got, ref, bound):
    """|got - ref| <= 2 bound element-wise; records and returns max err / bound."""
    assert got.dtype == F64 and tuple(got.shape) == tuple(ref.shape), (name, got.dtype, got.shape, ref.shape)
    g = got.detach().cpu()
    assert torch.isfinite(g).all(), name
    r = ratio_to_bound(g, ref, bound)
    record(name, err_over_bound=r, max_abs=float((g - ref).abs().max()), ref_max=float(ref.abs().max()))
    assert r <= 2.0, (name, r)
    return r


# ------------------------------------------------------------------------------------------------ Linear
LINEAR_SHAPES = [(1, 4, 3), (130, 72, 40), (33, 130, 257), (5, 96, 1000)]


def _linear_case(T, in_f, out_f):
    R, X, W = rnd64((T, out_f), T + 1), rnd64((T, in_f), in_f + 2), rnd64((out_f, in_f), out_f + 3, 0.1)
    g = torch.Generator().manual_seed(T + in_f + out_f)
    W[torch.rand(W.shape, generator=g) < 0.02] = 0.0           # 2 % of W exactly zero
    if T > 1:
        X[T // 2] = 0.0                                        # an all-zero input row
        R[T - 1] = 0.0                                         # a zero relevance row
    return R, X, W


@pytest.mark.parametrize("T,in_f,out_f", LINEAR_SHAPES)
def test_linear_f64_within_the_rounding_bound(T, in_f, out_f):
    """bound_i = (in_f + out_f + 6) u |x_i| (|S| |W^{sign x_i}|)_i  (f64_util.linear_bound; Z's terms are all non-negative:
    no cancellation).  |got - oracle_fp64| <= 2 bound; the fp32 kernels on the .float() copies violate the same bound (the
    test tells the precisions apart); zero rows give exact zeros; strided views and an 8-byte base offset give the
    contiguous tensor's bits; a second call and every sample alone give the batch's bits."""
    from transformer_explainability_amd import ops
    R, X, W = _linear_case(T, in_f, out_f)
    ref, bound = O.linear_relprop(R, X, W), linear_bound(R, X, W)
    Rd, Xd, Wd = R.to(dev()), X.to(dev()), W.to(dev())
    got = ops.linear_relprop(Rd, Xd, Wd)
    _within(f"f64.linear.{T}x{in_f}x{out_f}", got, ref, bound)
    if T > 1:
        assert not got[T // 2].any() and not got[T - 1].any()
    err32 = (ops.linear_relprop(Rd.float(), Xd.float(), Wd.float()).double().cpu() - ref).abs()
    r32 = float((err32 / bound.clamp(min=1e-300)).max())
    record(f"f64.linear.{T}x{in_f}x{out_f}.fp32_kernels", err_over_bound=r32)
    assert (err32 > 2 * bound).any(), r32
    # views: the cls rows [:, :1] of a [B, N, C] tensor, and a base offset of one element
    big = rnd64((T, 3, in_f), 7).to(dev())
    big[:, 0] = Xd
    assert bits_equal(ops.linear_relprop(Rd.unsqueeze(1), big[:, :1], Wd).reshape(T, in_f), got)
    off = torch.empty(T * in_f + 1, dtype=F64, device=dev())
    off[1:].view(T, in_f).copy_(Xd)
    assert off[1:].data_ptr() % 16 == 8
    assert bits_equal(ops.linear_relprop(Rd, off[1:].view(T, in_f), Wd), got)
    assert bits_equal(ops.linear_relprop(Rd, Xd, Wd), got)
    for i in sorted({0, T // 2, T - 1}):
        assert bits_equal(ops.linear_relprop(Rd[i:i + 1], Xd[i:i + 1], Wd), got[i:i + 1]), i


# ------------------------------------------------------------------------------------------------ attention rules
ATTN_SHAPES = [(1, 1, 1, 4), (2, 3, 17, 16), (1, 2, 197, 64)]


def _attn_case(B, H, N, D):
    C = H * D
    qkv = rnd64((B, N, 3 * C), N + D)
    q, k, v = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    attn = torch.softmax(q.matmul(k.transpose(-1, -2)) * D ** -0.5, dim=-1)
    R = rnd64((B, N, C), B + H).view(B, N, H, D).permute(0, 2, 1, 3)         # 'b n (h d)' relevance, read as heads
    if N > 1:
        R[:, :, 0] = 0.0
    return qkv, attn.contiguous(), R


@pytest.mark.parametrize("B,H,N,D", ATTN_SHAPES)
def test_attention_rules_f64_within_the_rounding_bound(B, H, N, D):
    """Operands are views of a fused qkv activation, outputs go into cam_qkv slots, Z is the product formed once on the
    device and handed to both sides.  Bounds (f64_util.matmul_rule_bounds): (n + 4) u |X| (|S| |X'|) with n the contraction
    length -- D for cam_attn, N for cam_v, cam_q and cam_k."""
    from transformer_explainability_amd import ops
    qkv, attn, R = _attn_case(B, H, N, D)
    C = H * D
    qkv_d, attn_d = qkv.to(dev()), attn.to(dev())
    q, k, v = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    qd, kd, vd = qkv_d.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    Rd = R.contiguous().to(dev()).permute(0, 2, 1, 3).contiguous().view(B, N, H, D).permute(0, 2, 1, 3)      # strided heads view
    tag = f"f64.attn.{B}x{H}x{N}x{D}"

    def run():
        cam_qkv = torch.full((B, N, 3 * C), float("nan"), dtype=F64, device=dev())
        slots = cam_qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
        z_av = torch.matmul(attn_d, vd)
        cam_attn, cam_v = ops.matmul_relprop_av(Rd, attn_d, vd, out_scale=0.5, cam_v_out=slots[2], z=z_av)
        z_qk = torch.matmul(qd, kd.transpose(-1, -2))
        ops.matmul_relprop_qk(cam_attn, qd, kd, out_scale=0.5, cam_q_out=slots[0], cam_k_out=slots[1], z=z_qk)
        return cam_attn, cam_qkv, z_av, z_qk

    cam_attn, cam_qkv, z_av, z_qk = run()
    slots = cam_qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    assert cam_v_is_slot(slots[2], cam_qkv)
    z_av_c, z_qk_c = z_av.cpu(), z_qk.cpu()
    ref_attn, ref_v = O.einsum_av_relprop(R, attn, v, z_av_c)
    b_attn, b_v = matmul_rule_bounds(R, attn, v, z_av_c)
    _within(tag + ".cam_attn", cam_attn, ref_attn / 2, b_attn / 2)
    _within(tag + ".cam_v", slots[2], ref_v / 2, b_v / 2)
    # the QK rule's relevance is the device's cam_attn (its own error is bounded above): bound the QK rule on that input
    r_qk = cam_attn.cpu()
    ref_q, ref_k = O.einsum_qk_relprop(r_qk, q, k, z_qk_c)
    b_q, b_kt = matmul_rule_bounds(r_qk, q, k.transpose(-1, -2), z_qk_c)
    _within(tag + ".cam_q", slots[0], ref_q / 2, b_q / 2)
    _within(tag + ".cam_k", slots[1], ref_k / 2, b_kt.transpose(-1, -2) / 2)
    if N > 1:
        assert not cam_attn[:, :, 0].any()
    # determinism, Z formed by ops when the caller has none, batch = samples
    again = run()
    assert bits_equal(again[0], cam_attn) and bits_equal(again[1], cam_qkv)
    assert bits_equal(ops.matmul_relprop_av(Rd, attn_d, vd, out_scale=0.5)[0], cam_attn)
    assert bits_equal(ops.matmul_relprop_qk(cam_attn, qd, kd, out_scale=0.5)[0].contiguous(), slots[0].contiguous())
    for i in range(B):
        ca, cv = ops.matmul_relprop_av(Rd[i:i + 1], attn_d[i:i + 1], vd[i:i + 1], out_scale=0.5, z=z_av[i:i + 1])
        cq, ck = ops.matmul_relprop_qk(ca, qd[i:i + 1], kd[i:i + 1], out_scale=0.5, z=z_qk[i:i + 1])
        for one, batch in ((ca, cam_attn), (cv, slots[2]), (cq, slots[0]), (ck, slots[1])):
            assert bits_equal(one.contiguous(), batch[i:i + 1].contiguous()), i


def cam_v_is_slot(slot, cam_qkv):
    return slot.data_ptr() >= cam_qkv.data_ptr() and not torch.isnan(cam_qkv).any()


# ------------------------------------------------------------------------------------------------ Add (ours)
def _add_check(tag, R, X0, X1):
    from transformer_explainability_amd import ops
    ref0, ref1 = O.add_relprop(R, X0, X1)
    b0, b1 = add_bounds(R, X0, X1)
    Rd, X0d, X1d = R.to(dev()), X0.to(dev()), X1.to(dev())
    out0, out1 = ops.add_relprop(Rd, X0d, X1d)
    _within(tag + ".out0", out0, ref0, b0)
    _within(tag + ".out1", out1, ref1, b1)
    d0, d1 = ops.add_relprop(Rd, X0d, X1d, deferred=True)          # plain tensors from the same kernels
    assert torch.is_tensor(d0) and torch.is_tensor(d1) and bits_equal(d0, out0) and bits_equal(d1, out1)
    B = R.shape[0]
    for i in range(B):
        x1 = X1d[i:i + 1] if X1d.shape[0] == B else X1d
        o0, o1 = ops.add_relprop(Rd[i:i + 1], X0d[i:i + 1], x1)
        assert bits_equal(o0, out0[i:i + 1]) and bits_equal(o1, out1[i:i + 1]), i
    return out0, out1


@pytest.mark.parametrize("shape", [(2, 5, 4), (3, 197, 64)])
def test_add_f64_same_shape_and_batchless_operand(shape):
    """f64_util.add_bounds: relative error 4 u of a = X0 sd(R, X0 + X1) plus the factors' error d, which carries the
    condition numbers sum|a| + sum|b| over |A| + |B| and sum|R| / |sum R| of the three per-sample sums (n + 4 terms each).
    The last sample's X1 is all zero: its second output is exactly zero."""
    R, X0, X1 = rnd64(shape, 1), rnd64(shape, 2), rnd64(shape, 3)
    X1[-1] = 0.0
    out0, out1 = _add_check("f64.add.same." + "x".join(map(str, shape)), R, X0, X1)
    assert not out1[-1].any()
    _add_check("f64.add.batchless." + "x".join(map(str, shape)), R, X0, rnd64((1,) + shape[1:], 4))


@pytest.mark.parametrize("mask_batch", [2, 1])
def test_add_f64_bert_mask_form(mask_batch):
    """X0 [2,2,24,24] against the mask [2|1,1,1,24] (padding -10000, soft entries, zeros); out1 = mask . column sums of S."""
    B, H, N = 2, 2, 24
    R, X0 = rnd64((B, H, N, N), 5), rnd64((B, H, N, N), 6, 3.0)
    m = torch.zeros(mask_batch, 1, 1, N, dtype=F64)
    m[..., N - 3:] = -10000.0
    m[..., 1:3] = -39.0625
    m[0, ..., 5] = -3.0
    R[:, :, 0] = 0.0
    out0, out1 = _add_check(f"f64.add.mask.m{mask_batch}", R, X0, m)
    assert out1.shape == (B, 1, 1, N) and not out0[:, :, 0].any()


# ------------------------------------------------------------------------------------------------ Clone, IndexSelect, head mean
def test_clone_and_index_select_f64_equal_the_oracle_to_4u():
    """Single products with a fixed rounding sequence: |got - oracle| <= 4 u |oracle| per element."""
    from transformer_explainability_amd import ops
    X = rnd64((3, 17, 40), 1)
    X[0, 0, :5] = 0.0
    Rs = [rnd64(X.shape, 2 + i) for i in range(3)]
    Xd, Rd = X.to(dev()), [r.to(dev()) for r in Rs]
    worst = 0.0
    for n in (2, 3):
        got, ref = ops.clone_relprop(Rd[:n], Xd), O.clone_relprop(Rs[:n], X)
        assert got.dtype == F64 and ((got.cpu() - ref).abs() <= 4 * U * ref.abs()).all(), n
        worst = max(worst, float(((got.cpu() - ref).abs() / ref.abs().clamp(min=1e-300)).max()) / U)
        assert bits_equal(ops.clone_relprop(Rd[:n], Xd), got)
        assert bits_equal(ops.clone_relprop([r[1:2] for r in Rd[:n]], Xd[1:2]), got[1:2])
    R1 = rnd64((3, 1, 40), 9)
    for index in (0, 16):
        got, ref = ops.index_select_relprop(R1.to(dev()), Xd, index), O.index_select_relprop(R1, X, 1, index)
        assert got.dtype == F64 and ((got.cpu() - ref).abs() <= 4 * U * ref.abs()).all(), index
        worst = max(worst, float(((got.cpu() - ref).abs() / ref.abs().clamp(min=1e-300)).max()) / U)
        assert bits_equal(ops.index_select_relprop(R1.to(dev()), Xd, index), got)
        assert bits_equal(ops.index_select_relprop(R1[2:3].to(dev()), Xd[2:3], index), got[2:3])
    record("f64.clone_index_select", max_rel_err_in_u=worst)


def test_gradcam_headmean_f64():
    """(H + 2) u mean_h |g c| (f64_util.headmean_bound)."""
    from transformer_explainability_amd import ops
    g, c = rnd64((2, 5, 23, 23), 1), rnd64((2, 5, 23, 23), 2)
    gd, cd = g.to(dev()), c.to(dev())
    got = ops.gradcam_headmean(gd, cd)
    _within("f64.headmean", got, O.gradcam_headmean(g, c), headmean_bound(g, c))
    stack = torch.zeros((3, 2, 23, 23), dtype=F64, device=dev())
    ops.gradcam_headmean(gd, cd, out=stack[1])
    assert bits_equal(stack[1], got) and not stack[0].any() and not stack[2].any()
    assert bits_equal(ops.gradcam_headmean(gd[1:], cd[1:]), got[1:])


# ------------------------------------------------------------------------------------------------ models
BAR = 1e-4
CLAIM = 2.0 ** -20


def _vit(img, patch, dim, depth, heads, classes, seed=0):
    """(the fp64 model, its .float() copy): fp32 parameters upcast exactly, so the copy is the model they came from."""
    from transformer_explainability_amd import vit
    torch.manual_seed(seed)
    model = vit.VisionTransformer(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads,
                                  num_classes=classes, qkv_bias=True).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.02 * torch.randn_like(p))
    return copy.deepcopy(model).to(dev()).double(), model.to(dev())


def _one_hot64(logits, index):
    oh = torch.zeros(logits.shape, dtype=F64)
    oh.scatter_(1, index.cpu().view(-1, 1), 1.0)
    return oh


def _vit_errors(tag, model, m32, x, heads, start_layer, samples=None):
    """(e64, e32): normalised same-cache errors of the fp64 path and of the fp32 path on the .float() copy."""
    from transformer_explainability_amd.generators import LRP
    B = x.shape[0]
    out = LRP(model).generate_LRP(x, start_layer=start_layer)
    assert out.dtype == F64 and out.shape[0] == B and torch.isfinite(out).all()
    index = model.head.Y.detach().argmax(-1)
    sel = slice(0, B) if samples is None else samples

    def oracle(m):
        if samples is None:
            cache = vit_cache_f64(m)
        else:
            with sliced_relprop_state(m, samples.start, B):
                cache = vit_cache_f64(m)
        return O.vit_relprop(_one_hot64(m.head.Y, index)[sel], cache, num_heads=heads, start_layer=start_layer)["map"]

    e64 = norm_err(out[sel], oracle(model))
    out32 = LRP(m32).generate_LRP(x.float(), index=index, start_layer=start_layer)
    assert out32.dtype == torch.float32
    e32 = norm_err(out32[sel], oracle(m32))
    record(tag, e64=e64, e32=e32, ratio=e64 / max(e32, 1e-300))
    return out, e64, e32


@pytest.fixture(scope="module")
def tiny_vit():
    return (*_vit(32, 8, 64, 3, 4, 10), rnd64((3, 3, 32, 32), 21).to(dev()))


@pytest.mark.parametrize("start_layer", [0, 1])
def test_tiny_vit_f64_vs_oracle_in_double(tiny_vit, start_layer):
    """LRP(model.double()).generate_LRP raises TeError on a tree without the fp64 path."""
    model, m32, x = tiny_vit
    out, e64, e32 = _vit_errors(f"f64.vit_tiny.sl{start_layer}", model, m32, x, 4, start_layer)
    assert out.shape == (3, 16)
    assert e64 <= BAR, e64
    assert e64 <= CLAIM * e32, (e64, e32)


def test_tiny_vit_f64_batch_equals_samples_and_ignores_the_producer_flag(tiny_vit):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model, _, x = tiny_vit
    B = x.shape[0]
    out = LRP(model).generate_LRP(x, start_layer=0).clone()
    oh = _one_hot64(model.head.Y, model.head.Y.detach().argmax(-1)).to(dev())
    for i in range(B):
        with sliced_relprop_state(model, i, B):
            one = model.relprop(oh[i:i + 1], method="transformer_attribution", start_layer=0, alpha=1)
        assert bits_equal(one, out[i:i + 1]), i
    old = ops.USE_FUSED_PRODUCERS
    try:
        ops.USE_FUSED_PRODUCERS = True
        fused = LRP(model).generate_LRP(x, start_layer=0).clone()
    finally:
        ops.USE_FUSED_PRODUCERS = old
    assert bits_equal(fused, out)
    assert bits_equal(LRP(model).generate_LRP(x, start_layer=0), out)
    idx = torch.tensor([1, 2, 3])
    assert LRP(model).generate_LRP(x, index=idx, start_layer=1).dtype == F64


def test_vit_b16_f64_vs_oracle_in_double():
    """ViT-B/16, B = 2, one call: sample 0 against the oracle in double (both bars); sample 1 finite and equal to its
    single-sample run."""
    model, m32 = _vit(224, 16, 768, 12, 12, 1000, seed=1)
    x = rnd64((2, 3, 224, 224), 22).to(dev())
    out, e64, e32 = _vit_errors("f64.vit_b16", model, m32, x, 12, 0, samples=slice(0, 1))
    assert out.shape == (2, 196)
    assert e64 <= BAR, e64
    assert e64 <= CLAIM * e32, (e64, e32)
    oh = _one_hot64(model.head.Y, model.head.Y.detach().argmax(-1)).to(dev())
    with sliced_relprop_state(model, 1, 2):
        one = model.relprop(oh[1:2], method="transformer_attribution", start_layer=0, alpha=1)
    assert torch.isfinite(out[1]).all() and bits_equal(one, out[1:2])


def _soft_mask_bert(hidden, heads, inter):
    """The soft-mask model of tests/test_gpu_bf16_bert.py: (in double, its .float() copy)."""
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=hidden, num_hidden_layers=2, num_attention_heads=heads,
                              intermediate_size=inter, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(11)
    model = bert.BertForSequenceClassification(cfg).eval()
    with torch.no_grad():
        for _, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    return copy.deepcopy(model).to(dev()).double(), model.to(dev())


def _soft_mask_inputs():
    B, N = 3, 24
    ids = torch.randint(1, 100, (B, N), generator=torch.Generator().manual_seed(12)).to(dev())
    mask = torch.ones(B, N)
    mask[:, 5:9] = 0.99609375
    mask[1, 20:] = 0.0
    return ids, mask.to(dev())


@pytest.mark.parametrize("hidden,heads,inter", [(64, 4, 128), (128, 2, 256)], ids=["head_dim16", "head_dim64"])
def test_bert_soft_mask_f64_vs_oracle_in_double(hidden, heads, inter):
    from transformer_explainability_amd.generators import Generator
    model, m32 = _soft_mask_bert(hidden, heads, inter)
    ids, mask = _soft_mask_inputs()
    out = Generator(model).generate_LRP(ids, mask, start_layer=0)
    assert out.dtype == F64 and out.shape == (3, 24) and torch.isfinite(out).all()
    ext = model.bert.encoder.layer[0].attention.self.add.X[1]
    assert ext.dtype == F64 and float(ext[0, 0, 0, 5]) == -39.0625 and float(ext[1, 0, 0, 21]) == -10000.0
    index = model.classifier.Y.detach().argmax(-1)

    def oracle(m):
        return O.bert_relprop(_one_hot64(m.classifier.Y, index), bert_cache_f64(m), num_heads=heads, start_layer=0)["map"]

    e64 = norm_err(out, oracle(model))
    out32 = Generator(m32).generate_LRP(ids, mask, index=index, start_layer=0)
    e32 = norm_err(out32, oracle(m32))
    record(f"f64.bert_soft_mask.hidden{hidden}", e64=e64, e32=e32, ratio=e64 / max(e32, 1e-300))
    assert e64 <= BAR, e64
    assert e64 <= CLAIM * e32, (e64, e32)
    assert bits_equal(Generator(model).generate_LRP(ids, mask, start_layer=0), out)


def test_fp32_maps_are_untouched_by_fp64_calls(tiny_vit):
    from transformer_explainability_amd.generators import LRP
    model, m32, x = tiny_vit
    before = LRP(m32).generate_LRP(x.float(), start_layer=0).clone()
    LRP(model).generate_LRP(x, start_layer=0)
    after = LRP(m32).generate_LRP(x.float(), start_layer=0)
    assert after.dtype == torch.float32 and torch.equal(after.view(torch.int32), before.view(torch.int32))
