"""AttnLRP with a class axis on the MI355X (te_relprop.h, "AttnLRP, a class axis"; generate_attnlrp_classes).

Kernels: for K in {1, 2, 3} slice k of every te_alrpk_* entry's output has the bits of the entry without a class axis on
(G[k], operand) -- aligned, at storage offsets (one phase, mixed phases), in place, eps 0 and 1e-6, at sizes whose class stride
breaks the 16-byte phase (n = 5, 1027 with K >= 2), fp32 and bf16 operands.

Models: ``maps["attnlrp"][:, k]`` has the bits of generate_attnlrp(index=classes[:, k]) on a fresh forward pass -- tiny ViT
(dim 128: every product but the head's on te_gemm_x6_f32, the attention rule on te_attention_backward_strided_f32), tiny BERT,
their bf16 copies; for every ``chunk``, for topk, for method="full", eager and under GraphedCall replay.  General seeds equal
model.attnlrp(seed_k) on the same caches bit for bit where the head's product runs on te_gemm_x6_f32 at B and at K B rows;
elsewhere, and for the dim-96 model (stock GEMMs, torch attention), every class stays within 2 x the error of the fp32
restatement against fp64 per sample (the bar of tests/test_gpu_attnlrp.py).  What was measured goes to
attnlrp_classes_parity.json next to the parity report (committed as profiles/attnlrp_classes_parity.json).

Every test calls generate_attnlrp_classes, or a binding / chain with a class axis: none works without the feature."""
import json
import os

import pytest
import torch

import attnlrp_ref as ref
import attnlrp_seed_ref as sref
from gpu_util import REPORT, dev, rnd
from test_gpu_attnlrp import SPECIAL_Y, _bert_inputs, _ln_case, _rel_l2, _tiny_bert, _tiny_vit, bits_equal, offset_view

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
PARITY = os.path.join(os.path.dirname(REPORT), "attnlrp_classes_parity.json")
_parity = {}
KS = [1, 2, 3]


def _record(tag, **kw):
    _parity[tag] = kw
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    with open(PARITY, "w") as f:
        json.dump(_parity, f, indent=1, sort_keys=True)


def _per_class(fn, G):
    """the entry without a class axis on every slice"""
    return torch.stack([fn(G[k]) for k in range(G.shape[0])])


# ------------------------------------------------------------------------------------------------ damp, act
def _binary_cases(call, G, operand, want):
    """aligned; every tensor one element behind a boundary (one phase); mixed phases; in place"""
    assert bits_equal(call(G, operand, None), want)
    Gv, ov = offset_view(G), offset_view(operand)
    assert Gv.data_ptr() % 16 == 4
    assert bits_equal(call(Gv, ov, offset_view(torch.zeros_like(G))), want)
    assert bits_equal(call(Gv, operand, None), want) and bits_equal(call(G, offset_view(operand, 3), None), want)
    assert bits_equal(call(G, operand, offset_view(torch.zeros_like(G), 2)), want)
    Gi = G.clone()
    assert call(Gi, operand, Gi) is Gi and bits_equal(Gi, want)


@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("K", KS)
def test_damp_slices_are_the_single_entry_bit_for_bit(K, n, eps):
    from transformer_explainability_amd import ops
    Y = rnd((n,), n + 1)
    Y[:min(n, len(SPECIAL_Y))] = torch.tensor(SPECIAL_Y[:n])
    if n > 8:
        Y[8:16] = torch.tensor(SPECIAL_Y)[torch.randperm(8, generator=torch.Generator().manual_seed(n))]
    G, Y = (rnd((K, n), n + 2) * 4.0).to(dev()), Y.to(dev())
    want = _per_class(lambda g: ops.alrp_damp(g, Y, eps), G)
    assert want.shape == (K, n) and torch.isfinite(want).all()
    if eps == 0.0:
        assert bits_equal(want, G)
    _binary_cases(lambda g, y, out: ops.alrp_damp(g, y, eps, out=out), G, Y, want)


def _act_operand(n):
    x = rnd((n,), n + 3) * 3.0
    special = [0.0, -0.0, 1e-20, -1e-20, 20.0, -20.0]
    x[:min(n, 6)] = torch.tensor(special[:n])
    return x.to(dev())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
@pytest.mark.parametrize("K", KS)
def test_gelu_identity_rule_slices_are_the_single_entry_bit_for_bit(K, n):
    from transformer_explainability_amd import ops
    G, x = (rnd((K, n), n + 4) * 2.0).to(dev()), _act_operand(n)
    want = _per_class(lambda g: ops.alrp_act(g, x, "gelu"), G)
    assert torch.isfinite(want).all()
    if n >= 2:
        assert bits_equal(want[:, :2], G[:, :2] * 0.5)          # f'(0) at x == +-0
    _binary_cases(lambda g, y, out: ops.alrp_act(g, y, "gelu", out=out), G, x, want)


@pytest.mark.parametrize("n", [6, 1027])
@pytest.mark.parametrize("K", KS)
def test_tanh_identity_rule_slices_are_the_single_entry_bit_for_bit(K, n):
    from transformer_explainability_amd import ops
    G, x = (rnd((K, n), n + 4) * 2.0).to(dev()), _act_operand(n)
    want = _per_class(lambda g: ops.alrp_act(g, x, "tanh"), G)
    assert bits_equal(want[:, :2], G[:, :2])
    _binary_cases(lambda g, y, out: ops.alrp_act(g, y, "tanh", out=out), G, x, want)


def test_shape_refusals_of_the_bindings():
    from transformer_explainability_amd import TeError, ops
    Y, x0 = torch.zeros(2, 8, device=dev()), torch.zeros(2, 3, 8, device=dev())
    for G in (torch.zeros(3, 2, 7, device=dev()), torch.zeros(3, 3, 8, device=dev()), torch.zeros(3, 1, 2, 8, device=dev())):
        with pytest.raises(TeError, match="differ in shape"):
            ops.alrp_damp(G, Y)
        with pytest.raises(TeError, match="differ in shape"):
            ops.alrp_act(G, Y)
    with pytest.raises(TeError, match="rstd"):
        ops.alrp_layernorm(torch.zeros(3, 2, 8, device=dev()), torch.ones(8, device=dev()), torch.ones(3, device=dev()))
    with pytest.raises(TeError, match="x0 and G"):
        ops.alrp_token_relevance(x0, torch.zeros(4, 2, 3, 7, device=dev()))


# ------------------------------------------------------------------------------------------------ LayerNorm rule
@pytest.mark.parametrize("C", [1, 64, 100, 768])
@pytest.mark.parametrize("rows", [1, 3, 197])
@pytest.mark.parametrize("K", KS)
def test_layernorm_slices_are_the_single_entry_bit_for_bit(K, rows, C):
    from transformer_explainability_amd import ops
    _, gamma, x = _ln_case(rows, C)
    G = rnd((K, rows, C), K + rows + C)
    G[0, 0, 0] = 0.0
    G = G.to(dev())
    rstd = ops.alrp_row_rstd(x, 2.0 ** -20)
    want = _per_class(lambda g: ops.alrp_layernorm(g, gamma, rstd), G)
    assert want.shape == (K, rows, C) and torch.isfinite(want).all()
    assert bits_equal(ops.alrp_layernorm(G, gamma, rstd), want)
    # a [B, N] batch of rows: rstd with two dimensions, G with four
    if rows == 3:
        assert bits_equal(ops.alrp_layernorm(G.view(K, 1, 3, C), gamma, rstd.view(1, 3)), want.view(K, 1, 3, C))
    assert bits_equal(ops.alrp_layernorm(offset_view(G), offset_view(gamma, 2), rstd), want)
    assert bits_equal(ops.alrp_layernorm(G, gamma, offset_view(rstd), out=offset_view(torch.zeros_like(G), 3)), want)
    Gi = G.clone()
    assert ops.alrp_layernorm(Gi, gamma, rstd, out=Gi) is Gi and bits_equal(Gi, want)


# ------------------------------------------------------------------------------------------------ token relevance
@pytest.mark.parametrize("B,N,C", [(1, 2, 1), (3, 17, 128), (2, 197, 768)])
@pytest.mark.parametrize("skip_first", [True, False])
@pytest.mark.parametrize("K", KS)
def test_token_relevance_slices_are_the_single_entry_bit_for_bit(K, B, N, C, skip_first):
    from transformer_explainability_amd import ops
    x0, G = rnd((B, N, C), B + N).to(dev()), rnd((K, B, N, C), K + B + N + C).to(dev())
    x0[0, N - 1] = 0.0
    got = ops.alrp_token_relevance(x0, G, skip_first=skip_first)
    first = int(skip_first)
    assert got.shape == (B, K, N - first) and got.dtype == torch.float32 and got.is_contiguous()
    for k in range(K):                                         # read from the batch-major [B, K, .] output
        assert bits_equal(got[:, k], ops.alrp_token_relevance(x0, G[k], skip_first=skip_first)), k
    assert not got[0, :, N - 1 - first].any()
    assert bits_equal(ops.alrp_token_relevance(offset_view(x0), offset_view(G, 2), skip_first=skip_first), got)


# ------------------------------------------------------------------------------------------------ bf16 operands
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("K", KS)
def test_bf16_operands_slices_are_the_single_entries_bit_for_bit(K, off):
    from transformer_explainability_amd import ops
    place = (lambda t: offset_view(t, off)) if off else (lambda t: t)
    n = 1027 if off else 1028
    Y = rnd((n,), 5).to(BF16)
    Y[:6] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0]).to(BF16)
    Y, G = place(Y.to(dev())), place((rnd((K, n), 6) * 4.0).to(dev()))
    for eps in (0.0, 1e-6):
        assert bits_equal(ops.alrp_damp(G, Y, eps), _per_class(lambda g: ops.alrp_damp(g, Y, eps), G)), eps
    for kind in ("gelu", "tanh"):
        assert bits_equal(ops.alrp_act(G, Y, kind), _per_class(lambda g: ops.alrp_act(g, Y, kind), G)), kind
    Gi = G.clone()
    assert ops.alrp_damp(Gi, Y, 1e-6, out=Gi) is Gi and bits_equal(Gi, _per_class(lambda g: ops.alrp_damp(g, Y, 1e-6), G))
    rows, C = 5, 100 if off else 768
    x, gamma = place((rnd((rows, C), 7) * 2.0).to(BF16).to(dev())), place((1.0 + 0.3 * rnd((C,), 8)).to(BF16).to(dev()))
    Gl = place(rnd((K, rows, C), 9).to(dev()))
    rstd = ops.alrp_row_rstd(x, 1e-6)
    assert bits_equal(ops.alrp_layernorm(Gl, gamma, rstd), _per_class(lambda g: ops.alrp_layernorm(g, gamma, rstd), Gl))
    x0, Gt = place(rnd((2, 17, C), 10).to(BF16).to(dev())), place(rnd((K, 2, 17, C), 11).to(dev()))
    got = ops.alrp_token_relevance(x0, Gt, skip_first=True)
    assert got.shape == (2, K, 16)
    for k in range(K):
        assert bits_equal(got[:, k], ops.alrp_token_relevance(x0, Gt[k], skip_first=True)), k


# ------------------------------------------------------------------------------------------------ models
CLASSES = [[1, 7, 4], [7, 7, 0], [4, 1, 9]]                    # (a duplicate in the second sample)


def _assert_within_twice(tag, got, R32, R64):
    e_chain, e_ref = _rel_l2(got, R64), _rel_l2(R32, R64)
    _record(tag, kernel_chain_rel_l2=e_chain.tolist(), fp32_restatement_rel_l2=e_ref.tolist(), ratio=(e_chain / e_ref).tolist())
    print(tag, "chain", e_chain.tolist(), "fp32 restatement", e_ref.tolist())
    assert torch.isfinite(got).all() and got.dtype == torch.float32
    assert bool((e_chain <= 2.0 * e_ref).all()), (tag, e_chain.tolist(), e_ref.tolist())


@pytest.fixture(scope="module")
def vit128():
    model, m32, m64 = _tiny_vit(128, 3)
    return model, rnd((3, 3, 32, 32), 31).to(dev()), (m32, m64)


def _single_maps(lrp, x, classes, **kw):
    """generate_attnlrp per class, each on a fresh forward pass -> [B,K,...]"""
    return torch.stack([lrp.generate_attnlrp(x, index=classes[:, k], **kw) for k in range(classes.shape[1])], 1)


def test_vit_routes_at_T_and_at_K_T():
    """What the bit-for-bit statements below rest on: the four Linear shapes of a block run on te_gemm_x6_f32 at T = 51 rows and
    at 2 T and 3 T, and the attention rule on te_attention_backward_strided_f32."""
    from transformer_explainability_amd import ops
    for T in (51, 102, 153):
        assert all(ops.gemm_x6_supported(T, k, m) for k, m in ((384, 128), (128, 128), (512, 128), (128, 512))), T
    assert ops._lib.load().te_attention_strided_supported(17, 64)


def test_vit_classes_have_the_bits_of_the_single_calls(vit128):
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit128
    lrp = LRP(model)
    classes = torch.tensor(CLASSES)
    out = lrp.generate_attnlrp_classes(x, classes=CLASSES)
    torch.cuda.synchronize()
    lrp.check()
    M = out.maps["attnlrp"]
    assert list(out.maps) == ["attnlrp"] and M.shape == (3, 3, 16) and M.dtype == torch.float32
    logits = model.head.Y.detach().clone()
    assert torch.equal(out.classes.cpu(), classes) and bits_equal(out.scores, logits.gather(1, classes.to(dev())))
    want = _single_maps(lrp, x, classes)
    for k in range(3):
        assert bits_equal(M[:, k], want[:, k]), k
    assert bits_equal(M[1, 0], M[1, 1])                        # the duplicate
    # [K] for every sample alike, a device tensor (not read back), TopAnd
    alike = lrp.generate_attnlrp_classes(x, classes=[7, 0])
    assert bits_equal(alike.maps["attnlrp"], _single_maps(lrp, x, torch.tensor([[7, 0]] * 3)))
    on_device = lrp.generate_attnlrp_classes(x, classes=classes.to(dev()))
    assert bits_equal(on_device.maps["attnlrp"], M)
    from transformer_explainability_amd.generators import TopAnd
    top = lrp.generate_attnlrp_classes(x, classes=TopAnd([4, 4, 4]))
    assert torch.equal(top.classes[:, 0], logits.argmax(-1)) and bits_equal(top.maps["attnlrp"][:, 0], lrp.generate_attnlrp(x))
    _record("vit_tiny_dim128.classes", bit_equal_to_single_calls=True, classes=CLASSES)


def test_vit_out_of_range_class_on_the_device_is_a_zero_seed(vit128):
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit128
    out = LRP(model).generate_attnlrp_classes(x, classes=torch.tensor([[1, 10], [7, -1], [4, 2]], device=dev()))
    assert out.classes.tolist() == [[1, -1], [7, -1], [4, 2]]
    assert bool(torch.isnan(out.scores[:2, 1]).all()) and not bool(torch.isnan(out.scores[:, 0]).any())
    M = out.maps["attnlrp"]
    assert not M[:2, 1].any() and bool(M[2, 1].any()) and bool(M[:, 0].any())


def test_vit_topk_chunk_and_full(vit128):
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit128
    lrp = LRP(model)
    out = lrp.generate_attnlrp_classes(x, topk=3)
    logits = model.head.Y.detach().clone()
    top = logits.topk(3, dim=-1)
    assert torch.equal(out.classes, top.indices) and bits_equal(out.scores, top.values)
    M = out.maps["attnlrp"]
    assert bits_equal(M, _single_maps(lrp, x, top.indices))
    for chunk in (1, 2, 3, 7):
        again = lrp.generate_attnlrp_classes(x, topk=3, chunk=chunk)
        assert bits_equal(again.maps["attnlrp"], M), chunk
        assert torch.equal(again.classes, out.classes) and bits_equal(again.scores, out.scores)
    full = lrp.generate_attnlrp_classes(x, topk=3, method="full")
    F = full.maps["attnlrp"]
    assert F.shape == (3, 3, 32, 32) and bits_equal(F, _single_maps(lrp, x, top.indices, method="full"))
    for chunk in (1, 2):
        assert bits_equal(lrp.generate_attnlrp_classes(x, topk=3, method="full", chunk=chunk).maps["attnlrp"], F), chunk
    # eps = 0 is allowed: damp is the identity
    assert bits_equal(lrp.generate_attnlrp_classes(x, topk=2, eps=0.0).maps["attnlrp"],
                      _single_maps(lrp, x, top.indices[:, :2], eps=0.0))
    torch.cuda.synchronize()
    lrp.check()


def test_vit_contrastive_seeds(vit128):
    """seeds [B,K,C] = onehot(c) - onehot(c'), and a second column with three non-zeros.  The head's product (10 classes) sees
    B rows in model.attnlrp(seed_k) and K B rows here: the same bits are asked where both run on te_gemm_x6_f32, whose order
    does not depend on the number of rows; on the stock GEMM each class is held to 2 x the fp32 restatement's error."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model, x, (m32, m64) = vit128
    lrp = LRP(model)
    B, C = 3, 10
    eye = torch.eye(C)
    c, d = torch.tensor([1, 7, 4]), torch.tensor([7, 0, 9])
    seeds = torch.stack([eye[c] - eye[d], eye[c] - 0.5 * eye[d] + 0.25 * eye[(d + 1) % C]], 1).to(dev())
    out = lrp.generate_attnlrp_classes(x, seeds=seeds)
    M = out.maps["attnlrp"]
    logits = model.head.Y.detach().clone()
    assert out.classes is None and M.shape == (3, 2, 16)
    assert bits_equal(out.scores, (seeds.permute(1, 0, 2).contiguous() * logits).sum(-1).t().contiguous())
    [single] = [lrp.generate_attnlrp_classes(x, seeds=seeds[:, 0].contiguous()).maps["attnlrp"]]      # [B,C]: K = 1
    assert single.shape == (3, 1, 16)
    with torch.no_grad():
        model(x)
        same_caches = torch.stack([model.attnlrp(seeds[:, k].contiguous()) for k in range(2)], 1)
    head_x6 = ops.gemm_x6_supported(B, C, 128) and ops.gemm_x6_supported(2 * B, C, 128)
    equal = bits_equal(M, same_caches) and bits_equal(single, same_caches[:, :1])
    _record("vit_tiny_dim128.seeds", head_product_on_x6=bool(head_x6), bit_equal_to_chain_per_seed=bool(equal))
    if head_x6:
        assert equal
    for k in range(2):
        R32 = sref.vit_attnlrp_seed(m32, x, seeds[:, k])[0]
        R64 = sref.vit_attnlrp_seed(m64, x.double(), seeds[:, k].double())[0]
        _assert_within_twice(f"vit_tiny_dim128.seeds.k{k}", M[:, k], R32, R64)


def test_vit_head_dim_48_stock_products_within_twice_the_restatement():
    """dim 96, 2 heads (D = 48): torch attention and stock GEMMs, whose order may depend on the number of rows: no bits are
    claimed, every class is held to the bar of the single call."""
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model, m32, m64 = _tiny_vit(96, 4)
    assert not ops._lib.load().te_attention_strided_supported(17, 48)
    assert not any(ops.gemm_x6_supported(T, k, m) for T in (51, 153) for k, m in ((288, 96), (96, 96), (384, 96), (96, 384)))
    x = rnd((3, 3, 32, 32), 41).to(dev())
    classes = torch.tensor(CLASSES)
    M = LRP(model).generate_attnlrp_classes(x, classes=CLASSES).maps["attnlrp"]
    assert M.shape == (3, 3, 16)
    for k in range(3):
        _assert_within_twice(f"vit_tiny_dim96.k{k}", M[:, k], ref.vit_attnlrp(m32, x, index=classes[:, k])[0],
                             ref.vit_attnlrp(m64, x.double(), index=classes[:, k])[0])


def test_bert_classes_have_the_bits_of_the_single_calls():
    from transformer_explainability_amd.generators import Generator
    model = _tiny_bert()[0]
    ids, mask = _bert_inputs()
    gen = Generator(model)
    classes = torch.tensor([[1, 0]] * 3)
    out = gen.generate_attnlrp_classes(ids, mask, classes=[[1, 0]] * 3)
    torch.cuda.synchronize()
    gen.check()
    M = out.maps["attnlrp"]
    logits = model.classifier.Y.detach().clone()
    assert M.shape == (3, 2, 12) and torch.equal(out.classes.cpu(), classes)
    assert bits_equal(out.scores, logits.gather(1, classes.to(dev())))
    for k in range(2):
        assert bits_equal(M[:, k], gen.generate_attnlrp(ids, mask, index=classes[:, k])), k
    for chunk in (1, 2):
        assert bits_equal(gen.generate_attnlrp_classes(ids, mask, topk=2, chunk=chunk).maps["attnlrp"],
                          gen.generate_attnlrp_classes(ids, mask, topk=2).maps["attnlrp"]), chunk
    _record("bert_tiny.classes", bit_equal_to_single_calls=True)


def test_bf16_models_have_the_bits_of_the_single_calls(vit128):
    from transformer_explainability_amd.generators import LRP, Generator
    model = _tiny_vit(128, 3)[0].to(BF16)
    x = vit128[1].to(BF16)
    lrp = LRP(model)
    classes = torch.tensor(CLASSES)
    out = lrp.generate_attnlrp_classes(x, classes=CLASSES)
    M = out.maps["attnlrp"]
    assert M.dtype == torch.float32 and out.scores.dtype == torch.float32 and M.shape == (3, 3, 16)
    assert bits_equal(M, _single_maps(lrp, x, classes))
    assert bits_equal(lrp.generate_attnlrp_classes(x, classes=CLASSES, chunk=2).maps["attnlrp"], M)
    F = lrp.generate_attnlrp_classes(x, classes=CLASSES, method="full").maps["attnlrp"]
    assert bits_equal(F, _single_maps(lrp, x, classes, method="full"))
    # fp32 seeds on a bf16 model: G is fp32
    eye = torch.eye(10, device=dev())
    seeded = lrp.generate_attnlrp_classes(x, seeds=eye[classes[:, 0].to(dev())])
    assert bits_equal(seeded.maps["attnlrp"][:, 0], M[:, 0])
    bert = _tiny_bert()[0].to(BF16)
    ids, mask = _bert_inputs()
    gen = Generator(bert)
    labels = torch.tensor([[1, 0]] * 3)
    Mb = gen.generate_attnlrp_classes(ids, mask, classes=labels).maps["attnlrp"]
    assert Mb.shape == (3, 2, 12) and Mb.dtype == torch.float32
    for k in range(2):
        assert bits_equal(Mb[:, k], gen.generate_attnlrp(ids, mask, index=labels[:, k])), k
    torch.cuda.synchronize()
    lrp.check()
    gen.check()
    _record("bf16.classes", bit_equal_to_single_calls=True)


def test_eager_and_graph_replay_give_the_same_bits(vit128):
    from transformer_explainability_amd.generators import LRP, GraphedCall
    model, x, _ = vit128
    lrp = LRP(model)
    keep = lambda o: (o.classes.clone(), o.scores.clone(), o.maps["attnlrp"].clone())      # noqa: E731
    eager = keep(lrp.generate_attnlrp_classes(x, topk=2))
    graphed = GraphedCall(lambda inp: lrp.generate_attnlrp_classes(inp, topk=2), (x,))
    first = keep(graphed(x))
    x2 = rnd((3, 3, 32, 32), 77).to(dev())
    second, eager2 = keep(graphed(x2)), keep(lrp.generate_attnlrp_classes(x2, topk=2))
    again = keep(graphed(x))
    for got, want in ((first, eager), (second, eager2), (again, first)):
        assert torch.equal(got[0], want[0]) and bits_equal(got[1], want[1]) and bits_equal(got[2], want[2])
    torch.cuda.synchronize()
    lrp.check()
