"""-m gpu: several classes per input from one forward pass.  ops.class_targets (te_class_targets_*: device top-K, gather,
one-hot seeds) against torch.topk and a host sort by (te_key descending, index ascending); LRP.generate_classes /
Generator.generate_classes against the single calls, each on a fresh forward pass -- the kernels are deterministic and a tail
reads only what the pass left on the model, so every comparison in this file is exact (NaN positions included)."""
import numpy as np
import pytest
import torch

from gpu_util import dev
from oracle.ref_harness import seeded_randn
from test_generate_all_host import BERT_METHODS, LRP_METHODS, _single_bert, _single_vit
from test_gpu_generate_all import F64_METHODS, bert_model, same, vit_model

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DTYPES = {"f32": torch.float32, "bf16": BF, "f64": torch.float64}


# ------------------------------------------------------------------------------------------------ ops.class_targets
def host_keys(rows):
    """te_key (and its 64-bit twin) of a CPU tensor [B,C], as unsigned integers: a > b as numbers, -0 == +0, NaN largest."""
    if rows.dtype == torch.float64:
        u = rows.contiguous().numpy().view(np.uint64).copy()
        sign, flip = np.uint64(1) << np.uint64(63), np.uint64(0xffffffffffffffff)
    else:
        u = rows.float().contiguous().numpy().view(np.uint32).copy()
        sign, flip = np.uint32(0x80000000), np.uint32(0xffffffff)
    u[u == sign] = 0
    return np.where(u & sign != 0, u ^ flip, u | sign)


def host_topk(rows, K):
    keys = host_keys(rows)
    idx = np.arange(keys.shape[1])
    return torch.from_numpy(np.stack([np.lexsort((idx, ~k))[:K] for k in keys]).astype(np.int64))


def distinct_rows(B, C, dtype, seed):
    """Tie-free rows, also in bf16: C distinct bit patterns (positive normal values), shuffled, every other one negated."""
    g = torch.Generator().manual_seed(seed)
    if dtype == BF:
        vals = (torch.arange(C, dtype=torch.int32) + 0x3000).to(torch.int16).view(BF).float()
    else:
        vals = (torch.arange(C, dtype=torch.float64) + 1.0) * 0.37
    rows = torch.stack([vals[torch.randperm(C, generator=g)] for _ in range(B)])
    rows[:, 1::2] *= -1
    return rows.to(dtype)


def special_rows(kind, B, C, dtype, seed):
    rows = distinct_rows(B, C, dtype, seed)
    g = torch.Generator().manual_seed(seed + 1)
    if kind == "equal":
        rows[:] = 1.5
    elif kind == "pairs":
        rows = torch.stack([((torch.arange(C) // 2).double() - C // 4)[torch.randperm(C, generator=g)] for _ in range(B)]).to(dtype)
    elif kind == "zeros_infs":
        for b in range(B):
            slots = torch.randperm(C, generator=g)[:8]
            for s, v in zip(slots.tolist(), (0.0, -0.0, float("inf"), -float("inf"), -0.0, 0.0, float("inf"), -float("inf"))):
                rows[b, s] = v
    elif kind == "nan":
        for b in range(B):
            rows[b, int(torch.randint(C, (1,), generator=g))] = float("nan")
    return rows


def placed(rows, layout):
    """The rows on the device as fresh rows, as rows of a wider buffer (ld > C), or starting at an odd element of one."""
    B, C = rows.shape
    if layout == "fresh":
        return rows.to(dev())
    off = 1 if layout == "odd" else 0
    buf = torch.full((B, C + 5 + off), -3.0, dtype=rows.dtype).to(dev())
    buf[:, off:off + C] = rows.to(dev())
    view = buf[:, off:off + C]
    assert view.stride(0) > C and (view.data_ptr() // view.element_size()) % 2 == off
    return view


GUARD = 5            # an odd number of guard cells: the seed rows start off the 16-byte grid


def guarded(shape, dtype):
    n = int(np.prod(shape))
    fill = -777 if dtype == torch.int64 else float("nan")
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
    return flat, flat[GUARD:GUARD + n].view(shape)


def guards_intact(flat, dtype):
    edge = torch.cat([flat[:GUARD], flat[-GUARD:]])
    return bool((edge == -777).all()) if dtype == torch.int64 else bool(torch.isnan(edge).all())


def run_targets(logits, classes=None, topk=None):
    from transformer_explainability_amd import ops
    B, C = logits.shape
    K = topk if classes is None else classes.shape[1]
    rel = ops.relevance_dtype(logits.dtype)
    bufs = [guarded((B, K), torch.int64), guarded((B, K), rel), guarded((K, B, C), rel)]
    out = ops.class_targets(logits, classes=classes, topk=topk, out=tuple(v for _, v in bufs))
    torch.cuda.synchronize()
    for (flat, _), dt in zip(bufs, (torch.int64, rel, rel)):
        assert guards_intact(flat, dt)
    return out


def expected(rows, cls):
    """(scores, seeds) of the classes ``cls`` [B,K] (all in range) on the CPU rows."""
    from transformer_explainability_amd import ops
    rel = ops.relevance_dtype(rows.dtype)
    B, C = rows.shape
    seeds = torch.zeros(cls.shape[1], B, C, dtype=rel).scatter_(2, cls.t().unsqueeze(-1), 1.0)
    return rows.to(rel).gather(1, cls), seeds


def assert_targets(got, rows, cls):
    scores, seeds = expected(rows, cls)
    assert torch.equal(got[0].cpu(), cls)
    assert same(got[1].cpu(), scores)
    assert torch.equal(got[2].cpu(), seeds)


@pytest.mark.parametrize("C", [1, 2, 10, 1000, 1001, 4097])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_class_targets(dt, C):
    dtype = DTYPES[dt]
    Ks = sorted({k for k in (1, 2, 5) if k <= C} | ({C} if C <= 10 else set()))
    for B in (1, 3):
        for layout in ("fresh", "wide") + (("odd",) if dtype == BF else ()):
            rows = distinct_rows(B, C, dtype, 10 * C + B)
            logits = placed(rows, layout)
            for K in Ks:
                got = run_targets(logits, topk=K)
                want = torch.topk(rows.double(), K, dim=-1).indices            # tie-free: torch.topk's indices
                assert torch.equal(want, host_topk(rows, K))
                assert_targets(got, rows, want)
            # explicit classes, duplicates included
            g = torch.Generator().manual_seed(C + B)
            cls = torch.randint(C, (B, 4), generator=g)
            cls[:, 3] = cls[:, 0]
            assert_targets(run_targets(logits, classes=cls.to(dev())), rows, cls)
        for kind in ("equal", "pairs", "zeros_infs", "nan"):
            if kind == "zeros_infs" and C < 8:
                continue
            rows = special_rows(kind, B, C, dtype, 20 * C + B)
            for K in Ks:
                assert_targets(run_targets(placed(rows, "wide"), topk=K), rows, host_topk(rows, K))
    if C >= 2:
        # one class of a DEVICE tensor out of range: -1 / NaN / a zero row, every other output intact
        rows = distinct_rows(3, C, dtype, 7)
        cls = torch.tensor([[0, 1, 1], [1, C, 0], [0, 0, -2 if C > 2 else 1]])
        got = run_targets(placed(rows, "fresh"), classes=cls.to(dev()))
        ok = (cls >= 0) & (cls < C)
        scores, seeds = expected(rows, cls.clamp(0, C - 1))
        assert torch.equal(got[0].cpu(), torch.where(ok, cls, torch.full_like(cls, -1)))
        assert same(got[1].cpu(), torch.where(ok, scores, torch.full_like(scores, float("nan"))))
        assert torch.equal(got[2].cpu(), seeds * ok.t().unsqueeze(-1).to(seeds.dtype))


def test_class_targets_refusals():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    logits = torch.zeros(2, 10, device=dev())
    for k in (0, 11):
        with pytest.raises(ValueError, match="topk"):
            ops.class_targets(logits, topk=k)
    with pytest.raises(ValueError, match="exactly one"):
        ops.class_targets(logits)
    with pytest.raises(TeError, match="float16"):
        ops.class_targets(logits.half(), topk=1)
    with pytest.raises(TeError, match="int64"):
        ops.class_targets(logits, classes=torch.zeros(2, 1, dtype=torch.int32, device=dev()))
    with pytest.raises(TeError, match="CPU"):
        ops.class_targets(logits.cpu(), topk=1)
    with pytest.raises(ValueError, match=r"\[0, 10\)"):
        ops.host_classes([[1, 10], [0, 0]], 2, 10, dev())
    lib = ops._lib.load()
    wide = torch.zeros(1, 2048, device=dev())
    assert lib.te_class_targets_f32(wide.data_ptr(), 2048, 1, 2048, 1025, None, wide.data_ptr(), wide.data_ptr(), None,
                                    None) == ops._lib.TE_ERR_UNSUPPORTED       # top-K beyond 1024
    assert lib.te_class_targets_f32(wide.data_ptr(), (1 << 20) + 1, 1, (1 << 20) + 1, 1, None, wide.data_ptr(),
                                    wide.data_ptr(), None, None) == ops._lib.TE_ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ equality
VIT_CLASSES = {"tiny": [[3, 8, 3], [8, 0, 5]], "w128": [[1, 15, 1], [15, 6, 0], [6, 6, 2]]}
BERT_CLASSES = [[1, 0, 1], [0, 0, 1]]
_REFS = {}


def vit_classes(kind):
    return torch.tensor(VIT_CLASSES["tiny" if kind == "tiny" else "w128"], device=dev())


def vit_methods(kind):
    return F64_METHODS if kind == "w128-f64" else LRP_METHODS


def vit_refs(kind, start_layer=1):
    """Per class slot, the single calls, each on a fresh forward pass; computed once and shared (clones)."""
    key = (kind, start_layer)
    if key not in _REFS:
        model, x, _ = vit_model(kind)
        cls = vit_classes(kind)
        _REFS[key] = [{m: _single_vit(model, x, m, cls[:, k], False, start_layer).clone() for m in vit_methods(kind)}
                      for k in range(cls.shape[1])]
        torch.cuda.synchronize()
    return _REFS[key]


def assert_maps(got, ref, methods, what):
    assert tuple(got.maps) == tuple(methods)
    for m in methods:
        for k in range(len(ref)):
            assert same(got.maps[m][:, k], ref[k][m]), (what, m, k)


@pytest.mark.parametrize("kind", ["tiny", "w128-f32", "w128-bf16", "w128-f64"])
def test_vit_generate_classes_equals_single_calls(kind):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit_model(kind)
    cls, methods, ref = vit_classes(kind), vit_methods(kind), vit_refs(kind)
    got = LRP(model).generate_classes(x, classes=cls, methods=methods, start_layer=1)
    torch.cuda.synchronize()
    assert_maps(got, ref, methods, kind)
    rel = ops.relevance_dtype(x.dtype)
    with torch.no_grad():
        logits = model(x)
    assert torch.equal(got.classes, cls) and got.scores.dtype == rel and torch.equal(got.scores, logits.to(rel).gather(1, cls))
    assert got.maps["transformer_attribution"].dtype == rel
    for sub in (("last_layer_attn", "attn_rollout"), ("attn_gradcam",), ("last_layer", "last_layer_attn")):
        assert_maps(LRP(model).generate_classes(x, classes=cls, methods=sub, start_layer=1), ref, sub, (kind, sub))
    # topk = the classes torch.topk names on the logits of a plain forward pass
    want = torch.topk(logits.to(rel), 2).indices
    top = LRP(model).generate_classes(x, topk=2, methods=("transformer_attribution", "attn_gradcam"), start_layer=1)
    exp = LRP(model).generate_classes(x, classes=want, methods=("transformer_attribution", "attn_gradcam"), start_layer=1)
    assert torch.equal(top.classes, want) and torch.equal(top.scores, exp.scores)
    assert all(same(top.maps[m], exp.maps[m]) for m in exp.maps)
    assert same(top.maps["transformer_attribution"][:, 0], _single_vit(model, x, "transformer_attribution", None, False, 1))
    LRP(model).check()


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_bert_generate_classes_equals_single_calls(dtype):
    from transformer_explainability_amd.generators import Generator
    model, ids, mask, _ = bert_model(dtype)
    cls = torch.tensor(BERT_CLASSES, device=dev())
    ref = [{m: _single_bert(Generator(model), ids, mask, m, cls[:, k], 1, 1).clone() for m in BERT_METHODS} for k in range(3)]
    for opts in ({}, {"prune": True}, {"overlap_backward": True}):
        for sub in (BERT_METHODS, ("attn_last_layer", "rollout"), ("LRP", "LRP_last_layer", "attn_gradcam")):
            got = Generator(model, **opts).generate_classes(ids, mask, classes=cls, methods=sub, start_layer=1,
                                                            rollout_start_layer=1)
            torch.cuda.synchronize()
            assert_maps(got, ref, sub, (dtype, opts))
    with torch.no_grad():
        logits = model(input_ids=ids, attention_mask=mask)[0].float()
    top = Generator(model).generate_classes(ids, mask, topk=2, start_layer=1)
    want = torch.topk(logits, 2).indices
    assert torch.equal(top.classes, want) and top.scores.dtype == torch.float32
    assert torch.equal(top.scores, logits.gather(1, want))
    assert same(top.maps["LRP"][:, 0], _single_bert(Generator(model), ids, mask, "LRP", None, 1, 1))
    Generator(model).check()
    assert same(Generator(model).generate_LRP(ids, mask, index=cls[:, 0], start_layer=1), ref[0]["LRP"])


# ------------------------------------------------------------------------------------------------ seeds
@pytest.mark.parametrize("kind", ["w128-f32", "w128-bf16", "w128-f64"])
def test_seeds(kind):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import LRP, _attention_gradients
    model, x, _ = vit_model(kind)
    cls, ref = vit_classes(kind), vit_refs(kind)
    rel = ops.relevance_dtype(x.dtype)
    methods = ("transformer_attribution", "last_layer", "attn_gradcam")
    onehot = torch.zeros(3, 3, 16, dtype=rel, device=dev()).scatter_(2, cls.unsqueeze(-1), 1.0)
    got = LRP(model).generate_classes(x, seeds=onehot, methods=methods, start_layer=1)
    assert got.classes is None
    assert_maps(got, ref, methods, kind)
    # contrastive: the same pass assembled by hand from the existing pieces
    seed = onehot[:, 0] - onehot[:, 1]
    got = LRP(model).generate_classes(x, seeds=seed, start_layer=1)
    with ops.gelu_backward_plane_handoff():
        out = model(x)
    _attention_gradients(torch.sum(seed * out), [blk.attn for blk in model.blocks])
    want = model.relprop(seed, method="transformer_attribution", start_layer=1, alpha=1)
    assert same(got.maps["transformer_attribution"][:, 0], want)
    assert torch.equal(got.scores[:, 0], (seed * out.detach().to(rel)).sum(-1))
    assert not same(want, ref[0]["transformer_attribution"])
    with pytest.raises(TeError, match="float16"):
        LRP(model).generate_classes(x, seeds=seed.half())


# ------------------------------------------------------------------------------------------------ options
@pytest.mark.parametrize("kind", ["w128-f32", "w128-bf16"])
def test_on_fused_producers(kind):
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit_model(kind)
    cls = vit_classes(kind)
    saved = ops.USE_FUSED_PRODUCERS
    ops.USE_FUSED_PRODUCERS = True
    try:
        # the single calls on the producer kernels are their own reference
        ref = [{m: _single_vit(model, x, m, cls[:, k], False, 1).clone() for m in LRP_METHODS} for k in range(3)]
        assert model.blocks[0].attn._fused_anchor is not None           # (the blocks did run on the producer kernels)
        for sub in (LRP_METHODS, ("attn_gradcam",)):
            got = LRP(model).generate_classes(x, classes=cls, methods=sub, start_layer=1)
            assert model.blocks[0].attn._fused_anchor is not None
            assert_maps(got, ref, sub, kind)
        LRP(model).check()
    finally:
        ops.USE_FUSED_PRODUCERS = saved


@pytest.mark.parametrize("opts", [{"overlap_backward": True}, {"prune": True}, {"overlap_backward": True, "prune": True}])
@pytest.mark.parametrize("kind", ["tiny", "w128-f32"])
def test_overlap_and_prune(kind, opts):
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit_model(kind)
    cls, ref = vit_classes(kind), vit_refs(kind)
    for sub in (LRP_METHODS, ("transformer_attribution", "last_layer", "attn_gradcam", "last_layer_attn"), ("full", "rollout")):
        got = LRP(model, **opts).generate_classes(x, classes=cls, methods=sub, start_layer=1)
        torch.cuda.synchronize()
        assert_maps(got, ref, sub, (kind, opts))
    assert model.prune_below_start_layer is False


@pytest.mark.parametrize("kind", ["tiny", "w128-bf16"])
def test_head_mask(kind):
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit_model(kind)
    cls = vit_classes(kind)
    L, H = len(model.blocks), model.blocks[0].attn.num_heads
    hm = torch.ones(L, H)
    hm[0, 0], hm[L - 1, H - 1] = 0.0, 0.5
    methods = ("transformer_attribution", "last_layer", "last_layer_attn")
    got = LRP(model).generate_classes(x, classes=cls, methods=methods + ("attn_gradcam",), start_layer=1, head_mask=hm)
    for k in range(3):
        for m in methods:
            assert same(got.maps[m][:, k], LRP(model).generate_LRP(x, index=cls[:, k], method=m, start_layer=1, head_mask=hm)), (m, k)
        want = LRP(model).generate_all(x, ("attn_gradcam",), index=cls[:, k], head_mask=hm)["attn_gradcam"]
        assert same(got.maps["attn_gradcam"][:, k], want)
    assert not same(got.maps["transformer_attribution"][:, 0], vit_refs(kind)[0]["transformer_attribution"])


# ------------------------------------------------------------------------------------------------ state
def test_state_left_on_the_model():
    from transformer_explainability_amd import ops, rules
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit_model("w128-f32")
    cls = vit_classes("w128-f32")
    lrp = LRP(model)
    lrp.generate_LRP(x, index=cls[:, 2], start_layer=1)
    want = [(b.attn.get_attn_cam().clone(), b.attn.get_attn_gradients().clone()) for b in model.blocks]
    lrp.generate_classes(x, classes=cls, start_layer=1)
    lrp.check()
    for b, (cam, grad) in zip(model.blocks, want):                   # the accessors hold the LAST class's tensors
        assert torch.equal(b.attn.get_attn_cam(), cam) and torch.equal(b.attn.get_attn_gradients(), grad)
    linears = [m for m in model.modules() if isinstance(m, rules.Linear)]
    assert all("x_abs_planes" not in rules.x6_cache(m) for m in linears) and ops._X_ABS_KEPT is None


def test_every_class_takes_the_planes_of_the_forward_product():
    """A batch of 16 (T = 272 rows: the x6 forward products and rules engage on the 128-wide model) on the producer kernels:
    the rule of every class receives the planes of |X| its layer's forward product left, and none is left afterwards."""
    from transformer_explainability_amd import ops, rules
    from transformer_explainability_amd.generators import LRP
    model, _, _ = vit_model("w128-f32")
    x = seeded_randn((16, 3, 64, 64), 5).to(dev())
    cls = torch.tensor([[1, 15, 1]], device=dev()).expand(16, 3).contiguous()
    linears = [m for m in model.modules() if isinstance(m, rules.Linear)]
    saved = (ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.take_x_abs_planes)
    taken = []

    def counting(cache, X, T, K):
        planes = saved[2](cache, X, T, K)
        taken.append(planes is not None)
        return planes
    ops.USE_FUSED_PRODUCERS, ops.X6_GEMM = True, "all"
    try:
        ref = [LRP(model).generate_LRP(x, index=cls[:, k], start_layer=0).clone() for k in range(3)]
        ops.take_x_abs_planes = counting
        LRP(model).generate_LRP(x, index=cls[:, 0], start_layer=0)
        single = list(taken)
        del taken[:]
        got = LRP(model).generate_classes(x, classes=cls, start_layer=0)
        for k in range(3):
            assert same(got.maps["transformer_attribution"][:, k], ref[k]), k
        takes = [ops.rule_takes_abs_planes(16 * 17, m.in_features, m.out_features) for m in linears]
        if any(takes) and any(single):
            assert taken == single * 3                               # every class got what a single call gets
        else:
            print("no Linear rule of w128-f32 at batch 16 reads the planes of |X| (rule_takes_abs_planes is false for every "
                  "layer): the per-class count is not asserted")
        assert all("x_abs_planes" not in rules.x6_cache(m) for m in linears)
        LRP(model).check()
    finally:
        ops.USE_FUSED_PRODUCERS, ops.X6_GEMM, ops.take_x_abs_planes = saved


# ------------------------------------------------------------------------------------------------ capture
def test_captured_topk_replays_equal_eager():
    """The device-side selection makes the call capturable: one capture, two replays on different batches."""
    from transformer_explainability_amd.generators import LRP, GraphedCall
    model, x, _ = vit_model("w128-f32")
    lrp = LRP(model)
    x2 = seeded_randn((3, 3, 64, 64), 9).to(dev())
    want = {}
    for name, inp in (("x", x), ("x2", x2)):
        r = lrp.generate_classes(inp, topk=2, start_layer=1)
        want[name] = (r.classes.clone(), r.scores.clone(), r.maps["transformer_attribution"].clone())
    assert not torch.equal(want["x"][2], want["x2"][2])
    call = GraphedCall(lambda inp: lrp.generate_classes(inp, topk=2, start_layer=1), (x,))
    for name, inp in (("x2", x2), ("x", x)):
        r = call(inp)
        torch.cuda.synchronize()
        assert torch.equal(r.classes, want[name][0]) and torch.equal(r.scores, want[name][1])
        assert same(r.maps["transformer_attribution"], want[name][2]), name
    lrp.check()


# ------------------------------------------------------------------------------------------------ sweep
def test_sweep_tuple_vis_class_equals_the_single_class_sweeps():
    from test_sweep import ToyImages, _generators
    from test_generate_all_host import _Counts, _RecordingStore
    from transformer_explainability_amd.sweep import SaliencySweepAll, shard_batches
    lrp, orig, base = _generators(dev())
    methods = ("transformer_attribution", "attn_gradcam")
    ds = ToyImages(5)                                # two batches: 3 + 2
    single = {}
    for v in ("top", "target"):
        st = {m: _RecordingStore([], m) for m in methods}
        SaliencySweepAll(methods, lrp=lrp, baselines=base, vis_class=v, device=dev()).run(shard_batches(ds, 3)[0], st)
        for m in methods:
            single[m, v] = st[m].vis
    stores = {k: _RecordingStore([], k) for k in single}
    sw = SaliencySweepAll(methods, lrp=lrp, baselines=base, vis_class=("top", "target"), device=dev())
    with _Counts(lrp.model) as c:
        sw.run(shard_batches(ds, 3)[0], stores)
    assert c.forward == 2 and c.relprop == 4         # one forward pass per batch, one chain per class
    assert len(stores) == 4
    for k, st in stores.items():
        assert len(st.vis) == 2
        for a, b in zip(st.vis, single[k]):
            assert same(a, b), k
