"""-m gpu: one forward and backward pass for all explanation methods of a batch.  Every entry of LRP.generate_all /
Generator.generate_all must be torch.equal (NaN positions included: attn_gradcam's min-max is 0 / 0 on an all-clamped map) to
the single call made on a fresh forward pass -- the kernels are deterministic and a tail reads only what the pass left on the
model, so no tolerance is involved anywhere in this file.  Also: the work actually done (counted), the sweep and the
rationale test built on the one-pass calls, and the state the calls leave on the model."""
import numpy as np
import pytest
import torch

from gpu_util import dev
from oracle.ref_harness import seeded_randn
from test_generate_all_host import BERT_METHODS, LRP_METHODS, _Counts, _single_bert, _single_vit

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64_METHODS = tuple(m for m in LRP_METHODS if m != "full")
VIT_SUBSETS = (("last_layer_attn", "attn_rollout"),                       # forward only
               ("transformer_attribution", "last_layer", "attn_gradcam"))
BERT_SUBSETS = (("attn_last_layer", "rollout"),                           # forward only
                ("LRP", "LRP_last_layer", "attn_gradcam"))


def same(a, b):
    a, b = a.detach(), b.detach()
    return (a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b))
            and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))


# ------------------------------------------------------------------------------------------------ models (built once)
_MODELS = {}


def vit_model(kind):
    """"tiny": the 3-block ViT of tests/golden/vit_tiny.npz (head dim 16: the fallback kernels); "w128-<dtype>": the 2-block
    128-wide model with 2 heads of 64 (the MFMA kernels) at batch 3."""
    if kind in _MODELS:
        return _MODELS[kind]
    from conftest import load_golden
    from transformer_explainability_amd import vit
    if kind == "tiny":
        g = load_golden("vit_tiny.npz")
        model = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=10,
                                      qkv_bias=True).eval()
        model.load_state_dict({k[6:]: v for k, v in g.items() if k.startswith("state.")})
        model.to(dev())
        x, index = g["x"].to(dev()), torch.tensor([3, 8], device=dev())
    else:
        dtype = {"w128-f32": torch.float32, "w128-bf16": BF, "w128-f64": torch.float64}[kind]
        torch.manual_seed(0)
        model = vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=16,
                                      qkv_bias=True).eval().to(dev()).to(dtype)
        x, index = seeded_randn((3, 3, 64, 64), 2).to(dev()).to(dtype), torch.tensor([1, 15, 6], device=dev())
    _MODELS[kind] = (model, x, index)
    return _MODELS[kind]


def bert_model(dtype):
    key = ("bert", dtype)
    if key in _MODELS:
        return _MODELS[key]
    from conftest import load_golden
    from transformer_explainability_amd import bert
    g = load_golden("bert_tiny.npz")
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=64, num_hidden_layers=3, num_attention_heads=4,
                              intermediate_size=128, max_position_embeddings=40, num_labels=2)
    model = bert.BertForSequenceClassification(cfg).eval()
    model.load_state_dict({k[6:]: v for k, v in g.items() if k.startswith("state.")})
    model.to(dev()).to(dtype)
    ids = g["input_ids"].long().to(dev())
    mask = torch.ones(ids.shape, device=dev())
    mask[1, ids.shape[1] - 5:] = 0                   # one sample padded
    _MODELS[key] = (model, ids, mask, torch.tensor([1, 0], device=dev()))
    return _MODELS[key]


_REFS = {}


def vit_refs(kind, use_index, methods=LRP_METHODS, is_ablation=False, start_layer=1):
    """The single calls, each on a fresh forward pass; computed once and shared (clones: a later call cannot touch them)."""
    key = (kind, use_index, methods, is_ablation, start_layer)
    if key not in _REFS:
        model, x, index = vit_model(kind)
        idx = index if use_index else None
        _REFS[key] = {m: _single_vit(model, x, m, idx, is_ablation, start_layer).clone() for m in methods}
        torch.cuda.synchronize()
    return _REFS[key]


def check_vit(kind, use_index, subsets, methods=LRP_METHODS, is_ablation=False, start_layer=1, **opts):
    from transformer_explainability_amd.generators import LRP
    model, x, index = vit_model(kind)
    ref = vit_refs(kind, use_index, methods, is_ablation, start_layer)
    for sub in subsets:
        got = LRP(model, **opts).generate_all(x, sub, index=index if use_index else None, is_ablation=is_ablation,
                                              start_layer=start_layer)
        torch.cuda.synchronize()
        assert tuple(got) == tuple(sub)
        for m in sub:
            assert same(got[m], ref[m]), (kind, m, sub, use_index, opts)


# ------------------------------------------------------------------------------------------------ equality
@pytest.mark.parametrize("use_index", [False, True])
@pytest.mark.parametrize("kind", ["tiny", "w128-f32", "w128-bf16"])
def test_vit_generate_all_equals_single_calls(kind, use_index):
    check_vit(kind, use_index, (LRP_METHODS,) + VIT_SUBSETS)
    from transformer_explainability_amd.generators import LRP
    LRP(vit_model(kind)[0]).check()


@pytest.mark.parametrize("kind", ["w128-f32", "w128-bf16"])
def test_vit_generate_all_ablation_and_start_layer_0(kind):
    """is_ablation=True: last_layer / second_layer multiply attn_cam by the block's gradient (the table's ablation rows)."""
    check_vit(kind, True, (LRP_METHODS, ("last_layer",), ("second_layer", "last_layer_attn")), is_ablation=True, start_layer=0)


@pytest.mark.parametrize("kind", ["w128-f32", "w128-bf16"])
def test_vit_generate_all_on_fused_producers(kind):
    from transformer_explainability_amd import ops
    model, x, index = vit_model(kind)
    saved = ops.USE_FUSED_PRODUCERS
    ops.USE_FUSED_PRODUCERS = True
    try:
        # the single calls on the producer kernels are their own reference (not shared with the stock-forward tests)
        ref = {m: _single_vit(model, x, m, index, False, 1).clone() for m in LRP_METHODS}
        assert model.blocks[0].attn._fused_anchor is not None           # (the blocks did run on the producer kernels)
        from transformer_explainability_amd.generators import LRP
        for sub in (LRP_METHODS,) + VIT_SUBSETS + (("attn_gradcam",),):
            got = LRP(model).generate_all(x, sub, index=index, start_layer=1)
            for m in sub:
                assert same(got[m], ref[m]), (kind, m, sub)
        LRP(model).check()
    finally:
        ops.USE_FUSED_PRODUCERS = saved


@pytest.mark.parametrize("opts", [{"overlap_backward": True}, {"prune": True}, {"overlap_backward": True, "prune": True}])
@pytest.mark.parametrize("kind", ["tiny", "w128-f32"])
def test_vit_generate_all_overlap_and_prune(kind, opts):
    """The options give the plain calls' bits (the references are the plain single calls); with prune, the second subset is
    served pruned (every method reads blocks >= start_layer), the full set is not."""
    check_vit(kind, False, (LRP_METHODS,) + VIT_SUBSETS + (("full", "rollout"),), **opts)


def test_vit_generate_all_fp64():
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import LRP
    model, x, index = vit_model("w128-f64")
    check_vit("w128-f64", True, (F64_METHODS, ("last_layer_attn", "attn_rollout"), ("grad", "attn_gradcam")),
              methods=F64_METHODS)
    got = LRP(model).generate_all(x, ("transformer_attribution", "last_layer"), start_layer=1)
    assert all(v.dtype == torch.float64 for v in got.values())
    with _Counts(model) as c, pytest.raises(TeError, match="float64"):
        LRP(model).generate_all(x, ("grad", "full"))
    assert c.forward == 0                            # refused before the forward pass


def test_fp16_is_refused_before_the_forward_pass():
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP
    model = vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=16,
                                  qkv_bias=True).eval().to(dev()).half()
    x = seeded_randn((1, 3, 64, 64), 2).to(dev()).half()
    for sub in (("transformer_attribution",), ("last_layer_attn", "attn_rollout")):
        with _Counts(model) as c, pytest.raises(TeError, match="bfloat16"):
            LRP(model).generate_all(x, sub)
        assert c.forward == 0
    with pytest.raises(ValueError):
        LRP(model).generate_all(x, ("transformer_attribution", "no_such_method"))


@pytest.mark.parametrize("use_index", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_bert_generate_all_equals_single_calls(dtype, use_index):
    from transformer_explainability_amd.generators import Generator
    model, ids, mask, index = bert_model(dtype)
    idx = index if use_index else None
    ref = {m: _single_bert(Generator(model), ids, mask, m, idx, 1, 1).clone() for m in BERT_METHODS}
    for opts in ({}, {"prune": True}, {"overlap_backward": True}):
        for sub in (BERT_METHODS,) + BERT_SUBSETS:
            got = Generator(model, **opts).generate_all(ids, mask, sub, index=idx, start_layer=1, rollout_start_layer=1)
            torch.cuda.synchronize()
            assert tuple(got) == tuple(sub)
            for m in sub:
                assert same(got[m], ref[m]), (m, sub, opts, use_index)
    Generator(model).check()
    # nothing spills over
    assert same(Generator(model).generate_LRP(ids, mask, index=idx, start_layer=1), ref["LRP"])


# ------------------------------------------------------------------------------------------------ work done
def test_vit_work_done():
    from transformer_explainability_amd.generators import LRP
    model, x, _ = vit_model("w128-f32")
    lrp = LRP(model)
    with _Counts(model) as c:
        lrp.generate_all(x, LRP_METHODS, start_layer=1)
    assert (c.forward, len(c.grad_inputs), c.relprop) == (1, 1, 1)
    chain = c.linear
    with _Counts(model) as c:
        lrp.generate_LRP(x, method="full")
    assert c.linear == chain and chain > 0           # "full" continued the one chain: no Linear rule ran twice
    with _Counts(model) as c:
        lrp.generate_all(x, ("last_layer_attn", "attn_rollout"), start_layer=1)
    assert (c.forward, len(c.grad_inputs), c.relprop, c.linear) == (1, 0, 0, 0)
    with _Counts(model) as c:
        lrp.generate_all(x, ("attn_gradcam",))
    assert (c.forward, c.grad_inputs, c.relprop, c.linear) == (1, [1], 0, 0)
    with _Counts(model) as c:                        # relprop methods that read no gradient: no backward pass
        lrp.generate_all(x, ("full", "last_layer", "rollout"))
    assert (c.forward, len(c.grad_inputs), c.relprop) == (1, 0, 1)


def test_bert_work_done():
    from transformer_explainability_amd.generators import Generator
    model, ids, mask, _ = bert_model(torch.float32)
    gen = Generator(model)
    with _Counts(model) as c:
        gen.generate_all(ids, mask, BERT_METHODS, start_layer=0)
    assert (c.forward, len(c.grad_inputs), c.relprop) == (1, 1, 1)
    with _Counts(model) as c:
        gen.generate_all(ids, mask, ("attn_last_layer", "rollout"))
    assert (c.forward, len(c.grad_inputs), c.relprop, c.linear) == (1, 0, 0, 0)
    with _Counts(model) as c:
        gen.generate_all(ids, mask, ("attn_gradcam",))
    assert (c.forward, c.grad_inputs, c.relprop, c.linear) == (1, [1], 0, 0)


# ------------------------------------------------------------------------------------------------ state
def _state(model, blocks, what):
    out = {}
    for i in blocks:
        a = model.blocks[i].attn
        for name in what:
            out[(i, name)] = getattr(a, name)().detach().clone()
    return out


@pytest.mark.parametrize("kind", ["tiny", "w128-bf16"])
def test_state_left_on_the_model_and_no_spill_over(kind):
    from transformer_explainability_amd.generators import LRP, Baselines
    model, x, index = vit_model(kind)
    L = len(model.blocks)
    every = ("get_attn", "get_attn_cam", "get_attn_gradients")
    plain = LRP(model).generate_LRP(x, index=index, start_layer=1).clone()
    want = _state(model, range(L), every)            # transformer_attribution reads cam and gradient of every block it serves
    LRP(model).generate_all(x, ("transformer_attribution", "attn_gradcam", "last_layer_attn"), index=index, start_layer=1)
    got = _state(model, range(L), every)
    assert all(torch.equal(got[k], want[k]) for k in want)
    Baselines(model).generate_cam_attn(x, index=index)
    want = _state(model, [L - 1], ("get_attn", "get_attn_gradients"))
    LRP(model).generate_all(x, ("attn_gradcam",), index=index)
    got = _state(model, [L - 1], ("get_attn", "get_attn_gradients"))
    assert all(torch.equal(got[k], want[k]) for k in want)
    LRP(model).generate_LRP(x, index=index, method="last_layer")
    want = _state(model, [L - 1], ("get_attn", "get_attn_cam"))
    LRP(model, prune=True).generate_all(x, ("last_layer", "attn_rollout"), index=index, start_layer=1)
    got = _state(model, [L - 1], ("get_attn", "get_attn_cam"))
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert model.prune_below_start_layer is False    # the flag was set for that call only
    assert torch.equal(LRP(model).generate_LRP(x, index=index, start_layer=1), plain)


# ------------------------------------------------------------------------------------------------ captured single call
@pytest.mark.parametrize("overlap", [False, True])
def test_graphed_lrp_replays_with_the_class_indices_in_force(overlap):
    """GraphedLRP with class indices: they are the graph's second static input.  A replay with other indices, and one without
    any (the last ones stay in force), are bitwise the eager generate_LRP with those indices."""
    from transformer_explainability_amd.generators import LRP, GraphedLRP
    model, x, _ = vit_model("w128-f32")
    lrp = LRP(model, overlap_backward=overlap)
    captured, other = [1, 15, 6], [6, 1, 15]
    want = {tuple(i): lrp.generate_LRP(x, index=i, method="transformer_attribution", start_layer=1).clone()
            for i in (captured, other)}
    assert not torch.equal(want[tuple(captured)], want[tuple(other)])         # (the indices do decide the maps)
    glrp = GraphedLRP(lrp, x, index=captured, method="transformer_attribution", start_layer=1)
    assert same(glrp(x, index=other), want[tuple(other)])
    assert same(glrp(x), want[tuple(other)])
    assert same(glrp(x, index=captured), want[tuple(captured)])
    lrp.check()


# ------------------------------------------------------------------------------------------------ sweep
def test_sweep_all_stores_equal_the_single_sweeps(tmp_path):
    from test_sweep import ToyImages, _generators
    from transformer_explainability_amd.sweep import (METHODS, ImagenetResults, ResultsStore, SaliencySweep,
                                                      SaliencySweepAll, shard_batches)
    lrp, orig, base = _generators(dev())
    assert base.model is lrp.model
    ds = ToyImages(5)                                # two batches: 3 + 2

    def stores(root):
        return {m: ResultsStore(str(root / m), len(ds), (3, 32, 32), (1, 32, 32), 0, len(ds), backend="npy") for m in METHODS}

    single = stores(tmp_path / "single")
    for m in METHODS:
        SaliencySweep(m, lrp=lrp, orig_lrp=orig, baselines=base, vis_class="target", device=dev()).run(
            shard_batches(ds, 3)[0], single[m])
        single[m].close()
    allst = stores(tmp_path / "all")
    sw = SaliencySweepAll(METHODS, lrp=lrp, orig_lrp=orig, baselines=base, vis_class="target", device=dev())
    assert [k for k, _, _ in sw.groups] == ["lrp", "orig_lrp"]
    with _Counts(lrp.model) as c:
        sw.run(shard_batches(ds, 3)[0], allst)
    assert c.forward == 2 and c.relprop == 2         # one pass per batch on the shared model
    for st in allst.values():
        st.close()

    def vis(root, m):
        res = ImagenetResults(str(root / m))
        assert len(res) == len(ds)
        return np.stack([res[i][1].numpy() for i in range(len(ds))])

    for m in METHODS:
        a, b = vis(tmp_path / "single", m), vis(tmp_path / "all", m)
        assert a.shape == (5, 1, 32, 32) and np.array_equal(a, b, equal_nan=True), m
    assert np.array_equal(vis(tmp_path / "all", "lrp"), vis(tmp_path / "all", "transformer_attribution"), equal_nan=True)


# ------------------------------------------------------------------------------------------------ rationale
def test_rationale_update_all_equals_update():
    from transformer_explainability_amd.generators import Generator
    from transformer_explainability_amd.rationale import RationaleEvaluator
    model, ids, mask, _ = bert_model(torch.float32)
    mask = mask.long()                               # (ops.token_erase takes integer tensors)
    B, N = ids.shape
    wid = (torch.arange(N, dtype=torch.int32) - 1).repeat(B, 1)
    wid[:, -1] = -1
    wid[1, N - 5:] = -1
    wid = wid.to(dev())
    truth = torch.zeros(B, N - 2, dtype=torch.bool)
    truth[0, 2:6] = True
    truth[1, 1] = True
    truth = truth.to(dev())
    gen = Generator(model)
    calls = {"LRP": lambda i, m, x: gen.generate_LRP(i, m, index=x, start_layer=0),
             "rollout": lambda i, m, x: gen.generate_rollout(i, m, start_layer=0)}
    classifier = lambda input_ids, attention_mask: model(input_ids=input_ids, attention_mask=attention_mask)  # noqa: E731
    one = {k: RationaleEvaluator(f, ks=(1, 3, 5), classifier=classifier) for k, f in calls.items()}
    both = {k: RationaleEvaluator(None, ks=(1, 3, 5), classifier=classifier) for k in calls}
    for _ in range(2):
        for ev in one.values():
            ev.update(ids, mask, wid, truth)
        with _Counts(model) as c:
            RationaleEvaluator.update_all(both, gen, ids, mask, wid, truth, start_layer=0)
        assert c.relprop == 1 and len(c.grad_inputs) == 1
    for k in calls:
        assert one[k].summary() == both[k].summary(), k
