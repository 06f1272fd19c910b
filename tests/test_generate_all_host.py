"""One pass for several explanation methods (LRP.generate_all, Generator.generate_all, SaliencySweepAll,
RationaleEvaluator.update_all): the host logic, without a device.  The needs table (methods.py), the refusals, the prune rule
and the grouping of the sweep are checked on their own; the composition is checked on CPU tensors with the device ops routed
to the oracle (tests/oracle_backend.py), where every entry of a one-pass result must be torch.equal to the single call."""
import itertools

import numpy as np
import pytest
import torch

CFG = dict(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=10, qkv_bias=True)
LRP_METHODS = ("transformer_attribution", "grad", "rollout", "full", "last_layer", "second_layer", "last_layer_attn",
               "attn_rollout", "attn_gradcam")
BERT_METHODS = ("LRP", "LRP_last_layer", "full_lrp", "attn_last_layer", "rollout", "attn_gradcam")


def M():
    from transformer_explainability_amd import methods
    return methods


# ------------------------------------------------------------------------------------------------ the needs table
#                       last_grad all_grads relprop pixels unpruned
EXPECTED_LRP = {
    "transformer_attribution": (False, True, True, False, False),
    "grad": (False, True, True, False, False),
    "rollout": (False, False, True, False, True),
    "full": (False, False, True, True, True),
    "last_layer": (False, False, True, False, False),
    "second_layer": (False, False, True, False, True),
    "last_layer_attn": (False, False, False, False, False),
    "attn_rollout": (False, False, False, False, False),
    "attn_gradcam": (True, False, False, False, False),
}
EXPECTED_BERT = {
    "LRP": (False, True, True, False, False),
    "LRP_last_layer": (False, False, True, False, False),
    "full_lrp": (False, False, True, True, True),
    "attn_last_layer": (False, False, False, False, False),
    "rollout": (False, False, False, False, False),
    "attn_gradcam": (True, False, False, False, False),
}


@pytest.mark.parametrize("table,expected", [("LRP_NEEDS", EXPECTED_LRP), ("GENERATOR_NEEDS", EXPECTED_BERT)])
def test_needs_table_singletons_and_full_set(table, expected):
    m = M()
    tab = getattr(m, table)
    assert set(tab) == set(expected)
    for name, row in expected.items():
        got = m.needs((name,), tab)
        assert got.forward and tuple(got[1:]) == row, (name, got)
        assert got.forward_only == (not any(row[:3])), name
    full = m.needs(tuple(expected), tab)
    assert tuple(full) == (True, True, True, True, True, True)
    assert not full.forward_only and full.backward


def test_needs_unions_and_ablation():
    m = M()
    n = m.needs(("last_layer_attn", "attn_rollout"), m.LRP_NEEDS)
    assert n.forward_only and not n.backward and not n.relprop
    n = m.needs(("attn_gradcam", "last_layer_attn"), m.LRP_NEEDS)
    assert n.last_grad and not n.all_grads and not n.relprop
    n = m.needs(("full", "last_layer"), m.LRP_NEEDS)
    assert n.relprop and n.pixels and not n.backward
    # is_ablation: the block's attn_cam is multiplied by its gradient
    assert m.needs(("last_layer",), m.LRP_NEEDS, True, m.LRP_ABLATION_NEEDS).last_grad
    assert m.needs(("second_layer",), m.LRP_NEEDS, True, m.LRP_ABLATION_NEEDS).all_grads
    assert not m.needs(("last_layer",), m.LRP_NEEDS, False, m.LRP_ABLATION_NEEDS).backward
    assert not m.needs(("full",), m.LRP_NEEDS, True, m.LRP_ABLATION_NEEDS).backward


def test_check_names():
    m = M()
    assert m.check(["grad", "full", "grad"], m.LRP_NEEDS) == ("grad", "full")
    for bad in (["grad", "no_such_method"], [], "grad", ["LRP"]):
        with pytest.raises(ValueError):
            m.check(bad, m.LRP_NEEDS)
    with pytest.raises(ValueError):
        m.check(["transformer_attribution"], m.GENERATOR_NEEDS)


def test_prune_rule():
    m = M()
    ok = ("transformer_attribution", "grad", "last_layer", "last_layer_attn", "attn_rollout", "attn_gradcam")
    for r in (1, 2, len(ok)):
        for sub in itertools.combinations(ok, r):
            assert m.prunable(sub, m.LRP_NEEDS), sub
    for spoil in ("rollout", "full", "second_layer"):
        assert not m.prunable((spoil,), m.LRP_NEEDS)
        assert not m.prunable(("transformer_attribution", spoil), m.LRP_NEEDS)
    assert m.prunable(("LRP", "LRP_last_layer", "attn_last_layer", "rollout", "attn_gradcam"), m.GENERATOR_NEEDS)
    assert not m.prunable(("LRP", "full_lrp"), m.GENERATOR_NEEDS)


# ------------------------------------------------------------------------------------------------ refusals
class _NoForward(torch.nn.Module):
    """A model whose forward pass must never be reached."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.prune_below_start_layer = False

    def forward(self, *a, **kw):
        raise AssertionError("the forward pass ran")


def test_refusals_come_before_the_forward_pass():
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import LRP, Generator
    lrp = LRP(_NoForward())
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="no_such_method"):
        lrp.generate_all(x, ["grad", "no_such_method"])
    with pytest.raises(ValueError):
        lrp.generate_all(x, "grad")
    with pytest.raises(TeError, match="float64"):
        lrp.generate_all(x.double(), ["grad", "full"])
    with pytest.raises(TeError, match="bfloat16"):
        lrp.generate_all(x.half(), ["last_layer_attn"])
    with pytest.raises(AssertionError, match="forward pass ran"):      # (the stub does raise when it is reached)
        lrp.generate_all(x, ["grad"])
    gen = Generator(_NoForward())
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="transformer_attribution"):
        gen.generate_all(ids, torch.ones_like(ids), ["LRP", "transformer_attribution"])


# ------------------------------------------------------------------------------------------------ sweep grouping
class _StubGen:
    """Records every call; returns maps whose value names the call (so a store can be traced to the call that fed it)."""

    def __init__(self, model, calls, tag):
        self.model, self.calls, self.tag = model, calls, tag

    def _map(self, B, k):
        return (torch.arange(16, dtype=torch.float32) ** (1.0 + 0.5 * k)).repeat(B, 1)

    def generate_all(self, x, methods, index=None, is_ablation=False, start_layer=0):
        self.calls.append((self.tag, "generate_all", tuple(methods), start_layer, is_ablation, index is not None))
        return {m: self._map(x.shape[0], i + 1) for i, m in enumerate(methods)}

    def generate_rollout(self, x, start_layer=0):
        self.calls.append((self.tag, "generate_rollout", start_layer))
        return self._map(x.shape[0], 7)

    def generate_cam_attn(self, x, index=None):
        self.calls.append((self.tag, "generate_cam_attn", index is not None))
        return self._map(x.shape[0], 8).reshape(x.shape[0], 4, 4)


def _stubs(shared_baselines=True, with_orig=True):
    calls = []
    model, other, orig = torch.nn.Linear(1, 1), torch.nn.Linear(1, 1), torch.nn.Linear(1, 1)
    lrp = _StubGen(model, calls, "lrp")
    base = _StubGen(model if shared_baselines else other, calls, "baselines")
    return calls, lrp, (_StubGen(orig, calls, "orig_lrp") if with_orig else None), base


ALL_SWEEP = ("rollout", "lrp", "transformer_attribution", "full_lrp", "lrp_last_layer", "attn_last_layer", "attn_gradcam")


def test_sweep_grouping_same_model_object():
    from oracle_backend import oracle_ops
    from transformer_explainability_amd.sweep import SaliencySweepAll
    calls, lrp, orig, base = _stubs(shared_baselines=True)
    sw = SaliencySweepAll(ALL_SWEEP, lrp=lrp, orig_lrp=orig, baselines=base)
    kinds = {k: (g, n) for k, g, n in sw.groups}
    assert set(kinds) == {"lrp", "orig_lrp"}
    assert kinds["lrp"][0] is lrp and kinds["orig_lrp"][0] is orig
    assert kinds["lrp"][1] == {"rollout": "attn_rollout", "lrp": "transformer_attribution",
                               "transformer_attribution": "transformer_attribution",
                               "attn_last_layer": "last_layer_attn", "attn_gradcam": "attn_gradcam"}
    assert kinds["orig_lrp"][1] == {"full_lrp": "full", "lrp_last_layer": "last_layer"}
    with oracle_ops():
        out = sw.explain(torch.zeros(2, 3, 16, 16), torch.tensor([1, 2]))
    assert tuple(out) == ALL_SWEEP and all(v.shape == (2, 1, 16, 16) for v in out.values())
    assert calls == [
        ("lrp", "generate_all", ("attn_rollout", "transformer_attribution", "last_layer_attn", "attn_gradcam"), 1, False, False),
        ("orig_lrp", "generate_all", ("full", "last_layer"), 0, False, False)]
    assert out["lrp"] is out["transformer_attribution"]        # computed once


def test_sweep_grouping_other_model_object_and_target_class():
    from oracle_backend import oracle_ops
    from transformer_explainability_amd.sweep import SaliencySweepAll
    calls, lrp, orig, base = _stubs(shared_baselines=False)
    sw = SaliencySweepAll(ALL_SWEEP, lrp=lrp, orig_lrp=orig, baselines=base, vis_class="target", is_ablation=True)
    assert [k for k, _, _ in sw.groups] == ["lrp", "orig_lrp", "baselines"]
    with oracle_ops():
        sw.explain(torch.zeros(2, 3, 16, 16), torch.tensor([1, 2]))
    assert calls == [
        ("lrp", "generate_all", ("transformer_attribution", "last_layer_attn"), 1, False, True),
        ("orig_lrp", "generate_all", ("full", "last_layer"), 0, True, True),
        ("baselines", "generate_rollout", 1),
        ("baselines", "generate_cam_attn", True)]


def test_sweep_grouping_missing_generators():
    from transformer_explainability_amd.sweep import SaliencySweepAll
    calls, lrp, _, base = _stubs(with_orig=False)
    sw = SaliencySweepAll(("lrp", "rollout"), lrp=lrp, baselines=base)          # orig_lrp absent and not needed
    assert [k for k, _, _ in sw.groups] == ["lrp"]
    for methods in (("lrp", "full_lrp"), ("lrp_last_layer",)):
        with pytest.raises(ValueError, match="orig_lrp"):
            SaliencySweepAll(methods, lrp=lrp, baselines=base)
    with pytest.raises(ValueError, match="baselines"):
        SaliencySweepAll(("rollout",), lrp=lrp)
    with pytest.raises(ValueError, match="lrp"):
        SaliencySweepAll(("attn_last_layer",), baselines=base)
    with pytest.raises(ValueError):
        SaliencySweepAll(("lrp", "no_such_method"), lrp=lrp)
    with pytest.raises(ValueError):
        SaliencySweepAll((), lrp=lrp)


class _RecordingStore:
    def __init__(self, log, name):
        self.log, self.name, self.vis = log, name, []

    def append(self, image, target, vis):
        self.log.append(self.name)
        self.vis.append(vis.clone())


def test_sweep_stores_written():
    from oracle_backend import oracle_ops
    from transformer_explainability_amd.sweep import SaliencySweepAll
    calls, lrp, orig, base = _stubs(shared_baselines=True)
    methods = ("lrp", "transformer_attribution", "attn_gradcam", "lrp_last_layer")
    sw = SaliencySweepAll(methods, lrp=lrp, orig_lrp=orig, baselines=base)
    log = []
    stores = {m: _RecordingStore(log, m) for m in methods}
    batches = [(torch.rand(2, 3, 16, 16), torch.tensor([0, 1])), (torch.rand(1, 3, 16, 16), torch.tensor([2]))]
    with oracle_ops():
        sw.run(batches, stores)
    assert log == list(methods) * 2                               # every store once per batch, in the requested order
    assert len(calls) == 4 and all(c[1] == "generate_all" for c in calls)       # two passes per batch, not four
    for a, b in zip(stores["lrp"].vis, stores["transformer_attribution"].vis):
        assert torch.equal(a, b)
    assert not torch.equal(stores["lrp"].vis[0], stores["attn_gradcam"].vis[0])
    with pytest.raises(ValueError, match="no store"):
        sw.run(batches, {"lrp": stores["lrp"]})


# ------------------------------------------------------------------------------------------------ composition (oracle ops)
class _Counts:
    """forward passes of the model, calls of model.relprop, torch.autograd.grad (with the number of tensors asked for) and
    ops.linear_relprop while the context is open."""

    def __init__(self, model):
        self.model = model
        self.forward = self.relprop = self.linear = 0
        self.grad_inputs = []

    def __enter__(self):
        from transformer_explainability_amd import ops
        self._ops = ops
        self._hook = self.model.register_forward_hook(lambda *a: setattr(self, "forward", self.forward + 1))
        self._relprop, self._grad, self._linear = self.model.relprop, torch.autograd.grad, ops.linear_relprop

        def relprop(*a, **kw):
            self.relprop += 1
            return self._relprop(*a, **kw)

        def grad(outputs, inputs, *a, **kw):
            self.grad_inputs.append(len(inputs))
            return self._grad(outputs, inputs, *a, **kw)

        def linear(*a, **kw):
            self.linear += 1
            return self._linear(*a, **kw)
        self.model.relprop, torch.autograd.grad, ops.linear_relprop = relprop, grad, linear
        return self

    def __exit__(self, *exc):
        self._hook.remove()
        del self.model.relprop
        torch.autograd.grad, self._ops.linear_relprop = self._grad, self._linear


def _single_vit(model, x, name, index, is_ablation, start_layer, **opts):
    from transformer_explainability_amd.generators import LRP, Baselines
    if name == "attn_rollout":
        return Baselines(model).generate_rollout(x, start_layer=start_layer)
    if name == "attn_gradcam":
        return Baselines(model).generate_cam_attn(x, index=index)
    return LRP(model, **opts).generate_LRP(x, index=index, method=name, is_ablation=is_ablation, start_layer=start_layer)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.detach()), torch.nan_to_num(b.detach())) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.mark.parametrize("opts", [{}, {"prune": True}])
def test_vit_generate_all_equals_single_calls_on_oracle_ops(opts):
    from oracle_backend import oracle_ops
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP
    torch.manual_seed(0)
    model = vit.VisionTransformer(**CFG).eval()
    x = torch.randn(2, 3, 32, 32)
    subsets = (LRP_METHODS, ("last_layer_attn", "attn_rollout"), ("transformer_attribution", "last_layer", "attn_gradcam"),
               ("full", "last_layer"), ("attn_gradcam",))
    with oracle_ops():
        for index, abl, sl in ((None, False, 1), (torch.tensor([3, 7]), True, 0)):
            ref = {m: _single_vit(model, x, m, index, abl, sl, **opts).clone() for m in LRP_METHODS}
            for sub in subsets:
                with _Counts(model) as c:
                    got = LRP(model, **opts).generate_all(x, sub, index=index, is_ablation=abl, start_layer=sl)
                assert tuple(got) == tuple(sub)
                for m in sub:
                    assert _same(got[m], ref[m]), (m, sub, index, opts)
                need = M().needs(sub, M().LRP_NEEDS, abl, M().LRP_ABLATION_NEEDS)
                assert c.forward == 1 and c.relprop == int(need.relprop) and len(c.grad_inputs) == int(need.backward)
                if not need.relprop:
                    assert c.linear == 0
                if sub == ("attn_gradcam",):
                    assert c.grad_inputs == [1]
            # nothing spills over: a plain call afterwards gives its usual bits
            assert _same(LRP(model, **opts).generate_LRP(x, index=index, start_layer=sl), ref["transformer_attribution"])


def _bert_tiny():
    from transformer_explainability_amd import bert
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=64, num_hidden_layers=3, num_attention_heads=4,
                              intermediate_size=128, max_position_embeddings=40, num_labels=2)
    torch.manual_seed(1)
    model = bert.BertForSequenceClassification(cfg).eval()
    ids = torch.randint(1, 100, (2, 12))
    mask = torch.ones(2, 12)
    mask[1, 9:] = 0                                  # one sample padded
    return model, ids, mask


def _single_bert(gen, ids, mask, name, index, sl, rsl):
    if name == "LRP":
        return gen.generate_LRP(ids, mask, index=index, start_layer=sl)
    if name == "rollout":
        return gen.generate_rollout(ids, mask, start_layer=rsl)
    return getattr(gen, "generate_" + name)(ids, mask, index=index)


@pytest.mark.parametrize("opts", [{}, {"prune": True}])
def test_bert_generate_all_equals_single_calls_on_oracle_ops(opts):
    from oracle_backend import oracle_ops
    from transformer_explainability_amd.generators import Generator
    model, ids, mask = _bert_tiny()
    subsets = (BERT_METHODS, ("attn_last_layer", "rollout"), ("LRP", "LRP_last_layer", "attn_gradcam"), ("attn_gradcam",),
               ("full_lrp",))
    with oracle_ops():
        for index, sl, rsl in ((None, 1, 0), (torch.tensor([1, 0]), 0, 1)):
            ref = {m: _single_bert(Generator(model, **opts), ids, mask, m, index, sl, rsl).clone() for m in BERT_METHODS}
            for sub in subsets:
                with _Counts(model) as c:
                    got = Generator(model, **opts).generate_all(ids, mask, sub, index=index, start_layer=sl,
                                                                rollout_start_layer=rsl)
                assert tuple(got) == tuple(sub)
                for m in sub:
                    assert _same(got[m], ref[m]), (m, sub, index, opts)
                need = M().needs(sub, M().GENERATOR_NEEDS)
                assert c.forward == 1 and c.relprop == int(need.relprop) and len(c.grad_inputs) == int(need.backward)
                if sub == ("attn_gradcam",):
                    assert c.grad_inputs == [1] and c.linear == 0
            assert _same(Generator(model, **opts).generate_LRP(ids, mask, index=index, start_layer=sl), ref["LRP"])


VIT_SINGLE_METHODS = LRP_METHODS[:7]                 # the ``method=`` names of LRP.generate_LRP
VIT_SINGLE_PRUNED = ("transformer_attribution", "grad")


def _work(model, call):
    """-> (what the call returned, (forward passes, model.relprop calls, tensors asked of autograd.grad, ops.linear_relprop calls))"""
    with _Counts(model) as c:
        out = call()
    return out, (c.forward, c.relprop, c.grad_inputs, c.linear)


def test_single_calls_keep_their_work():
    """Every single call does the reference's work -- one forward pass, the attention-gradient backward over all blocks (from
    start_layer when pruned) and the whole chain, whatever its tail reads -- and ``prune`` shortens it for exactly the calls
    listed here.  The figures are those of the tiny models of this file (ViT depth 3, BERT 3 layers)."""
    from oracle_backend import oracle_ops
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP, Baselines, Generator
    torch.manual_seed(0)
    model = vit.VisionTransformer(**CFG).eval()
    x = torch.randn(2, 3, 32, 32)
    bert, ids, mask = _bert_tiny()
    whole = (1, 1, [3], 13)
    vit_pruned = {0: (1, 1, [3], 12), 1: (1, 1, [2], 8)}
    with oracle_ops():
        for sl in (0, 1):
            index = None if sl else torch.tensor([3, 7])
            # ---- ViT.  user_flag: the model's own prune_below_start_layer, which a call honours like ``prune`` and leaves alone
            for prune, user_flag in ((False, False), (True, False), (False, True), (True, True)):
                model.prune_below_start_layer = user_flag
                for m in VIT_SINGLE_METHODS:
                    out, work = _work(model, lambda: LRP(model, prune=prune).generate_LRP(x, index=index, method=m,
                                                                                          start_layer=sl))
                    pruned = (prune or user_flag) and m in VIT_SINGLE_PRUNED
                    assert work == (vit_pruned[sl] if pruned else whole), (m, sl, prune, user_flag, work)
                    assert out is not None and model.prune_below_start_layer is user_flag
                # an unknown name: the pass runs, nothing is returned.  The two baselines are names of generate_all alone
                for m in ("no_such_method", "attn_rollout", "attn_gradcam"):
                    out, work = _work(model, lambda: LRP(model, prune=prune).generate_LRP(x, index=index, method=m,
                                                                                          start_layer=sl))
                    assert out is None and work == whole and model.prune_below_start_layer is user_flag, m
                # a call that raises inside the chain leaves the user's value too, and no block set to stop the chain
                def boom(*a, **kw):
                    raise RuntimeError("raised inside the chain")
                model.blocks[1].relprop = boom
                try:
                    with pytest.raises(RuntimeError, match="raised inside the chain"):
                        LRP(model, prune=prune).generate_LRP(x, index=index, start_layer=sl)
                finally:
                    del model.blocks[1].relprop
                assert model.prune_below_start_layer is user_flag
                assert not any(getattr(blk.attn, "_stop_after_attn_cam", False) for blk in model.blocks)
            model.prune_below_start_layer = False
            assert _work(model, lambda: Baselines(model).generate_rollout(x, start_layer=sl))[1] == (1, 0, [], 0)
            assert _work(model, lambda: Baselines(model).generate_cam_attn(x, index=index))[1] == (1, 0, [1], 0)
            # ---- BERT
            bert_whole = (1, 1, [3], 20)
            expected = {
                False: {"LRP": bert_whole, "LRP_last_layer": bert_whole, "full_lrp": bert_whole, "attn_gradcam": bert_whole},
                True: {"LRP": {0: (1, 1, [3], 17), 1: (1, 1, [2], 11)}[sl], "LRP_last_layer": (1, 1, [1], 5),
                       "full_lrp": bert_whole, "attn_gradcam": (1, 1, [1], 5)}}
            bindex = None if sl else torch.tensor([1, 0])
            for prune in (False, True):
                for m in BERT_METHODS:
                    out, work = _work(bert, lambda: _single_bert(Generator(bert, prune=prune), ids, mask, m, bindex, sl, sl))
                    want = (1, 0, [], 0) if m in ("attn_last_layer", "rollout") else expected[prune][m]
                    assert work == want, (m, sl, prune, work)
                    assert out is not None


def test_rationale_update_all_equals_update_on_oracle_ops():
    from oracle_backend import oracle_ops
    from transformer_explainability_amd.generators import Generator
    from transformer_explainability_amd.rationale import RationaleEvaluator
    model, ids, mask = _bert_tiny()
    wid = (torch.arange(12, dtype=torch.int32) - 1).repeat(2, 1)
    wid[:, -1] = -1
    wid[1, 9:] = -1
    truth = torch.zeros(2, 10, dtype=torch.bool)
    truth[0, 2:5] = True
    truth[1, 1] = True
    gen = Generator(model)
    calls = {"LRP": lambda i, m, x: gen.generate_LRP(i, m, index=x, start_layer=0),
             "attn_gradcam": lambda i, m, x: gen.generate_attn_gradcam(i, m, index=x)}
    classifier = lambda input_ids, attention_mask: model(input_ids=input_ids, attention_mask=attention_mask)  # noqa: E731
    with oracle_ops():
        one = {k: RationaleEvaluator(f, ks=(1, 3), classifier=classifier) for k, f in calls.items()}
        both = {k: RationaleEvaluator(None, ks=(1, 3), classifier=classifier) for k in calls}
        for _ in range(2):
            for ev in one.values():
                ev.update(ids, mask, wid, truth)
            with _Counts(model) as c:
                RationaleEvaluator.update_all(both, gen, ids, mask, wid, truth, start_layer=0)
            assert c.relprop == 1 and len(c.grad_inputs) == 1
    for k in calls:
        a, b = one[k].summary(), both[k].summary()
        assert a == b, k
    assert np.isfinite(one["LRP"].summary()["auprc"])
