"""Several classes per input from one forward pass (LRP.generate_classes, Generator.generate_classes, the tuple ``vis_class``
of SaliencySweepAll): the host logic, without a device.  The refusals come before the forward pass; the composition is checked
on CPU tensors with the device ops routed to the oracle (tests/oracle_backend.py) and ops.class_targets replaced by the torch
expression it stands for: every ``maps[m][:, k]`` must be torch.equal to the single call with ``index=classes[:, k]``."""
import contextlib

import pytest
import torch

from test_generate_all_host import (BERT_METHODS, CFG, LRP_METHODS, _bert_tiny, _Counts, _NoForward, _RecordingStore, _same,
                                    _single_bert, _single_vit)


def _torch_class_targets(logits, classes=None, topk=None, with_seeds=True, out=None):
    """What te_class_targets_* computes, as a torch expression (tie-free logits: torch.topk's order is the kernel's)."""
    from transformer_explainability_amd import ops
    logits = logits.detach()
    rel = ops.relevance_dtype(logits.dtype)
    cls = torch.topk(logits.to(rel), topk, dim=-1).indices if classes is None else classes
    B, C = logits.shape
    ok = (cls >= 0) & (cls < C)
    safe = cls.clamp(0, C - 1)
    scores = torch.where(ok, logits.to(rel).gather(1, safe), torch.full((), float("nan"), dtype=rel))
    seeds = None
    if with_seeds:
        seeds = torch.zeros((cls.shape[1], B, C), dtype=rel)
        seeds.scatter_(2, safe.t().unsqueeze(-1), ok.t().unsqueeze(-1).to(rel))
    return torch.where(ok, cls, torch.full_like(cls, -1)), scores, seeds


@contextlib.contextmanager
def host_ops():
    from oracle_backend import oracle_ops
    from transformer_explainability_amd import ops
    saved = ops.class_targets
    ops.class_targets = _torch_class_targets
    try:
        with oracle_ops():
            yield
    finally:
        ops.class_targets = saved


# ------------------------------------------------------------------------------------------------ refusals
class _NoForwardVit(_NoForward):
    num_classes = 10


class _NoForwardBert(_NoForward):
    num_labels = 2


def test_refusals_come_before_the_forward_pass():
    from transformer_explainability_amd._lib import TeError
    from transformer_explainability_amd.generators import LRP, Generator
    lrp = LRP(_NoForwardVit())
    x = torch.zeros(2, 3, 8, 8)
    seeds = torch.zeros(2, 10)
    for kw in ({}, {"classes": [1, 2], "topk": 2}, {"topk": 1, "seeds": seeds}, {"classes": [1], "seeds": seeds},
               {"classes": [1, 2], "topk": 2, "seeds": seeds}):
        with pytest.raises(ValueError, match="exactly one"):
            lrp.generate_classes(x, **kw)
    for k in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match="topk"):
            lrp.generate_classes(x, topk=k)
    for bad in ([1, 10], [[0, 1], [2, -1]], torch.tensor([3, 12]), [[0, 1]] * 3, [0.5, 1.0]):
        with pytest.raises(ValueError, match="classes"):
            lrp.generate_classes(x, classes=bad)
    with pytest.raises(ValueError):
        lrp.generate_classes(x, topk=2, methods="grad")
    with pytest.raises(ValueError, match="no_such_method"):
        lrp.generate_classes(x, topk=2, methods=["grad", "no_such_method"])
    with pytest.raises(TeError, match="float64"):
        lrp.generate_classes(x.double(), topk=2, methods=["grad", "full"])
    with pytest.raises(TeError, match="bfloat16"):
        lrp.generate_classes(x.half(), topk=2)
    with pytest.raises(TeError, match="float64"):                    # seeds follow the relevance dtype of the model
        lrp.generate_classes(x, seeds=seeds.double())
    with pytest.raises(TeError, match="bfloat16"):                   # (a bf16 model's relevance is fp32)
        lrp.generate_classes(x.bfloat16(), seeds=seeds.bfloat16())
    with pytest.raises(TeError, match="float32"):
        lrp.generate_classes(x.double(), seeds=seeds)
    for bad in (torch.zeros(2, 9), torch.zeros(3, 10), torch.zeros(2, 2, 9), torch.zeros(10), torch.zeros(2, 1, 1, 10)):
        with pytest.raises(ValueError, match="seeds"):
            lrp.generate_classes(x, seeds=bad)
    for ok in ({"topk": 10}, {"classes": [9, 0, 9]}, {"seeds": seeds}, {"seeds": torch.zeros(2, 3, 10)}):
        with pytest.raises(AssertionError, match="forward pass ran"):      # (the stub does raise when it is reached)
            lrp.generate_classes(x, **ok)
    gen = Generator(_NoForwardBert())
    ids = torch.zeros(2, 4, dtype=torch.long)
    mask = torch.ones_like(ids)
    with pytest.raises(ValueError, match="exactly one"):
        gen.generate_classes(ids, mask)
    with pytest.raises(ValueError, match="topk"):
        gen.generate_classes(ids, mask, topk=3)
    with pytest.raises(ValueError, match="classes"):
        gen.generate_classes(ids, mask, classes=[0, 2])
    with pytest.raises(ValueError, match="transformer_attribution"):
        gen.generate_classes(ids, mask, topk=1, methods=["LRP", "transformer_attribution"])
    with pytest.raises(TeError, match="float64"):
        gen.generate_classes(ids, mask, seeds=torch.zeros(2, 2, dtype=torch.float64))
    with pytest.raises(AssertionError, match="forward pass ran"):
        gen.generate_classes(ids, mask, topk=2)


# ------------------------------------------------------------------------------------------------ the planes of |X|
def test_x_abs_planes_stay_until_the_last_class():
    from transformer_explainability_amd import ops
    X = torch.zeros(4, 8)
    planes = torch.ones(3)
    a, b = {}, {}
    for c in (a, b):
        ops.post_x_abs_planes(c, X, 4, 8, planes)
    with ops.x_abs_planes_kept([a, b]) as kept:
        assert ops.take_x_abs_planes(a, X, 4, 8) is planes and "x_abs_planes" in a          # class 0: left in place
        assert ops.take_x_abs_planes(a, X, 4, 8) is planes
        assert ops.take_x_abs_planes(a, torch.zeros(4, 8), 4, 8) is None and "x_abs_planes" in a    # (another X: no planes)
        kept.last = True
        assert ops.take_x_abs_planes(a, X, 4, 8) is planes and "x_abs_planes" not in a      # the last class pops
        assert "x_abs_planes" in b                                                           # never read ...
    assert "x_abs_planes" not in b                                                           # ... dropped on exit
    ops.post_x_abs_planes(a, X, 4, 8, planes)
    with pytest.raises(RuntimeError), ops.x_abs_planes_kept([a]):
        assert ops.take_x_abs_planes(a, X, 4, 8) is planes
        raise RuntimeError("a chain raised")
    assert "x_abs_planes" not in a
    ops.post_x_abs_planes(a, X, 4, 8, planes)                        # outside the context: consumed once, as ever
    assert ops.take_x_abs_planes(a, X, 4, 8) is planes and ops.take_x_abs_planes(a, X, 4, 8) is None


# ------------------------------------------------------------------------------------------------ composition (oracle ops)
def _vit():
    from transformer_explainability_amd import vit
    torch.manual_seed(0)
    return vit.VisionTransformer(**CFG).eval(), torch.randn(2, 3, 32, 32)


VIT_CLASSES = torch.tensor([[3, 7, 3], [0, 9, 4]])                  # K = 3, a duplicate, per-sample different classes
VIT_SUBSETS = (LRP_METHODS, ("last_layer_attn", "attn_rollout"), ("transformer_attribution", "last_layer_attn", "attn_gradcam"),
               ("attn_gradcam",), ("full", "last_layer"))


@pytest.mark.parametrize("opts", [{}, {"prune": True}])
def test_vit_generate_classes_equals_single_calls_on_oracle_ops(opts):
    from transformer_explainability_amd import methods as M
    from transformer_explainability_amd.generators import LRP
    model, x = _vit()
    K = VIT_CLASSES.shape[1]
    with host_ops():
        for abl, sl in ((False, 1), (True, 0)):
            ref = [{m: _single_vit(model, x, m, VIT_CLASSES[:, k], abl, sl, **opts).clone() for m in LRP_METHODS}
                   for k in range(K)]
            logits = model(x).detach()
            for sub in VIT_SUBSETS:
                with _Counts(model) as c:
                    got = LRP(model, **opts).generate_classes(x, classes=VIT_CLASSES, methods=sub, is_ablation=abl,
                                                              start_layer=sl)
                assert tuple(got.maps) == tuple(sub) and torch.equal(got.classes, VIT_CLASSES)
                assert torch.equal(got.scores, logits.gather(1, VIT_CLASSES))
                for m in sub:
                    assert got.maps[m].shape[:2] == (2, K)
                    for k in range(K):
                        assert _same(got.maps[m][:, k], ref[k][m]), (m, k, sub, opts)
                need = M.needs(sub, M.LRP_NEEDS, abl, M.LRP_ABLATION_NEEDS)
                assert c.forward == 1
                assert c.relprop == (K if need.relprop else 0) and len(c.grad_inputs) == (K if need.backward else 0)
                if need.forward_only:
                    assert c.linear == 0
                if sub == ("attn_gradcam",):
                    assert c.grad_inputs == [1] * K and c.linear == 0
            # [K] broadcasts over the batch; a list is taken; topk = the classes torch.topk names
            got = LRP(model, **opts).generate_classes(x, classes=[7, 3], is_ablation=abl, start_layer=sl)
            for k, cls in enumerate((7, 3)):
                assert _same(got.maps["transformer_attribution"][:, k],
                             _single_vit(model, x, "transformer_attribution", torch.tensor([cls, cls]), abl, sl, **opts))
            top = LRP(model, **opts).generate_classes(x, topk=2, methods=("grad",), is_ablation=abl, start_layer=sl)
            assert torch.equal(top.classes, torch.topk(logits, 2).indices)
            assert _same(top.maps["grad"][:, 0], _single_vit(model, x, "grad", None, abl, sl, **opts))
            # nothing spills over: a plain call afterwards gives its usual bits
            assert _same(LRP(model, **opts).generate_LRP(x, index=VIT_CLASSES[:, 0], is_ablation=abl, start_layer=sl),
                         ref[0]["transformer_attribution"])


def test_vit_seeds_on_oracle_ops():
    from transformer_explainability_amd.generators import LRP, _attention_gradients
    model, x = _vit()
    with host_ops():
        onehot = torch.zeros(2, 3, 10).scatter_(2, VIT_CLASSES.unsqueeze(-1), 1.0)
        a = LRP(model).generate_classes(x, classes=VIT_CLASSES, methods=("transformer_attribution", "attn_gradcam"), start_layer=1)
        b = LRP(model).generate_classes(x, seeds=onehot, methods=("transformer_attribution", "attn_gradcam"), start_layer=1)
        assert b.classes is None and torch.equal(a.scores, b.scores)
        assert all(_same(a.maps[m], b.maps[m]) for m in a.maps)
        # a contrastive seed: the same pass assembled by hand from the existing pieces
        seed = onehot[:, 0] - onehot[:, 1]
        got = LRP(model).generate_classes(x, seeds=seed, start_layer=1)
        assert got.maps["transformer_attribution"].shape[:2] == (2, 1)
        out = model(x)
        assert torch.equal(got.scores[:, 0], (seed * out.detach()).sum(-1))
        _attention_gradients(torch.sum(seed * out), [blk.attn for blk in model.blocks])
        want = model.relprop(seed, method="transformer_attribution", start_layer=1, alpha=1)
        assert _same(got.maps["transformer_attribution"][:, 0], want)
        assert not _same(want, a.maps["transformer_attribution"][:, 0])


@pytest.mark.parametrize("opts", [{}, {"prune": True}])
def test_bert_generate_classes_equals_single_calls_on_oracle_ops(opts):
    from transformer_explainability_amd import methods as M
    from transformer_explainability_amd.generators import Generator
    model, ids, mask = _bert_tiny()
    classes = torch.tensor([[1, 0, 1], [0, 0, 1]])
    K = classes.shape[1]
    subsets = (BERT_METHODS, ("attn_last_layer", "rollout"), ("LRP", "LRP_last_layer", "attn_gradcam"), ("attn_gradcam",),
               ("full_lrp", "rollout"))
    with host_ops():
        for sl, rsl in ((1, 0), (0, 1)):
            ref = [{m: _single_bert(Generator(model, **opts), ids, mask, m, classes[:, k], sl, rsl).clone()
                    for m in BERT_METHODS} for k in range(K)]
            for sub in subsets:
                with _Counts(model) as c:
                    got = Generator(model, **opts).generate_classes(ids, mask, classes=classes, methods=sub, start_layer=sl,
                                                                    rollout_start_layer=rsl)
                assert tuple(got.maps) == tuple(sub) and torch.equal(got.classes, classes)
                for m in sub:
                    for k in range(K):
                        assert _same(got.maps[m][:, k], ref[k][m]), (m, k, sub, opts)
                need = M.needs(sub, M.GENERATOR_NEEDS)
                assert c.forward == 1
                assert c.relprop == (K if need.relprop else 0) and len(c.grad_inputs) == (K if need.backward else 0)
                if sub == ("attn_gradcam",):
                    assert c.grad_inputs == [1] * K and c.linear == 0
            assert _same(Generator(model, **opts).generate_LRP(ids, mask, index=classes[:, 0], start_layer=sl), ref[0]["LRP"])


def test_a_chain_that_raises_leaves_no_planes_behind():
    """A rule raises in class 2's chain: no layer's scratch dict holds x_abs_planes afterwards, the prune flag is the user's,
    and a plain call gives its usual bits.  (The oracle ops never post the planes: the forward hook below does, as the x6
    forward product would.)"""
    from transformer_explainability_amd import ops, rules
    from transformer_explainability_amd.generators import LRP
    model, x = _vit()
    linears = [m for m in model.modules() if isinstance(m, rules.Linear)]

    def post(module, args, output):
        for lin in linears:
            ops.post_x_abs_planes(rules.x6_cache(lin), lin.X, lin.X.numel() // lin.X.shape[-1], lin.X.shape[-1], torch.ones(1))
    with host_ops():
        ref = _single_vit(model, x, "transformer_attribution", VIT_CLASSES[:, 0], False, 1).clone()
        hook = model.register_forward_hook(post)
        chains = []
        block_relprop = model.blocks[1].relprop

        def second_chain_raises(*a, **kw):
            chains.append(1)
            if len(chains) == 2:
                raise RuntimeError("raised inside class 2's chain")
            return block_relprop(*a, **kw)
        model.blocks[1].relprop = second_chain_raises
        try:
            with pytest.raises(RuntimeError, match="class 2's chain"):
                LRP(model).generate_classes(x, classes=VIT_CLASSES, start_layer=1)
        finally:
            del model.blocks[1].relprop
            hook.remove()
        assert len(chains) == 2
        assert all("x_abs_planes" not in rules.x6_cache(lin) for lin in linears)
        assert ops._X_ABS_KEPT is None and model.prune_below_start_layer is False
        assert _same(LRP(model).generate_LRP(x, index=VIT_CLASSES[:, 0], start_layer=1), ref)


# ------------------------------------------------------------------------------------------------ sweep
class _StubClassGen:
    """Records every call; generate_classes takes the new keywords and returns maps whose value names method and class slot."""

    def __init__(self, model, calls, tag):
        self.model, self.calls, self.tag = model, calls, tag

    @staticmethod
    def _map(B, k):
        return (torch.arange(16, dtype=torch.float32) ** (1.0 + 0.5 * k)).repeat(B, 1)

    def generate_classes(self, x, classes=None, topk=None, seeds=None, methods=("transformer_attribution",), is_ablation=False,
                         start_layer=0, head_mask=None):
        from transformer_explainability_amd.generators import ClassMaps, TopAnd
        what = ("topk", topk) if topk is not None else \
            ("top_and", classes.top_first, tuple(classes.classes.reshape(-1).tolist())) if isinstance(classes, TopAnd) else \
            ("classes", tuple(classes.reshape(-1).tolist()))
        K = 2 if isinstance(classes, TopAnd) else 1
        self.calls.append((self.tag, "generate_classes", tuple(methods), start_layer, is_ablation, what))
        B = x.shape[0]
        maps = {m: torch.stack([self._map(B, 2 * i + k + 1) for k in range(K)], 1) for i, m in enumerate(methods)}
        return ClassMaps(None, torch.zeros(B, K), maps)

    def generate_all(self, x, methods, index=None, is_ablation=False, start_layer=0):
        self.calls.append((self.tag, "generate_all", tuple(methods), start_layer, is_ablation, index is not None))
        return {m: self._map(x.shape[0], i + 1) for i, m in enumerate(methods)}

    def generate_rollout(self, x, start_layer=0):
        self.calls.append((self.tag, "generate_rollout", start_layer))
        return self._map(x.shape[0], 7)

    def generate_cam_attn(self, x, index=None):
        self.calls.append((self.tag, "generate_cam_attn", index is not None))
        return self._map(x.shape[0], 8 + (index is not None)).reshape(x.shape[0], 4, 4)


def _class_stubs(shared_baselines=True):
    calls = []
    model, other, orig = torch.nn.Linear(1, 1), torch.nn.Linear(1, 1), torch.nn.Linear(1, 1)
    return (calls, _StubClassGen(model, calls, "lrp"), _StubClassGen(orig, calls, "orig_lrp"),
            _StubClassGen(model if shared_baselines else other, calls, "baselines"))


def test_sweep_tuple_vis_class_one_call_per_group_per_batch():
    from oracle_backend import oracle_ops
    from transformer_explainability_amd.sweep import SaliencySweepAll
    methods = ("lrp", "transformer_attribution", "attn_gradcam", "lrp_last_layer")
    calls, lrp, orig, base = _class_stubs()
    sw = SaliencySweepAll(methods, lrp=lrp, orig_lrp=orig, baselines=base, vis_class=("top", "target"), is_ablation=True)
    with oracle_ops():
        out = sw.explain(torch.zeros(2, 3, 16, 16), torch.tensor([1, 2]))
    assert tuple(out) == tuple((m, v) for m in methods for v in ("top", "target"))
    assert all(v.shape == (2, 1, 16, 16) for v in out.values())
    assert calls == [("lrp", "generate_classes", ("transformer_attribution", "attn_gradcam"), 1, False, ("top_and", True, (1, 2))),
                     ("orig_lrp", "generate_classes", ("last_layer",), 0, True, ("top_and", True, (1, 2)))]
    assert out["lrp", "top"] is out["transformer_attribution", "top"]
    assert not torch.equal(out["lrp", "top"], out["lrp", "target"])
    # the stores, keyed the same way: one call per group per batch, every store once per batch
    del calls[:]
    log = []
    stores = {k: _RecordingStore(log, k) for k in out}
    batches = [(torch.rand(2, 3, 16, 16), torch.tensor([0, 1])), (torch.rand(1, 3, 16, 16), torch.tensor([2]))]
    with oracle_ops():
        sw.run(batches, stores)
    assert log == list(out) * 2 and len(calls) == 4 and all(c[1] == "generate_classes" for c in calls)
    with pytest.raises(ValueError, match="no store"):
        sw.run(batches, {("lrp", "top"): stores["lrp", "top"]})
    # the column order follows the tuple; one entry: topk = 1 or the target column alone
    for vis, what in ((("target", "top"), ("top_and", False, (1, 2))), (("top",), ("topk", 1)), (("target",), ("classes", (1, 2)))):
        del calls[:]
        with oracle_ops():
            out = SaliencySweepAll(("lrp",), lrp=lrp, vis_class=vis).explain(torch.zeros(2, 3, 16, 16), torch.tensor([1, 2]))
        assert tuple(out) == tuple(("lrp", v) for v in vis) and calls[0][5] == what and len(calls) == 1
    # a Baselines object on a model of its own keeps its single calls
    calls, lrp, orig, base = _class_stubs(shared_baselines=False)
    with oracle_ops():
        out = SaliencySweepAll(("rollout", "attn_gradcam"), baselines=base, vis_class=("top", "target")).explain(
            torch.zeros(2, 3, 16, 16), torch.tensor([1, 2]))
    assert calls == [("baselines", "generate_rollout", 1), ("baselines", "generate_cam_attn", False),
                     ("baselines", "generate_cam_attn", True)]
    assert torch.equal(out["rollout", "top"], out["rollout", "target"])
    assert not torch.equal(out["attn_gradcam", "top"], out["attn_gradcam", "target"])
    for bad in ((), ("top", "top"), ("top", "bottom"), ["predicted"]):
        with pytest.raises(ValueError, match="vis_class"):
            SaliencySweepAll(("lrp",), lrp=lrp, vis_class=bad)
    with pytest.raises(ValueError, match="target"):
        SaliencySweepAll(("lrp",), lrp=lrp, vis_class=("top", "target")).explain(torch.zeros(2, 3, 16, 16))

    _string_vis_class_makes_the_calls_of_today()


def _string_vis_class_makes_the_calls_of_today():
    """With a string ``vis_class`` the generators see the calls they always saw, from stubs that do take the new keywords."""
    from oracle_backend import oracle_ops
    from transformer_explainability_amd.sweep import SaliencySweepAll
    methods = ("rollout", "lrp", "transformer_attribution", "full_lrp", "lrp_last_layer", "attn_last_layer", "attn_gradcam")
    for vis, with_index in (("top", False), ("target", True)):
        calls, lrp, orig, base = _class_stubs()
        with oracle_ops():
            out = SaliencySweepAll(methods, lrp=lrp, orig_lrp=orig, baselines=base, vis_class=vis).explain(
                torch.zeros(2, 3, 16, 16), torch.tensor([1, 2]))
        assert tuple(out) == methods
        assert calls == [
            ("lrp", "generate_all", ("attn_rollout", "transformer_attribution", "last_layer_attn", "attn_gradcam"), 1, False,
             with_index),
            ("orig_lrp", "generate_all", ("full", "last_layer"), 0, False, with_index)]
