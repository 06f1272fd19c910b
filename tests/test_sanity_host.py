"""CPU: the torch restatement of the map-similarity kernels (sanity.rank_deltas / rank_sums / pearson / ssim) pinned to
scipy.stats and to a window-by-window SSIM; the randomisation context; the evaluator and class_sensitivity on a stub generator;
the host refusals of ops.map_similarity."""
import numpy as np
import pytest
import torch

from host_util import same_bits
from mapsim_inputs import FAMILIES, FINITE, family, images

EPS = 2.0 ** -53
SIZES = (1, 2, 3, 63, 64, 65, 196, 255, 256)


# ------------------------------------------------------------------------------------------------ ranks, Spearman, Pearson
@pytest.mark.parametrize("kind", FAMILIES)
def test_rank_deltas_and_spearman_against_scipy(kind):
    stats = pytest.importorskip("scipy.stats")
    from transformer_explainability_amd import sanity
    for n in SIZES:
        a, b = family(kind, n)
        da, db = sanity.rank_deltas(a), sanity.rank_deltas(b)
        sums, sim = sanity.map_similarity(a, b)
        for i in range(a.shape[0]):
            x, y = a[i].numpy(), b[i].numpy()
            if np.isnan(x).any() or np.isnan(y).any():
                assert torch.isnan(sim[i]).all() and not sums[i].any(), (kind, n, i)
                continue
            for t, d in ((x, da[i]), (y, db[i])):
                want = 2 * stats.rankdata(t, method="average") - (n + 1)
                assert np.array_equal(d.numpy(), want.astype(np.int64)) and np.array_equal(want, np.round(want)), (kind, n, i)
            assert sums[i, 0].tolist() == [int((da[i] * db[i]).sum()), int((da[i] ** 2).sum()), int((db[i] ** 2).sum())]
            for col, (u, v) in ((1, (x, y)), (2, (np.abs(x), np.abs(y)))):
                constant = n < 2 or (u == u[0]).all() or (v == v[0]).all()
                if constant:
                    assert torch.isnan(sim[i, col]), (kind, n, i, col)
                else:
                    rho = stats.spearmanr(u, v)[0]
                    assert abs(float(sim[i, col]) - rho) <= 1e-12, (kind, n, i, col, float(sim[i, col]), rho)


def test_signed_zeros_tie_and_nan_sample_leaves_neighbours_alone():
    from transformer_explainability_amd import sanity
    x = torch.tensor([[0.0, -0.0, 1.0, -1.0]])
    assert sanity.rank_deltas(x).tolist() == [[0, 0, 3, -3]]
    a, b = family("nan", 65)
    clean = [i for i in range(3) if i != 1]
    sums, sim = sanity.map_similarity(a, b)
    for i in clean:
        s1, m1 = sanity.map_similarity(a[i:i + 1], b[i:i + 1])
        assert torch.equal(s1[0], sums[i]) and torch.equal(m1[0].view(torch.int64), sim[i].view(torch.int64))
    assert torch.isnan(sim[1]).all() and not sums[1].any()


@pytest.mark.parametrize("kind", FINITE)
def test_pearson_against_scipy(kind):
    stats = pytest.importorskip("scipy.stats")
    from transformer_explainability_amd import sanity
    for n in SIZES[1:]:
        a, b = family(kind, n)
        got = sanity.pearson(a, b)
        for i in range(a.shape[0]):
            x, y = a[i].double().numpy(), b[i].double().numpy()
            if (x == x[0]).all() or (y == y[0]).all():
                assert torch.isnan(got[i])
                continue
            want = stats.pearsonr(x, y)[0]
            assert abs(float(got[i]) - want) <= 8 * n * EPS, (kind, n, i, float(got[i]), want)
    a, b = family("constant", 64)
    assert torch.isnan(sanity.pearson(a, b)[1])


# ------------------------------------------------------------------------------------------------ SSIM
def ssim_by_windows(x, y, data_range=1.0):
    """scikit-image's structural_similarity at its defaults for a 2-D image, one window at a time (numpy, fp64)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    H, W = x.shape
    c1, c2, cov_norm = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, 49.0 / 48.0
    total = 0.0
    for r in range(H - 6):
        for c in range(W - 6):
            p, q = x[r:r + 7, c:c + 7], y[r:r + 7, c:c + 7]
            ux, uy = p.mean(), q.mean()
            vx, vy = cov_norm * ((p * p).mean() - ux * ux), cov_norm * ((q * q).mean() - uy * uy)
            vxy = cov_norm * ((p * q).mean() - ux * uy)
            total += ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return total / ((H - 6) * (W - 6))


SSIM_SIZES = ((7, 7), (8, 7), (14, 14), (15, 17))


@pytest.mark.parametrize("H,W", SSIM_SIZES)
def test_ssim_against_window_loops(H, W):
    from transformer_explainability_amd import sanity
    a, b = images(H, W)
    got = sanity.ssim(a, b, 1.0)
    worst = 0.0
    for i in range(a.shape[0]):
        want = ssim_by_windows(a[i].numpy(), b[i].numpy())
        worst = max(worst, abs(float(got[i]) - want))
    print(f"ssim {H}x{W}: max |torch - loops| = {worst:.3e}")
    assert worst <= 1e-9
    assert abs(float(sanity.ssim(a, a)[0]) - 1.0) <= 1e-9
    sums, sim = sanity.map_similarity(a, b)                    # 3-D maps turn SSIM on
    assert torch.equal(sim[:, 3], got)
    assert torch.isnan(sanity.map_similarity(a.flatten(1), b.flatten(1))[1][:, 3]).all()
    with pytest.raises(ValueError):
        sanity.ssim(a[:, :6], b[:, :6])


# ------------------------------------------------------------------------------------------------ randomisation
def tiny_vit():
    from conftest import load_golden
    from transformer_explainability_amd import vit
    g = load_golden("vit_tiny.npz")
    model = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=3, num_heads=4, num_classes=10, qkv_bias=True).eval()
    model.load_state_dict({k[6:]: v for k, v in g.items() if k.startswith("state.")})
    return model


def tiny_bert():
    from conftest import load_golden
    from transformer_explainability_amd import bert
    g = load_golden("bert_tiny.npz")
    cfg = bert.BertConfigLite(vocab_size=100, hidden_size=64, num_hidden_layers=3, num_attention_heads=4, intermediate_size=128,
                              max_position_embeddings=40, num_labels=2)
    model = bert.BertForSequenceClassification(cfg).eval()
    model.load_state_dict({k[6:]: v for k, v in g.items() if k.startswith("state.")})
    return model


def full_state(model):
    """Every parameter and buffer, the non-persistent ones included."""
    return {k: v.detach().clone() for k, v in list(model.named_parameters()) + list(model.named_buffers())}


def changed(model, before):
    return {k for k, v in full_state(model).items() if not same_bits(v, before[k])}


VIT_STAGES = ["head", "blocks.2", "blocks.1", "blocks.0", "embed"]
BERT_STAGES = ["classifier", "pooler", "encoder.layer.2", "encoder.layer.1", "encoder.layer.0", "embeddings"]
OWNER = {"head": ("head.", "norm."), "embed": ("patch_embed.", "pos_embed", "cls_token"), "classifier": ("classifier.",),
         "pooler": ("bert.pooler.",), "embeddings": ("bert.embeddings.",)}


def owned(stage, key):
    prefixes = OWNER.get(stage) or ((stage + ".") if stage.startswith("blocks") else ("bert." + stage + "."),)
    return key.startswith(tuple(prefixes) if not isinstance(prefixes, str) else prefixes)


@pytest.mark.parametrize("make,names", [(tiny_vit, VIT_STAGES), (tiny_bert, BERT_STAGES)], ids=["vit", "bert"])
def test_randomized_stages_seeds_and_restore(make, names, monkeypatch):
    from transformer_explainability_amd import sanity
    model = make()
    device_seeds = []                                # torch.manual_seed reseeds every device's generator too: never called
    monkeypatch.setattr(torch.cuda, "manual_seed_all", lambda seed: device_seeds.append(seed))
    first = next(model.parameters()).data.view(-1)
    first[0], first[1] = -0.0, float("nan")         # a signed zero and a NaN among the weights: restored as they are
    assert [s.name for s in sanity.randomization_stages(model)] == names
    before = full_state(model)
    rng = torch.get_rng_state()
    seen, weights = [], {}
    with sanity.randomized(model, "cascading", seed=3) as stages:
        touched = set()
        for name in stages:
            now = changed(model, before)
            new = now - touched
            assert new and all(owned(name, k) for k in new), (name, new)        # a stage touches only its own parameters
            assert touched <= now                                                # ... on top of the earlier stages
            touched = now
            seen.append(name)
            weights[name] = {k: v for k, v in full_state(model).items() if k in new}
    assert seen == names and not changed(model, before)
    assert torch.equal(rng, torch.get_rng_state())
    # independent: one stage at a time, the same values as the cascade gave that stage (same seed + stage index)
    with sanity.randomized(model, "independent", seed=3) as stages:
        for name in stages:
            now = changed(model, before)
            assert now == set(weights[name]), name
            assert all(same_bits(full_state(model)[k], v) for k, v in weights[name].items())
    assert not changed(model, before)
    # another seed: other weights
    with sanity.randomized(model, "independent", seed=4) as stages:
        name = next(iter(stages))
        assert any(not same_bits(full_state(model)[k], v) for k, v in weights[name].items())
    assert not changed(model, before)
    # the body raises: everything is restored all the same
    with pytest.raises(RuntimeError, match="boom"):
        with sanity.randomized(model) as stages:
            for i, name in enumerate(stages):
                if i == 2:
                    raise RuntimeError("boom")
    assert not changed(model, before) and torch.equal(rng, torch.get_rng_state())
    assert device_seeds == []
    with pytest.raises(ValueError):
        with sanity.randomized(model, mode="both"):
            pass


def test_randomized_drops_cached_planes_after_every_edit(monkeypatch):
    from transformer_explainability_amd import rules, sanity
    model = tiny_vit()
    calls = []
    monkeypatch.setattr(sanity, "_invalidate", lambda m: calls.append(m))
    with sanity.randomized(model) as stages:
        for i, _ in enumerate(stages):
            assert len(calls) == i + 1
    assert len(calls) == len(VIT_STAGES) + 1 and all(m is model for m in calls)      # every edit, then the restore
    monkeypatch.undo()
    for m in model.modules():
        if isinstance(m, rules.Linear):
            rules.x6_cache(m)["bf16_planes"] = ("stale",)
    with sanity.randomized(model) as stages:
        next(iter(stages))
        assert not any(m.__dict__.get("_te_cache") for m in model.modules())


def test_randomized_values_follow_the_models_init():
    """LayerNorm goes back to (1, 0), Linear biases to 0, Linear weights and pos_embed / cls_token to a truncated normal of
    std 0.02 -- what _init_weights and the constructor do."""
    from transformer_explainability_amd import sanity
    model = tiny_vit()
    with sanity.randomized(model) as stages:
        for _ in stages:
            pass
        sd = model.state_dict()
        assert torch.equal(sd["norm.weight"], torch.ones(64)) and not sd["blocks.1.norm1.bias"].any()
        assert not sd["blocks.0.attn.qkv.bias"].any()
        for k in ("blocks.0.mlp.fc1.weight", "pos_embed", "cls_token", "head.weight"):
            assert 0.01 < float(sd[k].std()) < 0.03 and float(sd[k].abs().max()) <= 2.0, k


# ------------------------------------------------------------------------------------------------ the protocols on a stub
class StubGen:
    """Stands in for an LRP: prescribed maps per call, and a record of what every call was asked for."""

    def __init__(self, model, maps_of_call, logits):
        self.model, self.maps_of_call, self.logits, self.calls = model, maps_of_call, logits, []

    def generate_classes(self, x, classes=None, topk=None, methods=(), **kw):
        from transformer_explainability_amd.generators import ClassMaps
        if topk is not None:
            classes = torch.topk(self.logits, topk).indices
        self.calls.append({"classes": classes.clone(), "topk": topk, "methods": tuple(methods), "kw": kw,
                           "head": self.model.head.weight.detach().clone()})
        maps = self.maps_of_call(len(self.calls) - 1, classes.shape[1])
        return ClassMaps(classes, self.logits.gather(1, classes), {m: maps[m] for m in methods})


def test_evaluator_on_a_stub_generator():
    from transformer_explainability_amd import sanity
    model = tiny_vit()
    B, n = 3, 64
    g = torch.Generator().manual_seed(5)
    base = {"m1": torch.rand((B, 1, n), generator=g), "m2": torch.rand((B, 1, n), generator=g)}
    noise = torch.rand((B, 1, n), generator=g)

    def maps_of_call(call, K):
        out = {"m1": base["m1"] + 0.5 * call * noise, "m2": base["m2"].clone()}       # m1 drifts away, m2 never moves
        if call == 2:
            out["m1"][1, 0, 7] = float("nan")
        return out
    logits = torch.tensor([[0.1, 2.0, 0.3], [3.0, 0.2, 0.1], [0.0, 0.1, 0.9]])
    gen = StubGen(model, maps_of_call, logits)
    ev = sanity.SanityCheckEvaluator(gen, ("m1", "m2"), seed=1, start_layer=1)
    head0 = model.head.weight.detach().clone()
    kept = ev.update(torch.zeros(B, 3, 32, 32))
    assert kept.tolist() == [[1], [0], [2]]
    first, rest = gen.calls[0], gen.calls[1:]
    assert first["topk"] == 1 and torch.equal(first["head"], head0) and first["kw"] == {"start_layer": 1}
    assert len(rest) == len(VIT_STAGES)
    for c in rest:                                   # the class explained is fixed, the model is randomised
        assert c["topk"] is None and torch.equal(c["classes"], kept) and not torch.equal(c["head"], head0)
        assert c["methods"] == ("m1", "m2")
    assert torch.equal(model.head.weight, head0)
    ev.update(torch.zeros(B, 3, 32, 32), index=[2, 2, 0])
    assert gen.calls[len(VIT_STAGES) + 1]["classes"].tolist() == [[2], [2], [0]]
    sims, sums = ev.arrays()
    assert sims["m1"].shape == (len(VIT_STAGES), 2 * B, 4) and sums["m2"].shape == (len(VIT_STAGES), 2 * B, 2, 3)
    # 8x8 token maps are images of at least 7x7: SSIM is there; m2 never moves
    assert np.all(sims["m2"][..., 1:3] == 1.0) and np.all(np.abs(sims["m2"] - 1.0) <= 1e-12)
    assert np.all(sums["m2"][..., 0] == sums["m2"][..., 1])
    want = sanity.map_similarity(base["m1"][:, 0], base["m1"][:, 0] + 0.5 * noise[:, 0])
    assert np.array_equal(sums["m1"][0, :B], want[0].numpy()) and np.array_equal(sims["m1"][0, :B, :3], want[1][:, :3].numpy())
    s = ev.summary()
    assert s["m1"]["stages"] == VIT_STAGES and s["m1"]["columns"] == sanity.SIM_COLUMNS
    nan = s["m1"]["nan"]
    assert nan[1].tolist() == [1, 1, 1, 1] and nan[0].tolist() == [0, 0, 0, 0]      # call 2 = stage 1 of the first update
    col = sims["m1"][1, :, 0]
    assert np.isclose(s["m1"]["mean"][1, 0], np.nanmean(col)) and np.isnan(col).sum() == 1
    assert s["m1"]["mean"][0, 1] > s["m1"]["mean"][-1, 1]                           # the drift shows
    off = sanity.SanityCheckEvaluator(gen, ("m1",), ssim=False)
    off.update(torch.zeros(B, 3, 32, 32))
    assert np.isnan(off.arrays()[0]["m1"][..., 3]).all()


def test_class_sensitivity_on_a_stub_generator():
    from transformer_explainability_amd import sanity
    model = tiny_vit()
    g = torch.Generator().manual_seed(6)
    agnostic = torch.rand((2, 1, 16), generator=g).expand(2, 2, 16)
    specific = torch.rand((2, 2, 16), generator=g)
    logits = torch.tensor([[0.1, 2.0, 0.3], [3.0, 0.2, 0.5]])
    gen = StubGen(model, lambda call, K: {"rollout": agnostic, "attribution": specific}, logits)
    got = sanity.class_sensitivity(gen, torch.zeros(2, 3, 32, 32), methods=("rollout", "attribution"), topk=2)
    assert len(gen.calls) == 1 and gen.calls[0]["topk"] == 2 and gen.calls[0]["classes"].tolist() == [[1, 2], [0, 2]]
    sums, sim = got["rollout"]
    assert torch.equal(sums[..., 0], sums[..., 1]) and torch.equal(sums[..., 0], sums[..., 2]) and bool((sim[:, 1:3] == 1).all())
    sums, sim = got["attribution"]
    assert bool((sums[:, 0, 0] < sums[:, 0, 1]).all()) and bool((sim[:, 1] < 1).all())
    with pytest.raises(ValueError):
        sanity.class_sensitivity(gen, torch.zeros(2, 3, 32, 32), methods=("rollout",), topk=1)


# ------------------------------------------------------------------------------------------------ host refusals
def test_ops_map_similarity_refuses_on_the_host():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    a = torch.zeros(2, 64)
    with pytest.raises(TeError, match="CPU"):
        ops.map_similarity(a, a)
    with pytest.raises(TeError, match="float32"):
        ops.map_similarity(a.double(), a.double())
    with pytest.raises(TeError, match="float32"):
        ops.map_similarity(a, a.half())
    for x, y, shape in ((a, a[:, :63], None), (a, a[:1], None), (a[0], a[0], None), (a, a, (8, 9)), (a.view(2, 8, 8), a.view(2, 8, 8), (4, 16))):
        with pytest.raises(TeError, match="map_similarity"):
            ops.map_similarity(x, y, shape=shape)
    for x, shape in ((torch.zeros(2, 6, 8), None), (torch.zeros(2, 48), (8, 6)), (torch.zeros(2, 36), (6, 6))):
        with pytest.raises(TeError, match="7x7"):
            ops.map_similarity(x, x, shape=shape)
    with pytest.raises(TeError):
        ops.map_similarity_packed(a, a)


def test_c_abi_refusals_without_a_device():
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    P = 4096                                         # a fake non-null, aligned address the host never dereferences
    ws = lib.te_map_similarity_workspace_bytes(2, 49)
    assert ws >= 2 * 4 * 2 * 49 * 8 and ws % 256 == 0
    assert lib.te_map_similarity_workspace_bytes(1, (1 << 20) + 1) == 0 and lib.te_map_similarity_workspace_bytes(65536, 4) == 0

    def call(a=P, b=P, sums=P, sim=P, B=2, n=49, H=0, W=0, flags=0, ws_ptr=P, ws_bytes=ws):
        return lib.te_map_similarity_f32(a, b, sums, sim, B, n, H, W, flags, 1.0, ws_ptr, ws_bytes, None)
    assert [call(a=None), call(sim=None), call(B=0), call(n=0), call(flags=2)] == [_lib.TE_ERR_INVALID_ARG] * 5
    ssim = dict(flags=_lib.TE_MAPSIM_SSIM)
    assert [call(H=7, W=6, **ssim), call(H=6, W=8, n=48, **ssim), call(H=8, W=7, **ssim), call(**ssim)] == [_lib.TE_ERR_INVALID_ARG] * 4
    assert [call(n=(1 << 20) + 1), call(B=65536)] == [_lib.TE_ERR_UNSUPPORTED] * 2
    assert [call(ws_ptr=None), call(ws_bytes=ws - 256), call(H=7, W=7, ws_bytes=0, **ssim)] == [_lib.TE_ERR_WORKSPACE] * 3
    assert call(ws_ptr=P + 4) == _lib.TE_ERR_INVALID_ARG
