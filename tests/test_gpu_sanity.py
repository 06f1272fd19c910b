"""-m gpu: the sanity-check protocols on the device.  The randomisation context on models that keep cached operand planes (the
x6 planes of an fp32 model, the bf16_planes of a bf16 one): at every stage the map of the model randomised IN PLACE must have
the bits of the map of a fresh model that loaded the same state dict and so has fresh caches -- which fails as soon as a stale
plane survives an edit.  class_sensitivity and SanityCheckEvaluator against the torch restatement on CPU copies of the same maps."""
import numpy as np
import pytest
import torch

from gpu_util import dev
from oracle.ref_harness import seeded_randn
from test_gpu_generate_all import same
from test_sanity_host import tiny_bert, tiny_vit

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ models
def make_vit(kind, dtype):
    """(factory of a fresh model on the device, input).  "tiny": the 64-wide model of tests/golden/vit_tiny.npz; "w128": 128
    wide with heads of 64, the smallest whose Linear layers run on the x6 / bf16 MFMA kernels and keep weight planes."""
    from transformer_explainability_amd import vit
    if kind == "tiny":
        def fresh():
            return tiny_vit().to(dev()).to(dtype)
        return fresh, seeded_randn((3, 3, 32, 32), 2).to(dev()).to(dtype)

    def fresh():
        torch.manual_seed(0)
        return vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=16,
                                     qkv_bias=True).eval().to(dev()).to(dtype)
    return fresh, seeded_randn((3, 3, 64, 64), 2).to(dev()).to(dtype)


def make_bert(kind, dtype):
    from transformer_explainability_amd import bert
    if kind == "tiny":
        def fresh():
            return tiny_bert().to(dev()).to(dtype)
    else:
        def fresh():
            torch.manual_seed(0)
            cfg = bert.BertConfigLite(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                      intermediate_size=256, max_position_embeddings=40, num_labels=2)
            return bert.BertForSequenceClassification(cfg).eval().to(dev()).to(dtype)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, 100, (2, 24), generator=g).to(dev())
    mask = torch.ones(ids.shape, device=dev())
    mask[1, 19:] = 0
    return fresh, (ids, mask)


def cached_planes(model):
    return sum(len(m.__dict__.get("_te_cache") or ()) for m in model.modules())


def check_protocol(fresh, explain, inputs):
    """explain(model, classes=None) -> ClassMaps.  Every stage against a fresh model with the same weights; the original back
    afterwards."""
    from transformer_explainability_amd import sanity
    model = fresh()
    base = explain(model)
    classes = base.classes
    original = {m: t.clone() for m, t in base.maps.items()}
    planes = cached_planes(model)
    stages = 0

    def rng():
        return torch.get_rng_state(), torch.cuda.get_rng_state(dev())

    def unchanged(before):
        return all(torch.equal(a, b) for a, b in zip(before, rng()))
    with sanity.randomized(model, "cascading", seed=1) as steps:
        while True:
            # the re-initialisation draws on a forked CPU generator: the global ones, the device's included, stay as they were
            # (snapshots around every step and around the restore: fresh() below seeds the generators itself)
            before = rng()
            name = next(steps, None)
            assert unchanged(before), name
            if name is None:
                break
            got = explain(model, classes)
            twin = fresh()
            twin.load_state_dict(model.state_dict())
            want = explain(twin, classes)
            torch.cuda.synchronize()
            for m in original:
                assert same(got.maps[m], want.maps[m]), (name, m)
            stages += 1
        assert any(not same(got.maps[m], original[m]) for m in original)          # the randomisation reached the maps
        before = rng()
    assert unchanged(before)
    again = explain(model, classes)
    for m in original:
        assert same(again.maps[m], original[m]), m
    assert stages == len(sanity.randomization_stages(model))
    return planes


VIT_METHODS = ("transformer_attribution", "attn_rollout")


@pytest.mark.parametrize("kind,dtype", [("tiny", torch.float32), ("tiny", BF), ("w128", torch.float32), ("w128", BF)],
                         ids=["tiny-f32", "tiny-bf16", "w128-f32", "w128-bf16"])
def test_vit_randomised_in_place_equals_a_fresh_model(kind, dtype):
    from transformer_explainability_amd.generators import LRP
    fresh, x = make_vit(kind, dtype)

    def explain(model, classes=None):
        which = {"topk": 1} if classes is None else {"classes": classes}
        return LRP(model).generate_classes(x, methods=VIT_METHODS, start_layer=1, **which)
    planes = check_protocol(fresh, explain, x)
    if kind == "w128":
        assert planes > 0             # the model does keep derived planes: the comparison above can see a stale one


@pytest.mark.parametrize("kind,dtype", [("tiny", torch.float32), ("tiny", BF), ("w128", torch.float32), ("w128", BF)],
                         ids=["tiny-f32", "tiny-bf16", "w128-f32", "w128-bf16"])
def test_bert_randomised_in_place_equals_a_fresh_model(kind, dtype):
    from transformer_explainability_amd.generators import Generator
    fresh, (ids, mask) = make_bert(kind, dtype)

    def explain(model, classes=None):
        which = {"topk": 1} if classes is None else {"classes": classes}
        return Generator(model).generate_classes(ids, mask, methods=("LRP", "rollout"), start_layer=0, **which)
    planes = check_protocol(fresh, explain, ids)
    if kind == "w128":
        assert planes > 0


# ------------------------------------------------------------------------------------------------ class sensitivity
def test_class_sensitivity_on_the_tiny_vit():
    """Input seed 2: on the CPU oracle's maps of this model the top two classes' transformer_attribution maps have a Spearman
    correlation of 0.08, 0.33 and -0.00 (cov 108, 444, -4 against va = 1360): cov < va with a wide margin."""
    from transformer_explainability_amd import sanity
    from transformer_explainability_amd.generators import LRP
    model = tiny_vit().to(dev())
    x = seeded_randn((3, 3, 32, 32), 2).to(dev())
    methods = ("transformer_attribution", "attn_rollout", "last_layer_attn")
    got = sanity.class_sensitivity(LRP(model), x, methods=methods, topk=2, start_layer=1)
    torch.cuda.synchronize()
    assert tuple(got) == methods
    for m in ("attn_rollout", "last_layer_attn"):
        sums, sim = got[m]
        assert sums.shape == (3, 2, 3) and bool((sums[..., 1] > 0).all())
        assert torch.equal(sums[..., 0], sums[..., 1]) and torch.equal(sums[..., 1], sums[..., 2]), m
        assert bool((sim[:, 1:3] == 1).all()), m
    sums, sim = got["transformer_attribution"]
    assert bool((sums[:, 0, 0] < sums[:, 0, 1]).any()) and bool((sim[:, 1] < 0.9).any())


# ------------------------------------------------------------------------------------------------ the evaluator
class Replay:
    """A generator that hands out recorded maps (CPU copies of what the real one produced), call by call."""

    def __init__(self, model, calls):
        self.model, self.calls, self.at = model, calls, 0

    def generate_classes(self, *inputs, **kw):
        self.at += 1
        return self.calls[self.at - 1]


class Recorder:
    def __init__(self, gen):
        self.gen, self.model, self.calls = gen, gen.model, []

    def generate_classes(self, *inputs, **kw):
        from transformer_explainability_amd.generators import ClassMaps
        r = self.gen.generate_classes(*inputs, **kw)
        self.calls.append(ClassMaps(r.classes.cpu(), r.scores.cpu(), {m: t.detach().cpu().clone() for m, t in r.maps.items()}))
        return r


def grid8_vit():
    """A 64-wide ViT on 64 x 64 images with patches of 8: an 8 x 8 token map, the smallest the SSIM window fits into."""
    from transformer_explainability_amd import vit
    torch.manual_seed(0)
    return vit.VisionTransformer(img_size=64, patch_size=8, embed_dim=64, depth=2, num_heads=4, num_classes=10, qkv_bias=True).eval()


class ImageTape:
    """Stands in for sanity._ssim_images: records the images the device evaluator compared (as CPU copies), or hands the
    recorded ones out again in the same order, so that both evaluators run SSIM on the very same images."""

    def __init__(self, real=None, tape=None):
        self.real, self.tape, self.at = real, [] if tape is None else tape, 0

    def __call__(self, maps, upsample):
        if self.real is not None:
            out = self.real(maps, upsample)
            self.tape.append(None if out is None else out.detach().cpu().clone())
            return out
        self.at += 1
        return self.tape[self.at - 1]


@pytest.mark.parametrize("kind,upsample", [("tiny", False), ("grid8", False), ("tiny", True)], ids=["tiny", "grid8", "tiny-upsampled"])
def test_evaluator_on_the_device_equals_the_evaluator_on_cpu_copies(kind, upsample, monkeypatch):
    """Integers equal, Pearson within 8 n 2^-53, Spearman within 4 ulp, SSIM within 1e-9 wherever the maps are images: the
    8 x 8 token maps of grid8 (min-max in fp32 is the same IEEE arithmetic on both sides, so both see the same images) and the
    upsampled 4 x 4 maps of the tiny model, where the CPU side is handed the device's heat maps.  The tiny model's 4 x 4 maps
    themselves are below the window: NaN."""
    from transformer_explainability_amd import sanity
    from transformer_explainability_amd.generators import LRP
    make, side = (tiny_vit, 32) if kind == "tiny" else (grid8_vit, 64)
    model = make().to(dev())
    x = seeded_randn((3, 3, side, side), 2).to(dev())
    n = (side // 8) ** 2
    methods = ("transformer_attribution", "attn_rollout")
    rec = Recorder(LRP(model))
    tape = ImageTape(real=sanity._ssim_images)
    monkeypatch.setattr(sanity, "_ssim_images", tape)
    ev = sanity.SanityCheckEvaluator(rec, methods, seed=1, upsample=upsample, start_layer=1)
    kept = ev.update(x)
    assert kept.is_cuda and kept.shape == (3, 1)
    sims, sums = ev.arrays()
    stages = len(sanity.randomization_stages(model))
    assert len(tape.tape) == len(methods) * (1 + stages)                 # the original's image once, then one per stage

    def on_cpu(images):
        monkeypatch.setattr(sanity, "_ssim_images", images)
        cpu = sanity.SanityCheckEvaluator(Replay(make(), rec.calls), methods, seed=1, upsample=upsample, start_layer=1)
        cpu.update(x.cpu())
        return cpu.arrays()
    # upsampled: the device's own heat maps; else whatever the CPU path makes of the CPU copies of the maps
    want_sims, want_sums = on_cpu(ImageTape(tape=tape.tape) if upsample else tape.real)
    has_images = upsample or kind == "grid8"
    for m in methods:
        assert sims[m].shape == (stages, 3, 4) and np.array_equal(sums[m], want_sums[m]), m
        assert np.array_equal(np.isnan(sims[m]), np.isnan(want_sims[m])), m
        d = np.abs(np.nan_to_num(sims[m]) - np.nan_to_num(want_sims[m]))
        print(kind, upsample, m, "max |device - cpu| per column:", d.max((0, 1)))
        assert d[..., 0].max() <= 8 * n * EPS and d[..., 1:3].max() <= 4 * EPS, (m, d.max((0, 1)))
        assert d[..., 3].max() <= 1e-9, (m, d[..., 3].max())
        assert np.isnan(sims[m][..., 3]).all() != has_images, m
    if upsample:
        # beside the tight comparison: against torch's own interpolate.  The device's bilinear heat map and F.interpolate are two
        # fp32 evaluations of the same image in [0, 1], a handful of fp32 roundings each, so the window statistics of the two
        # differ by about 1e-6 absolute, and the factors they enter are at least C1 = 1e-4: 1e-2 bounds the quotient.
        loose = on_cpu(tape.real)[0]
        for m in methods:
            d = np.abs(np.nan_to_num(sims[m][..., 3]) - np.nan_to_num(loose[m][..., 3])).max()
            print(m, "ssim against F.interpolate: max |device - cpu| =", d)
            assert d <= 1e-2, (m, d)
    s = ev.summary()
    assert s["transformer_attribution"]["mean"].shape == (stages, 4)
    # rollout does not read the head: its map survives the first stage untouched
    assert np.all(sims["attn_rollout"][0, :, 1] == 1.0) and np.all(sims["transformer_attribution"][-1, :, 1] < 1.0)
