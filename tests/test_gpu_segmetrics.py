"""-m gpu: ops.seg_metrics (te_seg_metrics_f32) against the torch functions of segmentation.py applied to the same tensors ON
THE CPU -- the reference of every case, never the kernel's own output -- and against the reference's own results in
tests/golden/seg_metrics.npz.  Integers and the per-row F1 (a quotient of integers in one expression) must be exact; AP within
1e-12: a restatement that forms AP from the integer run counts as sum (dtp / npos) (tp / n), summed sequentially in reversed
order, differs from segmentation.average_precision by at most 9.3e-15 at 224 x 224 on these input classes (CPU), so the bar
leaves two orders of magnitude."""
import pytest
import torch

from conftest import load_golden
from gpu_util import dev, record
from host_util import bits

pytestmark = pytest.mark.gpu

AP_TOL = 1e-12
HEATS = ["bilinear", "distinct", "quantised", "constant"]
LABELS = ["foreground30", "ignored_rows", "all_background", "all_ignored", "with_class_2"]


def sg():
    from transformer_explainability_amd import segmentation
    return segmentation


def ops():
    from transformer_explainability_amd import ops as o
    return o


def make_heat(kind, B, H, W, seed):
    """(heat, mask) CPU fp32 [B,H,W]"""
    g = torch.Generator().manual_seed(seed)
    if kind == "bilinear":                       # the evaluator's own input: real ties along the replicated borders
        assert H == W and H % 16 == 0
        maps = torch.rand((B, (H // 16) ** 2), generator=g)
        heat, mask = ops().heatmap(maps.to(dev()), scale=16, normalise=True, with_mask=True)
        return heat[:, 0].cpu(), mask[:, 0].cpu()
    if kind == "distinct":
        heat = torch.rand((B, H, W), generator=g)
    elif kind == "quantised":                    # 51 levels: heavy ties, and h = 1 - h = 0.5 ties across the classes
        heat = (torch.rand((B, H, W), generator=g) * 50).round() / 50
    elif kind == "constant":
        heat = torch.tensor([0.5, 0.25, 0.0, 1.0])[torch.arange(B) % 4].view(B, 1, 1).expand(B, H, W).contiguous()
    else:
        raise ValueError(kind)
    mask = (heat > heat.flatten(1).mean(1).view(-1, 1, 1)).float()
    if kind == "constant":
        mask[:, ::2] = 1.0                       # (a constant map is never above its mean: give the counts something)
    return heat, mask


def make_labels(kind, B, H, W, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    labels = (torch.rand((B, H, W), generator=g) > 0.7).long()          # 30 % foreground
    i = min(1, B - 1)
    if kind == "ignored_rows":
        labels[i, : max(1, H // 7)] = -1
        labels[i, H // 2] = -1
    elif kind == "all_background":               # class 1 has no positives, class 0 has
        labels[i] = 0
    elif kind == "all_ignored":                  # AP = 0
        labels[i] = -1
    elif kind == "with_class_2":                 # valid, in neither class
        labels[torch.rand((B, H, W), generator=g) > 0.9] = 2
    elif kind != "foreground30":
        raise ValueError(kind)
    return labels


def restate(heat, mask, labels):
    """The torch functions on CPU tensors: counts [B,6], ap [B], f1 [B,H]."""
    s = sg()
    assert not heat.is_cuda and not mask.is_cuda and not labels.is_cuda
    correct, labeled = s.pixel_accuracy(mask, labels)
    inter, union = s.intersection_union(mask, labels)
    counts = torch.cat([correct.view(-1, 1), labeled.view(-1, 1), inter, union], 1)
    return counts, s.average_precision(heat, labels), s.row_f1(mask, labels)


def compare(name, got, ref):
    counts, ap, f1 = (t.cpu() for t in got)
    rc, rap, rf1 = ref
    assert counts.dtype == torch.int64 and ap.dtype == torch.float64 and f1.dtype == torch.float64
    assert counts.shape == rc.shape and ap.shape == rap.shape and f1.shape == rf1.shape
    ap_err = float((ap - rap).abs().max())
    f1_err = float((f1 - rf1).abs().max())
    print(f"{name}: counts equal {torch.equal(counts, rc)}  max|ap - ref| {ap_err:.3e}  max|f1 - ref| {f1_err:.3e}")
    record(name, ap_max_abs=ap_err, f1_max_abs=f1_err, counts_equal=bool(torch.equal(counts, rc)))
    assert torch.equal(counts, rc), (name, counts, rc)
    assert torch.equal(f1, rf1), (name, f1_err)
    assert torch.isfinite(ap).all() and ap_err < AP_TOL, (name, ap_err)


def run(heat, mask, labels):
    d = dev()
    return ops().seg_metrics(heat.to(d), mask.to(d), labels.to(d))


def test_golden_reference_results():
    from test_segmentation import inputs
    g = load_golden("seg_metrics.npz")
    counts, ap, f1 = (t.cpu() for t in run(*inputs()))
    ap_err, f1_err = float((ap - g["ap"]).abs().max()), float((f1 - g["f1"]).abs().max())
    print(f"golden: max|ap - ref| {ap_err:.3e}  max|f1 - ref| {f1_err:.3e}")
    assert torch.equal(counts[:, 0], g["correct"].long()) and torch.equal(counts[:, 1], g["labeled"].long())
    assert torch.equal(counts[:, 2:4], g["inter"].long()) and torch.equal(counts[:, 4:6], g["union"].long())
    assert ap_err < 1e-12 and f1_err < 1e-12


@pytest.mark.parametrize("labels_kind", LABELS)
@pytest.mark.parametrize("heat_kind", HEATS)
def test_against_torch_on_cpu_224(heat_kind, labels_kind):
    B, H, W = 4, 224, 224
    heat, mask = make_heat(heat_kind, B, H, W, seed=11)
    labels = make_labels(labels_kind, B, H, W, seed=11)
    ref = restate(heat, mask, labels)
    if labels_kind == "all_ignored":
        assert float(ref[1][1]) == 0.0 and int(ref[0][1, 1]) == 0
    compare(f"seg_metrics_{heat_kind}_{labels_kind}", run(heat, mask, labels), ref)


# the seams of the sort's wave segments, in its 2*H*W elements: (16,32) 1024, the last size with one 64-element step per wave;
# (19,27) 1026, the first with two (waves 9 .. 15 get an empty segment); (1,33) 66: wave 1 holds 2 elements, waves 2 .. 15 none
@pytest.mark.parametrize("B,H,W", [(3, 30, 34), (2, 1, 1), (1, 224, 224), (2, 16, 32), (2, 19, 27), (1, 1, 33)])
@pytest.mark.parametrize("heat_kind", ["distinct", "quantised"])
def test_against_torch_on_cpu_shapes(heat_kind, B, H, W):
    heat, mask = make_heat(heat_kind, B, H, W, seed=5)
    labels = make_labels("ignored_rows" if H > 1 else "foreground30", B, H, W, seed=5)
    if (H, W) == (1, 1):
        labels[0], labels[1] = 1, 0              # one positive pixel per image: class 1 / class 0
    compare(f"seg_metrics_{heat_kind}_{B}x{H}x{W}", run(heat, mask, labels), restate(heat, mask, labels))


def test_labels_of_another_integer_dtype():
    heat, mask = make_heat("quantised", 2, 30, 34, seed=6)
    labels = make_labels("ignored_rows", 2, 30, 34, seed=6)
    compare("seg_metrics_int32_labels", run(heat, mask, labels.to(torch.int32)), restate(heat, mask, labels))


@pytest.fixture(scope="module")
def batch70():
    B, H, W = 70, 224, 224
    heat, mask = make_heat("bilinear", B, H, W, seed=21)
    labels = make_labels("ignored_rows", B, H, W, seed=21)
    labels[5] = -1
    labels[6] = 0
    labels[7][labels[7] == 1] = 2
    d = dev()
    return heat.to(d), mask.to(d), labels.to(d)


def test_batch_70_against_torch_on_cpu(batch70):
    heat, mask, labels = batch70
    compare("seg_metrics_batch70", ops().seg_metrics(heat, mask, labels), restate(heat.cpu(), mask.cpu(), labels.cpu()))


def test_batch_equals_its_samples_bit_for_bit(batch70):
    heat, mask, labels = batch70
    first = ops().seg_metrics(heat, mask, labels)
    again = ops().seg_metrics(heat, mask, labels)
    for a, b in zip(first, again):
        assert torch.equal(bits(a), bits(b))
    for b in range(heat.shape[0]):
        alone = ops().seg_metrics(heat[b:b + 1], mask[b:b + 1], labels[b:b + 1])
        for whole, one in zip(first, alone):
            assert torch.equal(bits(whole[b:b + 1]), bits(one)), b


def test_nan_heat_is_the_cleaned_map():
    B, H, W = 3, 64, 64
    heat, mask = make_heat("distinct", B, H, W, seed=8)
    labels = make_labels("ignored_rows", B, H, W, seed=8)
    heat[0, 3:9] = float("nan")
    heat[1] = float("nan")                       # the reference's 0/0 of a constant map
    heat[2, 10, ::3] = float("nan")
    mask[0, 3:6] = 1.0                           # whatever the mask says where the heat is NaN, it counts as 0
    nan = torch.isnan(heat)
    clean_heat = torch.where(nan, torch.zeros_like(heat), heat)       # foreground_split's rule
    clean_mask = torch.where(nan, torch.zeros_like(mask), mask)
    compare("seg_metrics_nan", run(heat, mask, labels), restate(clean_heat, clean_mask, labels))


def test_graph_capture_replays_bit_for_bit():
    """No host synchronisation inside the call: a HIP graph captures it, and the replay is the eager call."""
    from transformer_explainability_amd.generators import GraphedCall
    B, H, W = 4, 224, 224
    d = dev()
    first = [t.to(d) for t in (*make_heat("bilinear", B, H, W, seed=31), make_labels("foreground30", B, H, W, seed=31))]
    other = [t.to(d) for t in (*make_heat("quantised", B, H, W, seed=32), make_labels("ignored_rows", B, H, W, seed=32))]
    graphed = GraphedCall(ops().seg_metrics, first)
    for inputs in (first, other, first):
        replay = [t.clone() for t in graphed(*inputs)]
        eager = ops().seg_metrics(*inputs)
        for a, b in zip(replay, eager):
            assert torch.equal(bits(a), bits(b))
    compare("seg_metrics_graph_replay", replay, restate(*(t.cpu() for t in first)))


def test_evaluator_on_the_device():
    s = sg()
    B, H, W = 4, 224, 224
    heat, mask = make_heat("bilinear", B, H, W, seed=41)
    labels = make_labels("ignored_rows", B, H, W, seed=41)
    d = dev()
    ev, ref = s.SegmentationEvaluator(explain=None), s.SegmentationEvaluator(explain=None)
    out_ref = ref.update_from_heat(heat, mask, labels)                        # CPU tensors: the torch functions
    out = ev.update_from_heat(heat.to(d), mask.to(d), labels.to(d))
    assert len(out) == 6
    for k, (a, b) in enumerate(zip(out, out_ref)):
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype == torch.int64:
            assert torch.equal(a.cpu(), b), k
        else:
            assert float((a.cpu() - b).abs().max()) < AP_TOL, k
    assert torch.equal(out[5].cpu(), out_ref[5])
    assert ev.total_correct == ref.total_correct and ev.total_label == ref.total_label
    assert (ev.total_inter == ref.total_inter).all() and (ev.total_union == ref.total_union).all()
    assert len(ev.total_ap) == B and len(ev.total_f1) == B and ev.total_f1[0].shape == (H,)
    a, b = ev.summary(), ref.summary()
    assert a["pixAcc"] == b["pixAcc"] and a["mIoU"] == b["mIoU"] and a["mF1"] == b["mF1"]
    assert abs(a["mAP"] - b["mAP"]) < AP_TOL


def test_evaluator_update_end_to_end_on_the_device():
    """explain -> te_heatmap_f32 -> te_seg_metrics_f32 on a tiny ViT, as test_evaluator_end_to_end_cpu, on the device."""
    from transformer_explainability_amd import vit
    from transformer_explainability_amd.generators import LRP
    s = sg()
    torch.manual_seed(0)
    d = dev()
    m = vit.VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=2, num_heads=4, num_classes=10,
                              qkv_bias=True).eval().to(d)
    x = torch.randn(3, 3, 32, 32).to(d)
    labels = (torch.rand(3, 32, 32) > 0.5).long().to(d)
    lrp = LRP(m)
    seen = []

    def explain(im):
        seen.append(lrp.generate_LRP(im, start_layer=1).detach().clone())
        return seen[-1]

    ev = s.SegmentationEvaluator(explain, scale=8)
    out = ev.update(x, labels)
    assert all(t.is_cuda for t in out)
    summary = ev.summary()
    assert all(0.0 <= v <= 1.0 for v in summary.values()) and len(ev.total_ap) == 3 and len(ev.total_f1) == 3
    # the same maps through foreground_split and the torch functions on the CPU
    heat, mask = s.foreground_split(seen[0].reshape(3, -1), 8)
    ref = s.SegmentationEvaluator(explain=None)
    ref.update_from_heat(heat.cpu(), mask.cpu(), labels.cpu())
    b = ref.summary()
    assert summary["pixAcc"] == b["pixAcc"] and summary["mIoU"] == b["mIoU"] and summary["mF1"] == b["mF1"]
    assert abs(summary["mAP"] - b["mAP"]) < AP_TOL
