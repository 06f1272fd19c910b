"""-m gpu: ops.localisation_metrics (te_localisation_f32) against localisation.reference_metrics applied to the same tensors
ON THE CPU -- the reference of every case, never the kernel's own output.  stats are integers: equal.  energy: two fp64 sums
of the same non-negative terms in different orders differ by at most 2 n_valid 2^-53 of the sum (each is within (n - 1) u of
the exact sum, u = 2^-53): localisation_inputs.energy_bound, a bound known before any run."""
import pytest
import torch

from gpu_util import dev, record
from host_util import bits, same_bits
from localisation_inputs import (ENERGY_EPS, HEATS, SIZES, box_case, energy_bound, heat_maps, label_maps, mask_case, rasterise,
                                 special_cases, to)

pytestmark = pytest.mark.gpu


def ops():
    from transformer_explainability_amd import ops as o
    return o


def loc():
    from transformer_explainability_amd import localisation
    return localisation


def run(case):
    stats, energy = ops().localisation_metrics(**to(case, dev()))
    torch.cuda.synchronize()
    return stats.cpu(), energy.cpu()


def compare(name, got, ref):
    (stats, energy), (rs, re) = got, ref
    assert stats.dtype == torch.int64 and energy.dtype == torch.float64 and stats.shape == rs.shape and energy.shape == re.shape
    err = (energy - re).abs()
    rel = float((err / re.abs().clamp(min=1e-300)).max())
    print(f"{name}: stats equal {torch.equal(stats, rs)}  max rel energy error {rel:.3e}  bound/|ref| "
          f"{float(2.0 * rs[:, 0].max() * ENERGY_EPS):.3e}")
    record(name, stats_equal=bool(torch.equal(stats, rs)), energy_max_rel=rel)
    assert torch.equal(stats, rs), (name, stats, rs)
    assert bool((err <= energy_bound(rs, re)).all()), (name, energy, re)


_REFS = {}


def reference(key, case):
    """The CPU restatement of a case, computed once per session."""
    if key not in _REFS:
        assert not any(torch.is_tensor(v) and v.is_cuda for v in case.values())
        _REFS[key] = loc().reference_metrics(**case)
    return _REFS[key]


# ------------------------------------------------------------------------------------------------ kernel against the restatement
@pytest.mark.parametrize("kind", HEATS)
@pytest.mark.parametrize("H,W", SIZES)
def test_kernel_equals_the_restatement(H, W, kind):
    case = mask_case(H, W, kind, seed=H * 100 + W)
    compare(f"localisation_{kind}_{H}x{W}", run(case), reference(("mask", H, W, kind), case))


def case_224():
    heat = heat_maps(3, 224, 224, "smooth", seed=7)
    heat[2] = heat_maps(1, 224, 224, "distinct", seed=8)[0]
    return dict(heat=heat, labels=label_maps(2, 224, 224, 3, seed=7), target_id=torch.tensor([0, 2, 1]),
                image_index=torch.tensor([0, 0, 1]))


def test_kernel_equals_the_restatement_224():
    compare("localisation_224x224_P3", run(case_224()), reference("224", case_224()))


@pytest.mark.parametrize("name", sorted(special_cases()))
def test_cases_that_break_a_wrong_kernel(name):
    case, expected = special_cases()[name]
    ref = reference(("special", name), case)
    got = run(case)
    compare(f"localisation_{name}", got, ref)
    if expected is not None:
        for have, want in zip(got[0][0].tolist(), expected):
            assert want is None or have == want, (name, got[0][0].tolist(), expected)
    if name == "all_negative":
        assert got[1][0].tolist() == [0.0, 0.0]
    d2 = int(got[0][0, 3])
    if name == "distance_225_is_a_hit":
        assert d2 == 225 and 0 <= d2 <= 15 ** 2
    if name == "distance_244_is_a_miss":
        assert d2 == 244 and not d2 <= 15 ** 2


# ------------------------------------------------------------------------------------------------ boxes
@pytest.mark.parametrize("M", [1, 3])
def test_boxes_equal_the_restatement_and_the_rasterised_union(M):
    case = box_case(M)
    got = run(case)
    compare(f"localisation_boxes_M{M}", got, reference(("boxes", M), case))
    P, H, W = case["heat"].shape
    by_mask = run(dict(heat=case["heat"], labels=rasterise(case["boxes"], H, W), target_id=torch.ones(P, dtype=torch.long)))
    assert all(same_bits(x, y) for x, y in zip(got, by_mask))
    if M == 3:
        assert int(got[0][0, 1]) == 7 * 8 + 8 * 7 - 3 * 3 and got[0][2].tolist()[1:] == [0, int(got[0][2, 2]), -1, 0]


def test_boxes_most_rows_the_entry_point_takes():
    """M = 64, the most the entry point takes: 62 padding rows around two boxes, and an image_index that skips a pair."""
    heat = heat_maps(2, 64, 80, "smooth", seed=3)
    boxes = torch.zeros((2, 64, 4), dtype=torch.long)
    boxes[:, 7] = torch.tensor([10, 5, 30, 20])
    boxes[:, 63] = torch.tensor([25, 15, 90, 70])
    case = dict(heat=heat, boxes=boxes, image_index=torch.tensor([0, -1]))
    got = run(case)
    compare("localisation_boxes_M64", got, reference("boxes64", case))
    assert got[0][1].tolist() == list(loc().SKIPPED_STATS) and int(got[0][0, 1]) == 20 * 15 + 55 * 49 - 5 * 5


# ------------------------------------------------------------------------------------------------ image_index, skipped pairs
def test_shared_label_maps_equal_per_pair_copies():
    case = mask_case(17, 19, "levels", seed=5)
    shared = run(case)
    copies = run(dict(case, labels=case["labels"][case["image_index"]].contiguous(), image_index=None))
    assert all(same_bits(x, y) for x, y in zip(shared, copies))
    compare("localisation_shared_maps", shared, reference(("mask", 17, 19, "levels", 5), case))


def test_skipped_pairs_leave_their_neighbours_alone():
    case = mask_case(17, 19, "distinct", seed=6)
    whole = run(case)
    tid, idx = case["target_id"].clone(), case["image_index"].clone()
    tid[1], idx[4] = -1, 2                                                       # B = 2: image_index == B
    got = run(dict(case, target_id=tid, image_index=idx))
    for p in range(6):
        if p in (1, 4):
            assert got[0][p].tolist() == list(loc().SKIPPED_STATS) and bits(got[1][p]).tolist() == [0, 0]
        else:
            assert torch.equal(got[0][p], whole[0][p]) and torch.equal(bits(got[1][p]), bits(whole[1][p])), p
    far = case["image_index"].clone()
    far[0], far[5] = -(1 << 40), 1 << 40                                          # never used as an address
    got = run(dict(case, image_index=far))
    assert got[0][0].tolist() == list(loc().SKIPPED_STATS) and got[0][5].tolist() == list(loc().SKIPPED_STATS)
    assert torch.equal(got[0][1:5], whole[0][1:5]) and torch.equal(bits(got[1][1:5]), bits(whole[1][1:5]))


# ------------------------------------------------------------------------------------------------ determinism
def raw_call(case, ws):
    """The C ABI with a workspace of the caller's: (status, stats, energy)."""
    from transformer_explainability_amd import _lib
    lib = _lib.load()
    c = to(case, dev())
    P, H, W = c["heat"].shape
    stats = torch.full((P, 5), -7, dtype=torch.int64, device=dev())
    energy = torch.full((P, 2), -7.0, dtype=torch.float64, device=dev())
    rc = lib.te_localisation_f32(c["heat"].data_ptr(), c["labels"].data_ptr(), c["image_index"].data_ptr(),
                                 c["target_id"].data_ptr(), None, 0, stats.data_ptr(), energy.data_ptr(), P,
                                 c["labels"].shape[0], H, W, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, stats.cpu(), energy.cpu()


def five_pairs():
    case = mask_case(33, 47, "smooth", seed=9)                                   # 1551 pixels: two trips, a short last one
    return {k: v[:5].contiguous() if k != "labels" else v for k, v in case.items()}


def test_batch_equals_its_single_calls_bit_for_bit():
    case = five_pairs()
    whole = run(case)
    assert all(same_bits(x, y) for x, y in zip(whole, run(case)))
    for p in range(5):
        alone = run({k: v[p:p + 1] if k != "labels" else v for k, v in case.items()})
        assert torch.equal(alone[0], whole[0][p:p + 1]) and torch.equal(bits(alone[1]), bits(whole[1][p:p + 1])), p


def test_workspace_place_and_content_do_not_matter():
    from transformer_explainability_amd import _lib
    case = five_pairs()
    want = run(case)
    need = _lib.load().te_localisation_workspace_bytes(5, 33, 47)
    for offset, fill in ((0, 0), (8, 0xff), (264, 0x5a)):
        buf = torch.full((need + 512,), fill, dtype=torch.uint8, device=dev())
        rc, stats, energy = raw_call(case, buf[offset:offset + need])
        assert rc == 0 and torch.equal(stats, want[0]) and torch.equal(bits(energy), bits(want[1])), (offset, fill)
        assert bool((buf[offset + need:] == fill).all()) and bool((buf[:offset] == fill).all())      # nothing written outside
    rc, stats, energy = raw_call(case, buf[:need - 256])
    assert rc == _lib.TE_ERR_WORKSPACE and bool((stats == -7).all()) and bool((energy == -7).all())  # outputs untouched


# ------------------------------------------------------------------------------------------------ graph capture, packed buffer
def test_captured_call_replays_equal_eager():
    """One capture, two replays on different inputs: one launch, nothing read back, no memset node."""
    from transformer_explainability_amd.generators import GraphedCall
    keys = ("heat", "labels", "target_id", "image_index")
    cases = [to(mask_case(33, 47, kind, seed=s), dev()) for kind, s in (("smooth", 1), ("levels", 2))]
    want = []
    for c in cases:
        flat = ops().localisation_metrics_packed(**c)[2]
        torch.cuda.synchronize()
        want.append(flat.clone())
    assert not torch.equal(want[0], want[1])
    call = GraphedCall(lambda h, l, t, i: ops().localisation_metrics_packed(h, labels=l, target_id=t, image_index=i)[2],
                       [cases[0][k] for k in keys])
    for i in (1, 0):
        got = call(*[cases[i][k] for k in keys])
        torch.cuda.synchronize()
        assert torch.equal(got, want[i]), i


def test_packed_buffer_dtypes_and_contiguity():
    case = to(mask_case(17, 19, "distinct", seed=4), dev())
    stats, energy, flat = ops().localisation_metrics_packed(**case)
    torch.cuda.synchronize()
    assert flat.dtype == torch.int64 and flat.shape == (6 * 7,)
    host = flat.cpu()
    assert torch.equal(host[:30].view(6, 5), stats.cpu()) and torch.equal(host[30:], bits(energy.cpu()).flatten())
    wide = torch.zeros((6, 17, 25), device=dev())
    wide[:, :, 3:22] = case["heat"]                                      # a strided view is made contiguous
    narrow = dict(case, heat=wide[:, :, 3:22], labels=case["labels"].to(torch.int32), target_id=case["target_id"].to(torch.int16))
    got = ops().localisation_metrics(**narrow)
    assert torch.equal(got[0], stats) and torch.equal(bits(got[1]), bits(energy))


# ------------------------------------------------------------------------------------------------ the evaluator
def assert_same_totals(ev, ref, n_valid, n_pairs):
    """Counts equal.  The sum of energy ratios within the energy bound the kernel is held to, 2 n_valid 2^-53 relative with
    n_valid the largest of any pair scored (what the issue sets; a ratio of two sums that each meet that bound, added up in
    another order, could in general need (4 n_valid + 2 P + 2) 2^-53 -- the evaluator is held to the narrower figure).  The sum
    of rank accuracies has no fp64 energy sum in it: the same P quotients of integers in another order, 2 P 2^-53."""
    assert torch.equal(ev.hits.cpu(), ref.hits) and torch.equal(ev.total.cpu(), ref.total) and int(ev.pairs) == int(ref.pairs)
    got, want = ev.sums.cpu(), ref.sums
    bound = torch.tensor([2.0 * n_valid, 2.0 * n_pairs], dtype=torch.float64) * ENERGY_EPS
    print(f"evaluator sums: |got - want| / |want| = {((got - want).abs() / want.abs()).tolist()}  bounds {bound.tolist()}")
    assert bool(((got - want).abs() <= bound * want.abs()).all()), (got, want, bound)
    a, b = ev.summary(), ref.summary()
    assert a["pairs"] == b["pairs"] and a["pg_acc"] == b["pg_acc"] and a["pg_acc_overall"] == b["pg_acc_overall"]
    for k, rel in zip(("energy", "rank_acc"), bound.tolist()):
        assert abs(a[k] - b[k]) <= rel * abs(b[k]), (k, a[k], b[k])


def test_evaluator_on_the_device_equals_its_cpu_path():
    L = loc()
    ev, ref = L.LocalisationEvaluator(3, tolerance=4), L.LocalisationEvaluator(3, tolerance=4)
    n_valid = 0
    for seed, kind in ((1, "smooth"), (2, "levels")):
        case = mask_case(33, 47, kind, seed=seed)
        case["target_id"][3] = -1                                                # a padded pair
        out = ev.update_from_heat(**to(case, dev()))
        want = ref.update_from_heat(**case)
        assert all(t.is_cuda for t in out) and torch.equal(out[0].cpu(), want[0])
        n_valid = max(n_valid, int(want[0][:, 0].max()))
    assert ev.hits.is_cuda and ev.sums.is_cuda and int(ref.pairs) > 0 and int(ref.hits.sum()) > 0
    assert_same_totals(ev, ref, n_valid, 12)
    box = box_case(3)
    cls = torch.tensor([2, 2, 0, 1])
    ev.update_from_heat(**to(box, dev()), classes=cls.to(dev()))
    ref.update_from_heat(**box, classes=cls)
    assert_same_totals(ev, ref, n_valid, 16)


def test_evaluator_update_on_a_small_vit():
    """update = one generate_classes pass + one heat-map launch + one scoring launch: its totals are those of scoring the maps
    of the generate_classes call it wraps, K = 2 classes per image and one padded pair."""
    from test_gpu_generate_all import vit_model
    from transformer_explainability_amd.generators import LRP
    L = loc()
    model, x, _ = vit_model("tiny")                                              # 2 images of 32 x 32, patches of 8, 10 classes
    B, K, side = x.shape[0], 2, x.shape[-1]
    classes = torch.tensor([[3, 8], [5, -1]], device=dev())
    labels = label_maps(B, side, side, 10, seed=12)
    for c in (3, 8):
        assert bool((labels[0] == c).any())
    assert bool((labels[1] == 5).any())
    ev = L.LocalisationEvaluator(10, tolerance=3, scale=8)
    stats, energy = ev.update(LRP(model), x, labels=labels.to(dev()), classes=classes, start_layer=1)
    torch.cuda.synchronize()
    assert stats.shape == (B * K, 5) and stats.is_cuda and stats[3].tolist() == list(L.SKIPPED_STATS)
    # the same maps, scored by the restatement on the CPU
    got = LRP(model).generate_classes(x, classes=classes, methods=("transformer_attribution",), start_layer=1)
    assert got.classes.tolist() == classes.tolist()
    heat = ops().heatmap(got.maps["transformer_attribution"].reshape(B * K, -1), scale=8, normalise=True)[:, 0].cpu()
    ref = L.LocalisationEvaluator(10, tolerance=3, scale=8)
    want = ref.update_from_heat(heat, labels=labels, target_id=classes.cpu().reshape(-1),
                                image_index=torch.tensor([0, 0, 1, -1]))
    compare("localisation_update_vit", (stats.cpu(), energy.cpu()), want)
    assert int(ref.pairs) == 3 and ref.total.tolist() == [0, 0, 0, 1, 0, 1, 0, 0, 1, 0]
    assert_same_totals(ev, ref, int(want[0][:, 0].max()), B * K)
    LRP(model).check()
