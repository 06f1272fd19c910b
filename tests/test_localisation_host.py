"""CPU: the localisation test's definition (localisation.reference_metrics restates include/te_relprop.h in torch) against a
brute-force evaluation by plain loops over pixels and, where scipy is there, its Euclidean distance transform; the evaluator's
totals on CPU tensors against values computed by hand; what te_localisation_f32 refuses on the host, before any HIP call; and
the TeErrors of the ops wrapper."""
import math
import struct

import numpy as np
import pytest
import torch

from host_util import lib, status  # noqa: F401
from localisation_inputs import HEATS, SIZES, box_case, energy_bound, mask_case, rasterise, special_cases


def loc():
    from transformer_explainability_amd import localisation
    return localisation


# ------------------------------------------------------------------------------------------------ brute force
def key_of(v):
    """te_key of one cleaned value, from the bits of the fp32 number"""
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    if u == 0x80000000:
        u = 0
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def brute_force(heat, labels=None, target_id=None, image_index=None, boxes=None):
    """-> (stats rows, exact energies by math.fsum, target masks): one pixel at a time, straight from the header's text."""
    P, H, W = heat.shape
    rows, energies, masks = [], [], []
    for p in range(P):
        img = p if image_index is None else int(image_index[p])
        B = labels.shape[0] if labels is not None else P
        skip = img < 0 or img >= B or (labels is not None and int(target_id[p]) < 0)
        valid, target, ranked, terms_v, terms_t = [], [], [], [], []
        for y in range(H):
            for x in range(W):
                if skip:
                    v = t = False
                elif labels is not None:
                    lab = int(labels[img, y, x])
                    v = lab >= 0
                    t = v and lab == int(target_id[p])
                else:
                    v = True
                    t = any(int(b[0]) <= x < int(b[2]) and int(b[1]) <= y < int(b[3]) for b in boxes[p])
                h = float(heat[p, y, x])
                if math.isnan(h):
                    h = 0.0
                valid.append(v)
                target.append(t)
                if v:
                    ranked.append((-key_of(h), y * W + x))
                    terms_v.append(max(h, 0.0))
                    if t:
                        terms_t.append(max(h, 0.0))
        ranked.sort()                                                          # descending key, ascending index
        K = sum(target)
        argmax = ranked[0][1] if ranked else -1
        d2 = -1
        if ranked and K:
            ay, ax = divmod(argmax, W)
            d2 = min((i // W - ay) ** 2 + (i % W - ax) ** 2 for i in range(H * W) if target[i])
        hits = sum(1 for _, i in ranked[:K] if target[i])
        rows.append([sum(valid), K, argmax, d2, hits])
        energies.append([math.fsum(terms_t), math.fsum(terms_v)])
        masks.append(np.array(target).reshape(H, W))
    return torch.tensor(rows), torch.tensor(energies, dtype=torch.float64), masks


def assert_matches_brute_force(case, name):
    stats, energy = loc().reference_metrics(**case)
    want, exact, masks = brute_force(**case)
    assert stats.dtype == torch.int64 and energy.dtype == torch.float64
    assert stats.shape == want.shape and energy.shape == exact.shape
    assert torch.equal(stats, want), (name, stats, want)
    # against the exact sum a single fp64 sum is within n u; the bound of the tests is twice that
    assert bool(((energy - exact).abs() <= energy_bound(stats, exact)).all()), (name, energy, exact)
    return stats, energy, masks


@pytest.mark.parametrize("kind", HEATS)
@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_equals_brute_force_mask_mode(H, W, kind):
    case = mask_case(H, W, kind, seed=H * 100 + W)
    stats, _, masks = assert_matches_brute_force(case, (H, W, kind))
    try:
        from scipy import ndimage
    except ImportError:
        return
    for p in range(stats.shape[0]):                # d2_min is the squared Euclidean distance transform at the argmax
        if int(stats[p, 3]) >= 0:
            edt = ndimage.distance_transform_edt(~masks[p])
            ay, ax = divmod(int(stats[p, 2]), W)
            assert int(round(float(edt[ay, ax]) ** 2)) == int(stats[p, 3]), (H, W, kind, p)


@pytest.mark.parametrize("name", sorted(special_cases()))
def test_restatement_on_the_special_cases(name):
    case, expected = special_cases()[name]
    stats, energy, _ = assert_matches_brute_force(case, name)
    if expected is not None:
        for got, want in zip(stats[0].tolist(), expected):
            assert want is None or got == want, (name, stats[0].tolist(), expected)
    if name == "all_negative":
        assert energy[0].tolist() == [0.0, 0.0] and int(stats[0, 1]) > 0
    if name == "distance_225_is_a_hit":
        assert 0 <= int(stats[0, 3]) <= 15 ** 2
    if name == "distance_244_is_a_miss":
        assert int(stats[0, 3]) > 15 ** 2


@pytest.mark.parametrize("M", [1, 3])
def test_restatement_boxes_equal_the_rasterised_union(M):
    case = box_case(M)
    stats, energy, masks = assert_matches_brute_force(case, ("boxes", M))
    P, H, W = case["heat"].shape
    lab = rasterise(case["boxes"], H, W)
    for p in range(P):
        assert np.array_equal(masks[p], lab[p].numpy() == 1), p
    by_mask = loc().reference_metrics(case["heat"], labels=lab, target_id=torch.ones(P, dtype=torch.long))
    assert torch.equal(stats, by_mask[0]) and torch.equal(energy, by_mask[1])
    if M == 3:
        assert int(stats[0, 1]) == 7 * 8 + 8 * 7 - 3 * 3 and int(stats[2, 1]) == 0 and int(stats[3, 1]) == 9
        assert stats[2].tolist()[3:] == [-1, 0]
    else:
        assert stats[:, 1].tolist() == [7 * 8, 5 * 6, H * W, 0]


def test_restatement_skipped_pairs_and_shared_label_maps():
    case = mask_case(17, 19, "levels", seed=5)
    whole = loc().reference_metrics(**case)
    copies = dict(case, labels=case["labels"][case["image_index"]], image_index=None)
    each = loc().reference_metrics(**copies)
    assert torch.equal(whole[0], each[0]) and torch.equal(whole[1], each[1])
    tid, idx = case["target_id"].clone(), case["image_index"].clone()
    tid[1], idx[4] = -1, 2                                                       # B = 2: image 2 does not exist
    got = assert_matches_brute_force(dict(case, target_id=tid, image_index=idx), "skipped")
    for p in range(6):
        if p in (1, 4):
            assert got[0][p].tolist() == list(loc().SKIPPED_STATS) and got[1][p].tolist() == [0.0, 0.0]
        else:
            assert torch.equal(got[0][p], whole[0][p]) and torch.equal(got[1][p], whole[1][p])


# ------------------------------------------------------------------------------------------------ the evaluator
def hand_case():
    """Five pairs on 4 x 4 pixels, tolerance 1 -- see test_evaluator_totals_by_hand for the arithmetic."""
    lab0 = torch.tensor([[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, -1, -1], [2, 2, -1, -1]])
    labels = torch.stack([lab0, torch.zeros(4, 4, dtype=torch.long)])
    heat = torch.zeros(5, 4, 4)
    heat[0, 0, 0] = heat[0, 0, 2] = 1.0            # pair 0: image 0, class 0
    heat[1] = -1.0                                 # pair 1: image 0, class 1
    heat[1, 3, 0] = 2.0
    heat[2] = torch.arange(16.0).view(4, 4)        # pair 2: padded
    heat[3] = torch.arange(16.0).view(4, 4)        # pair 3: image 1, class 3 -- no pixel of it
    heat[4] = -torch.arange(1.0, 17.0).view(4, 4)  # pair 4: image 1, class 0 -- every pixel, all-negative map
    return dict(heat=heat, labels=labels, target_id=torch.tensor([0, 1, -1, 3, 0]), image_index=torch.tensor([0, 0, 0, 1, 1]))


def test_evaluator_totals_by_hand():
    """pair 0: the argmax (0, 0) is on class 0 -> hit; e = 1 / 2; top 4 = pixels 0, 2 (the ones) and 1, 3 (the first zeros), of
               which 0 and 1 are class 0 -> 2 / 4.
    pair 1: the argmax (3, 0) is sqrt(8) from class 1 -> miss at tolerance 1; e = 0 / 2; top 4 = pixel 12 and 0, 1, 2 -> 1 / 4.
    pair 2: padded (target_id -1), pair 3: class 3 has no pixel -> neither counts.
    pair 4: every pixel is class 0 -> hit, 16 / 16; all heat negative -> e_valid == 0, energy counts 0."""
    ev = loc().LocalisationEvaluator(n_classes=4, tolerance=1)
    assert ev.summary() == {"pg_acc": 0.0, "pg_acc_overall": 0.0, "energy": 0.0, "rank_acc": 0.0, "pairs": 0}
    stats, energy = ev.update_from_heat(**hand_case())
    assert stats.tolist() == [[12, 4, 0, 0, 2], [12, 4, 12, 8, 1], [0, 0, -1, -1, 0], [16, 0, 15, -1, 0], [16, 16, 0, 0, 16]]
    assert energy.tolist() == [[1.0, 2.0], [0.0, 2.0], [0.0, 0.0], [0.0, 120.0], [0.0, 0.0]]
    assert ev.hits.tolist() == [2, 0, 0, 0] and ev.total.tolist() == [2, 1, 0, 0] and int(ev.pairs) == 3
    s = ev.summary()
    assert s["pairs"] == 3 and s["pg_acc"] == 0.5 and s["pg_acc_overall"] == 2 / 3
    assert s["energy"] == (0.5 + 0.0 + 0.0) / 3 and s["rank_acc"] == (0.5 + 0.25 + 1.0) / 3
    # a second batch adds up; a class outside [0, n_classes) is not counted
    case = hand_case()
    ev.update_from_heat(**case, classes=torch.tensor([0, 1, -1, 3, 7]))
    assert ev.hits.tolist() == [3, 0, 0, 0] and ev.total.tolist() == [3, 2, 0, 0] and ev.summary()["pairs"] == 5
    # tolerance 3: sqrt(8) is inside
    wide = loc().LocalisationEvaluator(n_classes=4, tolerance=3)
    wide.update_from_heat(**hand_case())
    assert wide.hits.tolist() == [2, 1, 0, 0] and wide.summary()["pg_acc"] == 1.0


def test_evaluator_boxes_on_cpu():
    case = box_case(3)
    ev = loc().LocalisationEvaluator(n_classes=5)
    stats, _ = ev.update_from_heat(**case, classes=torch.tensor([4, 4, 2, 0]))
    assert ev.total.tolist() == [1, 0, 0, 0, 2] and int(ev.pairs) == 3          # pair 2 has no target
    with pytest.raises(ValueError):
        ev.update_from_heat(**case)                                              # no classes, no target_id


# ------------------------------------------------------------------------------------------------ refusals on the host
P = 4096      # a fake non-null, 16-byte-aligned address: every call below returns before the first HIP call


def test_entry_point_rejects_on_the_host(lib):
    from transformer_explainability_amd import _lib
    INVALID, WORKSPACE, UNSUPPORTED = _lib.TE_ERR_INVALID_ARG, _lib.TE_ERR_WORKSPACE, _lib.TE_ERR_UNSUPPORTED
    q = lib.te_localisation_workspace_bytes
    need = q(6, 17, 19)
    assert need >= 6 * (17 * 19 * 4 + 17 * 19 // 8) and need % 256 == 0 and lib.te_version() >= 703 and _lib.MIN_LIB_VERSION >= 703
    assert [q(*a) for a in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (65536, 4, 4), (2, 1025, 1024), (2, 1, (1 << 20) + 1))] == [0] * 6
    assert q(1, 1024, 1024) >= (4 << 20) + (1 << 17) and q(65535, 1, 1) > 0
    f = "te_localisation_f32"
    base = dict(heat=P, labels=P, image_index=P, target_id=P, boxes=None, M=0, stats=P, energy=P, P=6, B=2, H=17, W=19, ws=P,
                ws_bytes=need, stream=None)
    assert tuple(base) == _lib.PARAMS[f]
    assert [status(lib, f, base, heat=None), status(lib, f, base, stats=None), status(lib, f, base, energy=None),
            status(lib, f, base, target_id=None)] == [INVALID] * 4
    assert [status(lib, f, base, P=0), status(lib, f, base, B=0), status(lib, f, base, H=0), status(lib, f, base, W=-1)] == [INVALID] * 4
    assert status(lib, f, base, boxes=P, M=2) == INVALID                          # both
    assert status(lib, f, base, labels=None) == INVALID                           # neither
    boxes = dict(base, labels=None, target_id=None, boxes=P, M=3)
    assert [status(lib, f, boxes, M=0), status(lib, f, boxes, M=-2)] == [INVALID] * 2
    assert [status(lib, f, base, H=1025, W=1024), status(lib, f, base, P=65536), status(lib, f, boxes, M=65)] == [UNSUPPORTED] * 3
    assert [status(lib, f, base, ws=None), status(lib, f, base, ws_bytes=need - 256), status(lib, f, boxes, ws_bytes=0)] == [WORKSPACE] * 3
    # 8-byte alignment is an argument check: it comes first, also when the workspace is too small as well
    assert [status(lib, f, base, ws=P + 4), status(lib, f, base, ws=P + 4, ws_bytes=0),
            status(lib, f, base, ws=P + 4, P=65536)] == [INVALID] * 3
    # the order: an invalid argument before an unsupported size before the workspace
    assert status(lib, f, base, heat=None, P=65536, ws=None) == INVALID
    assert status(lib, f, boxes, M=0, H=1025, W=1024) == INVALID
    assert status(lib, f, base, P=65536, ws=None) == UNSUPPORTED
    assert status(lib, f, boxes, M=65, ws_bytes=0) == UNSUPPORTED
    # an image_index is optional in both modes
    assert status(lib, f, base, image_index=None, ws=None) == WORKSPACE


def test_ops_refuse_cpu_tensors_wrong_dtypes_and_wrong_shapes():
    from transformer_explainability_amd import TeError, ops
    case = mask_case(5, 13)
    box = box_case(3)
    heat, labels, tid, idx = case["heat"], case["labels"], case["target_id"], case["image_index"]
    with pytest.raises(TeError, match="no CPU fallback"):
        ops.localisation_metrics(**case)
    with pytest.raises(TeError, match="no CPU fallback"):
        ops.localisation_metrics_packed(**box)
    # every other refusal is named by its own message: none of them is the final "no CPU fallback" check
    lm = ops.localisation_metrics
    calls = [("float32 heat map", lambda: lm(heat.double(), labels=labels, target_id=tid, image_index=idx)),
             ("float32 heat map", lambda: lm(heat.half(), boxes=box["boxes"])),
             ("integer labels", lambda: lm(heat, labels=labels.float(), target_id=tid, image_index=idx)),
             ("integer target_id", lambda: lm(heat, labels=labels, target_id=tid.float(), image_index=idx)),
             ("integer image_index", lambda: lm(heat, labels=labels, target_id=tid, image_index=idx.bool())),
             ("integer boxes", lambda: lm(box["heat"], boxes=box["boxes"].float())),
             ("exactly one of", lambda: lm(heat)),
             ("exactly one of", lambda: lm(heat, labels=labels, target_id=tid, image_index=idx, boxes=box["boxes"])),
             ("needs target_id", lambda: lm(heat, labels=labels, image_index=idx)),
             ("need image_index", lambda: lm(heat, labels=labels, target_id=tid)),               # 2 label maps, 6 pairs
             (r"heat must be \[P,H,W\]", lambda: lm(heat[0], labels=labels, target_id=tid, image_index=idx)),
             (r"heat must be \[P,H,W\]", lambda: lm(heat[:0], labels=labels, target_id=tid[:0], image_index=idx[:0])),
             ("labels must be", lambda: lm(heat, labels=labels[:, :4], target_id=tid, image_index=idx)),
             ("labels must be", lambda: lm(heat, labels=labels[0], target_id=tid, image_index=idx)),
             ("target_id must be", lambda: lm(heat, labels=labels, target_id=tid[:5], image_index=idx)),
             ("image_index must be", lambda: lm(heat, labels=labels, target_id=tid, image_index=idx.view(2, 3))),
             ("boxes must be", lambda: lm(box["heat"], boxes=box["boxes"][:3])),
             ("boxes must be", lambda: lm(box["heat"], boxes=box["boxes"][:, :, :3])),
             ("boxes must be", lambda: lm(box["heat"], boxes=box["boxes"][:, :0])),
             ("heat must be a tensor", lambda: lm(heat.numpy(), labels=labels, target_id=tid, image_index=idx)),
             ("boxes must be a tensor", lambda: lm(box["heat"], boxes=box["boxes"].tolist()))]
    for i, (message, call) in enumerate(calls):
        with pytest.raises(TeError, match=message) as err:
            call()
        assert "no CPU fallback" not in str(err.value), i
