"""Inputs of the localisation tests (CPU and -m gpu), seeded and generated on the CPU.  A case is a dict of the arguments
of ops.localisation_metrics / localisation.reference_metrics: heat [P,H,W] and either labels [B,H,W] + target_id [P]
(+ image_index [P]) or boxes [P,M,4]."""
import torch

SIZES = [(1, 1), (1, 7), (7, 1), (5, 13), (16, 16), (17, 19), (96, 96)]
HEATS = ["distinct", "levels", "smooth"]
ENERGY_EPS = 2.0 ** -53


def gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum(int(s) * 7919 ** i for i, s in enumerate(seed)) % (2 ** 31))
    return g


def heat_maps(P, H, W, kind="distinct", seed=0):
    g = gen(1, seed, P, H, W)
    if kind == "distinct":                         # both signs
        return torch.randn((P, H, W), generator=g)
    if kind == "levels":                           # five values: the select meets heavy ties at every digit
        return torch.tensor([-1.0, 0.0, 0.25, 0.5, 2.0])[torch.randint(5, (P, H, W), generator=g)]
    if kind == "smooth":                           # what ops.heatmap makes: bilinear, replicated borders, in [0, 1]
        small = torch.rand((P, 1, max(1, H // 4), max(1, W // 4)), generator=g)
        big = torch.nn.functional.interpolate(small, size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        lo, hi = big.flatten(1).min(1).values.view(P, 1, 1), big.flatten(1).max(1).values.view(P, 1, 1)
        return ((big - lo) / (hi - lo).clamp(min=1e-30)).contiguous()
    raise ValueError(kind)


def label_maps(B, H, W, n_classes=3, seed=0, ignore=0.1):
    """Random regions: a class per 3 x 3 cell, and about ``ignore`` of the pixels at -1."""
    g = gen(2, seed, B, H, W)
    cells = torch.randint(n_classes, (B, (H + 2) // 3, (W + 2) // 3), generator=g)
    lab = cells.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :H, :W].contiguous()
    lab[torch.rand((B, H, W), generator=g) < ignore] = -1
    return lab


def mask_case(H, W, kind="distinct", seed=0):
    """Two images, three classes each: six pairs that share two label maps through image_index."""
    B, K = 2, 3
    return dict(heat=heat_maps(B * K, H, W, kind, seed), labels=label_maps(B, H, W, K, seed),
                target_id=torch.arange(K).repeat(B), image_index=torch.arange(B).repeat_interleave(K))


def single(heat, labels, target=1):
    """One pair from one [H,W] heat map and one [H,W] label map."""
    return dict(heat=heat[None].contiguous().float(), labels=labels[None].contiguous().long(),
                target_id=torch.tensor([target]))


SH, SW = 20, 23                                    # the special cases: an odd width, room for the offsets (10, 12)


def special_cases():
    """{name: (case, expected stats row or None)}: the inputs a wrong kernel gets wrong, 20 x 23 pixels each."""
    H, W, n = SH, SW, SH * SW
    g = gen(3)
    half = torch.zeros(H, W, dtype=torch.long)
    half[:, W // 2:] = 1                           # the right half is the target
    rnd = torch.randn((H, W), generator=g)
    out = {}

    # the top 240 of a constant map are the pixels 0 .. 239: ten rows of 12 targets, and ten pixels of row 10 left of them
    out["constant"] = (single(torch.full((H, W), 0.5), half), [n, H * (W - W // 2), 0, (W // 2) ** 2, 120])

    two = rnd.clone().clamp(max=1.0)
    two[7, 15] = two[3, 2] = 5.0                   # equal maxima: the lower index (3, 2) is the argmax
    out["two_equal_maxima"] = (single(two, half), [n, None, 3 * W + 2, (W // 2 - 2) ** 2, None])

    # K = 6 targets; two pixels at 1.0 (one a target), everything else ties at 0.25: the top 6 are the two and the FIRST four
    # tied pixels in index order (0, 1, 2, 3), of which 1 and 3 are targets -> 3 hits
    tie = torch.full((H, W), 0.25)
    lab = torch.zeros(H, W, dtype=torch.long)
    flat_t, flat_l = tie.view(-1), lab.view(-1)
    flat_t[200], flat_t[300] = 1.0, 1.0
    for i in (1, 3, 50, 51, 52, 300):
        flat_l[i] = 1
    out["kth_value_tied_across_target_and_not"] = (single(tie, lab), [n, 6, 200, None, 3])

    zeros = torch.zeros(H, W)
    zeros.view(-1)[::2] = -0.0                     # -0.0 at 0, 2, ...: equal to +0.0, so the argmax is pixel 0
    zeros[5, 5:9] = -1.0
    out["signed_zeros"] = (single(zeros, half), [n, None, 0, (W // 2) ** 2, None])

    nan = rnd.clone()
    nan[0, :] = float("nan")
    nan[10, 3::4] = float("nan")
    nan[nan > 0] *= -1                             # everything else negative: the NaN pixels (+0.0) are the maxima, pixel 0 first
    out["nan_pixels"] = (single(nan, half), [n, None, 0, (W // 2) ** 2, None])

    out["all_negative"] = (single(-rnd.abs() - 0.5, half), None)              # e_valid == 0
    out["every_pixel_ignored"] = (single(rnd, torch.full((H, W), -1)), [0, 0, -1, -1, 0])
    out["no_target"] = (single(rnd, torch.zeros(H, W, dtype=torch.long)), [n, 0, None, -1, 0])
    out["every_pixel_a_target"] = (single(rnd, torch.ones(H, W, dtype=torch.long)), [n, n, None, 0, n])

    corner = rnd.clone().clamp(max=1.0)
    corner[H - 1, W - 1] = 7.0
    lab = torch.zeros(H, W, dtype=torch.long)
    lab[0, 0] = 1
    out["argmax_in_the_last_corner"] = (single(corner, lab), [n, 1, n - 1, (H - 1) ** 2 + (W - 1) ** 2, None])

    for name, (dy, dx) in (("distance_225_is_a_hit", (9, 12)), ("distance_244_is_a_miss", (10, 12))):
        peak = rnd.clone().clamp(max=1.0)
        peak[3, 4] = 9.0
        lab = torch.zeros(H, W, dtype=torch.long)
        lab[3 + dy, 4 + dx] = 1
        lab[H - 1, 0] = 1                          # a farther target
        out[name] = (single(peak, lab), [n, 2, 3 * W + 4, dy * dy + dx * dx, None])
    return out


def rasterise(boxes, H, W):
    """labels [P,H,W]: 1 inside the union of a pair's boxes, 0 outside (every pixel valid), by plain loops."""
    P, M = boxes.shape[:2]
    lab = torch.zeros((P, H, W), dtype=torch.long)
    for p in range(P):
        for m in range(M):
            x0, y0, x1, y1 = (int(v) for v in boxes[p, m])
            if x1 <= x0 or y1 <= y0:
                continue
            lab[p, max(y0, 0):max(min(y1, H), 0), max(x0, 0):max(min(x1, W), 0)] = 1
    return lab


def box_case(M, H=17, W=19, seed=0):
    """Four pairs.  M = 3: overlapping boxes, a padding row, a box partly outside, boxes wholly outside (no target);
    M = 1: one box each -- inside, partly outside, covering everything, empty."""
    heat = heat_maps(4, H, W, "distinct", seed)
    if M == 1:
        boxes = torch.tensor([[[2, 3, 9, 11]], [[-4, -2, 5, 6]], [[-1, -1, W + 3, H + 3]], [[5, 5, 5, 9]]])
    else:
        boxes = torch.tensor([[[2, 3, 9, 11], [6, 8, 14, 15], [0, 0, 0, 0]],           # overlap + padding
                              [[W - 4, H - 3, W + 10, H + 10], [4, 4, 3, 9], [0, 0, 2, 2]],   # partly outside + empty row
                              [[W, 0, W + 5, H], [-7, -7, 0, 0], [0, H, W, H + 1]],     # wholly outside: no target
                              [[1, 1, 4, 4], [1, 1, 4, 4], [2, 2, 3, 3]]])              # the same box twice and one inside it
    assert boxes.shape == (4, M, 4)
    return dict(heat=heat, boxes=boxes)


def to(case, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in case.items()}


def energy_bound(stats, ref_energy):
    """|sum - sum'| <= 2 n_valid 2^-53 sum for two fp64 sums of the same non-negative terms in any order: each is within
    (n - 1) u (1 + O(n u)) of the exact sum, u = 2^-53."""
    return 2.0 * stats[:, 0:1].double() * ENERGY_EPS * ref_energy.abs()
