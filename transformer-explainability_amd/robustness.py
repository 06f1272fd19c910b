"""Robustness and complexity of a relevance map.

Robustness asks whether the map stays put when the input moves by an imperceptible amount: max- and average-sensitivity
(Yeh et al., NeurIPS 2019; captum's ``sensitivity_max``) and the local Lipschitz estimate (Alvarez-Melis & Jaakkola, 2018)
explain ``n_draws`` noisy copies of every image, drawn uniformly from the L-infinity ball of ``radius`` around the normalised
input, and compare their maps with the clean one.  Complexity asks whether the map is concentrated: Gini sparseness
(Chalasani et al., ICML 2020), entropy (Bhatt et al., IJCAI 2020) and the effective complexity at a relative threshold (Nguyen
& Martinez, 2020).  The reference tree has no such protocol: include/te_relprop.h ("robustness and complexity") is the
specification, the ``reference_*`` functions below restate it -- Philox in integer numpy, the noise in the kernels' own fp32
expression (equality is claimed), the sums in fp64 torch (a tolerance is claimed) -- and ``SensitivityEvaluator`` runs it
on the kernels of csrc/te_robust.hip: per chunk of draws one noise launch, one explanation of B n_d copies and two distance
launches, per batch one complexity launch (and, with more than one draw per pass, one reference pass of the clean images); nothing is read back before ``arrays()`` / ``summary()``.  On CPU tensors the
evaluator runs the restatements.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)
SCORE_NAMES = ("max_sens", "avg_sens", "lipschitz", "gini", "entropy", "n_eff")
# what integer inputs are refused with, here and by faithfulness.FaithfulnessEvaluator
DISCRETE_MSG = ("SensitivityEvaluator: noise on discrete inputs (BERT's token ids) is not defined here; "
                "the protocol takes the float images of a ViT / DeiT")


# ------------------------------------------------------------------------------------------------ the definitions
def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 (Salmon et al., SC 2011): counter [...,4] and key [...,2] of 32-bit words (broadcast against each other) ->
    uint32 [...,4].  Integer numpy on uint64, every product below 2^64."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK32
    k = np.asarray(key, dtype=np.uint64) & _MASK32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(int(rounds)):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _MASK32, (k1 + np.uint64(PHILOX_W1)) & _MASK32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def noise_words(B: int, n: int, n_draws: int, seed: int, id0: int = 0, d0: int = 0) -> np.ndarray:
    """uint32 [B,n_draws,n]: element e of draw d0 + j of sample id0 + b is word e & 3 of philox4x32 with the counter
    (e >> 2, d, low32(id), high32(id)) and the key (low32(seed), high32(seed)); seed and id are read as unsigned 64-bit."""
    B, n, n_draws, d0 = int(B), int(n), int(n_draws), int(d0)
    if B < 1 or n < 1 or n_draws < 1 or d0 < 0 or d0 + n_draws > 1 << 32:
        raise ValueError(f"noise_words: B {B}, n {n}, draws {d0} .. {d0 + n_draws - 1} do not name 32-bit draws of a batch")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    groups = -(-n // 4)
    ids = [(int(id0) + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)]
    counter = np.zeros((B, n_draws, groups, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(groups, dtype=np.uint64)
    counter[..., 1] = (np.arange(n_draws, dtype=np.uint64) + np.uint64(d0))[None, :, None]
    counter[..., 2] = np.array([i & 0xFFFFFFFF for i in ids], dtype=np.uint64)[:, None, None]
    counter[..., 3] = np.array([i >> 32 for i in ids], dtype=np.uint64)[:, None, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    return philox4x32(counter, key).reshape(B, n_draws, groups * 4)[:, :, :n]


def unit_noise(words: np.ndarray) -> np.ndarray:
    """s = 2 u - 1 in fp32 with u = float(w >> 8) 2^-24: both steps are exact; s lies in [-1, 1 - 2^-23]."""
    u = (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return np.float32(2.0) * u - np.float32(1.0)


def reference_noise(x, n_draws, radius, seed, id0=0, d0=0, out_dtype=torch.float32):
    """x [B,...] fp32 -> [B,n_draws,...]: x + s * radius in fp32, the product and the sum rounded once each (torch's own
    expression; the kernel's bits), then rounded once to ``out_dtype``.  On x's device, from words made on the host."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    radius = float(radius)
    if not (radius >= 0.0) or radius == float("inf"):
        raise ValueError(f"radius must be finite and not negative, got {radius}")
    B = x.shape[0]
    flat = x.reshape(B, -1).float()
    n = flat.shape[1]
    s = torch.from_numpy(unit_noise(noise_words(B, n, n_draws, seed, id0, d0))).to(flat.device)
    r = torch.tensor(radius, dtype=torch.float32, device=flat.device)
    y = flat[:, None, :] + s * r
    return y.to(out_dtype).reshape(B, int(n_draws), *x.shape[1:])


def reference_distance(a, b):
    """a [B,n], b [B,D,n] of any float dtype -> fp64 [B,D,3] = sum (b - a)^2, sum a^2, sum b^2 over n, in fp64 from the
    exact upcasts."""
    B = a.shape[0]
    a64 = a.reshape(B, 1, -1).double()
    b64 = b.reshape(B, b.shape[1], -1).double()
    if a64.shape[2] != b64.shape[2]:
        raise ValueError(f"reference_distance: a {tuple(a.shape)} and b {tuple(b.shape)} do not pair up")
    a64 = a64.expand_as(b64)
    return torch.stack([((b64 - a64) ** 2).sum(2), (a64 * a64).sum(2), (b64 * b64).sum(2)], 2)


def reference_complexity(maps, eps=1e-5):
    """maps [B,...] -> (out fp64 [B,2] = gini, entropy; counts int64 [B,2] = #(v > eps max v), #(v > 0)) of v = |maps[b]|:
    gini = sum_k (2k - n - 1) v_(k) / (n S) over v ascending, entropy = 0 - sum p ln p with p = v / S.  S == 0: NaN, NaN, 0,
    0; a NaN in the row: NaN, NaN, 0, 0."""
    eps = float(eps)
    if not (eps >= 0.0) or eps == float("inf"):
        raise ValueError(f"eps must be finite and not negative, got {eps}")
    B = maps.shape[0]
    v = maps.reshape(B, -1).double().abs()
    n = v.shape[1]
    bad = torch.isnan(v).any(1)
    v = torch.where(bad[:, None], torch.zeros_like(v), v)
    S = v.sum(1)
    weights = (2 * torch.arange(1, n + 1, device=v.device, dtype=torch.int64) - n - 1).double()
    gini = (weights * torch.sort(v, dim=1).values).sum(1) / (n * S)
    p = v / S[:, None]
    plogp = torch.where(v > 0, p * torch.log(torch.where(v > 0, p, torch.ones_like(p))), torch.zeros_like(p))
    entropy = 0.0 - plogp.sum(1)
    counts = torch.stack([(v > eps * v.max(1, keepdim=True).values).sum(1), (v > 0).sum(1)], 1).to(torch.int64)
    undefined = bad | (S == 0)
    out = torch.stack([gini, entropy], 1)
    out = torch.where(undefined[:, None], torch.full_like(out, float("nan")), out)
    counts = torch.where(undefined[:, None], torch.zeros_like(counts), counts)
    return out, counts


def scores_from_sums(map_sums, input_sums, norm0_sq=None):
    """The sums of map_distance for the map pairs and for the input pairs, fp64 [B,D,3] each -> {"sens" [B,D], "max_sens",
    "avg_sens", "lipschitz" [B]} in fp64 torch.  sens = sqrt(sum (dmap)^2) / (|map0| if |map0| != 0 else 1) (captum's rule)
    with |map0|^2 = norm0_sq [B] (default: the sum a^2 of the first pair); lipschitz = max_d |dmap| / |dx| over the pairs
    with |dx| != 0, NaN when there is none."""
    dmap = torch.sqrt(map_sums[..., 0])
    norm0 = torch.sqrt(map_sums[:, 0, 1] if norm0_sq is None else norm0_sq)
    sens = dmap / torch.where(norm0 != 0, norm0, torch.ones_like(norm0))[:, None]
    dx = torch.sqrt(input_sums[..., 0])
    moved = dx != 0
    ratio = torch.where(moved, dmap / torch.where(moved, dx, torch.ones_like(dx)), torch.full_like(dx, float("-inf")))
    lipschitz = torch.where(moved.any(1), ratio.max(1).values, torch.full_like(norm0, float("nan")))
    return {"sens": sens, "max_sens": sens.max(1).values, "avg_sens": sens.mean(1), "lipschitz": lipschitz}


def _paired_distance(distance, ref, maps):
    """ref and maps [B,D,n] -> sums [B,D,3] of the pairs (ref[b,d], maps[b,d]): ``distance`` on B D samples of one draw."""
    B, D, n = maps.shape
    return distance(ref.reshape(B * D, n), maps.reshape(B * D, 1, n)).reshape(B, D, 3)


def reference_scores(map0, maps, x0, xs, ref=None):
    """The clean maps [B,...], the copies' maps [B,D,...], the clean inputs [B,...] and the copies [B,D,...] ->
    ``scores_from_sums`` of their fp64 distances.  ref [B,D,...]: the clean map each copy's map is compared with (the
    evaluator's reference pass); default: map0 for every draw.  The norm is map0's either way."""
    B, D = maps.shape[0], maps.shape[1]
    norm0_sq = reference_distance(map0, map0.reshape(B, 1, -1))[:, 0, 1]
    if ref is None:
        map_sums = reference_distance(map0, maps)
    else:
        map_sums = _paired_distance(reference_distance, ref.reshape(B, D, -1), maps.reshape(B, D, -1))
    return scores_from_sums(map_sums, reference_distance(x0, xs), norm0_sq)


# ------------------------------------------------------------------------------------------------ the protocol
def _input_dtype(lrp, images, who: str, copies: str):
    """The dtype evaluator ``who`` makes its ``copies`` ("noisy" / "perturbed") in: the model's, else the images'."""
    model = getattr(lrp, "model", None)
    par = next(model.parameters(), None) if hasattr(model, "parameters") else None
    dtype = par.dtype if par is not None and par.is_floating_point() else images.dtype
    if dtype not in (torch.float32, torch.bfloat16):
        raise ops._lib.TeError(f"{who}: {ops.DTYPES_MSG}; the {copies} copies are made in float32 or "
                               f"bfloat16, the model is {dtype}")
    return dtype


class SensitivityEvaluator:
    """Sensitivity, local Lipschitz estimate and complexity of the maps of ``method`` over a dataset, batch by batch.

    ``update(images, index=None)`` explains the clean batch (generate_classes(topk=1), or ``classes=index``), keeps the classes
    on the device, and explains ``n_draws`` noisy copies of every image FOR THOSE CLASSES, ``draws_per_pass`` draws (default:
    all) as one batch of B n_d.  The copies are made in the model's dtype (fp32 or bf16) from the input the model saw, upcast
    exactly; sample ids run on across the calls, so that a dataset's noise does not depend on the batch size.  Per-sample
    results stay on the device until ``arrays()`` / ``summary()``.  ``generate_kwargs`` go to every generate_classes call.
    ViT / DeiT only: noise on token ids is not defined here.

    The reference pass.  A sample's map is not the same bits in a batch of B and in a batch of B n_d: the stock convolution
    and GEMMs of the forward pass pick their kernels by problem size (what is batch-independent bit for bit is relprop on the
    same cached tensors).  The difference a copy's map is measured by must not contain that, so with n_d > 1 the clean images
    are explained once more, for the fixed classes, in the shape of a pass of copies -- image b at the rows b n_d .. b n_d +
    n_d - 1 -- and the copy at row r is compared with the clean map of row r: the same launches on the same shapes, so that
    only the inputs differ and radius 0 gives exactly 0.  Every pass of copies has that one shape (the last one is filled up
    with further draws, which are dropped).  With draws_per_pass=1 the clean batch is its own reference and nothing is
    explained twice.  The norm in the sensitivity and the complexity scores are those of the clean batch's maps.

    ``keep_last=True`` is a hook of the tests: ``self.last`` then holds the tensors of the most recent ``update`` (clean
    maps, reference maps per draw, copies and their maps), nothing older."""

    def __init__(self, lrp, method="transformer_attribution", n_draws=10, radius=0.02, seed=0, draws_per_pass=None,
                 eps=1e-5, keep_last=False, **generate_kwargs):
        self.lrp, self.method = lrp, method
        self.n_draws, self.radius, self.seed, self.eps = int(n_draws), float(radius), int(seed), float(eps)
        if self.n_draws < 1:
            raise ValueError(f"n_draws must be at least 1, got {n_draws}")
        if not (self.radius >= 0.0) or self.radius == float("inf"):
            raise ValueError(f"radius must be finite and not negative, got {radius}")
        if not (self.eps >= 0.0) or self.eps == float("inf"):
            raise ValueError(f"eps must be finite and not negative, got {eps}")
        self.draws_per_pass = self.n_draws if draws_per_pass is None else min(int(draws_per_pass), self.n_draws)
        if self.draws_per_pass < 1:
            raise ValueError(f"draws_per_pass must be at least 1, got {draws_per_pass}")
        self.generate_kwargs = generate_kwargs
        self.keep_last = bool(keep_last)
        self.last = None                              # keep_last: the tensors the scores of the last update were made from
        self.samples = 0                              # the id of the next sample
        self._scores = {name: [] for name in SCORE_NAMES}

    def _explain(self, x, **which):
        got = self.lrp.generate_classes(x, methods=(self.method,), **which, **self.generate_kwargs)
        return got.classes, got.maps[self.method][:, 0]

    def update(self, images, index=None):
        if not torch.is_tensor(images) or not images.is_floating_point():
            raise ops._lib.TeError(DISCRETE_MSG)
        B = images.shape[0]
        dtype = _input_dtype(self.lrp, images, "SensitivityEvaluator", "noisy")
        device = images.is_cuda
        seen = images.to(dtype)                                        # the tensor the model sees
        clean = seen.float()                                           # ... upcast exactly
        if index is None:
            classes, map0 = self._explain(seen, topk=1)
        else:
            idx = index if torch.is_tensor(index) else torch.as_tensor(np.asarray(index))
            classes, map0 = self._explain(seen, classes=idx.reshape(B, 1))
        map0 = map0.detach().reshape(B, -1).float().clone()
        noise = ops.noise_inputs if device else reference_noise
        distance = ops.map_distance if device else reference_distance
        n_c = self.draws_per_pass                                      # every pass of copies has B n_c rows
        rows = (B * n_c,) + tuple(images.shape[1:])
        pass_classes = classes.repeat_interleave(n_c, 0)
        if n_c == 1:
            ref = map0.reshape(B, 1, -1)
        else:                                                          # the reference pass: the clean images in that shape
            _, ref = self._explain(seen.repeat_interleave(n_c, 0), classes=pass_classes)
            ref = ref.detach().reshape(B, n_c, -1).float().clone()
        map_sums, input_sums, kept = [], [], []
        for d0 in range(0, self.n_draws, n_c):
            n_d = min(n_c, self.n_draws - d0)                          # the draws of this pass that count
            copies = noise(clean, n_c, self.radius, self.seed, id0=self.samples, d0=d0, out_dtype=dtype)
            _, maps = self._explain(copies.reshape(rows), classes=pass_classes)
            maps = maps.detach().reshape(B, n_c, -1).float()
            map_sums.append(_paired_distance(distance, ref, maps)[:, :n_d])
            input_sums.append(distance(clean.reshape(B, -1), copies.reshape(B, n_c, -1))[:, :n_d])
            if self.keep_last:
                kept.append((maps[:, :n_d].clone(), copies[:, :n_d], ref[:, :n_d]))
        norm0_sq = distance(map0, map0.reshape(B, 1, -1))[:, 0, 1]
        scores = scores_from_sums(torch.cat(map_sums, 1), torch.cat(input_sums, 1), norm0_sq)
        out, counts = ops.map_complexity(map0, self.eps) if device else reference_complexity(map0, self.eps)
        for name in ("max_sens", "avg_sens", "lipschitz"):
            self._scores[name].append(scores[name])
        self._scores["gini"].append(out[:, 0])
        self._scores["entropy"].append(out[:, 1])
        self._scores["n_eff"].append(counts[:, 0])
        if self.keep_last:
            self.last = {"map0": map0, "x0": clean, "sens": scores["sens"], "id0": self.samples,
                         "maps": torch.cat([m for m, _, _ in kept], 1), "copies": torch.cat([c for _, c, _ in kept], 1),
                         "ref": torch.cat([r for _, _, r in kept], 1)}
        self.samples += B
        return classes

    def arrays(self):
        """{name: numpy [samples]} for SCORE_NAMES: the one place the results cross to the host."""
        return {name: (torch.cat(v, 0).cpu().numpy() if v else np.zeros((0,))) for name, v in self._scores.items()}

    def summary(self):
        """The means over the samples seen (NaN samples left out; NaN where none remains), plus ``samples``."""
        out = {}
        for name, a in self.arrays().items():
            a = a.astype(np.float64)
            ok = ~np.isnan(a)
            out[name] = float(a[ok].mean()) if ok.any() else float("nan")
        out["samples"] = self.samples
        return out
