"""Localisation test of a relevance map against a ground-truth region: the pointing game with its 15-pixel tolerance
(Zhang et al., IJCV 2018), the energy-based pointing game / relevance mass accuracy (Wang et al., CVPRW 2020; Arras et
al., Information Fusion 2022) and relevance rank accuracy (Arras et al. 2022).

The protocol is per (image, class) PAIR: for every class present in an image, explain that class and score the map
against that class's region -- the label map's pixels of that class, or the union of the class's boxes.  The reference
tree has no such protocol (its one ground-truth test thresholds the map at its mean, segmentation.py):
include/te_relprop.h ("localisation test") is the specification, ``reference_metrics`` below restates it in torch, and
``LocalisationEvaluator`` runs it on the kernel of csrc/te_localise.hip -- per batch one ``generate_classes`` pass, one
heat-map launch and one scoring launch; the running totals stay on the device until ``summary()``.  On CPU tensors the
evaluator runs the restatement.
"""
from __future__ import annotations

import torch

from . import ops

SKIPPED_STATS = (0, 0, -1, -1, 0)
_INDEX_BITS = 21                                   # H*W <= 2^20 < 2^21: key << 21 | (2^21 - 1 - index) fits an int64


# ------------------------------------------------------------------------------------------------ the definition
def clean_heat(heat):
    """NaN -> +0.0 and -0.0 -> +0.0: the values the scores are defined on."""
    h = torch.where(torch.isnan(heat), torch.zeros_like(heat), heat)
    return h + 0.0


def order_keys(h):
    """te_key (csrc/te_common.h) of cleaned fp32 values as int64 in (0, 2^32): a > b as numbers <=> key(a) > key(b)."""
    u = h.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    return torch.where(u >= 0x80000000, u ^ 0xffffffff, u | 0x80000000)


def pixel_sets(P, H, W, device, labels=None, target_id=None, image_index=None, boxes=None):
    """(valid, target, skipped): bool [P, H*W], [P, H*W], [P] as the specification defines them."""
    n = H * W
    if (labels is None) == (boxes is None):
        raise ValueError("give exactly one of labels= and boxes=")
    idx = torch.arange(P, device=device) if image_index is None else image_index.to(torch.int64)
    if labels is not None:
        B = labels.shape[0]
        tid = target_id.to(torch.int64)
        skipped = (tid < 0) | (idx < 0) | (idx >= B)
        lab = labels.reshape(B, n).to(torch.int64)[idx.clamp(0, B - 1)]
        valid = (lab >= 0) & ~skipped[:, None]
        return valid, valid & (lab == tid[:, None]), skipped
    skipped = (idx < 0) | (idx >= P)
    pix = torch.arange(n, device=device)
    y, x = (pix // W).view(1, 1, n), (pix % W).view(1, 1, n)
    b = boxes.to(torch.int64)
    inside = ((b[:, :, 0:1] <= x) & (x < b[:, :, 2:3]) & (b[:, :, 1:2] <= y) & (y < b[:, :, 3:4])).any(1)
    valid = (~skipped)[:, None].expand(P, n)
    return valid, inside & valid, skipped


def reference_metrics(heat, labels=None, target_id=None, image_index=None, boxes=None):
    """The specification in torch, on the tensors' own device (the tests run it on the CPU): the arguments of
    ops.localisation_metrics -> (stats int64 [P,5] = n_valid, n_target, argmax, d2_min, topk_hits; energy float64 [P,2] =
    e_target, e_valid).  The ranking is one sort per pair of key << 21 | (2^21 - 1 - index): descending value, ties in
    ascending pixel index, pixels that are not valid (key 0) last."""
    if heat.dtype != torch.float32 or heat.dim() != 3:
        raise ValueError(f"heat must be float32 [P,H,W], got {heat.dtype} {tuple(heat.shape)}")
    P, H, W = heat.shape
    n, dev = H * W, heat.device
    valid, target, _ = pixel_sets(P, H, W, dev, labels, target_id, image_index, boxes)
    h = clean_heat(heat.reshape(P, n))
    pix = torch.arange(n, device=dev)
    last = (1 << _INDEX_BITS) - 1
    comp = (torch.where(valid, order_keys(h), torch.zeros((), dtype=torch.int64, device=dev)) << _INDEX_BITS) | (last - pix)
    n_valid, n_target = valid.sum(1), target.sum(1)
    have = n_valid > 0
    argmax = last - (comp.max(1).values & last)
    ay, ax = (argmax // W)[:, None], (argmax % W)[:, None]
    d2 = (pix // W - ay) ** 2 + (pix % W - ax) ** 2
    far = torch.iinfo(torch.int64).max
    d2_min = torch.where(target, d2, torch.full_like(d2, far)).min(1).values
    minus = torch.full_like(argmax, -1)
    order = torch.argsort(comp, dim=1, descending=True)
    top = pix[None, :] < n_target[:, None]
    hits = (torch.gather(target, 1, order) & top).sum(1)
    stats = torch.stack([n_valid, n_target, torch.where(have, argmax, minus),
                         torch.where(have & (n_target > 0), d2_min, minus), hits], 1)
    e = h.clamp(min=0).double()
    zero = torch.zeros_like(e)
    energy = torch.stack([torch.where(target, e, zero).sum(1), torch.where(valid, e, zero).sum(1)], 1)
    return stats, energy


# ------------------------------------------------------------------------------------------------ the evaluator
class LocalisationEvaluator:
    """Running totals of the three scores over (image, class) pairs.  A pair counts when it has a target pixel, was not
    skipped and its class lies in [0, n_classes); ``tolerance`` is the pointing game's radius in pixels (a hit: the most
    relevant pixel lies within ``tolerance`` pixels of the region), ``scale`` the up-sampling factor of ``ops.heatmap``
    (the patch size)."""

    def __init__(self, n_classes, tolerance=15, scale=16):
        if int(n_classes) < 1 or int(tolerance) < 0:
            raise ValueError(f"n_classes must be positive and tolerance non-negative, got {n_classes}, {tolerance}")
        self.n_classes, self.tolerance, self.scale = int(n_classes), int(tolerance), int(scale)
        self.hits = self.total = self.pairs = self.sums = None      # int64 [C], [C], [1]; float64 [2] = sum ratio, sum rank acc

    def _totals_on(self, device):
        if self.hits is None:
            self.hits = torch.zeros(self.n_classes, dtype=torch.int64, device=device)
            self.total = torch.zeros_like(self.hits)
            self.pairs = torch.zeros(1, dtype=torch.int64, device=device)
            self.sums = torch.zeros(2, dtype=torch.float64, device=device)
        elif self.hits.device != device:
            self.hits, self.total, self.pairs, self.sums = (t.to(device) for t in (self.hits, self.total, self.pairs, self.sums))

    def add(self, stats, energy, classes):
        """Add the pairs of one scoring call to the totals, on the device of ``stats``; nothing is read back."""
        self._totals_on(stats.device)
        cls = classes.to(device=stats.device, dtype=torch.int64).reshape(-1)
        n_target, d2, topk = stats[:, 1], stats[:, 3], stats[:, 4]
        counted = (n_target > 0) & (cls >= 0) & (cls < self.n_classes)
        hit = counted & (d2 >= 0) & (d2 <= self.tolerance ** 2)
        at = cls.clamp(0, self.n_classes - 1)
        self.hits.index_add_(0, at, hit.to(torch.int64))
        self.total.index_add_(0, at, counted.to(torch.int64))
        e_t, e_v = energy[:, 0], energy[:, 1]
        zero = torch.zeros_like(e_t)
        ratio = torch.where(e_v == 0, zero, e_t / torch.where(e_v == 0, torch.ones_like(e_v), e_v))
        rank = topk.double() / n_target.clamp(min=1).double()
        self.sums += torch.stack([torch.where(counted, ratio, zero).sum(), torch.where(counted, rank, zero).sum()])
        self.pairs += counted.sum()

    def update_from_heat(self, heat, labels=None, boxes=None, target_id=None, image_index=None, classes=None):
        """heat [P,H,W] fp32 (or [P,1,H,W]) against ``labels`` [B,H,W] or ``boxes`` [P,M,4]; ``classes`` [P] is the class a
        pair is counted under (default: ``target_id``).  CUDA tensors are scored by ops.localisation_metrics, CPU tensors by
        reference_metrics; the totals are updated on that device and nothing is read back.  -> (stats, energy)."""
        if heat.dim() == 4 and heat.shape[1] == 1:
            heat = heat[:, 0]
        if classes is None:
            classes = target_id
        if classes is None:
            raise ValueError("update_from_heat: classes= [P] (or target_id=) says which class every pair is counted under")
        score = ops.localisation_metrics if heat.is_cuda else reference_metrics
        stats, energy = score(heat.float(), labels=labels, target_id=target_id, image_index=image_index, boxes=boxes)
        self.add(stats, energy, classes)
        return stats, energy

    def update(self, generator, images, labels=None, boxes=None, classes=None, target_id=None,
               method="transformer_attribution", **kw):
        """One ``generator.generate_classes(images, classes=classes, methods=(method,), **kw)`` pass for the K classes of
        every image (``classes`` [B,K]; -1 in a device tensor is a padded pair), one ``ops.heatmap`` over the B*K maps, then
        update_from_heat: ``labels`` [B,H,W] shared by an image's K pairs, or ``boxes`` [B,K,M,4].  ``target_id`` [B,K]: the
        label value of every pair's region (default: its class)."""
        if classes is None:
            raise ValueError("update: classes= [B,K], the classes to explain and score per image")
        got = generator.generate_classes(images, classes=classes, methods=(method,), **kw)
        maps = got.maps[method].detach()
        B, K = maps.shape[:2]
        cls = (got.classes if got.classes is not None else torch.as_tensor(classes).reshape(B, K)).to(maps.device).reshape(-1)
        heat = ops.heatmap(maps.reshape(B * K, -1).float(), scale=self.scale, normalise=True)[:, 0]
        image = torch.arange(B, device=maps.device).repeat_interleave(K)
        image = torch.where(cls < 0, torch.full_like(image, -1), image)        # a padded pair is a skipped pair
        tid = cls if target_id is None else torch.as_tensor(target_id).to(maps.device).reshape(-1)
        if boxes is not None:
            boxes = boxes.reshape(B * K, -1, 4)
        return self.update_from_heat(heat, labels=labels, boxes=boxes, target_id=None if labels is None else tid,
                                     image_index=image, classes=cls)

    def summary(self):
        """pg_acc: the mean over the classes that occurred of hits / total; pg_acc_overall: all hits / all pairs; energy: the
        mean of e_target / e_valid (0 where e_valid == 0); rank_acc: the mean of topk_hits / n_target; pairs: the pairs
        counted.  One device-to-host copy."""
        if self.hits is None:
            return {"pg_acc": 0.0, "pg_acc_overall": 0.0, "energy": 0.0, "rank_acc": 0.0, "pairs": 0}
        C = self.n_classes
        host = torch.cat([self.hits, self.total, self.pairs, self.sums.view(torch.int64)]).cpu()
        hits, total, pairs = host[:C].double(), host[C:2 * C].double(), int(host[2 * C])
        sums = host[2 * C + 1:].view(torch.float64)
        seen = total > 0
        if pairs == 0:
            return {"pg_acc": 0.0, "pg_acc_overall": 0.0, "energy": 0.0, "rank_acc": 0.0, "pairs": 0}
        return {"pg_acc": float((hits[seen] / total[seen]).mean()), "pg_acc_overall": float(hits.sum() / total.sum()),
                "energy": float(sums[0]) / pairs, "rank_acc": float(sums[1]) / pairs, "pairs": pairs}
