"""Sanity checks of an explanation method: how similar two relevance maps are, and the two protocols built on that number.

  * the model-parameter randomisation test of Adebayo et al., "Sanity Checks for Saliency Maps" (NeurIPS 2018): re-initialise
    the weights from the logits downwards, stage by stage, explain the SAME input for the SAME class at every stage and
    report how similar the map stays to the original (``randomized``, ``SanityCheckEvaluator``);
  * class sensitivity: the similarity of the maps of the two top classes of an input (``class_sensitivity``) -- the number
    behind "raw attention and rollout are class-agnostic, transformer_attribution is not".

The reference tree has neither protocol: the definitions in include/te_relprop.h ("map similarity") are the specification.
On the MI355X the similarity is the te_map_similarity_f32 kernel pair (ops.map_similarity: two launches per call, nothing
read back); the torch functions below are the CPU path and the restatement the kernels are tested against, themselves pinned
to scipy.stats (rankdata, spearmanr, pearsonr) and to a window-by-window SSIM in the CPU suite.

    ranks     ascending in the order of te_key (-0 == +0); a run of equal values at the 0-based sorted positions s .. e-1 gets
              the average rank (s + e + 1) / 2; kept as the integer d = 2 rank - (n + 1) = s + e - n
    rank_sums (cov, va, vb) = (sum d_a d_b, sum d_a^2, sum d_b^2) in int64, for the values and for the absolute values
    spearman  cov / (sqrt(va) sqrt(vb)), clamped to [-1, 1]; NaN when va == 0 or vb == 0; exactly +-1 when |cov| == va == vb
    pearson   two passes in fp64: the means, then sab / (sqrt(saa) sqrt(sbb)) of the centred values, clamped; NaN when
              saa == 0 or sbb == 0
    ssim      scikit-image's structural_similarity at its defaults for a 2-D image (7x7 uniform window, sample covariance,
              C1 = (0.01 L)^2, C2 = (0.03 L)^2), the mean over the (H-6)(W-6) windows inside the image
    NaN rule  a sample with a NaN anywhere in a or b: an all-NaN sim row, an all-zero rank_sums row
"""
from __future__ import annotations

import contextlib
import math
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

SIM_COLUMNS = ("pearson", "spearman", "spearman_abs", "ssim")
_WIN = 7


# ------------------------------------------------------------------------------------------------ the torch restatement
def _keys(x):
    """te_key (csrc/te_common.h) of fp32 values as int64: a > b as numbers (-0 == +0, NaN largest) <=> key(a) > key(b)."""
    u = x.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    return torch.where(u >= 0x80000000, u ^ 0xffffffff, u | 0x80000000)


def rank_deltas(x):
    """[..., n] -> int64 [..., n]: d = 2 rank - (n + 1) = s + e - n of every value, with tie-averaged ranks."""
    lead, n = x.shape[:-1], x.shape[-1]
    keys = _keys(x).reshape(-1, n)
    srt, order = torch.sort(keys, dim=1, stable=True)
    pos = torch.arange(n, dtype=torch.int64, device=keys.device).expand_as(srt)
    edge = srt[:, 1:] != srt[:, :-1]
    first = torch.ones_like(srt, dtype=torch.bool)
    first[:, 1:] = edge                                       # first element of every run of equal keys
    last = torch.ones_like(srt, dtype=torch.bool)
    last[:, :-1] = edge                                       # last element of every run
    s = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), dim=1).values
    e = torch.cummin(torch.where(last, pos + 1, torch.full_like(pos, n)).flip(1), dim=1).values.flip(1)
    d = torch.empty_like(srt)
    d.scatter_(1, order, s + e - n)
    return d.reshape(*lead, n)


def _has_nan(a, b):
    return torch.isnan(a).flatten(1).any(1) | torch.isnan(b).flatten(1).any(1)


def rank_sums(a, b):
    """a, b [B,n] -> int64 [B,2,3]: (cov, va, vb) of the rank deviations of the values and of the absolute values."""
    a, b = a.flatten(1).float(), b.flatten(1).float()
    rows = []
    for x, y in ((a, b), (a.abs(), b.abs())):
        dx, dy = rank_deltas(x), rank_deltas(y)
        rows.append(torch.stack([(dx * dy).sum(1), (dx * dx).sum(1), (dy * dy).sum(1)], 1))
    out = torch.stack(rows, 1)
    return out * (~_has_nan(a, b)).to(torch.int64).view(-1, 1, 1)


def _corr(sab, saa, sbb):
    nan = torch.full_like(sab, float("nan"))
    return torch.where((saa == 0) | (sbb == 0), nan, (sab / (saa.sqrt() * sbb.sqrt())).clamp(-1.0, 1.0))


def spearman(sums):
    """rank_sums [...,3] int64 -> float64 [...]: cov / (sqrt(va) sqrt(vb)), clamped; NaN when va == 0 or vb == 0."""
    s = sums.to(torch.float64)
    rho = _corr(s[..., 0], s[..., 1], s[..., 2])
    # the same (or the reversed) ranking: exactly +-1, which sqrt(va) * sqrt(va) == va does not promise in floating point
    cov, va, vb = sums[..., 0], sums[..., 1], sums[..., 2]
    exact = (va == vb) & (cov.abs() == va) & (va != 0)
    return torch.where(exact, torch.sign(cov).to(torch.float64), rho)


def pearson(a, b):
    """a, b [B,n] -> float64 [B]."""
    a, b = a.flatten(1).double(), b.flatten(1).double()
    n = a.shape[1]
    ca, cb = a - (a.sum(1) / n).unsqueeze(1), b - (b.sum(1) / n).unsqueeze(1)
    return _corr((ca * cb).sum(1), (ca * ca).sum(1), (cb * cb).sum(1))


def ssim(a, b, data_range=1.0):
    """a, b [B,H,W] (H, W >= 7) -> float64 [B]."""
    if a.dim() != 3 or a.shape != b.shape or min(a.shape[1:]) < _WIN:
        raise ValueError(f"ssim takes two [B,H,W] batches with H, W >= {_WIN}, got {tuple(a.shape)} and {tuple(b.shape)}")
    x, y = a.double().unsqueeze(1), b.double().unsqueeze(1)

    def box(t):
        return F.avg_pool2d(t, _WIN, stride=1)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    cov_norm = _WIN * _WIN / (_WIN * _WIN - 1.0)
    ux, uy = box(x), box(y)
    vx, vy, vxy = cov_norm * (box(x * x) - ux * ux), cov_norm * (box(y * y) - uy * uy), cov_norm * (box(x * y) - ux * uy)
    s = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return s.flatten(1).sum(1) / s[0].numel()


def map_similarity(a, b, shape=None, data_range=1.0):
    """ops.map_similarity in torch, on any device: a, b [B,n] or [B,H,W] -> (rank_sums int64 [B,2,3], sim float64 [B,4])."""
    if a.shape != b.shape or a.dim() not in (2, 3) or a.numel() == 0:
        raise ValueError(f"map_similarity: the maps must be [B,n] or [B,H,W] alike and not empty, got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    B = a.shape[0]
    hw = tuple(a.shape[1:]) if a.dim() == 3 else None if shape is None else tuple(shape)
    a2, b2 = a.reshape(B, -1).float(), b.reshape(B, -1).float()
    sums = rank_sums(a2, b2)
    sim = torch.full((B, 4), float("nan"), dtype=torch.float64, device=a.device)
    sim[:, 0] = pearson(a2, b2)
    sim[:, 1:3] = spearman(sums)
    if hw is not None:
        sim[:, 3] = ssim(a2.reshape(B, *hw), b2.reshape(B, *hw), data_range)
    sim[_has_nan(a2, b2)] = float("nan")
    return sums, sim


# ------------------------------------------------------------------------------------------------ randomisation
class Stage(NamedTuple):
    """One step of the randomisation: ``modules`` (names in the model) are re-initialised by the model's own _init_weights,
    ``tensors`` (names of bare parameters: pos_embed, cls_token) as the constructor does."""
    name: str
    modules: tuple
    tensors: tuple


def randomization_stages(model):
    """The ordered stages, top down.  ViT / DeiT: head (with the final norm), blocks.{L-1} ... blocks.0, embed (patch
    embedding, pos_embed, cls_token).  BERT sequence classifier: classifier, pooler, encoder.layer.{L-1} ... encoder.layer.0,
    embeddings."""
    if hasattr(model, "blocks") and hasattr(model, "patch_embed") and hasattr(model, "head"):
        L = len(model.blocks)
        return ([Stage("head", ("head", "norm"), ())]
                + [Stage(f"blocks.{i}", (f"blocks.{i}",), ()) for i in reversed(range(L))]
                + [Stage("embed", ("patch_embed",), ("pos_embed", "cls_token"))])
    if hasattr(model, "bert") and hasattr(model, "classifier"):
        L = len(model.bert.encoder.layer)
        return ([Stage("classifier", ("classifier",), ()), Stage("pooler", ("bert.pooler",), ())]
                + [Stage(f"encoder.layer.{i}", (f"bert.encoder.layer.{i}",), ()) for i in reversed(range(L))]
                + [Stage("embeddings", ("bert.embeddings",), ())])
    raise ops._lib.TeError(f"randomization_stages: {type(model).__name__} is neither a VisionTransformer of vit.py nor a "
                           f"BertForSequenceClassification of bert.py")


def _shadow(m):
    """A CPU fp32 stand-in of leaf module ``m`` that the model's _init_weights recognises, with uninitialised parameters."""
    if isinstance(m, nn.Linear):
        s = nn.Linear(m.in_features, m.out_features, bias=m.bias is not None, device="meta")
    elif isinstance(m, nn.LayerNorm):
        s = nn.LayerNorm(m.normalized_shape, eps=m.eps, elementwise_affine=m.elementwise_affine, device="meta")
    elif isinstance(m, nn.Embedding):
        s = nn.Embedding(m.num_embeddings, m.embedding_dim, padding_idx=m.padding_idx, device="meta")
    elif isinstance(m, nn.Conv2d):
        s = nn.Conv2d(m.in_channels, m.out_channels, m.kernel_size, stride=m.stride, padding=m.padding,
                      bias=m.bias is not None, device="meta")
    else:
        raise ops._lib.TeError(f"randomized: no re-initialisation for the parameters of a {type(m).__name__}")
    return s.to_empty(device="cpu")


def _stage_leaves(model, stage):
    """[(qualified name, module)] of the modules of a stage that own parameters, in the order their values are drawn."""
    out = []
    for prefix in stage.modules:
        for name, sub in model.get_submodule(prefix).named_modules():
            if next(sub.parameters(recurse=False), None) is not None:
                out.append((".".join(x for x in (prefix, name) if x), sub))
    return out


def _stage_parameters(model, stage):
    """[(qualified name, parameter)] of a stage."""
    out = [(f"{name}.{pname}", p) for name, sub in _stage_leaves(model, stage) for pname, p in sub.named_parameters(recurse=False)]
    return out + [(name, getattr(model, name)) for name in stage.tensors]


def _reinitialise(model, stage, seed):
    """New values for the parameters of ``stage``: drawn on the CPU (so they do not depend on the device) under a generator
    state of their own (so the global one is left as it was), then copied in place through ``.data``.  Only the CPU generator
    is forked and seeded: torch.manual_seed would reseed every device's generator as well, which nothing here draws from."""
    from .vit import _trunc_normal_
    with torch.random.fork_rng(devices=[]):
        torch.default_generator.manual_seed(int(seed))
        for _, sub in _stage_leaves(model, stage):
            shadow = _shadow(sub)
            with torch.no_grad():
                shadow.reset_parameters()                     # what the constructor leaves where _init_weights does not reach
                model._init_weights(shadow)
            for pname, p in sub.named_parameters(recurse=False):
                p.data.copy_(getattr(shadow, pname).data)
        for name in stage.tensors:
            p = getattr(model, name)
            p.data.copy_(_trunc_normal_(torch.empty(p.shape, dtype=torch.float32), std=.02))


@contextlib.contextmanager
def randomized(model, mode="cascading", seed=0):
    """``with randomized(model) as stages: for name in stages: ...``: every step of the iteration re-initialises the next
    stage of randomization_stages(model) IN PLACE -- "cascading": on top of the earlier stages; "independent": the previous
    stage is restored first -- with values drawn on the CPU from a generator seeded with seed + the stage index.  On exit, also
    on an exception, every parameter and buffer is bit for bit what it was.

    The edits go through ``param.data``, which autograd's version counter does not see: after every edit and after the
    restore the cached operand planes of the model are dropped (ops.x6_invalidate: the x6 planes and the bf16_planes
    entries alike).  A captured GraphedLRP / GraphedCall of this model baked the old planes in and must be re-captured."""
    if mode not in ("cascading", "independent"):
        raise ValueError(f"mode must be 'cascading' or 'independent', got {mode!r}")
    stages = randomization_stages(model)
    saved = {}                                                # qualified name -> (parameter, its original values)

    def restore(names=None):
        for name in list(saved) if names is None else names:
            p, value = saved.pop(name)
            p.data.copy_(value)
        _invalidate(model)

    def steps():
        previous = None
        for i, stage in enumerate(stages):
            if mode == "independent" and previous is not None:
                restore([n for n, _ in _stage_parameters(model, previous)])
            for name, p in _stage_parameters(model, stage):
                saved.setdefault(name, (p, p.detach().clone()))
            _reinitialise(model, stage, seed + i)
            _invalidate(model)
            previous = stage
            yield stage.name
    try:
        yield steps()
    finally:
        restore()


def _invalidate(model):
    """The hook the tests replace to see that a stale plane is caught: every in-place edit of ``randomized`` ends here."""
    return ops.x6_invalidate(model)


# ------------------------------------------------------------------------------------------------ the protocols
def _minmax(maps):
    flat = maps.flatten(1)
    lo, hi = flat.min(1, keepdim=True).values, flat.max(1, keepdim=True).values
    return ((flat - lo) / (hi - lo)).reshape(maps.shape)


def _grid(n) -> Optional[int]:
    g = math.isqrt(n)
    return g if g * g == n else None


def _similarity(a, b, shape=None, data_range=1.0):
    a, b = a.detach().float(), b.detach().float()
    if a.is_cuda:
        return ops.map_similarity(a, b, shape, data_range)
    return map_similarity(a, b, shape, data_range)


def _ssim_images(maps, upsample):
    """The [B,H,W] images SSIM compares, min-max normalised per map, or None when the maps are no image of at least 7x7: an
    image as it is, a token map [B, g*g] as g x g, or (upsample) through the bilinear x16 heat map of the segmentation test."""
    m = maps.detach().float()
    B = m.shape[0]
    if m.dim() >= 3 and m.shape[-1] >= _WIN and m.shape[-2] >= _WIN and m[0].numel() == m.shape[-1] * m.shape[-2]:
        return _minmax(m.reshape(B, m.shape[-2], m.shape[-1]))
    g = _grid(m[0].numel())
    if g is None:
        return None
    if upsample:
        if m.is_cuda:
            return ops.heatmap(m.reshape(B, g * g), scale=16, normalise=True)[:, 0]
        return _minmax(F.interpolate(m.reshape(B, 1, g, g), scale_factor=16, mode="bilinear")[:, 0])
    return _minmax(m.reshape(B, g, g)) if g >= _WIN else None


def compare_maps(a, b, ssim=True, upsample=False, a_image=None):
    """(rank_sums [B,2,3], sim [B,4]) of two batches of maps of any shape [B,...]: Pearson and both Spearman columns on the
    maps as they are; SSIM (if the maps are images, see _ssim_images) on the min-max normalised maps with data_range 1 -- the
    normalisation is not monotone on |x|, so it takes a call of its own.  a_image: ``_ssim_images(a, upsample)`` where the
    caller compares the same ``a`` many times and has it already."""
    B = a.shape[0]
    sums, sim = _similarity(a.reshape(B, -1), b.reshape(B, -1))
    if ssim:
        ia = _ssim_images(a, upsample) if a_image is None else a_image
        ib = _ssim_images(b, upsample) if ia is not None else None
        if ia is not None and ib is not None:
            sim = sim.clone()
            sim[:, 3] = _similarity(ia, ib, data_range=1.0)[1][:, 3]
    return sums, sim


class SanityCheckEvaluator:
    """The cascading (or independent) randomisation test of ``methods`` on the model of ``gen`` (an LRP or a Generator).
    ``update(*inputs)`` explains the batch on the original model (generate_classes(topk=1), or ``classes=index``), keeps the
    classes ON THE DEVICE and explains the same inputs FOR THOSE CLASSES after every stage of ``randomized(gen.model)``; per
    method and stage it keeps (rank_sums, sim) of (original map, stage map) on the device.  ``generate_kwargs`` go to every
    generate_classes call (start_layer, ...).  Nothing is read back until ``arrays()`` / ``summary()``."""

    def __init__(self, gen, methods, mode="cascading", seed=0, ssim=True, upsample=False, **generate_kwargs):
        self.gen, self.methods = gen, tuple(methods)
        self.mode, self.seed, self.ssim, self.upsample = mode, int(seed), bool(ssim), bool(upsample)
        self.generate_kwargs = generate_kwargs
        self.stages = [s.name for s in randomization_stages(gen.model)]
        self._sums = {m: [] for m in self.methods}
        self._sims = {m: [] for m in self.methods}

    def _explain(self, inputs, **which):
        return self.gen.generate_classes(*inputs, methods=self.methods, **which, **self.generate_kwargs)

    def update(self, *inputs, index=None):
        B = inputs[0].shape[0]
        if index is None:
            base = self._explain(inputs, topk=1)
        else:
            idx = index if torch.is_tensor(index) else torch.as_tensor(np.asarray(index))
            base = self._explain(inputs, classes=idx.reshape(B, 1))
        classes = base.classes                    # int64 [B,1], where the maps are: the class explained stays fixed
        original = {m: base.maps[m][:, 0].detach().clone() for m in self.methods}
        # the image SSIM sees of an original map does not change from stage to stage: made once
        images = {m: _ssim_images(original[m], self.upsample) if self.ssim else None for m in self.methods}
        per_stage = {m: [] for m in self.methods}
        with randomized(self.gen.model, self.mode, self.seed) as stages:
            for _ in stages:
                got = self._explain(inputs, classes=classes)
                for m in self.methods:
                    per_stage[m].append(compare_maps(original[m], got.maps[m][:, 0], self.ssim, self.upsample, images[m]))
        for m in self.methods:
            self._sums[m].append(torch.stack([s for s, _ in per_stage[m]]))
            self._sims[m].append(torch.stack([s for _, s in per_stage[m]]))
        return classes

    def arrays(self):
        """({method: float64 [stages, samples, 4]}, {method: int64 [stages, samples, 2, 3]}) as numpy arrays: the one place
        the results cross to the host."""
        sims = {m: torch.cat(v, 1).cpu().numpy() for m, v in self._sims.items() if v}
        sums = {m: torch.cat(v, 1).cpu().numpy() for m, v in self._sums.items() if v}
        return sims, sums

    def summary(self):
        """{method: {"stages": names, "columns": SIM_COLUMNS, "mean": [stages,4] over the non-NaN samples (NaN where there
        is none), "nan": [stages,4] how many samples were NaN}}."""
        out = {}
        for m, v in self.arrays()[0].items():
            nan = np.isnan(v)
            count = (~nan).sum(1)
            total = np.where(nan, 0.0, v).sum(1)
            mean = np.where(count > 0, total / np.maximum(count, 1), np.nan)
            out[m] = {"stages": list(self.stages), "columns": SIM_COLUMNS, "mean": mean, "nan": nan.sum(1)}
        return out


def class_sensitivity(gen, *inputs, methods, topk=2, **generate_kwargs):
    """One generate_classes(topk=) call -> {method: (rank_sums [B,2,3], sim [B,4])} between the maps of the top class (column
    0) and of the runner-up (column 1).  A class-agnostic method gives cov == va == vb and spearman == 1."""
    if topk < 2:
        raise ValueError("class_sensitivity compares the two top classes: topk must be at least 2")
    got = gen.generate_classes(*inputs, topk=topk, methods=tuple(methods), **generate_kwargs)
    return {m: compare_maps(got.maps[m][:, 0], got.maps[m][:, 1], ssim=False) for m in got.maps}
