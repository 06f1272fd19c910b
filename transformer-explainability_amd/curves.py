"""Deletion and insertion curves (RISE: Petsiuk et al., BMVC 2018, ``CausalMetric``) of a relevance map.

The pixels of an image are ranked by relevance and switched ``step`` at a time, most relevant first: deletion goes from the
image towards a neutral substrate, insertion from a blurred image towards the image.  After every step the classifier's
probability of one class is recorded; the area under each curve is the reported number (a low deletion AUC and a high
insertion AUC speak for the map).  The reference tree has no such protocol (its one faithfulness test is the nine-step
perturbation test, perturbation.py): include/te_relprop.h ("deletion / insertion curves") is the specification, the
``reference_*`` functions below restate it in torch -- in fp64 where the kernels are held to a tolerance against fp64
(blur, scores, AUC), in the kernels' own fp32 expression where equality is claimed (ranks, images) -- and
``CurveEvaluator`` runs it on the device kernels of csrc/te_curves.hip: per batch one rank, one blur, and per chunk of
steps one compose launch, one forward and one score launch; nothing is read back before ``arrays()`` / ``save()``.
On CPU tensors the evaluator runs the restatements.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import ops

MODES = ("deletion", "insertion")
DEFAULT_SUBSTRATE = {"deletion": "zero", "insertion": "blur"}


# ------------------------------------------------------------------------------------------------ the definitions
def gaussian_taps(klen: int = 11, nsig: float = 5.0) -> np.ndarray:
    """RISE's ``gkern`` in one dimension, fp64 [klen]: scipy.ndimage.gaussian_filter1d(delta, nsig) on a length-klen delta
    (boundary "reflect", truncate 4).  The truncated Gaussian w[-R..R], R = int(4 nsig + 0.5), is folded back into the klen
    positions by the reflection (d c b a | a b c d | d c b a); the 2-D kernel is the outer product of the taps."""
    klen = int(klen)
    if klen < 1 or klen % 2 == 0:
        raise ValueError(f"gaussian_taps: klen must be odd and positive, got {klen}")
    sigma = float(nsig)
    radius = int(4.0 * sigma + 0.5)
    k = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k.astype(np.float64) ** 2)
    w /= w.sum()
    at = (np.arange(klen)[:, None] + k[None, :]) % (2 * klen)          # position in the reflected, 2 klen-periodic signal
    at = np.where(at >= klen, 2 * klen - 1 - at, at)
    return (w[None, :] * (at == klen // 2)).sum(1)


def _per_channel(values, C, dtype, what):
    if values is None:
        return None
    t = torch.tensor([float(v) for v in values], dtype=dtype)
    if t.numel() != C:
        raise ValueError(f"{what} has {t.numel()} values for {C} channels")
    return t


def normalise(data, mean=None, std=None):
    """z = (data - mean[c]) / std[c] in fp32: the expression of te_perturb_f32 (None = 0 / 1)."""
    C = data.shape[1]
    m = _per_channel(mean, C, torch.float32, "mean")
    s = _per_channel(std, C, torch.float32, "std")
    m = torch.zeros(C) if m is None else m
    s = torch.ones(C) if s is None else s
    shape = (1, C) + (1,) * (data.dim() - 2)
    return (data.float() - m.to(data.device).reshape(shape)) / s.to(data.device).reshape(shape)


def substrate_fill(kind, C, mean=None, std=None):
    """The per-channel constants of a constant substrate, in normalised space and rounded as the kernel's fp32 expression
    rounds them: "zero" -> 0 (the mean colour), "black" -> (0 - mean[c]) / std[c], a tuple of pixel values v ->
    (v[c] - mean[c]) / std[c].  None for "blur" (a tensor, not constants)."""
    if isinstance(kind, str):
        if kind == "blur":
            return None
        if kind == "zero":
            return [0.0] * C
        if kind != "black":
            raise ValueError(f"substrate must be 'blur', 'zero', 'black' or per-channel pixel values, got {kind!r}")
        kind = (0.0,) * C
    v = _per_channel(kind, C, torch.float32, "the substrate's pixel values")
    return [float(x) for x in normalise(v.reshape(1, C, 1), mean, std).reshape(C)]


def reference_blur(data, klen=11, nsig=5.0, mean=None, std=None, magnitude=False, dtype=torch.float64):
    """blur(z) [B,C,H,W] in fp64 with the fp32 taps the kernel gets and zero padding in normalised space;
    ``magnitude=True``: blur(|z|), the scale of the kernel's rounding bound.  ``dtype=torch.float32``: RISE's own
    conv2d(..., padding=klen // 2) with the klen x klen kernel, what benchmarks/curves_bench.py times."""
    taps = torch.from_numpy(gaussian_taps(klen, nsig).astype(np.float32)).to(dtype)
    z = normalise(data, mean, std).to(dtype)
    if magnitude:
        z = z.abs()
    B, C, H, W = z.shape
    r = int(klen) // 2
    k2 = torch.outer(taps, taps).reshape(1, 1, int(klen), int(klen)).to(z.device)
    return torch.nn.functional.conv2d(z.reshape(B * C, 1, H, W), k2, padding=r).reshape(B, C, H, W)


def reference_ranks(vis):
    """rank int32 [B,n]: the position of every pixel in torch.sort(vis, 1, descending=True, stable=True)."""
    B = vis.shape[0]
    vis = vis.reshape(B, -1).float()
    order = torch.sort(vis, dim=1, descending=True, stable=True).indices
    ranks = torch.empty_like(order)
    ranks.scatter_(1, order, torch.arange(vis.shape[1], device=vis.device).expand_as(order))
    return ranks.to(torch.int32)


def n_steps(HW: int, step: int) -> int:
    """S = ceil(HW / step): a curve has S + 1 images."""
    return -(-int(HW) // int(step))


def reference_inputs(data, ranks, step, s0, n_s, mode, substrate=None, fill=None, mean=None, std=None,
                     out_dtype=torch.float32):
    """The images s0 .. s0 + n_s - 1 [n_s,B,C,H,W]: image i has the k_i = min(i step, HW) top-ranked pixels switched, from z
    to the substrate (deletion) or back (insertion); fp32, or that value rounded once to bf16."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if (substrate is None) == (fill is None):
        raise ValueError("give a substrate tensor or the fill constants, one of the two")
    B, C, H, W = data.shape
    HW = H * W
    S = n_steps(HW, step)
    if step < 1 or s0 < 0 or n_s < 1 or s0 + n_s > S + 1:
        raise ValueError(f"step {step}, s0 {s0}, n_s {n_s} do not name images of the {S + 1} of {HW} pixels")
    z = normalise(data, mean, std).reshape(1, B, C, HW)
    if substrate is not None:
        sub = substrate.float().reshape(1, B, C, HW)
    else:
        sub = _per_channel(fill, C, torch.float32, "fill").to(data.device).reshape(1, 1, C, 1)
    k = torch.clamp(torch.arange(s0, s0 + n_s, device=data.device) * int(step), max=HW)
    switched = ranks.reshape(1, B, 1, HW) < k.reshape(n_s, 1, 1, 1)
    out = torch.where(switched, sub, z) if mode == "deletion" else torch.where(switched, z, sub)
    return out.reshape(n_s, B, C, H, W).to(out_dtype)


def reference_scores(logits, target):
    """p [n_s,B] fp64 = softmax(logits)[target], logits [n_s*B,K] or [n_s,B,K] of any float dtype, evaluated in fp64."""
    B = target.shape[0]
    p = torch.softmax(logits.double().reshape(-1, B, logits.shape[-1]), dim=-1)
    return torch.gather(p, -1, target.to(torch.int64).reshape(1, B, 1).expand(p.shape[0], B, 1)).squeeze(-1)


def reference_auc(prob):
    """auc [B] fp64 = the trapezoid of prob [S+1,B] over x = i / S."""
    prob = prob.double()
    S = prob.shape[0] - 1
    return (prob.sum(0) - prob[0] / 2 - prob[-1] / 2) / S


# ------------------------------------------------------------------------------------------------ the protocol
class CurveEvaluator:
    """Deletion / insertion curves of a classifier over a dataset, batch by batch.

    ``update(data, vis, target)`` takes data [B,C,H,W] in [0,1], vis [B,1,H,W] or [B,H*W] relevance and target [B] labels;
    results stay on the device until ``arrays()`` / ``save(dir)``: per mode ``<mode>_scores.npy`` [S+1,N] (the class
    probability after every step) and ``<mode>_auc.npy`` [N].  ``summary()`` gives the mean AUCs.  ``step`` defaults to
    max(1, HW // 224) pixels (224 at 224 x 224, as RISE).  A substrate is "blur", "zero" (the mean colour), "black" or a
    tuple of per-channel pixel values."""

    def __init__(self, model, modes=MODES, step=None, substrate=None, klen=11, nsig=5.0, mean=(0.5, 0.5, 0.5),
                 std=(0.5, 0.5, 0.5), max_forward_batch=512):
        self.model = model.eval() if hasattr(model, "eval") else model
        # the classifier's dtype decides the input dtype, as in PerturbationEvaluator: a bf16 model gets bf16 images straight
        # from te_curve_inputs_bf16 (the fp32 values rounded once); other dtypes have no kernel
        par = next(self.model.parameters(), None) if hasattr(self.model, "parameters") else None
        self.input_dtype = torch.bfloat16 if par is not None and par.dtype == torch.bfloat16 else torch.float32
        if par is not None and par.is_floating_point() and par.dtype not in (torch.float32, torch.bfloat16):
            raise ops._lib.TeError(f"CurveEvaluator: {ops.DTYPES_MSG}; the classifier is {par.dtype}")
        self.modes = tuple(modes)
        if not self.modes or any(m not in MODES for m in self.modes):
            raise ValueError(f"modes must be taken from {MODES}, got {modes!r}")
        self.substrate = {**DEFAULT_SUBSTRATE, **(substrate or {})}
        if step is not None and int(step) < 1:
            raise ValueError(f"step must be at least 1, got {step}")
        self.step = None if step is None else int(step)
        self.klen, self.nsig = int(klen), float(nsig)
        gaussian_taps(self.klen, self.nsig)                              # refuses an even klen here, not in the first batch
        self.mean, self.std = tuple(mean), tuple(std)
        self.max_forward_batch = int(max_forward_batch)
        self._scores = {m: [] for m in self.modes}
        self._auc = {m: [] for m in self.modes}

    @torch.no_grad()
    def update(self, data, vis, target):
        B, C, H, W = data.shape
        HW = H * W
        step = self.step if self.step is not None else max(1, HW // 224)
        S = n_steps(HW, step)
        device = data.is_cuda
        data = data.float()
        vis = vis.reshape(B, -1).float()
        target = target.to(torch.int64)
        fills = {m: substrate_fill(self.substrate[m], C, self.mean, self.std) for m in self.modes}
        ranks = ops.pixel_ranks(vis) if device else reference_ranks(vis)
        blurred = None
        if any(f is None for f in fills.values()):
            blurred = (ops.gaussian_blur(data, self.klen, self.nsig, self.mean, self.std) if device else
                       reference_blur(data, self.klen, self.nsig, self.mean, self.std).float())
        inputs = ops.curve_inputs if device else reference_inputs
        chunk = max(1, self.max_forward_batch // B)
        for mode in self.modes:
            sub = dict(substrate=blurred) if fills[mode] is None else dict(fill=fills[mode])
            prob = torch.empty((S + 1, B), dtype=torch.float64, device=data.device)
            for s0 in range(0, S + 1, chunk):
                n_s = min(chunk, S + 1 - s0)
                x = inputs(data, ranks, step, s0, n_s, mode, mean=self.mean, std=self.std, out_dtype=self.input_dtype, **sub)
                logits = self.model(x.reshape(n_s * B, C, H, W))
                if device:
                    if logits.dtype not in (torch.float32, torch.bfloat16):
                        logits = logits.float()
                    ops.curve_scores(logits, target, prob, s0)
                else:
                    prob[s0:s0 + n_s] = reference_scores(logits, target)
            self._scores[mode].append(prob)
            self._auc[mode].append(ops.curve_auc(prob) if device else reference_auc(prob))

    # ------------------------------------------------------------------------------------------
    def arrays(self):
        """``<mode>_scores.npy`` [S+1,N] and ``<mode>_auc.npy`` [N] per mode, keyed by file name."""
        out = {}
        for m in self.modes:
            if len({p.shape[0] for p in self._scores[m]}) > 1:
                raise ValueError("the batches have different numbers of steps: fix `step` and the image size for one evaluation")
            out[f"{m}_scores.npy"] = (torch.cat(self._scores[m], 1).cpu().numpy() if self._scores[m] else np.zeros((0, 0)))
            out[f"{m}_auc.npy"] = torch.cat(self._auc[m], 0).cpu().numpy() if self._auc[m] else np.zeros((0,))
        return out

    def summary(self):
        """{"<mode>_auc": the mean AUC over the samples seen}"""
        arrs = self.arrays()
        return {f"{m}_auc": float(arrs[f"{m}_auc.npy"].mean()) if arrs[f"{m}_auc.npy"].size else float("nan")
                for m in self.modes}

    def save(self, experiment_dir):
        os.makedirs(experiment_dir, exist_ok=True)
        arrs = self.arrays()
        for name, a in arrs.items():
            np.save(os.path.join(experiment_dir, name), a)
        return arrs
