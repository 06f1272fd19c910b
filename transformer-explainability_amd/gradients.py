"""Gradient baselines of a ViT / DeiT: Input x Gradient (Shrikumar et al., 2016), SmoothGrad (Smilkov et al., 2017) and
Integrated Gradients (Sundararajan et al., ICML 2017) -- the three methods the AttnLRP paper (Achtibat et al., ICML 2024)
makes its case against, next to ``transformer_attribution`` and AttnLRP.

Each method is a loop around the model's own forward and backward pass: a pass is B chunk copies of the batch through the model
with ``requires_grad`` on the copies, and ONE ``autograd.grad`` of the selected logits.  What surrounds the loop runs on the
kernels of csrc/te_gradients.hip: the path or noise copies written in the model's dtype (``ops.path_inputs``,
``ops.gauss_inputs``), the fp64 reduction of the B S input gradients in a fixed order (``ops.grad_accumulate``) and the
channel reduction to a [B,H,W] map with its per-sample sum (``ops.grad_finish``).  The reference tree has no such methods:
include/te_relprop.h ("gradient baselines") is the specification and the ``reference_*`` functions below restate it -- the
path copies, the accumulation and Philox in numpy, where equality is claimed, Box-Muller and the sums in fp64 numpy, where a
tolerance is claimed.  On CPU tensors the ops run these restatements, so ``GradientBaselines`` serves a float32 model on the
host as well.  Parity with captum is not claimed.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import ops
from .curves import substrate_fill
from .generators import _drop_rule_planes, _x6_bracket
from .robustness import philox4x32

GAUSS_STREAM = 1 << 30            # bit 30 of the first counter word: apart from the noise stream and the subset stream
RULES = ("midpoint", "trapezoid", "gauss_legendre")
DEFAULT_CHUNK = 10                # copies per sample and pass: the B n_d rows of SensitivityEvaluator's default n_draws


class Completeness(NamedTuple):
    """The completeness record of Integrated Gradients, fp64 [B] each, on the images' device: ``sum`` of the map over its
    pixels (te_grad_finish_f64's fixed order), the selected logit ``f_x`` at the input and ``f_base`` at the baseline.  The
    axiom asks sum = f_x - f_base; the gap is the quadrature's error plus the model's rounding."""
    sum: torch.Tensor
    f_x: torch.Tensor
    f_base: torch.Tensor


# ------------------------------------------------------------------------------------------------ the definitions
def quadrature(rule: str, steps: int):
    """(alphas, weights), fp64 numpy [steps]: the nodes in [0, 1] and the weights (sum 1) of the path integral.
    "midpoint": (k + 1/2) / S, 1 / S.  "trapezoid": k / (S - 1), 1 / (S - 1) with half weights at both ends (S >= 2).
    "gauss_legendre": numpy's leggauss(S) moved from [-1, 1] to [0, 1].  The kernels take the nodes rounded to fp32."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
    S = int(steps)
    if S < 1 or (rule == "trapezoid" and S < 2):
        raise ValueError(f"steps must be at least {2 if rule == 'trapezoid' else 1} for rule {rule!r}, got {steps}")
    if rule == "midpoint":
        return (np.arange(S, dtype=np.float64) + 0.5) / S, np.full(S, 1.0 / S)
    if rule == "trapezoid":
        w = np.full(S, 1.0 / (S - 1))
        w[0] = w[-1] = 0.5 / (S - 1)
        return np.arange(S, dtype=np.float64) / (S - 1), w
    x, w = np.polynomial.legendre.leggauss(S)
    return (x + 1.0) / 2.0, w / 2.0


def gauss_normals(B: int, n: int, n_draws: int, seed: int, id0: int = 0, d0: int = 0) -> np.ndarray:
    """fp64 [B,n_draws,n]: the standard normals of te_gauss_inputs_*.  The elements 4g .. 4g + 3 of draw d0 + j of sample
    id0 + b come from the words w0 .. w3 of philox4x32 with the counter (2^30 | g, d, low32(id), high32(id)) and the key
    (low32(seed), high32(seed)): u = (w + 0.5) 2^-32, r = sqrt(-2 ln u1), z = r cos(2 pi u2), r sin(2 pi u2) from (w0, w1),
    and the same from (w2, w3)."""
    B, n, n_draws, d0 = int(B), int(n), int(n_draws), int(d0)
    if B < 1 or n < 1 or n_draws < 1 or d0 < 0 or d0 + n_draws > 1 << 32:
        raise ValueError(f"gauss_normals: B {B}, n {n}, draws {d0} .. {d0 + n_draws - 1} do not name 32-bit draws of a batch")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    groups = -(-n // 4)
    ids = [(int(id0) + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)]
    counter = np.zeros((B, n_draws, groups, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(groups, dtype=np.uint64) | np.uint64(GAUSS_STREAM)
    counter[..., 1] = (np.arange(n_draws, dtype=np.uint64) + np.uint64(d0))[None, :, None]
    counter[..., 2] = np.array([i & 0xFFFFFFFF for i in ids], dtype=np.uint64)[:, None, None]
    counter[..., 3] = np.array([i >> 32 for i in ids], dtype=np.uint64)[:, None, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    u = (philox4x32(counter, key).astype(np.float64) + 0.5) * 2.0 ** -32
    z = np.empty_like(u)
    for p in (0, 2):
        r, t = np.sqrt(-2.0 * np.log(u[..., p])), 2.0 * np.pi * u[..., p + 1]
        z[..., p], z[..., p + 1] = r * np.cos(t), r * np.sin(t)
    return z.reshape(B, n_draws, groups * 4)[:, :, :n]


def _rounded(y64: np.ndarray, shape, out_dtype, device) -> torch.Tensor:
    """fp64 -> fp32 (one rounding) -> ``out_dtype`` (bfloat16: once more, to nearest even), as the kernels round"""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    return torch.from_numpy(y64.astype(np.float32)).to(out_dtype).reshape(shape).to(device)


def reference_path_inputs(x, base, alphas, s0=0, n_s=None, out_dtype=torch.float32):
    """x, base [B,...] fp32, alphas [S] fp32 -> [B,n_s,...]: base + alphas[s0 + j] (x - base) in fp64, the subtraction, the
    product and the sum rounded once each, then one rounding to fp32: the kernel's bits."""
    S, s0 = alphas.numel(), int(s0)
    n_s = S - s0 if n_s is None else int(n_s)
    if s0 < 0 or n_s < 1 or s0 + n_s > S:
        raise ValueError(f"nodes {s0} .. {s0 + n_s - 1} are not nodes of the {S} alphas")
    B = x.shape[0]
    x64 = x.detach().cpu().reshape(B, 1, -1).numpy().astype(np.float64)
    b64 = base.detach().cpu().reshape(B, 1, -1).numpy().astype(np.float64)
    a64 = alphas.detach().cpu().numpy().astype(np.float64)[s0:s0 + n_s].reshape(1, n_s, 1)
    return _rounded(b64 + a64 * (x64 - b64), (B, n_s) + tuple(x.shape[1:]), out_dtype, x.device)


def reference_gauss_inputs(x, n_draws, sigma, seed, id0=0, d0=0, out_dtype=torch.float32):
    """x [B,...] fp32 -> [B,n_draws,...]: x + sigma z in fp64 with z = ``gauss_normals``, rounded once to fp32.  numpy's
    ln, cos and sin are not the device's: the result is within one step of ``out_dtype`` of the kernel's."""
    sigma = float(sigma)
    if not (sigma >= 0.0) or sigma == float("inf"):
        raise ValueError(f"sigma must be finite and not negative, got {sigma}")
    B = x.shape[0]
    x64 = x.detach().cpu().reshape(B, 1, -1).numpy().astype(np.float64)
    z = gauss_normals(B, x64.shape[2], n_draws, seed, id0, d0)
    return _rounded(x64 + sigma * z, (B, int(n_draws)) + tuple(x.shape[1:]), out_dtype, x.device)


def reference_accumulate(g, w, acc, s0=0, square=False):
    """acc [B,...] fp64 += sum_j w[s0 + j] t(g[:, j]) in place, j ascending, the product and the sum rounded once each
    (numpy's two ufuncs: never an FMA): the kernel's bits.  g [B,n_s,...] of any float dtype, upcast exactly."""
    B, n_s = g.shape[0], g.shape[1]
    g64 = g.detach().cpu().double().reshape(B, n_s, -1).numpy()
    w64 = w.detach().cpu().double().numpy()
    a = acc.detach().cpu().reshape(B, -1).numpy().copy()
    for j in range(n_s):
        t = g64[:, j] * g64[:, j] if square else g64[:, j]
        a = a + w64[int(s0) + j] * t
    acc.copy_(torch.from_numpy(a).reshape(acc.shape))
    return acc


def reference_finish(acc, m=None, reduce="sum"):
    """acc [B,C,...] fp64, m like acc (any float dtype, upcast exactly) or None -> (map fp32 [B,...], sums fp64 [B]): per
    pixel the channels folded in order from +0.0 ("sum", "abs_sum": added; "max_abs": the maximum, a NaN kept), the map
    rounded once; sums = the pixels of v added in fp64 (numpy's order: within the kernel's bound, not its bits)."""
    if reduce not in ops.GRAD_REDUCE:
        raise ValueError(f"reduce must be one of {tuple(ops.GRAD_REDUCE)}, got {reduce!r}")
    B, C = acc.shape[0], acc.shape[1]
    t = acc.detach().cpu().reshape(B, C, -1).numpy()
    if m is not None:
        t = m.detach().cpu().double().reshape(B, C, -1).numpy() * t
    v = np.zeros((B, t.shape[2]), dtype=np.float64)
    for c in range(C):
        if reduce == "sum":
            v = v + t[:, c]
        elif reduce == "abs_sum":
            v = v + np.abs(t[:, c])
        else:
            a = np.abs(t[:, c])
            v = np.where((a > v) | np.isnan(a), a, v)
    out = torch.from_numpy(v.astype(np.float32)).reshape((B,) + tuple(acc.shape[2:])).to(acc.device)
    return out, torch.from_numpy(v.sum(1)).to(acc.device)


# ------------------------------------------------------------------------------------------------ the methods
def _positive_int(what: str, name: str, value, least: int = 1) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError(f"{what}: {name} must be an integer >= {least}, got {value!r}")
    return int(value)


def _refuse(what: str, model, images):
    """The refusals every call shares, raised before any forward pass: the gradient baselines are implemented for float32
    models, and for bfloat16 models on the GPU, in eval mode, on [B,C,H,W] images of the parameters' dtype."""
    if getattr(model, "training", False):
        raise ops._lib.TeError(f"{what}: the model is in train mode; the gradient baselines differentiate an eval-mode "
                               "forward pass (dropout is the identity): call model.eval()")
    if not torch.is_tensor(images) or not images.is_floating_point() or images.dim() != 4 or images.numel() == 0:
        raise ops._lib.TeError(f"{what}: images must be a float tensor [B,C,H,W] and not empty (a ViT / DeiT input; token "
                               "ids have no input gradient)")
    params = list(model.parameters()) if hasattr(model, "parameters") else []
    dtypes = [t.dtype for t in params + [images] if t.is_floating_point()]
    for dt in dtypes:
        if dt not in (torch.float32, torch.bfloat16):
            raise ops._lib.TeError(f"{what}: the gradient baselines are implemented for torch.float32 and torch.bfloat16 models "
                                   f"and inputs only, got {dt}: run them on a float32 or bfloat16 copy of the model")
    if torch.bfloat16 in dtypes:
        if torch.float32 in dtypes:
            raise ops._lib.TeError(f"{what}: torch.bfloat16 mixed with torch.float32 among the model's parameters and its "
                                   "inputs; the copies are made in ONE format: convert the model and its inputs alike "
                                   "(model.to(torch.bfloat16), images.to(torch.bfloat16))")
        if any(not t.is_cuda for t in params + [images]):
            raise ops._lib.TeError(f"{what}: a torch.bfloat16 model and its inputs must be on the GPU -- bfloat16 copies and "
                                   "gradients are served by the HIP kernels only, there is no host path")


class GradientBaselines:
    """Input x Gradient, SmoothGrad and Integrated Gradients of a ViT / DeiT ``model`` (float32, or bfloat16 on the GPU; eval
    mode).  ``images`` [B,C,H,W] is the model's input, already normalised, in the model's dtype; ``index`` None (the class a
    clean forward pass predicts), an integer or [B] integers.  Every call returns an fp32 [B,H,W] map, the shape of
    ``generate_LRP(method="full")``.  ``mean`` / ``std`` (per channel, of the normalisation the images went through) and
    ``klen`` / ``nsig`` only resolve the named baselines of ``integrated_gradients``, as ``CurveEvaluator`` resolves its
    substrates."""

    def __init__(self, model, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), klen=11, nsig=5.0):
        self.model = model
        self.mean, self.std = tuple(mean), tuple(std)
        self.klen, self.nsig = int(klen), float(nsig)

    # ------------------------------------------------------------------------------------------ the passes
    def _index(self, what, images, index):
        """index as the caller gave it -> None, or int64 [B] on the images' device (checked before any forward pass)"""
        if index is None:
            return None
        B = images.shape[0]
        idx = index if torch.is_tensor(index) else torch.as_tensor(np.asarray(index))
        if idx.dtype.is_floating_point or idx.dtype == torch.bool or idx.numel() not in (1, B):
            raise ValueError(f"{what}: index must be None, an integer or {B} integers, got {index!r}")
        idx = idx.reshape(-1).to(torch.int64).expand(B) if idx.numel() == 1 else idx.reshape(B).to(torch.int64)
        n = getattr(self.model, "num_classes", None)
        if isinstance(n, int) and n > 0 and not idx.is_cuda and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError(f"{what}: index names classes outside 0 .. {n - 1}")
        return idx.to(images.device).contiguous()

    def _logits(self, x):
        """The clean forward pass: logits [B,K], no graph"""
        with torch.no_grad():
            out = self.model(x)
        self._forward_done()
        return out

    def _forward_done(self):
        if hasattr(self.model, "modules"):
            _drop_rule_planes(self.model)      # the operand planes the x6 forward products leave for relprop rules: no reader here

    @staticmethod
    def _selected(logits, index):
        return logits.gather(1, index.view(-1, 1)).squeeze(1)

    def _gradients(self, copies, index):
        """copies [B,n_c,C,H,W] in the model's dtype -> the gradient of each copy's selected logit w.r.t. that copy, same
        shape and dtype: one forward pass of B n_c rows and ONE autograd.grad."""
        B, n_c = copies.shape[0], copies.shape[1]
        rows = copies.reshape((B * n_c,) + tuple(copies.shape[2:])).detach().requires_grad_(True)
        sel = self._selected(self.model(rows), index.repeat_interleave(n_c))
        (g,) = torch.autograd.grad(sel, rows, grad_outputs=torch.ones_like(sel))
        self._forward_done()
        return g.reshape(copies.shape)

    @staticmethod
    def _weights(values, device):
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(device)

    # ------------------------------------------------------------------------------------------ the methods
    def input_x_gradient(self, images, index=None):
        """sum over the channels of x d f_index / d x at the input the model saw: one pass of B rows."""
        what = "input_x_gradient"
        _refuse(what, self.model, images)
        index = self._index(what, images, index)
        with _x6_bracket(images):
            if index is None:
                index = self._logits(images).argmax(-1)
            g = self._gradients(images[:, None], index)
            acc = torch.zeros(images.shape, dtype=torch.float64, device=images.device)
            ops.grad_accumulate(g, self._weights([1.0], images.device), acc)
            out, _ = ops.grad_finish(acc, images.float().contiguous(), "sum", with_sums=False)
        return out

    def smoothgrad(self, images, index=None, n_draws=25, sigma=0.15, squared=False, reduce="abs_sum", seed=0, chunk=None):
        """The mean over ``n_draws`` noisy copies x + sigma (max - min) z of the copy's gradient (``squared``: of its square,
        SmoothGrad-Squared), reduced over the channels by ``reduce`` ("abs_sum", "sum", "max_abs").  sigma is a fraction of
        the batch's max - min (SmoothGrad's convention; the one value read back from the device); copy j of image b is draw
        j of sample b under ``seed``.  ``chunk`` draws per pass (default: min(n_draws, 10)): the map's bits do not depend on
        it wherever the model's gradient of a copy does not depend on the pass's batch size."""
        what = "smoothgrad"
        _refuse(what, self.model, images)
        n_draws = _positive_int(what, "n_draws", n_draws)
        chunk = min(n_draws, DEFAULT_CHUNK) if chunk is None else min(_positive_int(what, "chunk", chunk), n_draws)
        if reduce not in ops.GRAD_REDUCE:
            raise ValueError(f"{what}: reduce must be one of {tuple(ops.GRAD_REDUCE)}, got {reduce!r}")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not 0.0 <= sigma < float("inf"):
            raise ValueError(f"{what}: sigma must be a finite number >= 0, got {sigma!r}")
        seed = int(seed)
        index = self._index(what, images, index)
        with _x6_bracket(images):
            if index is None:
                index = self._logits(images).argmax(-1)
            x = images.float().contiguous()                            # the input the model saw, upcast exactly
            scale = float(sigma) * float(x.max() - x.min())
            w = self._weights(np.full(n_draws, 1.0 / n_draws), images.device)
            acc = torch.zeros(images.shape, dtype=torch.float64, device=images.device)
            for d0 in range(0, n_draws, chunk):
                n_d = min(chunk, n_draws - d0)
                copies = ops.gauss_inputs(x, n_d, scale, seed, d0=d0, out_dtype=images.dtype)
                ops.grad_accumulate(self._gradients(copies, index), w, acc, s0=d0, square=bool(squared))
            out, _ = ops.grad_finish(acc, None, reduce, with_sums=False)
        return out

    def baseline(self, images, baseline="black"):
        """The fp32 [B,C,H,W] baseline of ``integrated_gradients`` in normalised space: "black", "zero" (the mean colour),
        per-channel pixel values, "blur" (the Gaussian blur of the images, ``klen`` x ``klen``, zero padding) or a tensor
        shaped like the images (or broadcastable to them).  Rounded to the images' dtype and upcast again, so that it is the
        tensor the model sees at the path's start: the path copies, x - base and f(base) share one end point."""
        x = images.float()
        if torch.is_tensor(baseline):
            base = baseline.to(x.device).float().expand_as(x)
        else:
            C = x.shape[1]
            fill = substrate_fill(baseline, C, self.mean, self.std)
            if fill is not None:
                base = torch.tensor(fill, dtype=torch.float32, device=x.device).view(1, C, 1, 1).expand_as(x)
            elif x.is_cuda:
                base = ops.gaussian_blur(x.contiguous(), self.klen, self.nsig)
            else:
                from .curves import reference_blur
                base = reference_blur(x, self.klen, self.nsig).float()
        return base.to(images.dtype).float().contiguous()

    def integrated_gradients(self, images, index=None, steps=32, baseline="black", rule="midpoint", chunk=None):
        """-> (map, Completeness).  map = sum over the channels of (x - base) sum_s w_s d f_index / d x at base + a_s (x - base)
        with the ``steps`` nodes a_s and weights w_s of ``rule`` ("midpoint", "trapezoid", "gauss_legendre": ``quadrature``,
        computed on the host in fp64; the nodes enter the kernel rounded to fp32).  x - base is formed in fp32.  ``chunk``
        nodes per pass (default: min(steps, 10)).  Completeness: the map's sum, f(x) and f(base), fp64 [B] on the device."""
        what = "integrated_gradients"
        _refuse(what, self.model, images)
        steps = _positive_int(what, "steps", steps)
        try:
            alphas, weights = quadrature(rule, steps)
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None
        chunk = min(steps, DEFAULT_CHUNK) if chunk is None else min(_positive_int(what, "chunk", chunk), steps)
        if not torch.is_tensor(baseline) and isinstance(baseline, str) and baseline not in ("black", "zero", "blur"):
            raise ValueError(f"{what}: baseline must be 'black', 'zero', 'blur', per-channel pixel values or a tensor, got "
                             f"{baseline!r}")
        index = self._index(what, images, index)
        with _x6_bracket(images):
            x = images.float().contiguous()                            # the input the model saw, upcast exactly
            base = self.baseline(images, baseline)
            logits_x = self._logits(images)
            if index is None:
                index = logits_x.argmax(-1)
            f_x = self._selected(logits_x, index).double()
            f_base = self._selected(self._logits(base.to(images.dtype)), index).double()
            a32 = torch.from_numpy(alphas.astype(np.float32)).to(images.device)
            w = self._weights(weights, images.device)
            acc = torch.zeros(images.shape, dtype=torch.float64, device=images.device)
            for s0 in range(0, steps, chunk):
                n_s = min(chunk, steps - s0)
                copies = ops.path_inputs(x, base, a32, s0, n_s, out_dtype=images.dtype)
                ops.grad_accumulate(self._gradients(copies, index), w, acc, s0=s0)
            out, sums = ops.grad_finish(acc, x - base, "sum")
        return out, Completeness(sums, f_x, f_base)
