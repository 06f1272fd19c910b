"""Faithfulness of a relevance map under random perturbations.

Does the map predict what the model does when an arbitrary part of the input is changed?  Infidelity (Yeh et al., NeurIPS
2019; captum's ``infidelity``) compares, over ``n_draws`` random perturbations I = x - x', the product I . attribution with
the drop of the model's score f(x) - f(x'); the faithfulness correlation (Bhatt et al., IJCAI 2020) replaces a random subset
of patches by a baseline and correlates the attribution summed over the subset with that drop.  The reference tree has no
such protocol: include/te_relprop.h ("faithfulness") is the specification, the ``reference_*`` functions below restate it --
the subsets in integer numpy on ``robustness.philox4x32`` and a stable argsort (equality is claimed), the sums in fp64 torch (a
tolerance is claimed) -- and ``FaithfulnessEvaluator`` runs it on the kernels of csrc/te_faithful.hip: per pass of draws one
launch pair for the copies, one forward of B n_d copies, one score launch and one dot launch; nothing is read back before
``arrays()`` / ``summary()``.  On CPU tensors the evaluator runs the restatements.  Parity with captum or quantus is not
claimed: neither is a dependency and neither was run against this.
"""
from __future__ import annotations

import numpy as np
import torch

from . import curves, ops, robustness

SCORE_NAMES = ("infidelity", "infidelity_norm", "beta", "faith_corr")
SUBSET_STREAM = 0x80000000          # the top bit of the first counter word: apart from the noise stream (below 2^29)
MAX_CELLS = 4096


# ------------------------------------------------------------------------------------------------ the definitions
def _grid(grid):
    g_h, g_w = (int(v) for v in grid) if isinstance(grid, (tuple, list)) else (int(grid), int(grid))
    if g_h < 1 or g_w < 1:
        raise ValueError(f"grid must be positive, got {grid!r}")
    if g_h * g_w > MAX_CELLS:
        raise ValueError(f"at most {MAX_CELLS} cells, got a grid of {g_h} x {g_w}")
    return g_h, g_w


def subset_keys(B: int, G: int, n_draws: int, seed: int, id0: int = 0, d0: int = 0) -> np.ndarray:
    """uint64 [B,n_draws,G]: cell c of draw d0 + j of sample id0 + b has the key (w << 32) | c, w = word c & 3 of philox4x32
    with the counter (0x80000000 | (c >> 2), d, low32(id), high32(id)) and the key (low32(seed), high32(seed))."""
    B, G, n_draws, d0 = int(B), int(G), int(n_draws), int(d0)
    if B < 1 or G < 1 or n_draws < 1 or d0 < 0 or d0 + n_draws > 1 << 32:
        raise ValueError(f"subset_keys: B {B}, G {G}, draws {d0} .. {d0 + n_draws - 1} do not name 32-bit draws of a batch")
    if G > MAX_CELLS:
        raise ValueError(f"at most {MAX_CELLS} cells, got {G}")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    groups = -(-G // 4)
    ids = [(int(id0) + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)]
    counter = np.zeros((B, n_draws, groups, 4), dtype=np.uint64)
    counter[..., 0] = np.arange(groups, dtype=np.uint64) | np.uint64(SUBSET_STREAM)
    counter[..., 1] = (np.arange(n_draws, dtype=np.uint64) + np.uint64(d0))[None, :, None]
    counter[..., 2] = np.array([i & 0xFFFFFFFF for i in ids], dtype=np.uint64)[:, None, None]
    counter[..., 3] = np.array([i >> 32 for i in ids], dtype=np.uint64)[:, None, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    words = robustness.philox4x32(counter, key).reshape(B, n_draws, groups * 4)[:, :, :G].astype(np.uint64)
    return (words << np.uint64(32)) | np.arange(G, dtype=np.uint64)


def reference_subsets(B: int, G: int, k: int, n_draws: int, seed: int, id0: int = 0, d0: int = 0) -> np.ndarray:
    """member uint8 [B,n_draws,G]: 1 for the k cells with the smallest keys of ``subset_keys`` (a stable argsort; the keys are
    distinct, because the cell index is part of them)."""
    k, G = int(k), int(G)
    if k < 1 or k > G:
        raise ValueError(f"k must name 1 .. {G} cells, got {k}")
    order = np.argsort(subset_keys(B, G, n_draws, seed, id0, d0), axis=2, kind="stable")
    member = np.zeros(order.shape, dtype=np.uint8)
    np.put_along_axis(member, order[:, :, :k], np.uint8(1), axis=2)
    return member


def reference_subset_inputs(x, k, grid, seed, id0=0, d0=0, n_draws=1, substrate=None, fill=None, attr=None,
                            out_dtype=torch.float32):
    """``ops.subset_inputs`` restated: x [B,C,H,W] fp32 -> (out [B,n_draws,C,H,W], member uint8 [B,n_draws,G], attr_sum fp64
    [B,n_draws] or None), on x's device from subsets made on the host.  A pixel of a chosen cell takes the substrate's value
    (a [B,C,H,W] tensor or the per-channel constants ``fill``), every other pixel x's; rounded once to ``out_dtype``."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out_dtype must be float32 or bfloat16, got {out_dtype}")
    if (substrate is None) == (fill is None):
        raise ValueError("give a substrate tensor or the fill constants, one of the two")
    if x.dim() != 4:
        raise ValueError(f"x must be [B,C,H,W], got {tuple(x.shape)}")
    g_h, g_w = _grid(grid)
    B, C, H, W = x.shape
    if H % g_h or W % g_w or H // g_h != W // g_w:
        raise ValueError(f"a grid of {g_h} x {g_w} does not cut x {tuple(x.shape)} into square cells")
    p, G, n_draws = H // g_h, g_h * g_w, int(n_draws)
    member = torch.from_numpy(reference_subsets(B, G, k, n_draws, seed, id0, d0)).to(x.device)
    x = x.float()
    if substrate is not None:
        if substrate.shape != x.shape:
            raise ValueError(f"substrate {tuple(substrate.shape)} is not shaped like x {tuple(x.shape)}")
        sub = substrate.float()[:, None]
    else:
        sub = curves._per_channel(fill, C, torch.float32, "fill").to(x.device).reshape(1, 1, C, 1, 1)
    pixels = member.reshape(B, n_draws, 1, g_h, g_w).bool().repeat_interleave(p, 3).repeat_interleave(p, 4)
    out = torch.where(pixels, sub, x[:, None]).to(out_dtype)
    attr_sum = None
    if attr is not None:
        a = attr.reshape(B, 1, G).double()
        attr_sum = torch.where(member.bool(), a, torch.zeros_like(a)).sum(2)
    return out, member, attr_sum


def reference_dot(x, y, w, magnitude=False):
    """x [B,n], y [B,D,n] of any float dtype, w [B,m] with n % m == 0 -> fp64 [B,D,2] = sum (x - y) w[e mod m], sum (x - y)^2
    over n, in fp64 from the exact upcasts.  ``magnitude=True``: sum |(x - y) w| in the first place, the scale of the
    rounding bound."""
    B = x.shape[0]
    x64 = x.reshape(B, 1, -1).double()
    y64 = y.reshape(B, y.shape[1], -1).double()
    w64 = w.reshape(B, 1, -1).double()
    n, m = x64.shape[2], w64.shape[2]
    if y64.shape[2] != n or n % m != 0:
        raise ValueError(f"reference_dot: x {tuple(x.shape)}, y {tuple(y.shape)} and w {tuple(w.shape)} do not pair up")
    df = x64 - y64
    term = df * w64.repeat(1, 1, n // m)
    return torch.stack([(term.abs() if magnitude else term).sum(2), (df * df).sum(2)], 2)


def reference_heat(maps, p):
    """The pixel-level attribution of the CPU path: maps [B,g*g] -> [B,1,g p,g p] fp32, bilinear up-sampling without
    normalisation (what ``ops.heatmap(maps, scale=p, normalise=False)`` computes on the device)."""
    B = maps.shape[0]
    g = int(round(maps[0].numel() ** 0.5))
    if g * g != maps[0].numel():
        raise ValueError(f"{tuple(maps.shape)} is not a batch of square patch maps")
    m = maps.reshape(B, 1, g, g).float()
    return m.clone() if int(p) == 1 else torch.nn.functional.interpolate(m, scale_factor=int(p), mode="bilinear")


def scores_from_sums(ip, delta, attr_sum=None):
    """ip [B,D] = sum (x - x') attribution, delta [B,D] = f(x) - f(x') and, in subset mode, attr_sum [B,D], all fp64 ->
    {"infidelity", "beta", "infidelity_norm", "faith_corr" [B]} in fp64 torch on their device.  infidelity = mean_d (ip -
    delta)^2; beta = sum ip delta / sum ip^2, 1 when the denominator is 0 (captum's normalize=True); infidelity_norm = mean_d
    (beta ip - delta)^2; faith_corr = Pearson_d(attr_sum, delta) from centred sums, clamped to [-1, 1], NaN for D < 2, a
    constant side or no attr_sum."""
    ip, delta = ip.double(), delta.double()
    infidelity = ((ip - delta) ** 2).mean(1)
    den = (ip * ip).sum(1)
    beta = torch.where(den != 0, (ip * delta).sum(1) / torch.where(den != 0, den, torch.ones_like(den)), torch.ones_like(den))
    infidelity_norm = ((beta[:, None] * ip - delta) ** 2).mean(1)
    nan = torch.full_like(den, float("nan"))
    corr = nan
    if attr_sum is not None and ip.shape[1] >= 2:
        a = attr_sum.double()
        ca, cd = a - a.mean(1, keepdim=True), delta - delta.mean(1, keepdim=True)
        saa, sdd, sad = (ca * ca).sum(1), (cd * cd).sum(1), (ca * cd).sum(1)
        corr = torch.where((saa == 0) | (sdd == 0), nan, (sad / (saa.sqrt() * sdd.sqrt())).clamp(-1.0, 1.0))
    return {"infidelity": infidelity, "beta": beta, "infidelity_norm": infidelity_norm, "faith_corr": corr}


# ------------------------------------------------------------------------------------------------ the protocol
class FaithfulnessEvaluator:
    """Infidelity and faithfulness correlation of the maps of ``method`` over a dataset, batch by batch.

    ``update(images, index=None)`` explains the clean batch once (generate_classes(topk=1), or ``classes=index``), keeps the
    classes and the map on the device, forms the pixel-level attribution ``ops.heatmap(map, scale=p, normalise=False)`` and
    runs ``n_draws`` perturbed copies of every image through ``lrp.model`` under no_grad, ``draws_per_pass`` draws (default:
    all) as one batch of B n_d.  perturbation="subset": ``subset_size`` random patches (default max(1, G // 4)) take the
    baseline -- "black", "zero" (the mean colour), per-channel pixel values or "blur", resolved by curves.py in the normalised
    space of ``mean`` / ``std`` --; "noise": the uniform noise of ``robustness`` within ``radius``, same seed / id / draw
    convention.  The copies are made in the model's dtype (fp32 or bf16) from the input the model saw, upcast exactly.
    The score f is the probability of the class in fp64 (output="prob") or its logit.  f(clean) comes from a reference pass
    of the clean images in the shape of a pass of copies -- image b at the rows b n_d .. b n_d + n_d - 1 --, so that
    radius 0, or a baseline equal to the image, gives a drop of exactly 0 (see ``robustness.SensitivityEvaluator``).  Every
    pass has that one shape; the last one is filled up with further draws, which are dropped.  Sample ids run on across the
    calls.  Per-sample results stay on the device until ``arrays()`` / ``summary()``.  ViT / DeiT with a square patch grid
    only.  faith_corr is NaN in noise mode.

    ``keep_last=True`` is a hook of the tests: ``self.last`` then holds the tensors of the most recent ``update``."""

    def __init__(self, lrp, method="transformer_attribution", perturbation="subset", n_draws=50, subset_size=None,
                 baseline="black", radius=0.02, output="prob", seed=0, draws_per_pass=None, keep_last=False,
                 mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), klen=11, nsig=5.0, **generate_kwargs):
        self.lrp, self.method = lrp, method
        if perturbation not in ("subset", "noise"):
            raise ValueError(f"perturbation must be 'subset' or 'noise', got {perturbation!r}")
        if output not in ("prob", "logit"):
            raise ValueError(f"output must be 'prob' or 'logit', got {output!r}")
        self.perturbation, self.output = perturbation, output
        self.n_draws, self.radius, self.seed = int(n_draws), float(radius), int(seed)
        if self.n_draws < 1:
            raise ValueError(f"n_draws must be at least 1, got {n_draws}")
        if not (self.radius >= 0.0) or self.radius == float("inf"):
            raise ValueError(f"radius must be finite and not negative, got {radius}")
        if subset_size is not None and int(subset_size) < 1:
            raise ValueError(f"subset_size must be at least 1, got {subset_size}")
        self.subset_size = None if subset_size is None else int(subset_size)
        self.draws_per_pass = self.n_draws if draws_per_pass is None else min(int(draws_per_pass), self.n_draws)
        if self.draws_per_pass < 1:
            raise ValueError(f"draws_per_pass must be at least 1, got {draws_per_pass}")
        self.baseline, self.mean, self.std = baseline, tuple(mean), tuple(std)
        self.klen, self.nsig = int(klen), float(nsig)
        if isinstance(baseline, str) and baseline not in ("blur", "zero", "black"):
            raise ValueError(f"baseline must be 'blur', 'zero', 'black' or per-channel pixel values, got {baseline!r}")
        curves.gaussian_taps(self.klen, self.nsig)                       # refuses an even klen here, not in the first batch
        self.generate_kwargs = generate_kwargs
        self.keep_last = bool(keep_last)
        self.last = None
        self.samples = 0                              # the id of the next sample
        self._scores = {name: [] for name in SCORE_NAMES}

    def _substrate(self, clean, device):
        """dict(substrate=tensor) or dict(fill=constants) in normalised space: curves.py's own resolution"""
        C = clean.shape[1]
        mean, std = (self.mean, self.std) if C == len(self.mean) else (None, None)
        fill = curves.substrate_fill(self.baseline, C, mean, std)
        if fill is not None:
            return dict(fill=fill)
        # the images are normalised already: the blur is linear and pads with zeros in normalised space
        if device:
            return dict(substrate=ops.gaussian_blur(clean, self.klen, self.nsig))
        return dict(substrate=curves.reference_blur(clean, self.klen, self.nsig).float())

    def _score(self, logits, target, device):
        """f [rows] fp64 of logits [rows,K] for target int64 [rows]"""
        rows = target.shape[0]
        logits = logits.reshape(rows, -1)
        if self.output == "logit":
            return torch.gather(logits.double(), 1, target.reshape(rows, 1)).reshape(rows)
        if not device:
            return curves.reference_scores(logits, target).reshape(rows)
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        prob = torch.empty((1, rows), dtype=torch.float64, device=logits.device)
        return ops.curve_scores(logits, target, prob, 0).reshape(rows)

    def update(self, images, index=None):
        if not torch.is_tensor(images) or not images.is_floating_point():
            raise ops._lib.TeError(robustness.DISCRETE_MSG)
        if images.dim() != 4:
            raise ops._lib.TeError(f"FaithfulnessEvaluator: images must be [B,C,H,W], got {tuple(images.shape)}")
        B, C, H, W = images.shape
        dtype = robustness._input_dtype(self.lrp, images, "FaithfulnessEvaluator", "perturbed")
        device = images.is_cuda
        seen = images.to(dtype)                                        # the tensor the model sees
        clean = seen.float()                                           # ... upcast exactly
        which = dict(topk=1)
        if index is not None:
            idx = index if torch.is_tensor(index) else torch.as_tensor(np.asarray(index))
            which = dict(classes=idx.to(images.device).reshape(B, 1))
        got = self.lrp.generate_classes(seen, methods=(self.method,), **which, **self.generate_kwargs)
        classes = got.classes
        map0 = got.maps[self.method][:, 0].detach().reshape(B, -1).float().clone()
        G = map0.shape[1]
        g = int(round(G ** 0.5))
        if g * g != G or H != W or H % g:
            raise ops._lib.TeError(f"FaithfulnessEvaluator: a map of {G} values is not a square patch grid of the images "
                                   f"{tuple(images.shape)}; the protocol takes a ViT / DeiT")
        p = H // g
        heat = ops.heatmap(map0, scale=p, normalise=False) if device else reference_heat(map0, p)
        weight = heat.reshape(B, H * W)
        subset = self.perturbation == "subset"
        k = max(1, G // 4) if self.subset_size is None else self.subset_size
        if subset and k > G:
            raise ValueError(f"subset_size {k} is more than the {G} patches of the images {tuple(images.shape)}")
        sub = self._substrate(clean, device) if subset else None
        subset_inputs = ops.subset_inputs if device else reference_subset_inputs
        noise = ops.noise_inputs if device else robustness.reference_noise
        dot = ops.perturbation_dot if device else reference_dot
        n_c = self.draws_per_pass                                      # every pass of copies has B n_c rows
        rows = (B * n_c, C, H, W)
        target = classes.reshape(B).to(torch.int64).repeat_interleave(n_c, 0)
        with torch.no_grad():                                          # the reference pass: the clean images in that shape
            f0 = self._score(self.lrp.model(seen.repeat_interleave(n_c, 0)), target, device).reshape(B, n_c)
        ips, deltas, sums, kept = [], [], [], []
        for d0 in range(0, self.n_draws, n_c):
            n_d = min(n_c, self.n_draws - d0)                          # the draws of this pass that count
            member = attr_sum = None
            if subset:
                copies, member, attr_sum = subset_inputs(clean, k, g, self.seed, id0=self.samples, d0=d0, n_draws=n_c,
                                                         attr=map0, out_dtype=dtype, **sub)
            else:
                copies = noise(clean, n_c, self.radius, self.seed, id0=self.samples, d0=d0, out_dtype=dtype)
            with torch.no_grad():
                f = self._score(self.lrp.model(copies.reshape(rows)), target, device).reshape(B, n_c)
            deltas.append((f0 - f)[:, :n_d])
            ips.append(dot(clean.reshape(B, -1), copies.reshape(B, n_c, -1), weight)[:, :n_d, 0])
            if subset:
                sums.append(attr_sum[:, :n_d])
            if self.keep_last:
                kept.append((copies[:, :n_d], None if member is None else member[:, :n_d]))
        ip, delta = torch.cat(ips, 1), torch.cat(deltas, 1)
        attr_sum = torch.cat(sums, 1) if subset else None
        scores = scores_from_sums(ip, delta, attr_sum)
        for name in SCORE_NAMES:
            self._scores[name].append(scores[name])
        if self.keep_last:
            self.last = {"map0": map0, "heat": heat, "x0": clean, "id0": self.samples, "ip": ip, "delta": delta,
                         "attr_sum": attr_sum, "classes": classes, "copies": torch.cat([c for c, _ in kept], 1),
                         "member": torch.cat([m for _, m in kept], 1) if subset else None}
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
