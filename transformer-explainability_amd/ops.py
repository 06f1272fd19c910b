"""Tensor-level wrappers over the C ABI: shape/stride plumbing, output + workspace allocation.

Every function takes fp32 tensors that live on one MI355X (or, on the rules of an explanation, bf16 operands with fp32
relevance, or fp64 tensors throughout: DTYPES_MSG), enqueues HIP kernels on torch's current stream for that device and
returns torch tensors (no synchronisation).  Shapes follow the reference's
relprop rules; see include/te_relprop.h for the exact semantics and reference citations.
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (TE_HEADMEAN_CLAMP, TE_HEADMEAN_ROW0, TE_IMPL_SIMPLE, TE_RATIONALE_CLAMP, TE_ROLLOUT_CLS_FIXUP,
                   TE_ROLLOUT_NORMALISE, TE_ROLLOUT_ROW0, TE_VARIANT_LRP, TE_VARIANT_OURS)
# te_relprop.h's x6 flag bits (TE_X6_WHOLE_TILES: whole-tile ranges always, for callers that keep several streams busy; same bits)
from ._lib import (TE_X6_PHASE_C, TE_X6_PHASE_SPLIT, TE_X6_PHASE_Z, TE_X6_TEST_DROP_HANDOVER,  # noqa: F401
                   TE_X6_TEST_SMALL_GRID, TE_X6_TILE_C_SHIFT, TE_X6_TILE_Z_SHIFT, TE_X6_WHOLE_TILES, TE_X6_X_PLANES_SIGNED)
# (A/B and tests: TE_X6_SLACK_RULE = the schedule rule before the cost comparison, TE_X6_STATIC_TILES = whole tiles in static ranges)
from ._lib import (TE_X6_PASS_C, TE_X6_PASS_PRODUCT, TE_X6_PASS_Z, TE_X6_SCHEDULE_STREAM_K,  # noqa: F401
                   TE_X6_SCHEDULE_WHOLE_CLAIMED, TE_X6_SCHEDULE_WHOLE_STATIC, TE_X6_SLACK_RULE, TE_X6_STATIC_TILES)

Tensor = torch.Tensor
_VARIANTS = {"ours": TE_VARIANT_OURS, "lrp": TE_VARIANT_LRP}

# Tests flip this to run the simple (non-MFMA) device kernels as an on-device cross-check.
FORCE_SIMPLE = False
# bench.py installs a callable (name, flops, bytes) -> context manager here: every C-ABI call of the relprop path is
# then bracketed by HIP events on the stream it launches on, tagged with its ALGORITHMIC work.
KERNEL_TIMER = None
_NULL = contextlib.nullcontext()


def _timed(name: str, flops: float = 0.0, nbytes: float = 0.0):
    return _NULL if KERNEL_TIMER is None else KERNEL_TIMER(name, float(flops), float(nbytes))


class Deferred:
    """A relevance tensor whose per-sample factor has not been applied yet: value = t * scale[b] with scale a strided
    view into the [B,2] factor pair of te_add_relprop_deferred_f32.  Consumers (clone_relprop, linear_relprop) take the
    factor into their kernels; ``materialise()`` gives the plain tensor (bitwise what Add.relprop returns)."""
    __slots__ = ("t", "scale")

    def __init__(self, t: Tensor, scale: Tensor):
        self.t, self.scale = t, scale

    @property
    def shape(self):
        return self.t.shape

    def materialise(self) -> Tensor:
        return self.t * self.scale.view(-1, *([1] * (self.t.dim() - 1)))


def _split_deferred(x):
    return (x.t, x.scale) if isinstance(x, Deferred) else (x, None)
_checked_device = False


def _variant(v) -> int:
    code = _VARIANTS[v] if isinstance(v, str) else int(v)
    return code | (TE_IMPL_SIMPLE if FORCE_SIMPLE else 0)


# The dtypes the kernels take: fp32 everywhere; bf16 OPERANDS (activations, weights, attention gradients of a bf16 model)
# on the rules of a ViT / DeiT or BERT explanation (variant ours, alpha = 1), with fp32 relevance (the *_bf16 paths below);
# float64 everywhere -- operands AND relevance -- on the same rules (the *_f64 paths at the end of this file).
DTYPES_MSG = ("relprop kernels take float32 tensors, or bfloat16 operands with float32 relevance, or float64 operands with "
              "float64 relevance, the latter two on the ViT / DeiT and BERT rules of variant 'ours' with alpha = 1")


def _prep(t: Tensor) -> Tensor:
    if t.dtype != torch.float32:
        raise _lib.TeError(f"{DTYPES_MSG}; got {t.dtype} here")
    if not t.is_cuda:
        raise _lib.TeError("relprop kernels need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
    return t


def _is_bf16(t) -> bool:
    return torch.is_tensor(t) and t.dtype == torch.bfloat16


def _prep_bf16(t: Tensor) -> Tensor:
    if t.dtype != torch.bfloat16:
        raise _lib.TeError(f"{DTYPES_MSG}; this bf16 rule got a {t.dtype} operand")
    if not t.is_cuda:
        raise _lib.TeError("relprop kernels need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
    return t


def _is_f64(t) -> bool:
    if isinstance(t, Deferred):
        t = t.t
    return torch.is_tensor(t) and t.dtype == torch.float64


def _any_f64(*ts) -> bool:
    return any(_is_f64(t) for t in ts)


def _f64_rule(variant, alpha, what, **tensors):
    """The fp64 paths: variant ours with alpha = 1, EVERY tensor float64 (operands and relevance alike: nothing of an fp64
    explanation is computed in a narrower format), on the MI355X.  Raises before any HIP call."""
    var = (_VARIANTS[variant] if isinstance(variant, str) else int(variant)) & 0xff
    if var != TE_VARIANT_OURS or alpha != 1:
        raise _lib.TeError(f"{what} with torch.float64 operands: only variant 'ours' with alpha = 1 is implemented "
                           f"(got variant {variant!r}, alpha {alpha}); run the model in float32 for other rules")
    bad = {n: t.dtype for n, t in tensors.items() if t is not None and t.dtype != torch.float64}
    if bad:
        raise _lib.TeError(f"{DTYPES_MSG}; {what} got torch.float64 mixed with "
                           + ", ".join(f"{n}: {d}" for n, d in bad.items())
                           + " -- an fp64 rule takes fp64 operands and fp64 relevance only")
    for t in tensors.values():
        if t is not None and not t.is_cuda:
            raise _lib.TeError("relprop kernels need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")


def _c16(t: Tensor) -> Tensor:
    t = _prep_bf16(t)
    return t if t.is_contiguous() else t.contiguous()


def _bf16_rule(variant, alpha=1.0, what="rule"):
    """The bf16 paths implement variant ours with alpha = 1 (what LRP.generate_LRP passes); anything else is refused."""
    var = _variant(variant) & 0xff
    if var != TE_VARIANT_OURS or alpha != 1:
        raise _lib.TeError(f"{what} with bf16 operands: only variant 'ours' with alpha = 1 is implemented "
                           f"(got variant {variant!r}, alpha {alpha}); run the model in float32 for other rules")


def _c(t: Tensor) -> Tensor:
    t = _prep(t)
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream(t: Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ws(nbytes: int, like: Tensor) -> Tensor:
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=like.device)


class _on_device:
    """Make the tensor's device current for the duration of the call (multi-GPU processes)."""

    def __init__(self, t: Tensor):
        global _checked_device
        if not _is_f64(t):           # (an fp64 rule has validated its tensors itself: _f64_rule)
            _prep_bf16(t) if _is_bf16(t) else _prep(t)
        if not _checked_device:
            _lib.require_device()
            _checked_device = True
        self.ctx = torch.cuda.device(t.device)

    def __enter__(self):
        self.ctx.__enter__()
        return _lib.load()

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)


# ---------------------------------------------------------------------------------------- a3
# Linear.relprop obtains Z from the forward output when the caller supplies it (te_linear_relprop_fwd_f32): one GEMM
# less per rule.  Tests flip this to run the two-GEMM Z-pass on the same inputs.
USE_FORWARD_OUTPUT = True
# The attention rules take Z = the forward product of the very einsum / MatMul whose rule is evaluated (what the
# reference's autograd re-evaluation reproduces bit for bit) instead of recomputing it in another summation order.
USE_FORWARD_PRODUCTS = True


# Linear.relprop (variant ours, alpha = 1, cached forward output) on bf16 MFMAs at fp32 accuracy: every fp32 operand = the
# exact sum of three bf16 parts, the six partial products above 2^-24 kept, fp32 accumulation (csrc/te_linear_x6.hip).
# DEFAULT since round 3; TE_LINEAR_X6=0 or ops.USE_LINEAR_X6 = False selects the fp32-MFMA kernels
# of te_linear.hip, which remain the path of variant lrp, alpha != 1, shapes the x6 kernels do not tile, and rules
# without a cached forward output.
USE_LINEAR_X6 = os.environ.get("TE_LINEAR_X6", "1") not in ("", "0")
X6_CHECK = False     # tests: synchronise after every x6 rule and raise if a bounded hand-over wait expired
X6_TILE = 0          # te_relprop.h TE_X6_TILE_*: 0 auto, 1 = 128-row weight tiles (measurement knob; results are identical)
X6_FLAGS = int(os.environ.get("TE_X6_FLAGS", "0"), 0)   # extra te_relprop.h flag bits for every x6 launch (per-pass tile pins, test hooks)


# A workgroup of an x6 kernel that continues a tile another workgroup started waits for that one's accumulators; the wait
# is bounded, and a wait that expires must never yield a plausible-looking map (VERDICT r3 / ADVICE r3).  Every x6 launch
# of this process ORs into ONE sticky device word per GPU; the kernels also poison what they computed from the missing
# accumulators with NaN.  Nothing on the hot path reads the word (no synchronisation is added to a step): the generators
# expose ``check()`` and ``x6_raise_if_failed`` is called where a caller synchronises anyway (bench.py after its final
# synchronise, the sweep after its gather, tests after every rule).
_x6_status = {}


def _x6_device_index(device) -> int:
    """The GPU index `device` names -- an index-less 'cuda' means the CURRENT device (one rule for x6_status, x6_failed
    and the reset: ADVICE r4)."""
    dev = torch.device(device)
    return torch.cuda.current_device() if dev.index is None else dev.index


def x6_status(device) -> Tensor:
    """The sticky hand-over status word of `device` (int32 [4], word 0 is the one the kernels OR into)."""
    idx = _x6_device_index(device)
    t = _x6_status.get(idx)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.TeError("the x6 status word must exist before a HIP graph is captured: run the step once eagerly "
                               "(GraphedLRP / GraphedCall warm up before they capture)")
        t = _x6_status[idx] = torch.zeros(4, dtype=torch.int32, device=torch.device("cuda", idx))
    return t


def _x6_failed_words(device=None) -> list:
    """Synchronises `device` (default: every GPU an x6 kernel ran on); the status words that were READ and are non-zero."""
    keys = list(_x6_status) if device is None else [_x6_device_index(device)]
    bad = []
    for k in keys:
        t = _x6_status.get(k)
        if t is not None:
            torch.cuda.synchronize(t.device)
            if int(t[0].item()) != 0:
                bad.append(t)
    return bad


def x6_failed(device=None) -> bool:
    """Synchronises `device` (default: every GPU an x6 kernel ran on) and reports whether a hand-over wait ever expired."""
    return bool(_x6_failed_words(device))


def x6_raise_if_failed(device=None, reset: bool = True):
    """Raise TeError if any x6 launch since the last reset lost a hand-over (its outputs are NaN-poisoned and invalid).
    Synchronises; call it where the caller synchronises anyway.  `reset` clears only the words that were read and found
    set: a failure on another GPU of the process stays recorded until that GPU is checked."""
    bad = _x6_failed_words(device)
    if bad:
        if reset:
            for t in bad:
                t.zero_()
        raise _lib.TeError("an x6 Linear kernel waited in vain for the accumulators of a tile it shares with another "
                           "workgroup (bounded stream-K hand-over expired): the affected outputs were poisoned with NaN and "
                           "every map computed since the last check is invalid.  Typical causes: several persistent x6 "
                           "launches competing for the CUs (more than one step in flight), a profiler or another process "
                           "holding CUs.  Re-run the step; set TE_LINEAR_X6=0 to use the fp32-MFMA kernels instead")


# A caller that never calls check() (plain ``LRP.generate_LRP`` in a loop) must still hear about a lost hand-over ONCE, not
# read NaN maps for the rest of the process: the generators post a NON-BLOCKING copy of the status word into
# pinned host memory after each call (x6_post) and look at the copy of the PREVIOUS call before the next one starts
# (x6_poll: an event query, no synchronisation).  The failure is reported one call late, raised once, the word reset.
_x6_posted = {}


def x6_post(device):
    """After a generator call: copy the sticky status word to the host without waiting (no-op during graph capture, and
    before any x6 launch ran on the device)."""
    if not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
        return
    idx = _x6_device_index(device)
    t = _x6_status.get(idx)
    if t is None:
        return
    ent = _x6_posted.get(idx)
    if ent is None:
        ent = _x6_posted[idx] = [torch.zeros(4, dtype=torch.int32).pin_memory(), torch.cuda.Event(), False]
    elif ent[2] and not ent[1].query():
        return                                   # the previous copy is still in flight: keep it
    with torch.cuda.device(idx):
        ent[0].copy_(t, non_blocking=True)
        ent[1].record()
    ent[2] = True


def x6_poll(device):
    """Before a generator call: if the copy posted by an earlier call has landed and shows a lost hand-over, reset the word
    and raise TeError -- every map computed since the last check is invalid (NaN-poisoned).  Never waits."""
    if not _x6_posted or torch.cuda.is_current_stream_capturing():
        return
    ent = _x6_posted.get(_x6_device_index(device))
    if ent is None or not ent[2] or not ent[1].query():
        return
    ent[2] = False
    if int(ent[0][0]) != 0:
        x6_raise_if_failed(device)               # synchronises, resets the word that was read, raises


def _weight_key(W: Tensor):
    """Identity of a weight AS THE CALLER HOLDS IT (never of a contiguous copy, whose fresh version counter and recycled
    address could collide): storage address, strides, shape, device and autograd's version counter.  What the counter
    cannot see -- writes through ``.data`` (``p.data.copy_(ckpt)``, ``p.data.normal_()``, pruning masks) -- needs
    ``x6_invalidate``; rules.Linear also drops its planes on ``load_state_dict`` and on ``.to()`` / ``.float()``."""
    return (W.data_ptr(), W._version, tuple(W.shape), tuple(W.stride()), str(W.device))


def x6_invalidate(obj) -> int:
    """Drop the cached bf16 operand planes of a layer, or of every layer of a model (returns how many caches were cleared).
    The planes outlive a forward pass and are keyed on autograd's version counter: call this after editing weights in a
    way autograd does not record (``param.data...``), and re-capture any HIP graph that baked the old planes in."""
    mods = obj.modules() if hasattr(obj, "modules") else [obj]
    n = 0
    for m in mods:
        c = getattr(m, "__dict__", {}).get("_te_cache")
        if c:
            c.clear()
            n += 1
    return n


def _cached_planes(W: Tensor, cache: Optional[dict], name: str, build) -> tuple:
    """The payload of cache[name] = (_weight_key(W), *payload), built by ``build(W.detach())`` once per weight version (an
    optimiser step or an in-place edit of the weight changes the key); cache = None builds every time.  `cache` is the
    layer's scratch dict (rules.x6_cache; DESIGN.md "The layer's scratch dict")."""
    key = _weight_key(W)
    hit = None if cache is None else cache.get(name)
    if hit is None or hit[0] != key:
        hit = (key, *build(W.detach()))
        if cache is not None:
            cache[name] = hit
    return hit[1:]


def _prepare_planes(Wc: Tensor, bytes_fn: str, prepare_fn: str, dims: tuple, *extra) -> Tensor:
    """planes = prepare_fn(Wc, *dims, *extra) in a buffer of bytes_fn(*dims) bytes (the weight-side prepare calls of the C ABI)."""
    with _on_device(Wc) as lib:
        planes = _ws(getattr(lib, bytes_fn)(*dims), Wc)
        _lib.check(getattr(lib, prepare_fn)(_ptr(Wc), *dims, *extra, _ptr(planes), planes.numel(), _stream(Wc)), prepare_fn)
    return planes


def x6_weight_planes(W: Tensor, cache: Optional[dict] = None) -> Tensor:
    """bf16 operand planes of a Linear weight for te_linear_relprop_x6_f32 (cached: _cached_planes)."""
    out_f, in_f = W.shape
    return _cached_planes(W, cache, "x6_planes", lambda Wd: (_prepare_planes(
        _c(Wd), "te_linear_x6_weight_planes_bytes", "te_linear_x6_prepare_weights_f32", (in_f, out_f)),))[0]


# The forward output and the input gradient of a Linear layer on the x6 kernels (te_gemm_x6_f32) under
# ops.USE_FUSED_PRODUCERS, PER DIRECTION.  Measured on the MI355X, ViT-B/16 batch 64 (profiles/r03_x6_gemm_study.log,
# profiles/r03_x6_gemm_step_ab.log): the x6 product runs at 125-171 TF fp32-equivalent against 110-120 TF (default) /
# 117-148 TF (TunableOp) for the stock fp32 GEMM, but pays a split pass over its activation operand first (6 B written
# per element: 16 us for K = 768, 85 us for K = 3072 at T = 12 608).  In the step, one trip, A B A B: every supported
# product on x6 73.3 ms, only the narrow-operand ones (K <= 1024, M >= 2 K: qkv / fc1 forward, fc2 input gradient)
# 74.6-74.8 ms, none 78.9 ms.  X6_GEMM = "all" (default) | "auto" (the narrow-operand policy) | "off"; TE_X6_GEMM=0 / 1 =
# off / all.  Both kernels are fp32 GEMMs to fp32 rounding (tests/test_gpu_producers.py).
X6_GEMM = {"": "all", "1": "all", "0": "off"}.get(os.environ.get("TE_X6_GEMM", "all"), os.environ.get("TE_X6_GEMM", "all"))
if X6_GEMM not in ("all", "auto", "off"):
    raise ValueError(f"TE_X6_GEMM={X6_GEMM!r}: expected all / auto / off (or 1 / 0)")


def gemm_x6_wanted(T: int, K: int, M: int) -> bool:
    """Should out [T, M] = X [T, K] . W^T run on te_gemm_x6_f32 (policy above)?"""
    if X6_GEMM == "off" or T < 256 or not gemm_x6_supported(T, K, M):
        return False
    return X6_GEMM == "all" or (K <= 1024 and M >= 2 * K)


def x6_weight_planes_lrp(W: Tensor, cache: Optional[dict] = None) -> Tensor:
    """P3 planes of max(W,0), min(W,0) and of their transposes: the weight side of te_linear_relprop_x6_general_f32 for
    variant lrp (one-sided products); cached like x6_weight_planes."""
    out_f, in_f = W.shape
    return _cached_planes(W, cache, "x6_planes_lrp", lambda Wd: (_prepare_planes(
        _c(Wd), "te_linear_x6_weight_planes_lrp_bytes", "te_linear_x6_prepare_weights_lrp_f32", (in_f, out_f)),))[0]


def x6_matrix_planes(W: Tensor, transposed: bool, cache: Optional[dict] = None) -> Tensor:
    """Signed bf16 operand planes of W [out, in] (transposed=False: rows = out, the forward product's weight side) or of
    W^T (transposed=True: rows = in, the input gradient's); cached like x6_weight_planes."""
    out_f, in_f = W.shape
    dims = (in_f, out_f) if transposed else (out_f, in_f)
    return _cached_planes(W, cache, "x6_gemm_planes_T" if transposed else "x6_gemm_planes", lambda Wd: (_prepare_planes(
        _c(Wd), "te_linear_x6_planes_bytes", "te_linear_x6_split_matrix_f32", dims, int(transposed)),))[0]


def linear_relprop_x6_supported(T: int, in_f: int, out_f: int) -> bool:
    return bool(_lib.load().te_linear_relprop_x6_supported(int(T), int(in_f), int(out_f)))


def gemm_x6_supported(T: int, K: int, M: int) -> bool:
    return bool(_lib.load().te_gemm_x6_supported(int(T), int(K), int(M)))


X6_KEEP_ABS = os.environ.get("TE_X6_KEEP_ABS", "1") not in ("", "0")     # measurement switch for the plane reuse below
# The plane set a layer's forward product leaves for its rule: True = the SIGNED planes the product itself read (the rule's
# Z-pass forms |X| while it stages them: TE_X6_X_PLANES_SIGNED), so that no producer stores a second set; False = the planes
# of |X| from a dual split / a producer's second store.  Same results, bit for bit (tests, A/B runs).
X6_SIGNED_PLANES = True


def _signed(planes: Tensor) -> Tensor:
    """Marks a plane set in the ``x_abs_planes`` mailbox as the signed planes of X."""
    planes._te_signed_planes = True
    return planes


def planes_are_signed(planes: Optional[Tensor]) -> bool:
    return planes is not None and getattr(planes, "_te_signed_planes", False)


def _x_abs_key(X: Tensor, T: int, K: int):
    return (X.data_ptr(), X._version, T, K, str(X.device))


# The three plane hand-overs between layers, each a mailbox in the consuming layer's scratch dict: one function posts, one
# takes (pops the entry, validates it, returns the planes or None).  Who calls them, and how long an entry may live:
# DESIGN.md "The layer's scratch dict".
def post_x_planes(cache: dict, X: Tensor, xs: Tensor, xa: Optional[Tensor] = None):
    """A producer of X leaves the signed planes of X [T, K] for the Linear that consumes X (xa: with X6_SIGNED_PLANES off, the
    planes of |X| as well).  The entry HOLDS X: while it exists, X's address cannot be recycled for a tensor that would meet the
    key by accident."""
    K = X.shape[-1]
    cache["x_planes_from_producer"] = (_x_abs_key(X, X.numel() // K, K), xs, xa, X)


def take_x_planes(cache: dict, X: Tensor, T: int, K: int):
    """(xs, xa) if a producer posted the planes of exactly this X (xa = None: it posted the signed planes only), else None."""
    hit = cache.pop("x_planes_from_producer", None)
    if hit is not None and hit[0] == _x_abs_key(X, T, K) and hit[3].data_ptr() == X.data_ptr():
        return hit[1], hit[2]
    return None


def drop_x_planes(cache: dict, with_abs: bool = False):
    """Nothing of an earlier call may wait for this call's input (with_abs: nor for its rule)."""
    cache.pop("x_planes_from_producer", None)
    if with_abs:
        cache.pop("x_abs_planes", None)


def post_x_abs_planes(cache: dict, X: Tensor, T: int, K: int, xa: Tensor):
    """The layer's forward product leaves the plane set its own relprop rule reads: the planes of |X|, or the signed planes
    the product read, marked as such (_signed)."""
    cache["x_abs_planes"] = (_x_abs_key(X, T, K), xa)


def take_x_abs_planes(cache: dict, X: Tensor, T: int, K: int) -> Optional[Tensor]:
    """The plane set (of |X|, or signed: planes_are_signed) if the forward product of exactly this X left one, else None.
    Consumed once: 6 B per input element (0.4 GB per ViT-B block at batch 64) must not outlive the rule."""
    keep = _X_ABS_KEPT
    hit = cache.get("x_abs_planes") if keep is not None and not keep.last else cache.pop("x_abs_planes", None)
    return hit[1] if hit is not None and hit[0] == _x_abs_key(X, T, K) else None


_X_ABS_KEPT = None


class x_abs_planes_kept:
    """Around the relprop chains of SEVERAL classes over one forward pass (generators._PassDriver._class_pass): while open,
    take_x_abs_planes leaves the entry where it is, so that every class's rule reads the planes the forward product left;
    the caller sets ``last = True`` in front of the last class's chain, whose rules pop them as a single call's do.  On exit
    -- however the chains ended -- the ``x_abs_planes`` entry of every dict in ``caches`` is dropped: 6 B per input element
    must not outlive the call.  The planes are a function of X alone, so a rule that takes them and one that splits |X| itself
    write the same bits."""

    def __init__(self, caches):
        self.caches, self.last = list(caches), False

    def __enter__(self):
        global _X_ABS_KEPT
        self._outer, _X_ABS_KEPT = _X_ABS_KEPT, self
        return self

    def __exit__(self, *exc):
        global _X_ABS_KEPT
        _X_ABS_KEPT = self._outer
        for c in self.caches:
            c.pop("x_abs_planes", None)
        return False


def post_dy_planes(cache: dict, planes: Tensor, like: Tensor) -> Tensor:
    """A consumer's backward leaves the planes of its input gradient for the backward of the Linear that produced `like`;
    returns what autograd carries instead of the fp32 gradient: a zero-stride NaN placeholder of like's shape (whoever
    reads it reads NaN, not stale memory)."""
    base = torch.full((1,), float("nan"), dtype=like.dtype, device=like.device)
    cache["dy_planes_from_consumer"] = (base, tuple(like.shape), planes)
    return base.expand(like.shape)


def take_dy_planes(cache: dict, dy: Tensor) -> Optional[Tensor]:
    """The posted planes if dy is the placeholder of that post (its address, shape, all-zero strides), else None."""
    hit = cache.pop("dy_planes_from_consumer", None)
    if hit is not None and dy.data_ptr() == hit[0].data_ptr() and tuple(dy.shape) == hit[1] and not any(dy.stride()):
        return hit[2]
    return None


def rule_takes_abs_planes(T: int, in_f: int, out_f: int) -> bool:
    """Will Linear.relprop of a [T, in_f] input run on te_linear_relprop_x6_f32 and read the planes of |X| its forward
    product leaves behind?  (The rule-side half of producers.takes_producer_planes.)"""
    return bool(USE_LINEAR_X6 and X6_KEEP_ABS and linear_relprop_x6_supported(T, in_f, out_f))


def gemm_x6(X: Tensor, w_planes: Tensor, bias: Optional[Tensor], M: int, timer_name: str = "gemm_x6",
            keep_abs: Optional[dict] = None, x_planes: Optional[Tensor] = None) -> Tensor:
    """out [..., M] = X [..., K] . W^T + bias with W as signed planes of an [M, K] matrix (x6_matrix_planes).
    keep_abs: the layer's scratch dict -- the signed planes of X are taken from X's producer if it posted them there, else
    split here, and where the layer's rule will read planes they are posted for that rule and live until it has run (DESIGN.md
    "The layer's scratch dict").  X6_SIGNED_PLANES off: the rule gets the planes of |X| instead, from the producer's second
    set or te_linear_x6_split_dual_f32 (bit for bit those of a split of |X|).
    x_planes: the signed planes of X from its producer (gelu_backward_planes) -- X is then used for its shape only and never
    read (it may be the zero-stride placeholder the producer returned instead of an fp32 tensor)."""
    K = X.shape[-1]
    lead = X.shape[:-1]
    T = X.numel() // K
    Xc = None if x_planes is not None else _c(X).reshape(-1, K)
    like = X if Xc is None else Xc
    out = torch.empty((T, M), dtype=torch.float32, device=X.device)
    bc = None if bias is None else _c(bias.detach())
    with _on_device(like) as lib:
        ws = _ws(lib.te_gemm_x6_workspace_bytes(T, K, M), like)
        x_bytes = (6.0 if x_planes is not None else 10.0) * T * K      # planes read / fp32 read + planes written
        xs = x_planes
        if xs is None and keep_abs is not None:
            got = take_x_planes(keep_abs, X, T, K)
            if got is not None:
                xs, x_bytes = got[0], 6.0 * T * K
                post_x_abs_planes(keep_abs, X, T, K, got[1] if got[1] is not None else _signed(xs))
        if xs is not None and xs.numel() * xs.element_size() < lib.te_linear_x6_planes_bytes(T, K):
            raise _lib.TeError(f"gemm_x6: the operand planes handed in hold {xs.numel() * xs.element_size()} bytes, "
                               f"[{T}, {K}] needs {lib.te_linear_x6_planes_bytes(T, K)}")
        for_rule = xs is None and keep_abs is not None and rule_takes_abs_planes(T, K, M)
        if for_rule and not X6_SIGNED_PLANES:
            x_bytes += 6.0 * T * K                                     # the dual split writes two plane sets
        with _timed(timer_name, 12.0 * T * K * M, x_bytes + 6.0 * K * M + 4.0 * T * M):
            if for_rule:
                nb = lib.te_linear_x6_planes_bytes(T, K)
                if X6_SIGNED_PLANES:      # the single split, into a buffer that outlives the call: the rule reads it too
                    xs = _signed(_ws(nb, Xc))
                    _lib.check(lib.te_linear_x6_split_matrix_f32(_ptr(Xc), T, K, 0, _ptr(xs), nb, _stream(Xc)),
                               "te_linear_x6_split_matrix_f32")
                    post_x_abs_planes(keep_abs, X, T, K, xs)
                else:
                    xs, xa = _ws(nb, Xc), _ws(nb, Xc)
                    _lib.check(lib.te_linear_x6_split_dual_f32(_ptr(Xc), T, K, _ptr(xs), _ptr(xa), nb, _stream(Xc)),
                               "te_linear_x6_split_dual_f32")
                    post_x_abs_planes(keep_abs, X, T, K, xa)
            _lib.check(lib.te_gemm_x6_f32(_ptr(Xc) if Xc is not None else None, _ptr(xs), _ptr(w_planes), _ptr(bc), _ptr(out),
                                          T, K, M, (X6_TILE | X6_FLAGS) & ~0x3c00, _ptr(x6_status(X.device)), _ptr(ws),
                                          ws.numel(), _stream(like)), "te_gemm_x6_f32")
    return out.reshape(*lead, M)


def linear_relprop(R: Tensor, X: Tensor, W: Tensor, alpha: float = 1.0, variant="ours",
                   Y: Optional[Tensor] = None, bias: Optional[Tensor] = None, cache: Optional[dict] = None) -> Tensor:
    """Linear.relprop: R [..., out], X [..., in], W [out, in] -> [..., in].
    Y [..., out] (optional) is the forward output F.linear(X, W, bias) the rule module cached as self.Y; with it
    (variant ours, alpha = 1) the Z-pass needs one product instead of two.  cache: a dict owned by the layer, where the
    bf16 operand planes of W are kept between calls (x6_weight_planes).
    bf16 X / W (a bf16 model): linear_relprop_bf16."""
    if _any_f64(R, X, W):
        return linear_relprop_f64(R, X, W, alpha=alpha, variant=variant)
    if _is_bf16(X) or _is_bf16(W):
        return linear_relprop_bf16(R, X, W, alpha=alpha, variant=variant, cache=cache)
    out_f, in_f = W.shape
    lead = X.shape[:-1]
    R, r_scale = _split_deferred(R)
    Rc, Xc, Wc = _c(R).reshape(-1, out_f), _c(X).reshape(-1, in_f), _c(W)
    T = Xc.shape[0]
    if Rc.shape[0] != T:
        raise _lib.TeError(f"Linear.relprop: R has {Rc.shape[0]} rows, X has {T}")
    out = torch.empty((T, in_f), dtype=torch.float32, device=X.device)
    var = _variant(variant)
    fast_ok = (var == TE_VARIANT_OURS and alpha == 1 and in_f % 4 == 0 and out_f % 4 == 0 and
               all(t.data_ptr() % 16 == 0 for t in (Rc, Xc, Wc)))      # (else: the any-shape entry point)
    fwd = fast_ok and USE_FORWARD_OUTPUT and Y is not None
    if r_scale is not None and not fwd:      # only the forward-output Z-pass takes the factor into its epilogue
        Rc = _c(Deferred(R, r_scale).materialise()).reshape(-1, out_f)
        r_scale = None
    rs_ptr, rs_stride, rps = None, 0, 1
    if r_scale is not None:
        rs_ptr, rs_stride, rps = r_scale.data_ptr(), r_scale.stride(0), T // r_scale.shape[0]
    # variant lrp and / or alpha != 1 on the x6 kernels (round 4; te_linear_relprop_x6_general_f32): one-sided products for
    # lrp, the inhibitor half from the same |X||W|^T product for ours (which needs the cached forward output)
    var_code = var & 0xff
    general = (USE_LINEAR_X6 and not (var & TE_IMPL_SIMPLE) and not (var_code == TE_VARIANT_OURS and alpha == 1)
               and all(t.data_ptr() % 16 == 0 for t in (Rc, Xc, Wc))
               and (var_code == TE_VARIANT_LRP or (USE_FORWARD_OUTPUT and Y is not None))
               and bool(_lib.load().te_linear_relprop_x6_general_supported(T, in_f, out_f, var_code)))
    if general:
        Yg = bg = None
        if var_code == TE_VARIANT_OURS:
            Yg = _c(Y.detach()).reshape(-1, out_f)
            bg = None if bias is None else _c(bias.detach())
            general = Yg.shape[0] == T and Yg.data_ptr() % 16 == 0 and (bg is None or bg.data_ptr() % 16 == 0)
    if general:
        wp = x6_weight_planes(W, cache) if var_code == TE_VARIANT_OURS else None
        wpl = x6_weight_planes_lrp(W, cache) if var_code == TE_VARIANT_LRP else None
        xa = take_x_abs_planes(cache, X, T, in_f) if cache is not None and var_code == TE_VARIANT_OURS else None
        if planes_are_signed(xa):      # (this entry point takes the planes of |X| only: it splits them itself)
            xa = None
        gemm = 2.0 * T * in_f * out_f
        halves = 2 if alpha != 1 else 1
        units = (18.0 if var_code == TE_VARIANT_OURS else 24.0) * halves
        with _on_device(Xc) as lib, _timed("linear_x6_general", units * gemm,
                                           halves * (6.0 * (2 * T * in_f + 3 * in_f * out_f + 2 * T * out_f) + 16.0 * T * in_f)):
            ws = _ws(lib.te_linear_relprop_x6_general_workspace_bytes(T, in_f, out_f, var_code), Xc)
            _lib.check(lib.te_linear_relprop_x6_general_f32(_ptr(Rc), rs_ptr, rs_stride, rps, _ptr(Xc), _ptr(Wc), _ptr(wp),
                                                            _ptr(wpl), _ptr(xa), _ptr(Yg), _ptr(bg), _ptr(out), T, in_f,
                                                            out_f, float(alpha), var_code, (X6_TILE | X6_FLAGS) & ~0x3c00,
                                                            _ptr(x6_status(Xc.device)), _ptr(ws), ws.numel(), _stream(Xc)),
                       "te_linear_relprop_x6_general_f32")
            if X6_CHECK:
                x6_raise_if_failed(Xc.device)
        return out.reshape(*lead, in_f)
    if fwd:
        Yc = _c(Y.detach()).reshape(-1, out_f)
        bc = None if bias is None else _c(bias.detach())
        if Yc.shape[0] != T:
            raise _lib.TeError(f"Linear.relprop: Y has {Yc.shape[0]} rows, X has {T}")
    if (fwd and USE_LINEAR_X6 and Yc.data_ptr() % 16 == 0 and (bc is None or bc.data_ptr() % 16 == 0)
            and _lib.load().te_linear_relprop_x6_supported(T, in_f, out_f)):
        planes = x6_weight_planes(W, cache)           # (keyed on W as the caller holds it, not on a contiguous copy)
        # the planes of |X| the layer's own forward product left behind (gemm_x6 keep_abs), if X is that tensor
        # (or the signed planes that product read: TE_X6_X_PLANES_SIGNED)
        xa = take_x_abs_planes(cache, X, T, in_f) if cache is not None else None
        x_signed = TE_X6_X_PLANES_SIGNED if planes_are_signed(xa) else 0
        with _on_device(Xc) as lib:
            ws = _ws(lib.te_linear_relprop_x6_workspace_bytes(T, in_f, out_f), Xc)
            status = x6_status(Xc.device)

            def call(flags):
                _lib.check(lib.te_linear_relprop_x6_f32(_ptr(Rc), rs_ptr, rs_stride, rps, _ptr(Xc), _ptr(Wc), _ptr(planes),
                                                        _ptr(xa), _ptr(Yc), _ptr(bc), _ptr(out), T, in_f, out_f,
                                                        X6_TILE | X6_FLAGS | x_signed | flags, _ptr(status), _ptr(ws), ws.numel(),
                                                        _stream(Xc)),
                           "te_linear_relprop_x6_f32")
            if KERNEL_TIMER is None:
                call(0)
            else:
                # bench.py roofline probe: the three phases one by one so that each is bracketed by HIP events.
                # flops = the bf16 MFMA work EXECUTED (six partial products per fp32 product); bytes = algorithmic
                gemm = 2.0 * T * in_f * out_f
                if xa is None:
                    with _timed("linear_x6_split", 0.0, 10.0 * T * in_f):
                        call(TE_X6_PHASE_SPLIT)
                else:       # the planes came with the forward product: this phase only resets the hand-over flags
                    call(TE_X6_PHASE_SPLIT)
                with _timed("linear_x6_zpass", 6.0 * gemm, 6.0 * (T * in_f + in_f * out_f + T * out_f) + 8.0 * T * out_f):
                    call(TE_X6_PHASE_Z)
                with _timed("linear_x6_cpass", 12.0 * gemm, 6.0 * (T * out_f + 2 * in_f * out_f) + 8.0 * T * in_f):
                    call(TE_X6_PHASE_C)
            if X6_CHECK:
                rc = lib.te_linear_relprop_x6_check(_ptr(ws), T, in_f, out_f, _stream(Xc))
                if rc != 0:
                    status.zero_()
                    raise _lib.TeError(f"te_linear_relprop_x6_f32({T},{in_f},{out_f}): a workgroup waited in vain for the "
                                       f"accumulators of a shared tile (status {rc}); the result is invalid")
                x6_raise_if_failed(Xc.device)
        return out.reshape(*lead, in_f)
    if KERNEL_TIMER is not None and fast_ok:
        # bench.py roofline probe: same two kernels, launched one by one so that each launch can be
        # bracketed by HIP events on the stream it runs on
        with _on_device(Xc) as lib:
            S = torch.empty((T, out_f), dtype=torch.float32, device=X.device)
            st = _stream(Xc)
            if fwd:
                with _timed("linear_zpass_fwd", 2.0 * T * in_f * out_f, 4.0 * (T * in_f + 3 * T * out_f + in_f * out_f)):
                    _lib.check(lib.te_linear_zpass_fwd_f32(_ptr(Rc), rs_ptr, rs_stride, rps, _ptr(Xc), _ptr(Wc),
                                                           _ptr(Yc), _ptr(bc), _ptr(S), T, in_f, out_f, st),
                               "te_linear_zpass_fwd_f32")
            else:
                with _timed("linear_zpass", 2.0 * T * (2 * in_f) * out_f, 4.0 * (T * in_f + 2 * T * out_f + in_f * out_f)):
                    _lib.check(lib.te_linear_zpass_f32(_ptr(Rc), _ptr(Xc), _ptr(Wc), _ptr(S), T, in_f, out_f, st),
                               "te_linear_zpass_f32")
            with _timed("linear_cpass", 2.0 * T * (2 * in_f) * out_f, 4.0 * (T * out_f + 2 * T * in_f + in_f * out_f)):
                _lib.check(lib.te_linear_cpass_f32(_ptr(S), _ptr(Xc), _ptr(Wc), _ptr(out), T, in_f, out_f, st),
                           "te_linear_cpass_f32")
        return out.reshape(*lead, in_f)
    with _on_device(Xc) as lib:
        ws = _ws(lib.te_linear_relprop_workspace_bytes(T, in_f, out_f, var), Xc)
        if fwd:
            _lib.check(lib.te_linear_relprop_fwd_f32(_ptr(Rc), rs_ptr, rs_stride, rps, _ptr(Xc), _ptr(Wc),
                                                     _ptr(Yc), _ptr(bc), _ptr(out), T, in_f, out_f, _ptr(ws),
                                                     ws.numel(), _stream(Xc)),
                       "te_linear_relprop_fwd_f32")
        else:
            _lib.check(lib.te_linear_relprop_f32(_ptr(Rc), _ptr(Xc), _ptr(Wc), _ptr(out), T, in_f, out_f, float(alpha),
                                                 var, _ptr(ws), ws.numel(), _stream(Xc)), "te_linear_relprop_f32")
    return out.reshape(*lead, in_f)


# ---------------------------------------------------------------------------------------- a4
def _bhnd(t: Tensor) -> Tuple[Tensor, int, int, int]:
    """[B,H,N,D] view with contiguous D -> (tensor, sb, sh, sn) in elements (copy only if needed)."""
    t = _prep(t)
    if t.stride(-1) != 1 or min(t.stride()[:3]) < 0:
        t = t.contiguous()
    sb, sh, sn, _ = t.stride()
    return t, sb, sh, sn


def _cached_z(z: Optional[Tensor], shape) -> Optional[Tensor]:
    """The forward product the einsum / MatMul module cached as self.Y, if it has the expected shape."""
    if z is None or not USE_FORWARD_PRODUCTS or tuple(z.shape) != tuple(shape):
        return None
    return _c(z.detach())


def matmul_relprop_av(R: Tensor, attn: Tensor, v: Tensor, out_scale: float = 1.0,
                      cam_v_out: Optional[Tensor] = None, variant="ours", z: Optional[Tensor] = None
                      ) -> Tuple[Tensor, Tensor]:
    """AV rule.  R, v: [B,H,N,D] (any strides with contiguous D); attn [B,H,N,N].
    Returns (cam_attn [B,H,N,N], cam_v [B,H,N,D]); cam_v is written into `cam_v_out` if given (a
    [B,H,N,D] view, e.g. a slice of the 'b n (qkv h d)' relevance buffer).  z (optional) = attn @ v as the
    forward pass computed it (self.Y of the product module).  bf16 attn / v: matmul_relprop_av_bf16."""
    if _any_f64(R, attn, v):
        return matmul_relprop_av_f64(R, attn, v, out_scale, cam_v_out, variant, z)
    if _is_bf16(attn) or _is_bf16(v):
        return matmul_relprop_av_bf16(R, attn, v, out_scale, cam_v_out, variant, z)
    B, H, N, D = v.shape
    zc = None
    z_str = (H * N * D, N * D, D)
    if z is not None and USE_FORWARD_PRODUCTS and tuple(z.shape) == (B, H, N, D):
        zd = _prep(z.detach())
        if zd.stride(-1) == 1 and min(zd.stride()[:3]) > 0:
            zc, z_str = zd, tuple(zd.stride()[:3])        # read in place (e.g. a view of the 'b n (h d)' activation)
        else:
            zc = zd.contiguous()
    R, r_sb, r_sh, r_sn = _bhnd(R)
    v, v_sb, v_sh, v_sn = _bhnd(v)
    attn = _c(attn)
    cam_attn = torch.empty((B, H, N, N), dtype=torch.float32, device=attn.device)
    cam_v = cam_v_out if cam_v_out is not None else torch.empty((B, H, N, D), dtype=torch.float32, device=attn.device)
    if cam_v.stride(-1) != 1:
        raise _lib.TeError("cam_v_out must have a contiguous last dim")
    cv_sb, cv_sh, cv_sn, _ = cam_v.stride()
    with _on_device(attn) as lib, _timed("attention_av_rule", 4.0 * B * H * N * N * D,
                                         4.0 * B * H * (2 * N * N + 5 * N * D)):
        ws = _ws(lib.te_matmul_relprop_av_workspace_bytes(B, H, N, D), attn)
        head = (_ptr(R), r_sb, r_sh, r_sn, _ptr(attn), _ptr(v), v_sb, v_sh, v_sn)
        tail = (_ptr(cam_attn), _ptr(cam_v), cv_sb, cv_sh, cv_sn, B, H, N, D, float(out_scale), _variant(variant),
                _ptr(ws), ws.numel(), _stream(attn))
        rc = lib.te_matmul_relprop_av_f32(*head, _ptr(zc), *z_str, *tail)
        if rc == _lib.TE_ERR_UNSUPPORTED and zc is not None and not zc.is_contiguous():
            zc = zc.contiguous()       # kernels that read Z as a contiguous [B,H,N,D] tensor
            rc = lib.te_matmul_relprop_av_f32(*head, _ptr(zc), H * N * D, N * D, D, *tail)
        _lib.check(rc, "te_matmul_relprop_av_f32")
    return cam_attn, cam_v


def matmul_relprop_qk(R: Tensor, q: Tensor, k: Tensor, out_scale: float = 1.0,
                      cam_q_out: Optional[Tensor] = None, cam_k_out: Optional[Tensor] = None,
                      variant="ours", z: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """QK rule.  R [B,H,N,N]; q, k [B,H,N,D] -> (cam_q, cam_k) [B,H,N,D].  z (optional) = the UNSCALED q @ k^T as
    the forward pass computed it (self.Y of the product module).  bf16 q / k: matmul_relprop_qk_bf16."""
    if _any_f64(R, q, k):
        return matmul_relprop_qk_f64(R, q, k, out_scale, cam_q_out, cam_k_out, variant, z)
    if _is_bf16(q) or _is_bf16(k):
        return matmul_relprop_qk_bf16(R, q, k, out_scale, cam_q_out, cam_k_out, variant, z)
    B, H, N, D = q.shape
    zc = _cached_z(z, (B, H, N, N))
    q, q_sb, q_sh, q_sn = _bhnd(q)
    k, k_sb, k_sh, k_sn = _bhnd(k)
    R, r_scale = _split_deferred(R)
    R = _c(R)
    dev = R.device
    cam_q = cam_q_out if cam_q_out is not None else torch.empty((B, H, N, D), dtype=torch.float32, device=dev)
    cam_k = cam_k_out if cam_k_out is not None else torch.empty((B, H, N, D), dtype=torch.float32, device=dev)
    if cam_q.stride(-1) != 1 or cam_k.stride(-1) != 1:
        raise _lib.TeError("cam_q_out / cam_k_out must have a contiguous last dim")
    cq, ck = cam_q.stride(), cam_k.stride()
    with _on_device(R) as lib, _timed("attention_qk_rule", 4.0 * B * H * N * N * D,
                                      4.0 * B * H * (2 * N * N + 4 * N * D)):
        ws = _ws(lib.te_matmul_relprop_qk_workspace_bytes(B, H, N, D), R)
        tail = (_ptr(q), q_sb, q_sh, q_sn, _ptr(k), k_sb, k_sh, k_sn, _ptr(zc), _ptr(cam_q), cq[0], cq[1], cq[2],
                _ptr(cam_k), ck[0], ck[1], ck[2], B, H, N, D, float(out_scale), _variant(variant), _ptr(ws), ws.numel(),
                _stream(R))
        rc = lib.te_matmul_relprop_qk_f32(_ptr(R), _ptr(r_scale), 0 if r_scale is None else r_scale.stride(0), *tail)
        if rc == _lib.TE_ERR_UNSUPPORTED and r_scale is not None:
            R = _c(Deferred(R, r_scale).materialise())     # kernels that take a plain relevance operand
            rc = lib.te_matmul_relprop_qk_f32(_ptr(R), None, 0, *tail)
        _lib.check(rc, "te_matmul_relprop_qk_f32")
    return cam_q, cam_k


# ---------------------------------------------------------------------------------------- 8f.1 producers
# Attention blocks run their forward (and attention-gradient backward) on the hand-written producer kernels where
# te_attention_forward_supported(N, D) (head dim 64, N <= 224); stock PyTorch otherwise.  bench.py --producers fused.
USE_FUSED_PRODUCERS = False


class stock_forward:
    """``with ops.stock_forward(): model(...)``: this forward pass runs on stock PyTorch whatever USE_FUSED_PRODUCERS says
    (the flag is read while the graph is built; the backward pass follows the nodes that were recorded).  A head-masked pass
    of BertModel / VisionTransformer runs inside it: the attention producers know no mask, and with every other producer off
    as well a masked pass gives the same bits under either setting of the flag."""

    def __enter__(self):
        global USE_FUSED_PRODUCERS
        self.was, USE_FUSED_PRODUCERS = USE_FUSED_PRODUCERS, False

    def __exit__(self, *exc):
        global USE_FUSED_PRODUCERS
        USE_FUSED_PRODUCERS = self.was


def attention_forward_supported(N: int, D: int) -> bool:
    """One of the producer kernel families takes the shape: the one-workgroup-per-head kernels (N <= 224) or the
    row-tile kernels of csrc/te_attn_long.hip (N <= 640)."""
    lib = _lib.load()
    return bool(lib.te_attention_forward_supported(int(N), int(D)) or lib.te_attention_strided_supported(int(N), int(D)))


def attention_forward_bf16_supported(N: int, D: int) -> bool:
    """The bf16 producer kernels of csrc/te_attn_bf16.hip take the shape (head dim 64, 1 <= N <= 640)."""
    return bool(_lib.load().te_attention_bf16_supported(int(N), int(D)))


def _heads(t: Tensor, H: int):
    """[B,N,H*64] activation (any batch / token strides, contiguous features) -> (pointer tensor, sb, sh, sn) of its
    [B,H,N,64] view."""
    sb, sn, sc = t.stride()
    if sc != 1:
        raise _lib.TeError("attention producers need a contiguous feature dimension")
    return t, sb, 64, sn


def attention_forward_qkv(q: Tensor, k: Tensor, v: Tensor, num_heads: int, scale: float,
                          mask: Optional[Tensor] = None, want_z: bool = True, want_x: bool = False):
    """q, k, v: [B,N,C] views ('b n (h d)', e.g. thirds of the fused ViT activation or BERT's three Linear outputs);
    mask [B,N] additive or None -> (out [B,N,C], attn [B,H,N,N], z_qk [B,H,N,N] unscaled or None, x = z_qk * scale
    [B,H,N,N] or None: the scaled scores BEFORE the mask is added, i.e. the first operand of BERT's Add module).
    csrc/te_attn_long.hip."""
    if _is_bf16(q) or _is_bf16(k) or _is_bf16(v):
        return attention_forward_qkv_bf16(q, k, v, num_heads, scale, mask, want_z, want_x)
    B, N, C = q.shape
    H, D = num_heads, C // num_heads
    dev = q.device
    out = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    attn = torch.empty((B, H, N, N), dtype=torch.float32, device=dev)
    zqk = torch.empty((B, H, N, N), dtype=torch.float32, device=dev) if want_z else None
    xsc = torch.empty((B, H, N, N), dtype=torch.float32, device=dev) if want_x else None
    mk = None if mask is None else _c(mask.reshape(B, N))
    (q, qb, qh, qn), (k, kb, kh, kn), (v, vb, vh, vn) = _heads(_prep(q), H), _heads(_prep(k), H), _heads(_prep(v), H)
    with _on_device(q) as lib, _timed("attention_forward", 4.0 * B * H * N * N * D,
                                      4.0 * B * ((2 + bool(want_x)) * H * N * N + 4 * N * C)):
        _lib.check(lib.te_attention_forward_strided_f32(_ptr(q), qb, qh, qn, _ptr(k), kb, kh, kn, _ptr(v), vb, vh, vn,
                                                        _ptr(mk), _ptr(zqk), _ptr(xsc), _ptr(attn), _ptr(out), N * C, 64, C,
                                                        B, H, N, D, float(scale), _stream(q)),
                   "te_attention_forward_strided_f32")
    return out, attn, zqk, xsc


def attention_forward_qkv_bf16(q: Tensor, k: Tensor, v: Tensor, num_heads: int, scale: float,
                               mask: Optional[Tensor] = None, want_z: bool = True, want_x: bool = False):
    """attention_forward_qkv on bf16 views (a bf16 model): every result is bf16, rounded once from fp32 where the stock bf16
    path rounds -- z_qk = bf16(q k^T), x = bf16(z_qk * scale), attn = bf16(softmax(bf16(x + mask))), out = bf16(attn v) with
    the rounded attn.  csrc/te_attn_bf16.hip; head dim 64, N <= 640 (attention_forward_bf16_supported)."""
    q, k, v = _prep_bf16(q), _prep_bf16(k), _prep_bf16(v)
    B, N, C = q.shape
    H, D = num_heads, C // num_heads
    dev = q.device
    new = lambda *shape: torch.empty(shape, dtype=torch.bfloat16, device=dev)      # noqa: E731
    out, attn = new(B, N, C), new(B, H, N, N)
    zqk = new(B, H, N, N) if want_z else None
    xsc = new(B, H, N, N) if want_x else None
    mk = None if mask is None else _c16(mask.reshape(B, N))
    (q, qb, qh, qn), (k, kb, kh, kn), (v, vb, vh, vn) = _heads(q, H), _heads(k, H), _heads(v, H)
    with _on_device(q) as lib, _timed("attention_forward", 4.0 * B * H * N * N * D,
                                      2.0 * B * ((2 + bool(want_x)) * H * N * N + 4 * N * C)):
        _lib.check(lib.te_attention_forward_strided_bf16(_ptr(q), qb, qh, qn, _ptr(k), kb, kh, kn, _ptr(v), vb, vh, vn,
                                                         _ptr(mk), _ptr(zqk), _ptr(xsc), _ptr(attn), _ptr(out), N * C, 64, C,
                                                         B, H, N, D, float(scale), _stream(q)),
                   "te_attention_forward_strided_bf16")
    return out, attn, zqk, xsc


def attention_backward_qkv_bf16(d_out: Tensor, q: Optional[Tensor], k: Optional[Tensor], v: Tensor, attn: Tensor,
                                num_heads: int, scale: float, d_q: Optional[Tensor], d_k: Optional[Tensor], d_v: Tensor,
                                need_qk: bool = True) -> Tensor:
    """attention_backward_qkv on bf16 tensors: d_attn = bf16(d_out v^T), d_v = bf16(attn^T d_out), and with need_qk
    d_q = bf16(scale d_s k), d_k = bf16(scale d_s^T q), d_s = bf16(attn (d_attn - rowsum(attn d_attn))).  The row sums are
    taken over the N x N tensors: the forward output is not an operand.  csrc/te_attn_bf16.hip."""
    B, N, C = d_out.shape
    H, D = num_heads, C // num_heads
    d_out, attn = _c16(d_out), _c16(attn)
    d_attn = torch.empty_like(attn)
    hd = lambda t: (None, 0, 0, 0) if t is None else _heads(_prep_bf16(t), H)      # noqa: E731
    (q, qb, qh, qn), (k, kb, kh, kn), (v, vb, vh, vn) = hd(q), hd(k), hd(v)
    (dq, dqb, dqh, dqn), (dk, dkb, dkh, dkn), (dv, dvb, dvh, dvn) = hd(d_q), hd(d_k), hd(d_v)
    with _on_device(d_out) as lib, _timed("attention_backward", (8.0 if need_qk else 4.0) * B * H * N * N * D,
                                          2.0 * B * ((5 if need_qk else 2) * H * N * N + 8 * N * C)):
        ws = _ws(lib.te_attention_backward_strided_bf16_workspace_bytes(B, H, N), d_out)
        _lib.check(lib.te_attention_backward_strided_bf16(_ptr(d_out), N * C, 64, C, _ptr(q), qb, qh, qn, _ptr(k), kb, kh, kn,
                                                          _ptr(v), vb, vh, vn, _ptr(attn), _ptr(d_attn), _ptr(dq), dqb, dqh,
                                                          dqn, _ptr(dk), dkb, dkh, dkn, _ptr(dv), dvb, dvh, dvn, B, H, N, D,
                                                          float(scale), int(bool(need_qk)), _ptr(ws), ws.numel(),
                                                          _stream(d_out)), "te_attention_backward_strided_bf16")
    return d_attn


def attention_backward_qkv(d_out: Tensor, q: Tensor, k: Tensor, v: Tensor, attn: Tensor, num_heads: int, scale: float,
                           d_q: Optional[Tensor], d_k: Optional[Tensor], d_v: Tensor, need_qk: bool = True,
                           out: Optional[Tensor] = None) -> Tensor:
    """Gradient of attention_forward_qkv: d_out [B,N,C]; d_q / d_k / d_v: [B,N,C] views written in place (d_q, d_k may be
    None with need_qk=False).  Returns d_attn [B,H,N,N].  out: the forward output [B,N,C] attention_forward_qkv returned for
    these inputs, if the caller still holds it -- the softmax backward's row sums are then d_out . out and the row side runs
    on csrc/te_attn_bwd6l.hip (the `out` operand of te_attention_backward_strided_f32)."""
    if any(_is_bf16(t) for t in (d_out, q, k, v, attn)):
        return attention_backward_qkv_bf16(d_out, q, k, v, attn, num_heads, scale, d_q, d_k, d_v, need_qk=need_qk)
    B, N, C = d_out.shape
    H, D = num_heads, C // num_heads
    d_out, attn = _c(d_out), _c(attn)
    d_attn = torch.empty_like(attn)
    hd = lambda t: (None, 0, 0, 0) if t is None else _heads(_prep(t), H)      # noqa: E731
    (q, qb, qh, qn), (k, kb, kh, kn), (v, vb, vh, vn) = hd(q), hd(k), hd(v)
    (dq, dqb, dqh, dqn), (dk, dkb, dkh, dkn), (dv, dvb, dvh, dvn) = hd(d_q), hd(d_k), hd(d_v)
    with _on_device(d_out) as lib, _timed("attention_backward", (8.0 if need_qk else 4.0) * B * H * N * N * D,
                                          4.0 * B * ((4 if need_qk else 2) * H * N * N + 8 * N * C)):
        ws = _ws(lib.te_attention_backward_strided_workspace_bytes(B, H, N), d_out)
        if not (out is not None and tuple(out.shape) == (B, N, C) and out.dtype == d_out.dtype and out.stride(-1) == 1):
            out = None
        (o, ob, oh, on) = hd(out)
        _lib.check(lib.te_attention_backward_strided_f32(_ptr(d_out), N * C, 64, C, _ptr(o), ob, oh, on, _ptr(q), qb, qh, qn,
                                                         _ptr(k), kb, kh, kn, _ptr(v), vb, vh, vn, _ptr(attn), _ptr(d_attn),
                                                         _ptr(dq), dqb, dqh, dqn, _ptr(dk), dkb, dkh, dkn, _ptr(dv), dvb, dvh,
                                                         dvn, B, H, N, D, float(scale), int(bool(need_qk)), _ptr(ws),
                                                         ws.numel(), _stream(d_out)), "te_attention_backward_strided_f32")
    return d_attn


def attention_forward_planes_supported(qkv: Tensor, num_heads: int) -> bool:
    """Can attention_forward emit the operand planes of its output (the out_planes of te_attention_forward_f32: N <= 224, head dim 64)?"""
    B, N, C3 = qkv.shape
    C = C3 // 3
    return (qkv.is_cuda and qkv.dtype == torch.float32 and C % num_heads == 0 and C // num_heads == 64 and N <= 224
            and bool(_lib.load().te_attention_forward_supported(N, 64)))


def attention_forward(qkv: Tensor, num_heads: int, scale: float, planes: bool = False, planes_abs: bool = True):
    """qkv [B,N,3C] ('b n (qkv h d)') -> (out [B,N,C] = softmax(q k^T * scale) v as 'b n (h d)', attn [B,H,N,N],
    z_qk [B,H,N,N] = the unscaled q k^T).  ViT_LRP.py:132-152 without the q/k/v, scale, softmax and transpose passes.
    planes=True (attention_forward_planes_supported): additionally the signed planes of out [B N, C] and the planes of |out| --
    what gemm_x6's split pass over out would build -- as a fourth and fifth result (planes_abs=False: the second set is not
    stored, the fifth result is None).
    A bf16 qkv (a bf16 model) runs on csrc/te_attn_bf16.hip and returns bf16 tensors; planes=True is fp32-only."""
    if _is_bf16(qkv):
        if planes:
            raise _lib.TeError("attention_forward(planes=True): operand planes are emitted from float32 activations only")
        qkv = _c16(qkv)
        C = qkv.shape[-1] // 3
        out, attn, zqk, _ = attention_forward_qkv_bf16(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], num_heads, scale)
        return out, attn, zqk
    qkv = _c(qkv)
    B, N, C3 = qkv.shape
    C = C3 // 3
    H, D = num_heads, C // num_heads
    if not _lib.load().te_attention_forward_supported(N, D):
        if planes:
            raise _lib.TeError("attention_forward(planes=True): shape not served by te_attention_forward_f32")
        out, attn, zqk, _ = attention_forward_qkv(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], num_heads, scale)
        return out, attn, zqk
    out = torch.empty((B, N, C), dtype=torch.float32, device=qkv.device)
    attn = torch.empty((B, H, N, N), dtype=torch.float32, device=qkv.device)
    zqk = torch.empty((B, H, N, N), dtype=torch.float32, device=qkv.device)
    extra = (12.0 if planes_abs else 6.0) * B * N * C if planes else 0.0
    with _on_device(qkv) as lib, _timed("attention_forward", 4.0 * B * H * N * N * D, 4.0 * B * (2 * H * N * N + 4 * N * C) + extra):
        nb, xs, xa = 0, None, None
        if planes:
            nb = lib.te_linear_x6_planes_bytes(B * N, C)
            xs, xa = _ws(nb, qkv), _ws(nb, qkv) if planes_abs else None
        _lib.check(lib.te_attention_forward_f32(_ptr(qkv), _ptr(zqk), _ptr(attn), _ptr(out), _ptr(xs), _ptr(xa), nb, B, H, N,
                                                D, float(scale), _stream(qkv)), "te_attention_forward_f32")
    return (out, attn, zqk, xs, xa) if planes else (out, attn, zqk)


def attention_backward(d_out: Tensor, qkv: Tensor, attn: Tensor, num_heads: int, scale: float,
                       need_qk: bool = True, out: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """Gradient of attention_forward: d_out [B,N,C] -> (d_attn [B,H,N,N], d_qkv [B,N,3C]).  need_qk=False: nothing below
    consumes d_qkv (the lowest block whose attention gradient is wanted): only d_attn is meaningful, d_qkv is scratch.
    out: the forward output attention_forward returned for these inputs, if the caller still holds it -- the softmax half then
    takes its row sums from d_out . out (the `out` operand of te_attention_backward_f32).  bf16 tensors: csrc/te_attn_bf16.hip (`out` unused)."""
    if _is_bf16(d_out) or _is_bf16(qkv) or _is_bf16(attn):
        qkv = _c16(qkv)
        C = qkv.shape[-1] // 3
        d_qkv = torch.empty_like(qkv)
        th = lambda t, i: t[..., i * C:(i + 1) * C]      # noqa: E731
        d_attn = attention_backward_qkv_bf16(d_out, th(qkv, 0), th(qkv, 1), th(qkv, 2), attn, num_heads, scale,
                                             th(d_qkv, 0), th(d_qkv, 1), th(d_qkv, 2), need_qk=need_qk)
        return d_attn, d_qkv
    d_out, qkv, attn = _c(d_out), _c(qkv), _c(attn)
    B, N, C3 = qkv.shape
    C = C3 // 3
    H, D = num_heads, C // num_heads
    d_qkv = torch.empty_like(qkv)
    if not _lib.load().te_attention_forward_supported(N, D):
        th = lambda t, i: t[..., i * C:(i + 1) * C]      # noqa: E731
        d_attn = attention_backward_qkv(d_out, th(qkv, 0), th(qkv, 1), th(qkv, 2), attn, num_heads, scale,
                                        th(d_qkv, 0), th(d_qkv, 1), th(d_qkv, 2), need_qk=need_qk, out=out)
        return d_attn, d_qkv
    d_attn = torch.empty_like(attn)
    with _on_device(qkv) as lib, _timed("attention_backward", (8.0 if need_qk else 4.0) * B * H * N * N * D,
                                        4.0 * B * ((4 if need_qk else 2) * H * N * N + 8 * N * C)):
        if not (out is not None and need_qk and tuple(out.shape) == tuple(d_out.shape) and out.is_contiguous()
                and out.dtype == d_out.dtype):
            out = None
        _lib.check(lib.te_attention_backward_f32(_ptr(d_out), _ptr(out), _ptr(qkv), _ptr(attn), _ptr(d_attn), _ptr(d_qkv), B,
                                                 H, N, D, float(scale), int(bool(need_qk)), _stream(qkv)),
                   "te_attention_backward_f32")
    return d_attn, d_qkv


def layernorm_supported(x: Tensor) -> bool:
    """The LayerNorm / GELU producer kernels take contiguous fp32 device tensors, rows of <= 2048 elements (multiple of 4)."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2
            and bool(_lib.load().te_layernorm_supported(int(x.shape[-1]))))


def layernorm_forward(x: Tensor, weight: Tensor, bias: Optional[Tensor], eps: float) -> Tuple[Tensor, Tensor, Tensor]:
    """nn.LayerNorm over the last dimension (modules/layers_ours.py:76): x [..., C] -> (y, mean [T], rstd [T])."""
    x = _c(x)
    C = x.shape[-1]
    T = x.numel() // C
    y = torch.empty_like(x)
    mean = torch.empty((T,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((T,), dtype=torch.float32, device=x.device)
    with _on_device(x) as lib, _timed("layernorm_forward", 0.0, 4.0 * 2 * T * C):
        _lib.check(lib.te_layernorm_forward_f32(_ptr(x), _ptr(_c(weight)), _ptr(_c(bias)) if bias is not None else None,
                                                _ptr(y), _ptr(mean), _ptr(rstd), T, C, float(eps), _stream(x)),
                   "te_layernorm_forward_f32")
    return y, mean, rstd


def layernorm_backward(dy: Tensor, x: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor,
                       add: Optional[Tensor] = None) -> Tensor:
    """Input gradient of layernorm_forward; `add` (same shape) is summed in -- the gradient of the residual branch that
    bypasses the LayerNorm (ViT_LRP.py:203-205)."""
    dy, x = _c(dy), _c(x)
    C = x.shape[-1]
    T = x.numel() // C
    dx = torch.empty_like(x)
    with _on_device(x) as lib, _timed("layernorm_backward", 0.0, 4.0 * (3 + (add is not None)) * T * C):
        _lib.check(lib.te_layernorm_backward_f32(_ptr(dy), _ptr(x), _ptr(_c(weight)), _ptr(mean), _ptr(rstd),
                                                 _ptr(_c(add)) if add is not None else None, _ptr(dx), T, C, _stream(x)),
                   "te_layernorm_backward_f32")
    return dx


def gelu_forward(x: Tensor) -> Tensor:
    """nn.GELU (exact erf form; modules/layers_ours.py:70, ViT_LRP.py:57)."""
    x = _c(x)
    y = torch.empty_like(x)
    with _on_device(x) as lib, _timed("gelu_forward", 0.0, 4.0 * 2 * x.numel()):
        _lib.check(lib.te_gelu_forward_f32(_ptr(x), _ptr(y), x.numel(), _stream(x)), "te_gelu_forward_f32")
    return y


X6_FUSE_GELU = os.environ.get("TE_X6_FUSE_GELU", "1") not in ("", "0")     # measurement switch: GELU emits operand planes


# The backward hand-off (GELU-backward writes the planes of the hidden gradient into the producing Linear's cache and autograd
# carries a NaN placeholder instead of the fp32 gradient) is only sound where the WHOLE backward graph is known: nobody but
# that Linear's backward may consume the gradient (no tensor hook / retain_grad / autograd.grad on the hidden activation, no
# second consumer).  It is therefore OFF unless the caller that owns forward + backward opts in for its own forward pass
# (ADVICE r5): LRP / Baselines / Generator do, inside ``gelu_backward_plane_handoff()``; a plain ``model(x)`` never does.
_GELU_BWD_HANDOFF = 0


class gelu_backward_plane_handoff:
    """Context manager for a forward pass whose backward the caller drives itself with torch.autograd.grad towards attention
    tensors only (generators.py).  Re-entrant; the decision is taken at forward time (per GELU node)."""

    def __enter__(self):
        global _GELU_BWD_HANDOFF
        _GELU_BWD_HANDOFF += 1
        return self

    def __exit__(self, *exc):
        global _GELU_BWD_HANDOFF
        _GELU_BWD_HANDOFF -= 1


def gelu_backward_handoff_active() -> bool:
    return _GELU_BWD_HANDOFF > 0


def gelu_planes_supported(x: Tensor) -> bool:
    return bool(X6_FUSE_GELU and x.dim() >= 2 and x.shape[-1] >= 16 and x.shape[-1] % 16 == 0)


def gelu_forward_planes(x: Tensor, planes_abs: bool = True):
    """y = gelu(x) (gelu_forward's bits) plus the signed planes of y and the planes of |y| -- what gemm_x6's split pass
    over y would build (te_gelu_forward_x6_planes_f32).  Returns (y, planes, planes_abs); planes_abs=False: the second set is
    not stored and comes back as None."""
    x = _c(x)
    K = x.shape[-1]
    T = x.numel() // K
    y = torch.empty_like(x)
    with _on_device(x) as lib, _timed("gelu_forward", 0.0, (4.0 * 2 + (12.0 if planes_abs else 6.0)) * x.numel()):
        nb = lib.te_linear_x6_planes_bytes(T, K)
        xs, xa = _ws(nb, x), _ws(nb, x) if planes_abs else None
        _lib.check(lib.te_gelu_forward_x6_planes_f32(_ptr(x), _ptr(y), T, K, _ptr(xs), _ptr(xa), nb, _stream(x)),
                   "te_gelu_forward_x6_planes_f32")
    return y, xs, xa


def gelu_backward_planes(dy: Tensor, x: Tensor) -> Tensor:
    """The signed planes of dx = dy . gelu'(x), [T, K] with K = x.shape[-1]: the x_planes of the gemm_x6 that consumes the
    gradient (te_gelu_backward_x6_planes_f32); the fp32 dx is never written."""
    dy, x = _c(dy), _c(x)
    K = x.shape[-1]
    T = x.numel() // K
    with _on_device(x) as lib, _timed("gelu_backward", 0.0, (4.0 * 2 + 6.0) * x.numel()):
        nb = lib.te_linear_x6_planes_bytes(T, K)
        planes = _ws(nb, x)
        _lib.check(lib.te_gelu_backward_x6_planes_f32(_ptr(dy), _ptr(x), T, K, _ptr(planes), nb, _stream(x)),
                   "te_gelu_backward_x6_planes_f32")
    return planes


def gelu_backward(dy: Tensor, x: Tensor) -> Tensor:
    dy, x = _c(dy), _c(x)
    dx = torch.empty_like(x)
    with _on_device(x) as lib, _timed("gelu_backward", 0.0, 4.0 * 3 * x.numel()):
        _lib.check(lib.te_gelu_backward_f32(_ptr(dy), _ptr(x), _ptr(dx), x.numel(), _stream(x)), "te_gelu_backward_f32")
    return dx


# ---------------------------------------------------------------------------------------- a5
# Model-internal Add rules hand their per-sample rescale to the consuming Clone / Linear kernels (one streaming pass
# instead of two).  Tests flip this to run the two-pass rule on the same inputs.
USE_DEFERRED_ADD = True


def _is_bcast_mask(X0: Tensor, X1: Tensor) -> bool:
    """X1 is the BERT broadcast mask [B,1,1,N] (or [1,1,1,N]) against the scores X0 [B,H,N,N] (BERT.py:342,386-388)."""
    return X1.dim() == 4 and X0.dim() == 4 and X1.shape[1] == 1 and X1.shape[2] == 1 and X0.shape[1] * X0.shape[2] != 1


def add_relprop(R: Tensor, X0: Tensor, X1: Tensor, variant="ours", deferred: bool = False):
    """Add.relprop with per-sample sums.  dim 0 is the batch.  X1 has X0's shape, or batch 1 (shared by
    all samples), or is the BERT broadcast mask [B,1,1,N] against X0 [B,H,N,N].
    deferred=True (variant ours, same-shape operands): one streaming pass; returns two ``Deferred`` (unscaled tensor +
    per-sample factor) for clone_relprop / linear_relprop to consume.  bf16 X0 / X1: add_relprop_bf16."""
    if _any_f64(R, X0, X1):
        return add_relprop_f64(R, X0, X1, variant, deferred)
    if _is_bf16(X0) or _is_bf16(X1):
        return add_relprop_bf16(R, X0, X1, variant, deferred)
    B = X0.shape[0]
    R, X0 = _c(R), _c(X0)
    n = X0[0].numel()
    if _is_bcast_mask(X0, X1):
        H, N = X0.shape[1], X0.shape[3]
        mask = _c(X1).reshape(X1.shape[0], N)
        if mask.shape[0] == 1 and B > 1:
            mask = mask.expand(B, N).contiguous()
        out0 = torch.empty_like(X0)
        out1 = torch.empty((B, 1, 1, N), dtype=torch.float32, device=X0.device)
        if deferred and _variant(variant) == TE_VARIANT_OURS:
            fac = torch.empty((B, 2), dtype=torch.float32, device=X0.device)
            with _on_device(X0) as lib, _timed("add_bcast_mask_deferred", 0.0, 4.0 * B * (3 * H * N * N + 2 * N)):
                ws = _ws(lib.te_add_bcast_relprop_workspace_bytes(B, H, N), X0)
                _lib.check(lib.te_add_bcast_relprop_deferred_f32(_ptr(R), _ptr(X0), _ptr(mask), _ptr(out0), _ptr(out1),
                                                                 _ptr(fac), B, H, N, _ptr(ws), ws.numel(), _stream(X0)),
                           "te_add_bcast_relprop_deferred_f32")
            return Deferred(out0, fac[:, 0]), out1
        with _on_device(X0) as lib, _timed("add_bcast_mask", 0.0, 4.0 * B * (3 * H * N * N + 2 * N)):
            ws = _ws(lib.te_add_bcast_relprop_workspace_bytes(B, H, N), X0)
            _lib.check(lib.te_add_bcast_relprop_f32(_ptr(R), _ptr(X0), _ptr(mask), _ptr(out0), _ptr(out1), B, H, N,
                                                    _variant(variant), _ptr(ws), ws.numel(), _stream(X0)),
                       "te_add_bcast_relprop_f32")
        return out0, out1
    X1 = _c(X1)
    if X1.shape == X0.shape:
        x1_bs = n
    elif X1.shape[0] == 1 and X1.shape[1:] == X0.shape[1:]:
        x1_bs = 0
    else:
        raise _lib.TeError(f"Add.relprop: unsupported operand shapes {tuple(X0.shape)} + {tuple(X1.shape)}")
    out0, out1 = torch.empty_like(X0), torch.empty_like(X0)
    var = _variant(variant)
    x1_elems = n if x1_bs else n / B
    if deferred and var == TE_VARIANT_OURS:
        fac = torch.empty((B, 2), dtype=torch.float32, device=X0.device)
        with _on_device(X0) as lib, _timed("add_deferred", 0.0, 4.0 * B * (4 * n + x1_elems)):
            ws = _ws(lib.te_add_relprop_deferred_workspace_bytes(B, n), X0)
            _lib.check(lib.te_add_relprop_deferred_f32(_ptr(R), _ptr(X0), _ptr(X1), _ptr(out0), _ptr(out1), _ptr(fac), B,
                                                       n, x1_bs, _ptr(ws), ws.numel(), _stream(X0)),
                       "te_add_relprop_deferred_f32")
        return Deferred(out0, fac[:, 0]), Deferred(out1, fac[:, 1])
    with _on_device(X0) as lib, _timed("add", 0.0, 4.0 * B * (4 * n + x1_elems)):
        ws = _ws(lib.te_add_relprop_workspace_bytes(B, n), X0)
        _lib.check(lib.te_add_relprop_f32(_ptr(R), _ptr(X0), _ptr(X1), _ptr(out0), _ptr(out1), B, n, x1_bs,
                                          var, _ptr(ws), ws.numel(), _stream(X0)), "te_add_relprop_f32")
    return out0, out1


# ---------------------------------------------------------------------------------------- a6
def clone_relprop(Rs: Sequence, X: Tensor) -> Tensor:
    """Clone.relprop; relevance operands may be ``Deferred`` (their per-sample factor is applied inside the kernel).
    bf16 X: te_clone_relprop(_scaled)_bf16, fp32 relevance and output."""
    if len(Rs) not in (2, 3):
        raise _lib.TeError(f"Clone.relprop supports 2 or 3 aliases, got {len(Rs)}")
    if _any_f64(X, *Rs):
        return clone_relprop_f64(Rs, X)
    bf = _is_bf16(X)
    X = _c16(X) if bf else _c(X)
    sfx = "bf16" if bf else "f32"
    pairs = [_split_deferred(r) for r in Rs]
    Rs = [_c(r) for r, _ in pairs]
    scales = [sc for _, sc in pairs]
    for r in Rs:
        if r.numel() != X.numel():
            raise _lib.TeError("Clone.relprop: relevance / input size mismatch")
    out = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    nb = 4.0 * X.numel() * (len(Rs) + 1) + X.element_size() * X.numel()
    if any(sc is not None for sc in scales):
        B = X.shape[0]
        sp = [(None, 0) if sc is None else (sc.data_ptr(), sc.stride(0)) for sc in scales] + [(None, 0)]
        with _on_device(X) as lib, _timed("clone", 0.0, nb):
            _lib.check(getattr(lib, "te_clone_relprop_scaled_" + sfx)(
                _ptr(Rs[0]), sp[0][0], sp[0][1], _ptr(Rs[1]), sp[1][0], sp[1][1], _ptr(Rs[2]) if len(Rs) == 3 else None,
                sp[2][0], sp[2][1], _ptr(X), _ptr(out), B, X.numel() // B, _stream(X)), "te_clone_relprop_scaled_" + sfx)
        return out
    with _on_device(X) as lib, _timed("clone", 0.0, nb):
        _lib.check(getattr(lib, "te_clone_relprop_" + sfx)(_ptr(Rs[0]), _ptr(Rs[1]), _ptr(Rs[2]) if len(Rs) == 3 else None,
                                                           _ptr(X), _ptr(out), X.numel(), _stream(X)),
                   "te_clone_relprop_" + sfx)
    return out


# ---------------------------------------------------------------------------------------- a7
def index_select_relprop(R: Tensor, X: Tensor, index: int) -> Tensor:
    """IndexSelect.relprop for dim=1: R [B,1,C] or [B,C], X [B,N,C] -> [B,N,C] (fp32; X may be bf16; fp64 R and X -> fp64)."""
    if _any_f64(R, X):
        return index_select_relprop_f64(R, X, index)
    bf = _is_bf16(X)
    X = _c16(X) if bf else _c(X)
    B, N, C = X.shape
    R = _c(R).reshape(B, C)
    out = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    sfx = "bf16" if bf else "f32"
    with _on_device(X) as lib:
        _lib.check(getattr(lib, "te_index_select_relprop_" + sfx)(_ptr(R), _ptr(X), _ptr(out), B, N, C, int(index),
                                                                   _stream(X)), "te_index_select_relprop_" + sfx)
    return out


# ---------------------------------------------------------------------------------------- a10
def gradcam_headmean(grad: Tensor, cam: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """grad, cam [B,H,N,N] -> [B,N,N] = mean_h max(grad*cam, 0), per sample (grad may be bf16; cam and out fp32; fp64 grad
    and cam -> fp64)."""
    if _any_f64(grad, cam, out):
        return gradcam_headmean_f64(grad, cam, out)
    bf = _is_bf16(grad)
    grad, cam = (_c16(grad) if bf else _c(grad)), _c(cam)
    B, H, N, _ = cam.shape
    if out is None:
        out = torch.empty((B, N, N), dtype=torch.float32, device=cam.device)
    sfx = "bf16" if bf else "f32"
    with _on_device(cam) as lib, _timed("headmean", 0.0, (grad.element_size() + 4.0) * B * H * N * N + 4.0 * B * N * N):
        _lib.check(getattr(lib, "te_gradcam_headmean_" + sfx)(_ptr(grad), _ptr(cam), _ptr(out), B, H, N, _stream(cam)),
                   "te_gradcam_headmean_" + sfx)
    return out


def attn_headmean(attn: Tensor, out: Optional[Tensor] = None, clamp: bool = False, row0: bool = False) -> Tensor:
    """bf16 attention probabilities [B,H,N,N] (batch / head strides, last two dims contiguous) -> fp32 [B,N,N] =
    mean_h attn (clamp: mean_h max(attn, 0)), heads summed in order in fp32; row0=True -> [B,N], query row 0 alone.
    ``out``: a contiguous fp32 destination, e.g. one layer's slice of the rollout stack.  fp32 attention has no kernel
    here: the generators keep their torch expressions for it."""
    attn = _prep_bf16(attn)
    if attn.dim() != 4 or attn.shape[2] != attn.shape[3]:
        raise _lib.TeError(f"attn_headmean: expected [B,H,N,N] attention probabilities, got {tuple(attn.shape)}")
    B, H, N, _ = attn.shape
    if attn.stride(3) != 1 or attn.stride(2) != N:
        attn = attn.contiguous()
    shape = (B, N) if row0 else (B, N, N)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=attn.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != attn.device:
        raise _lib.TeError(f"attn_headmean: out must be a contiguous float32 {shape} on {attn.device}")
    flags = (TE_HEADMEAN_CLAMP if clamp else 0) | (TE_HEADMEAN_ROW0 if row0 else 0)
    n = N if row0 else N * N
    with _on_device(attn) as lib, _timed("attn_headmean", 0.0, 2.0 * B * H * n + 4.0 * B * n):
        _lib.check(lib.te_attn_headmean_bf16(_ptr(attn), attn.stride(0), attn.stride(1), _ptr(out), B, H, N, flags,
                                             _stream(attn)), "te_attn_headmean_bf16")
    return out


# ---------------------------------------------------------------------------------------- a11
# The generators consume row 0 of the rollout only: chain it as a row vector (te_rollout_f32 with TE_ROLLOUT_ROW0).
# Tests flip this to run the full (N x N)(N x N) product chain and slice row 0 afterwards.
USE_ROW0_CHAIN = True


def rollout(cams: Tensor, start_layer: int = 0, normalise: bool = False, cls_fixup: bool = False,
            row0_only: bool = False) -> Tensor:
    """cams [L,B,N,N] -> joint [B,N,N] (compute_rollout_attention); row0_only=True -> joint[:, 0] as [B,N] (the only row
    the generators read: ViT_LRP.py:369, ExplanationGenerator.py:58-59).  fp64 cams: rollout_f64."""
    if _is_f64(cams):
        return rollout_f64(cams, start_layer, normalise, cls_fixup, row0_only)
    cams = _c(cams)
    L, B, N, _ = cams.shape
    flags = (TE_ROLLOUT_NORMALISE if normalise else 0) | (TE_ROLLOUT_CLS_FIXUP if cls_fixup else 0) | \
        (TE_IMPL_SIMPLE if FORCE_SIMPLE else 0)
    if row0_only and USE_ROW0_CHAIN and not FORCE_SIMPLE and N <= 1024:
        row = torch.empty((B, N), dtype=torch.float32, device=cams.device)
        with _on_device(cams) as lib, _timed("rollout_row0_chain", 2.0 * (L - start_layer) * B * N * N,
                                             4.0 * (L - start_layer) * B * N * N):
            ws = _ws(lib.te_rollout_row0_workspace_bytes(B, N), cams)
            _lib.check(lib.te_rollout_f32(_ptr(cams), L, int(start_layer), B, N, flags | TE_ROLLOUT_ROW0, _ptr(row),
                                          _ptr(ws), ws.numel(), _stream(cams)), "te_rollout_f32")
        return row
    joint = torch.empty((B, N, N), dtype=torch.float32, device=cams.device)
    with _on_device(cams) as lib, _timed("rollout_matrix_chain", 2.0 * (L - 1 - start_layer) * B * N * N * N,
                                         4.0 * (L - start_layer) * B * N * N):
        ws = _ws(lib.te_rollout_workspace_bytes(L, B, N), cams)
        _lib.check(lib.te_rollout_f32(_ptr(cams), L, int(start_layer), B, N, flags, _ptr(joint), _ptr(ws), ws.numel(),
                                      _stream(cams)), "te_rollout_f32")
    return joint[:, 0] if row0_only else joint


# ---------------------------------------------------------------------------------------- 8f.3 Conv2d z^B
def conv2d_zb_relprop(R: Tensor, X: Tensor, W: Tensor, Y: Optional[Tensor], bias: Optional[Tensor] = None,
                      cache: Optional[dict] = None) -> Tensor:
    """Conv2d.relprop, z^B rule (layers_ours.py:242-256), for a stride == kernel, padding 0 convolution (the ViT patch
    embedding).  R [B,E,Hp,Wp] with any strides (the token-major view PatchEmbed.relprop builds is consumed in
    place), X [B,C,H,W], W [E,C,p,p], Y = the layer's forward output [B,E,Hp,Wp] -> relevance [B,C,H,W].
    bf16 X / W (a bf16 model): conv2d_zb_relprop_bf16, which reads neither Y nor the bias; `cache` keeps its weight planes."""
    if _any_f64(R, X, W):
        raise _lib.TeError(f"{DTYPES_MSG}; Conv2d.relprop (the z^B patch rule of method='full') has no torch.float64 "
                           "kernel: run method='full' on a float32 or bfloat16 model")
    if _is_bf16(X) or _is_bf16(W):
        return conv2d_zb_relprop_bf16(R, X, W, cache=cache)
    B, C, H, Wd = X.shape
    E, p = W.shape[0], W.shape[2]
    if W.shape[1] != C or W.shape[3] != p or H % p or Wd % p:
        raise _lib.TeError(f"conv2d_zb_relprop: not a patch convolution: X {tuple(X.shape)}, W {tuple(W.shape)}")
    Hp, Wp = H // p, Wd // p
    P = Hp * Wp
    if Y is None:
        raise _lib.TeError("conv2d_zb_relprop: float32 X / W need Y, the layer's forward output (only bfloat16 operands do without)")
    if tuple(R.shape) != (B, E, Hp, Wp) or tuple(Y.shape) != (B, E, Hp, Wp):
        raise _lib.TeError(f"conv2d_zb_relprop: R {tuple(R.shape)} / Y {tuple(Y.shape)} do not match [B,E,H/p,W/p]")
    Rt = R.permute(0, 2, 3, 1)                       # [B,Hp,Wp,E]
    st = Rt.stride()
    if R.dtype != torch.float32 or not (st[3] == 1 and st[2] == E and st[1] == Wp * E and st[0] >= P * E
                                        and R.data_ptr() % 16 == 0):
        Rt = Rt.float().contiguous()
        st = Rt.stride()
    X, W, Y = _c(X), _c(W), _c(Y)
    bias = None if bias is None else _c(bias)
    out = torch.empty_like(X)
    with _on_device(X) as lib:
        ws = _ws(lib.te_conv2d_zb_relprop_workspace_bytes(B, C, H, Wd, E, p), X)
        _lib.check(lib.te_conv2d_zb_relprop_f32(_ptr(Rt), st[0], _ptr(X), _ptr(W), _ptr(Y), _ptr(bias), _ptr(out), B, C,
                                                H, Wd, E, p, TE_IMPL_SIMPLE if FORCE_SIMPLE else 0, _ptr(ws),
                                                ws.numel(), _stream(X)), "te_conv2d_zb_relprop_f32")
    return out


# ---------------------------------------------------------------------------------------- 8f.2 consumer
def heatmap(maps: Tensor, scale: int = 16, normalise: bool = True, with_mask: bool = False):
    """maps [B, g*g] or [B,1,g,g] -> heat [B,1,g*scale,g*scale]: bilinear up-sampling + per-map min-max
    (imagenet_seg_eval.py:214-217); with_mask also returns the mean-threshold foreground mask (:219-221)."""
    m = _c(maps)
    B = m.shape[0]
    g = int(round((m.numel() // B) ** 0.5))
    if g * g * B != m.numel():
        raise _lib.TeError(f"heatmap: {tuple(maps.shape)} is not a batch of square patch maps")
    side = g * scale
    heat = torch.empty((B, 1, side, side), dtype=torch.float32, device=m.device)
    mask = torch.empty_like(heat) if with_mask else None
    with _on_device(m) as lib:
        _lib.check(lib.te_heatmap_f32(_ptr(m), _ptr(heat), _ptr(mask), B, g, int(scale), int(bool(normalise)), _stream(m)),
                   "te_heatmap_f32")
    return (heat, mask) if with_mask else heat


def _is_integer(t: Tensor) -> bool:
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def _dense(t: Tensor) -> Tensor:
    """t itself when it is contiguous (a dense view that starts off a 16-byte boundary stays a view: the kernels have an
    element-wise form), else a contiguous copy; never a cast (that is ``_c``)."""
    return t if t.is_contiguous() else t.contiguous()


def seg_metrics_packed(heat: Tensor, mask: Tensor, labels: Tensor):
    """``seg_metrics`` and the flat int64 buffer its results are views of -- counts [B*6], then the bits of ap [B], then
    the bits of f1 [B*H]: one device-to-host copy of it brings all three over."""
    if heat.dtype != torch.float32 or mask.dtype != torch.float32:
        raise _lib.TeError(f"seg_metrics takes a float32 heat map and a float32 0/1 mask, got {heat.dtype} / {mask.dtype}")
    if not _is_integer(labels):
        raise _lib.TeError(f"seg_metrics takes integer labels, got {labels.dtype}")
    if not (heat.is_cuda and mask.is_cuda and labels.is_cuda):
        raise _lib.TeError("seg_metrics needs tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
    if heat.dim() != 3 or mask.shape != heat.shape or labels.shape != heat.shape:
        raise _lib.TeError(f"seg_metrics: heat, mask and labels must be [B,H,W] alike, got {tuple(heat.shape)}, "
                           f"{tuple(mask.shape)}, {tuple(labels.shape)}")
    heat, mask = _c(heat), _c(mask)
    labels = labels.to(torch.int64).contiguous()
    B, H, W = heat.shape
    flat = torch.empty((B * (7 + H),), dtype=torch.int64, device=heat.device)
    counts = flat[:6 * B].view(B, 6)
    ap = flat[6 * B:7 * B].view(torch.float64)
    f1 = flat[7 * B:].view(torch.float64).view(B, H)
    with _on_device(heat) as lib:
        ws = _ws(lib.te_seg_metrics_workspace_bytes(B, H, W), heat)
        _lib.check(lib.te_seg_metrics_f32(_ptr(heat), _ptr(mask), _ptr(labels), _ptr(counts), _ptr(ap), _ptr(f1), B, H, W,
                                          _ptr(ws), ws.numel(), _stream(heat)), "te_seg_metrics_f32")
    return counts, ap, f1, flat


def seg_metrics(heat: Tensor, mask: Tensor, labels: Tensor):
    """The segmentation test of imagenet_seg_eval.py:219-232,263-273 per image, one launch, no synchronisation: heat
    [B,H,W] fp32, mask [B,H,W] fp32 0/1 (ops.heatmap's outputs as they are: NaN heat counts as 0 with mask 0), labels
    [B,H,W] of an integer dtype (< 0 = ignore) -> (counts int64 [B,6] = correct, labeled, inter0, inter1, union0, union1;
    ap float64 [B]; f1 float64 [B,H] = the F1 of every image row), as segmentation.pixel_accuracy / intersection_union /
    average_precision / row_f1 define them."""
    return seg_metrics_packed(heat, mask, labels)[:3]


# ---------------------------------------------------------------------------------------- map similarity (sanity.py)
def _map_pair(a: Tensor, b: Tensor, shape):
    """The checks of map_similarity that need no device -> (B, n, H, W, ssim): raises TeError before any HIP call."""
    if not (torch.is_tensor(a) and torch.is_tensor(b)):
        raise _lib.TeError("map_similarity takes two tensors")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise _lib.TeError(f"map_similarity takes float32 maps, got {a.dtype} / {b.dtype}")
    if a.shape != b.shape or a.dim() not in (2, 3) or a.numel() == 0:
        raise _lib.TeError(f"map_similarity: the maps must be [B,n] or [B,H,W] alike and not empty, got {tuple(a.shape)} and "
                           f"{tuple(b.shape)}")
    if a.dim() == 3 and shape is not None and tuple(shape) != tuple(a.shape[1:]):
        raise _lib.TeError(f"map_similarity: shape={tuple(shape)} does not match the maps {tuple(a.shape)}")
    B, n = a.shape[0], a[0].numel()
    hw = tuple(a.shape[1:]) if a.dim() == 3 else None if shape is None else tuple(int(s) for s in shape)
    if hw is not None:
        if len(hw) != 2 or hw[0] * hw[1] != n:
            raise _lib.TeError(f"map_similarity: shape={hw} does not match maps of {n} values")
        if min(hw) < 7:
            raise _lib.TeError(f"map_similarity: SSIM needs maps of at least 7x7 (the window), got {hw[0]}x{hw[1]}")
    if not (a.is_cuda and b.is_cuda):
        raise _lib.TeError("map_similarity needs tensors on the MI355X (got a CPU tensor); there is no CPU fallback here -- "
                           "sanity.map_similarity is the torch restatement")
    return (B, n, 0, 0, False) if hw is None else (B, n, hw[0], hw[1], True)


def map_similarity_packed(a: Tensor, b: Tensor, shape=None, data_range: float = 1.0):
    """``map_similarity`` and the flat int64 buffer its results are views of -- rank_sums [B*6], then the bits of sim [B*4]:
    one device-to-host copy of it brings both over."""
    B, n, H, W, ssim = _map_pair(a, b, shape)
    a, b = _c(a).reshape(B, n), _c(b).reshape(B, n)
    flat = torch.empty((B * 10,), dtype=torch.int64, device=a.device)
    rank_sums = flat[:6 * B].view(B, 2, 3)
    sim = flat[6 * B:].view(torch.float64).view(B, 4)
    with _on_device(a) as lib:
        ws = _ws(lib.te_map_similarity_workspace_bytes(B, n), a)
        _lib.check(lib.te_map_similarity_f32(_ptr(a), _ptr(b), _ptr(rank_sums), _ptr(sim), B, n, H, W,
                                             _lib.TE_MAPSIM_SSIM if ssim else 0, float(data_range), _ptr(ws), ws.numel(),
                                             _stream(a)), "te_map_similarity_f32")
    return rank_sums, sim, flat


def map_similarity(a: Tensor, b: Tensor, shape=None, data_range: float = 1.0):
    """How similar two relevance maps are, per sample, two launches, no synchronisation: a, b fp32 [B,n] or [B,H,W] (3-D maps or
    ``shape=(H, W)`` turn SSIM on) -> (rank_sums int64 [B,2,3] = (cov, va, vb) of the rank deviations d = 2 rank - (n + 1)
    of the values and of the absolute values; sim float64 [B,4] = pearson, spearman, spearman_abs, ssim), as
    sanity.rank_sums / pearson / ssim define them (include/te_relprop.h, "map similarity").  A NaN anywhere in a sample
    gives a NaN row and zero sums; n <= 2^20."""
    return map_similarity_packed(a, b, shape, data_range)[:2]


# ---------------------------------------------------------------------------------------- localisation test (localisation.py)
def _localisation_args(heat, labels, target_id, image_index, boxes):
    """The checks of localisation_metrics that need no device -> (P, B, H, W, M): raises TeError before any HIP call."""
    given = {"heat": heat, "labels": labels, "target_id": target_id, "image_index": image_index, "boxes": boxes}
    for name, t in given.items():
        if t is not None and not torch.is_tensor(t):
            raise _lib.TeError(f"localisation_metrics: {name} must be a tensor, got {type(t).__name__}")
    if heat is None or heat.dtype != torch.float32:
        raise _lib.TeError(f"localisation_metrics takes a float32 heat map, got {None if heat is None else heat.dtype}")
    if (labels is None) == (boxes is None):
        raise _lib.TeError("localisation_metrics: give exactly one of labels= (a label map per image) and boxes=")
    for name in ("labels", "target_id", "image_index", "boxes"):
        if given[name] is not None and not _is_integer(given[name]):
            raise _lib.TeError(f"localisation_metrics takes an integer {name}, got {given[name].dtype}")
    if heat.dim() != 3 or heat.numel() == 0:
        raise _lib.TeError(f"localisation_metrics: heat must be [P,H,W] and not empty, got {tuple(heat.shape)}")
    P, H, W = heat.shape
    B, M = P, 0
    if labels is not None:
        if target_id is None:
            raise _lib.TeError("localisation_metrics: labels= needs target_id= [P], the class of every pair")
        if labels.dim() != 3 or tuple(labels.shape[1:]) != (H, W) or labels.shape[0] == 0:
            raise _lib.TeError(f"localisation_metrics: labels must be [B,{H},{W}] like the heat maps, got {tuple(labels.shape)}")
        B = labels.shape[0]
        if image_index is None and B != P:
            raise _lib.TeError(f"localisation_metrics: {B} label maps for {P} pairs need image_index= [P]")
    else:
        if boxes.dim() != 3 or boxes.shape[0] != P or boxes.shape[1] == 0 or boxes.shape[2] != 4:
            raise _lib.TeError(f"localisation_metrics: boxes must be [{P},M,4] = x0, y0, x1, y1 with M >= 1, got "
                               f"{tuple(boxes.shape)}")
        M = boxes.shape[1]
    for name in ("target_id", "image_index"):
        if given[name] is not None and tuple(given[name].shape) != (P,):
            raise _lib.TeError(f"localisation_metrics: {name} must be [{P}], one entry per pair, got {tuple(given[name].shape)}")
    if not all(t.is_cuda for t in given.values() if t is not None):
        raise _lib.TeError("localisation_metrics needs tensors on the MI355X (got a CPU tensor); there is no CPU fallback "
                           "here -- localisation.reference_metrics is the torch restatement")
    return P, B, H, W, M


def localisation_metrics_packed(heat: Tensor, labels: Optional[Tensor] = None, target_id: Optional[Tensor] = None,
                                image_index: Optional[Tensor] = None, boxes: Optional[Tensor] = None):
    """``localisation_metrics`` and the flat int64 buffer its results are views of -- stats [P*5], then the bits of energy
    [P*2]: one device-to-host copy of it brings both over."""
    P, B, H, W, M = _localisation_args(heat, labels, target_id, image_index, boxes)
    heat = _c(heat)
    labels, target_id, image_index, boxes = (None if t is None else t.to(device=heat.device, dtype=torch.int64).contiguous()
                                             for t in (labels, target_id, image_index, boxes))
    flat = torch.empty((P * 7,), dtype=torch.int64, device=heat.device)
    stats = flat[:5 * P].view(P, 5)
    energy = flat[5 * P:].view(torch.float64).view(P, 2)
    with _on_device(heat) as lib:
        ws = _ws(lib.te_localisation_workspace_bytes(P, H, W), heat)
        _lib.check(lib.te_localisation_f32(_ptr(heat), _ptr(labels), _ptr(image_index), _ptr(target_id), _ptr(boxes), M,
                                           _ptr(stats), _ptr(energy), P, B, H, W, _ptr(ws), ws.numel(), _stream(heat)),
                   "te_localisation_f32")
    return stats, energy, flat


def localisation_metrics(heat: Tensor, labels: Optional[Tensor] = None, target_id: Optional[Tensor] = None,
                         image_index: Optional[Tensor] = None, boxes: Optional[Tensor] = None):
    """The localisation test per (image, class) pair, one launch, no synchronisation: heat fp32 [P,H,W] against either
    ``labels`` [B,H,W] of an integer dtype (< 0 = ignore; a pixel is a target iff label == ``target_id[p]``; pair p reads the
    label map ``image_index[p]``, p itself when image_index is None) or ``boxes`` [P,M,4] = x0, y0, x1, y1 (half-open; an empty
    row pads) -> (stats int64 [P,5] = n_valid, n_target, argmax, d2_min, topk_hits; energy float64 [P,2] = e_target, e_valid),
    as localisation.reference_metrics defines them (include/te_relprop.h, "localisation test").  A pair with target_id < 0
    or an image_index outside [0, B) is skipped: rows {0, 0, -1, -1, 0} and {0, 0}.  H*W <= 2^20, P <= 65535, M <= 64."""
    return localisation_metrics_packed(heat, labels, target_id, image_index, boxes)[:2]


# ---------------------------------------------------------------------------------------- 8f rationale test (BERT)
class _on_device_of_ids(_on_device):
    """``_on_device`` for a call whose tensors are all integers (te_token_erase): no dtype rule to apply."""

    def __init__(self, t: Tensor):
        global _checked_device
        if not _checked_device:
            _lib.require_device()
            _checked_device = True
        self.ctx = torch.cuda.device(t.device)


def rationale_metrics(scores: Tensor, word_ids: Tensor, truth: Tensor, ks: Sequence[int], clamp: bool = True):
    """The rationale test of bert_pipeline.py:547-582 + metrics.py:168-253 per document, one launch, no synchronisation:
    scores [B,N] fp32 relevance per wordpiece, word_ids [B,N] of an integer dtype (the word of a wordpiece, -1 = none),
    truth [B,Wmax] bool / uint8 (the human rationale per word), ks: at most 16 positive rationale sizes ->
    (word_scores fp32 [B,Wmax], n_words int32 [B], order int32 [B,Wmax], counts int32 [B,len(ks),2] = (tp_k, pred_k),
    soft fp64 [B,4] = AP, AUPRC, ROC-AUC, npos), as rationale.word_scores / topk_counts / soft_scores define them:
    ties in ascending word index, pred_k = min(k, n_words), NaN scores count as 0."""
    import ctypes
    if scores.dtype != torch.float32:
        raise _lib.TeError(f"rationale_metrics takes float32 scores, got {scores.dtype}")
    if not _is_integer(word_ids):
        raise _lib.TeError(f"rationale_metrics takes integer word ids, got {word_ids.dtype}")
    if truth.dtype not in (torch.bool, torch.uint8):
        raise _lib.TeError(f"rationale_metrics takes a bool or uint8 truth mask, got {truth.dtype}")
    if not (scores.is_cuda and word_ids.is_cuda and truth.is_cuda):
        raise _lib.TeError("rationale_metrics needs tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
    if scores.dim() != 2 or word_ids.shape != scores.shape or truth.dim() != 2 or truth.shape[0] != scores.shape[0]:
        raise _lib.TeError(f"rationale_metrics: scores and word_ids must be [B,N] alike and truth [B,Wmax], got "
                           f"{tuple(scores.shape)}, {tuple(word_ids.shape)}, {tuple(truth.shape)}")
    ks = [int(k) for k in ks]
    scores = _c(scores)
    word_ids = word_ids.to(torch.int32).contiguous()
    truth = truth.contiguous().view(torch.uint8)
    (B, N), Wmax, K = scores.shape, truth.shape[1], len(ks)
    dev = scores.device
    word_scores = torch.empty((B, Wmax), dtype=torch.float32, device=dev)
    n_words = torch.empty((B,), dtype=torch.int32, device=dev)
    order = torch.empty((B, Wmax), dtype=torch.int32, device=dev)
    counts = torch.empty((B, K, 2), dtype=torch.int32, device=dev)
    soft = torch.empty((B, 4), dtype=torch.float64, device=dev)
    k_arr = (ctypes.c_int64 * max(K, 1))(*ks)
    with _on_device(scores) as lib:
        ws = _ws(lib.te_rationale_metrics_workspace_bytes(B, N, Wmax), scores)
        _lib.check(lib.te_rationale_metrics_f32(_ptr(scores), _ptr(word_ids), _ptr(truth), _ptr(word_scores),
                                                _ptr(n_words), _ptr(order), _ptr(counts), _ptr(soft), B, N, Wmax, k_arr,
                                                K, TE_RATIONALE_CLAMP if clamp else 0, _ptr(ws), ws.numel(),
                                                _stream(scores)), "te_rationale_metrics_f32")
    return word_scores, n_words, order, counts, soft


def token_erase(input_ids: Tensor, attention_mask: Tensor, word_ids: Tensor, order: Tensor, n_words: Tensor,
                fractions: Sequence[float], pad_id: int = 0):
    """Every erased copy ERASER's faithfulness numbers need, in one launch: input_ids / attention_mask [B,N] of an integer
    dtype, word_ids [B,N], order [B,Wmax] and n_words [B] as ``rationale_metrics`` takes / gives them, fractions: at most 8
    values in (0, 1] -> (ids_out int64 [2,T,B,N], mask_out int64 [2,T,B,N], n_rationale int32 [T,B]).  For fraction t the
    first min(n_words, max(1, ceil(t n_words))) words of ``order`` form the rationale; copy [0] (comprehensiveness) drops
    their wordpieces, copy [1] (sufficiency) keeps only those; tokens with word id -1 and mask 1 stay in both; the kept
    tokens move to the left in their order, the rest is ``pad_id`` with mask 0 (rationale.token_erase_torch)."""
    import ctypes
    tensors = (input_ids, attention_mask, word_ids, order, n_words)
    for name, t in zip(("input_ids", "attention_mask", "word_ids", "order", "n_words"), tensors):
        if not (_is_integer(t) or (name == "attention_mask" and t.dtype == torch.bool)):
            raise _lib.TeError(f"token_erase takes integer tensors, got {t.dtype} for {name}")
    if not all(t.is_cuda for t in tensors):
        raise _lib.TeError("token_erase needs tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
    if (input_ids.dim() != 2 or attention_mask.shape != input_ids.shape or word_ids.shape != input_ids.shape
            or order.dim() != 2 or order.shape[0] != input_ids.shape[0] or tuple(n_words.shape) != (input_ids.shape[0],)):
        raise _lib.TeError(f"token_erase: input_ids, attention_mask and word_ids must be [B,N] alike, order [B,Wmax] and "
                           f"n_words [B], got {[tuple(t.shape) for t in tensors]}")
    fr = [float(t) for t in fractions]
    input_ids = input_ids.to(torch.int64).contiguous()
    attention_mask = attention_mask.to(torch.int64).contiguous()
    word_ids, order, n_words = (t.to(torch.int32).contiguous() for t in (word_ids, order, n_words))
    (B, N), Wmax, T = input_ids.shape, order.shape[1], len(fr)
    ids_out = torch.empty((2, T, B, N), dtype=torch.int64, device=input_ids.device)
    mask_out = torch.empty_like(ids_out)
    n_rationale = torch.empty((T, B), dtype=torch.int32, device=input_ids.device)
    f_arr = (ctypes.c_double * max(T, 1))(*fr)
    with _on_device_of_ids(input_ids) as lib:
        _lib.check(lib.te_token_erase(_ptr(input_ids), _ptr(attention_mask), _ptr(word_ids), _ptr(order), _ptr(n_words),
                                      _ptr(ids_out), _ptr(mask_out), _ptr(n_rationale), B, N, Wmax, f_arr, T, int(pad_id),
                                      _stream(input_ids)), "te_token_erase")
    return ids_out, mask_out, n_rationale


# ---------------------------------------------------------------------------------------- 8f.4 perturbation inputs
def perturb(vis: Tensor, data: Tensor, ks: Sequence[int], mean: Optional[Sequence[float]] = None,
            std: Optional[Sequence[float]] = None, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """pertubation_eval_from_hdf5.py:88-101 for all steps at once: vis [B, H*W] (or [B,1,H,W]) relevance, data
    [B,C,H,W] -> [len(ks), B, C, H, W]: the ks[s] most relevant pixels of every sample zeroed in every channel, then
    (x - mean[c]) / std[c].  out_dtype=torch.bfloat16 (the input of a bf16 classifier): the same fp32 values rounded once
    to bf16, to nearest even -- ``perturb(...).to(torch.bfloat16)`` bit for bit, without the fp32 tensor."""
    import ctypes
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise _lib.TeError(f"perturb: out_dtype must be float32 or bfloat16, got {out_dtype}")
    data = _c(data)
    B, C, H, W = data.shape
    HW = H * W
    vis = _c(vis).reshape(B, -1)
    if vis.shape[1] != HW:
        raise _lib.TeError(f"perturb: vis {tuple(vis.shape)} does not cover the {H}x{W} pixels of data")
    S = len(ks)
    out = torch.empty((S, B, C, H, W), dtype=out_dtype, device=data.device)
    k_arr = (ctypes.c_int64 * S)(*[int(k) for k in ks])
    m_arr = None if mean is None else (ctypes.c_float * C)(*[float(v) for v in mean])
    s_arr = None if std is None else (ctypes.c_float * C)(*[float(v) for v in std])
    name = "te_perturb_f32" if out_dtype == torch.float32 else "te_perturb_bf16"
    with _on_device(data) as lib:
        ws = _ws(lib.te_perturb_workspace_bytes(B, S), data)
        _lib.check(getattr(lib, name)(_ptr(vis), _ptr(data), _ptr(out), B, C, HW, k_arr, S, m_arr, s_arr, _ptr(ws),
                                      ws.numel(), _stream(data)), name)
    return out


# ---------------------------------------------------------------------------------------- deletion / insertion curves (curves.py)
_RESTATED_IN = {"curves": "curves.py has the torch restatement",
                "robustness": "robustness.py has the numpy / torch restatement"}


def _eval_tensor(module: str, what: str, name: str, t, dtypes) -> Tensor:
    """A check that needs no device: raises TeError before any HIP call.  module: where the protocol is restated."""
    if not torch.is_tensor(t):
        raise _lib.TeError(f"{what}: {name} must be a tensor")
    if t.dtype not in dtypes:
        raise _lib.TeError(f"{what} takes {' or '.join(str(d) for d in dtypes)} for {name}, got {t.dtype}")
    if not t.is_cuda:
        raise _lib.TeError(f"{what} needs tensors on the MI355X (got a CPU tensor for {name}); there is no CPU fallback here -- "
                           f"{_RESTATED_IN[module]}")
    return t


def _floats(values, C: int, what: str, name: str):
    import ctypes
    if values is None:
        return None
    values = [float(v) for v in values]
    if len(values) != C:
        raise _lib.TeError(f"{what}: {name} has {len(values)} values for {C} channels")
    return (ctypes.c_float * C)(*values)


def gaussian_blur(data: Tensor, klen: int = 11, nsig: float = 5.0, mean: Optional[Sequence[float]] = None,
                  std: Optional[Sequence[float]] = None) -> Tensor:
    """RISE's blurred image in normalised space: data [B,C,H,W] fp32 -> blur((data - mean[c]) / std[c]) [B,C,H,W] fp32 with the
    separable klen x klen kernel of ``curves.gaussian_taps(klen, nsig)`` and zero padding (include/te_relprop.h, "deletion /
    insertion curves"; ``curves.reference_blur`` is the restatement)."""
    import ctypes
    from .curves import gaussian_taps
    data = _eval_tensor("curves", "gaussian_blur", "data", data, (torch.float32,))
    if data.dim() != 4 or data.numel() == 0:
        raise _lib.TeError(f"gaussian_blur: data must be [B,C,H,W] and not empty, got {tuple(data.shape)}")
    klen = int(klen)
    if klen < 1 or klen % 2 == 0 or klen > _lib.TE_BLUR_MAX_TAPS:
        raise _lib.TeError(f"gaussian_blur: klen must be odd and at most {_lib.TE_BLUR_MAX_TAPS}, got {klen}")
    B, C, H, W = data.shape
    data = _dense(data)
    taps = gaussian_taps(klen, nsig)
    t_arr = (ctypes.c_float * klen)(*[float(v) for v in taps])
    m_arr, s_arr = _floats(mean, C, "gaussian_blur", "mean"), _floats(std, C, "gaussian_blur", "std")
    out = torch.empty((B, C, H, W), dtype=torch.float32, device=data.device)
    with _on_device(data) as lib:
        _lib.check(lib.te_blur_normalised_f32(_ptr(data), _ptr(out), B, C, H, W, t_arr, klen, m_arr, s_arr, _stream(data)),
                   "te_blur_normalised_f32")
    return out


def pixel_ranks(vis: Tensor) -> Tensor:
    """vis [B,n] (or [B,1,H,W]) fp32 relevance -> rank int32 [B,n]: the position of every pixel when its row is sorted by
    descending value, equal values in ascending pixel index (rank 0 = the most relevant pixel; ``curves.reference_ranks``).
    One launch, n <= 2^20."""
    vis = _eval_tensor("curves", "pixel_ranks", "vis", vis, (torch.float32,))
    if vis.dim() < 2 or vis.numel() == 0:
        raise _lib.TeError(f"pixel_ranks: vis must be [B,n] and not empty, got {tuple(vis.shape)}")
    B = vis.shape[0]
    vis = vis.reshape(B, -1)
    vis = _dense(vis)
    n = vis.shape[1]
    rank = torch.empty((B, n), dtype=torch.int32, device=vis.device)
    with _on_device(vis) as lib:
        ws = _ws(lib.te_pixel_rank_workspace_bytes(B, n), vis)
        _lib.check(lib.te_pixel_rank_f32(_ptr(vis), _ptr(rank), B, n, _ptr(ws), ws.numel(), _stream(vis)), "te_pixel_rank_f32")
    return rank


def curve_inputs(data: Tensor, ranks: Tensor, step: int, s0: int, n_s: int, mode: str, substrate: Optional[Tensor] = None,
                 fill: Optional[Sequence[float]] = None, mean: Optional[Sequence[float]] = None,
                 std: Optional[Sequence[float]] = None, out_dtype: torch.dtype = torch.float32) -> Tensor:
    """The images s0 .. s0 + n_s - 1 of a deletion or insertion curve, one launch: data [B,C,H,W] fp32, ranks int32 [B,HW]
    (``pixel_ranks``) -> [n_s,B,C,H,W].  Image i has the min(i step, HW) top-ranked pixels switched: mode "deletion" from
    z = (data - mean[c]) / std[c] to the substrate, "insertion" from the substrate to z.  The substrate is a [B,C,H,W] fp32
    tensor in normalised space, or (substrate=None) the per-channel constants ``fill``, already normalised.
    out_dtype=torch.bfloat16: the fp32 values rounded once, to nearest even (``curves.reference_inputs``)."""
    what = "curve_inputs"
    if mode not in ("deletion", "insertion"):
        raise _lib.TeError(f"{what}: mode must be 'deletion' or 'insertion', got {mode!r}")
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise _lib.TeError(f"{what}: out_dtype must be float32 or bfloat16, got {out_dtype}")
    data = _eval_tensor("curves", what, "data", data, (torch.float32,))
    ranks = _eval_tensor("curves", what, "ranks", ranks, (torch.int32,))
    if data.dim() != 4 or data.numel() == 0:
        raise _lib.TeError(f"{what}: data must be [B,C,H,W] and not empty, got {tuple(data.shape)}")
    B, C, H, W = data.shape
    HW = H * W
    if tuple(ranks.shape) != (B, HW):
        raise _lib.TeError(f"{what}: ranks {tuple(ranks.shape)} does not cover the {H}x{W} pixels of data {tuple(data.shape)}")
    if (substrate is None) == (fill is None):
        raise _lib.TeError(f"{what}: give a substrate tensor or the fill constants, one of the two")
    if substrate is not None:
        substrate = _eval_tensor("curves", what, "substrate", substrate, (torch.float32,))
        if substrate.shape != data.shape:
            raise _lib.TeError(f"{what}: substrate {tuple(substrate.shape)} is not shaped like data {tuple(data.shape)}")
        substrate = _dense(substrate)
    step, s0, n_s = int(step), int(s0), int(n_s)
    S = -(-HW // step) if step >= 1 else 0
    if step < 1 or s0 < 0 or n_s < 1 or s0 + n_s > S + 1:
        raise _lib.TeError(f"{what}: step {step}, s0 {s0}, n_s {n_s} do not name images of the {S + 1} of {HW} pixels")
    data = _dense(data)
    ranks = _dense(ranks)
    f_arr, m_arr, s_arr = _floats(fill, C, what, "fill"), _floats(mean, C, what, "mean"), _floats(std, C, what, "std")
    out = torch.empty((n_s, B, C, H, W), dtype=out_dtype, device=data.device)
    name = "te_curve_inputs_f32" if out_dtype == torch.float32 else "te_curve_inputs_bf16"
    with _on_device(data) as lib:
        _lib.check(getattr(lib, name)(_ptr(data), _ptr(substrate), f_arr, _ptr(ranks), _ptr(out), B, C, HW, step, s0, n_s,
                                      1 if mode == "insertion" else 0, m_arr, s_arr, _stream(data)), name)
    return out


def curve_scores(logits: Tensor, target: Tensor, prob: Tensor, s0: int) -> Tensor:
    """logits [n_s B, K] (or [n_s,B,K]) fp32 or bf16 of the images s0 .. s0 + n_s - 1, target int64 [B], prob float64 [S+1,B]:
    writes prob[s0 + i, b] = softmax(logits[i, b])[target[b]], evaluated in fp64, in place (one launch) and returns prob
    (``curves.reference_scores``)."""
    what = "curve_scores"
    logits = _eval_tensor("curves", what, "logits", logits, (torch.float32, torch.bfloat16))
    target = _eval_tensor("curves", what, "target", target, (torch.int64,))
    prob = _eval_tensor("curves", what, "prob", prob, (torch.float64,))
    if prob.dim() != 2 or not prob.is_contiguous() or target.dim() != 1 or target.shape[0] != prob.shape[1]:
        raise _lib.TeError(f"{what}: prob must be a contiguous [S+1,B] table and target [B], got {tuple(prob.shape)} and "
                           f"{tuple(target.shape)}")
    B = prob.shape[1]
    if logits.dim() not in (2, 3) or logits.numel() == 0 or logits[..., 0].numel() % B != 0:
        raise _lib.TeError(f"{what}: logits must be [n_s*B,K] or [n_s,B,K] with B = {B}, got {tuple(logits.shape)}")
    K = logits.shape[-1]
    n_s = logits[..., 0].numel() // B
    s0 = int(s0)
    if s0 < 0 or s0 + n_s > prob.shape[0]:
        raise _lib.TeError(f"{what}: rows {s0} .. {s0 + n_s - 1} are outside the {prob.shape[0]} rows of prob")
    logits = _dense(logits)
    target = _dense(target)
    name = "te_curve_scores_f32" if logits.dtype == torch.float32 else "te_curve_scores_bf16"
    with _on_device(logits) as lib:
        _lib.check(getattr(lib, name)(_ptr(logits), _ptr(target), _ptr(prob), B, K, s0, n_s, _stream(logits)), name)
    return prob


def curve_auc(prob: Tensor) -> Tensor:
    """prob float64 [S+1,B] -> auc float64 [B]: the trapezoid over x = i / S (``curves.reference_auc``), one launch."""
    prob = _eval_tensor("curves", "curve_auc", "prob", prob, (torch.float64,))
    if prob.dim() != 2 or prob.shape[0] < 2 or prob.shape[1] == 0:
        raise _lib.TeError(f"curve_auc: prob must be [S+1,B] with S >= 1, got {tuple(prob.shape)}")
    prob = _dense(prob)
    S1, B = prob.shape
    auc = torch.empty((B,), dtype=torch.float64, device=prob.device)
    with _on_device_of_ids(prob) as lib:
        _lib.check(lib.te_curve_auc_f64(_ptr(prob), _ptr(auc), S1, B, _stream(prob)), "te_curve_auc_f64")
    return auc


# ---------------------------------------------------------------------------------------- robustness and complexity (robustness.py)
def _finite_not_negative(what: str, name: str, value) -> float:
    value = float(value)
    if not (value >= 0.0) or value == float("inf"):
        raise _lib.TeError(f"{what}: {name} must be finite and not negative, got {value}")
    return value


def _philox_args(what: str, seed, id0, d0, n_draws: int):
    """(seed, id0, d0) of the draws d0 .. d0 + n_draws - 1 as the ABI carries them: checked, and the 64 bits of seed and id0,
    which the device reads as unsigned, wrapped into an int64_t."""
    d0, seed, id0 = int(d0), int(seed), int(id0)
    if d0 < 0 or d0 + n_draws > 1 << 32:
        raise _lib.TeError(f"{what}: draws {d0} .. {d0 + n_draws - 1} are not draws 0 .. 2^32 - 1")
    if not (-(1 << 63) <= seed < 1 << 64) or not (-(1 << 63) <= id0 < 1 << 64):
        raise _lib.TeError(f"{what}: seed and id0 are 64-bit integers, got {seed} and {id0}")
    seed, id0 = (v - (1 << 64) if v >= 1 << 63 else v for v in (seed, id0))
    return seed, id0, d0


def noise_inputs(x: Tensor, n_draws: int, radius: float, seed: int, id0: int = 0, d0: int = 0,
                 out_dtype: torch.dtype = torch.float32) -> Tensor:
    """The noisy copies of the sensitivity protocol, one launch: x [B,...] fp32 (the model's normalised input) ->
    [B,n_draws,...] in ``out_dtype`` (float32, or bfloat16: the fp32 value rounded once more, to nearest even).  Copy j of
    sample b is draw d0 + j of the sample with the global id id0 + b: x + s * radius in fp32 with s uniform in [-1, 1) from
    Philox4x32-10 keyed by ``seed`` (include/te_relprop.h, "robustness and complexity"; ``robustness.reference_noise``).
    The bits of a sample's copies do not depend on the batch or on the chunk (d0, n_draws) they are made in."""
    what = "noise_inputs"
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise _lib.TeError(f"{what}: out_dtype must be float32 or bfloat16, got {out_dtype}")
    x = _eval_tensor("robustness", what, "x", x, (torch.float32,))
    if x.dim() < 2 or x.numel() == 0:
        raise _lib.TeError(f"{what}: x must be [B,...] and not empty, got {tuple(x.shape)}")
    n_draws = int(n_draws)
    if n_draws < 1:
        raise _lib.TeError(f"{what}: n_draws must be at least 1, got {n_draws}")
    x = _dense(x)
    out = torch.empty((x.shape[0], n_draws) + tuple(x.shape[1:]), dtype=out_dtype, device=x.device)
    return _noise_inputs_into(x, out, radius, seed, id0, d0)


def _noise_inputs_into(x: Tensor, out: Tensor, radius: float, seed: int, id0: int = 0, d0: int = 0) -> Tensor:
    """The launch of ``noise_inputs``, into out [B,n_draws,...] fp32 or bf16, dense.  Not part of the interface: the tests
    call it to hand the kernel an output view that starts off a 16-byte boundary."""
    what = "noise_inputs"
    x = _eval_tensor("robustness", what, "x", x, (torch.float32,))
    out = _eval_tensor("robustness", what, "out", out, (torch.float32, torch.bfloat16))
    if x.dim() < 2 or out.dim() != x.dim() + 1 or out.shape[0] != x.shape[0] or out.shape[2:] != x.shape[1:] or \
            out.numel() == 0 or not x.is_contiguous() or not out.is_contiguous():
        raise _lib.TeError(f"{what}: x must be a dense [B,...] and out a dense [B,n_draws,...], got {tuple(x.shape)} and "
                           f"{tuple(out.shape)}")
    radius = _finite_not_negative(what, "radius", radius)
    B, n_draws = out.shape[0], out.shape[1]
    seed, id0, d0 = _philox_args(what, seed, id0, d0, n_draws)
    name = "te_noise_inputs_f32" if out.dtype == torch.float32 else "te_noise_inputs_bf16"
    with _on_device(x) as lib:
        _lib.check(getattr(lib, name)(_ptr(x), _ptr(out), B, x[0].numel(), d0, n_draws, radius, seed, id0, _stream(x)), name)
    return out


def map_distance(a: Tensor, b: Tensor) -> Tensor:
    """a fp32 [B,...] and b fp32 or bf16 [B,D,...] with as many values per sample -> sums float64 [B,D,3] = sum (b - a)^2,
    sum a^2, sum b^2, every term in fp64 from the exact upcasts, in an order fixed by the size alone; one launch, no
    synchronisation (``robustness.reference_distance``).  Serves the map pairs and the input pairs of the sensitivity
    protocol."""
    what = "map_distance"
    a = _eval_tensor("robustness", what, "a", a, (torch.float32,))
    b = _eval_tensor("robustness", what, "b", b, (torch.float32, torch.bfloat16))
    if a.dim() < 2 or b.dim() < 3 or a.numel() == 0 or b.numel() == 0 or a.shape[0] != b.shape[0] or \
            a[0].numel() != b[0, 0].numel():
        raise _lib.TeError(f"{what}: a must be [B,n] and b [B,D,n] and not empty, got {tuple(a.shape)} and {tuple(b.shape)}")
    B, D, n = b.shape[0], b.shape[1], a[0].numel()
    a = _dense(a)
    b = _dense(b)
    out = torch.empty((B, D, 3), dtype=torch.float64, device=a.device)
    name = "te_map_distance_f32" if b.dtype == torch.float32 else "te_map_distance_bf16"
    with _on_device(a) as lib:
        _lib.check(getattr(lib, name)(_ptr(a), _ptr(b), _ptr(out), B, D, n, _stream(a)), name)
    return out


def map_complexity(maps: Tensor, eps: float = 1e-5):
    """maps fp32 [B,...] -> (out float64 [B,2] = Gini sparseness, entropy of v = |maps[b]|; counts int64 [B,2] = the number of
    v > eps max v, the number of v > 0), one launch, no synchronisation (include/te_relprop.h, "robustness and complexity";
    ``robustness.reference_complexity``).  A zero map or a NaN anywhere in a sample gives a NaN row and zero counts;
    n <= 2^20."""
    what = "map_complexity"
    maps = _eval_tensor("robustness", what, "maps", maps, (torch.float32,))
    if maps.dim() < 2 or maps.numel() == 0:
        raise _lib.TeError(f"{what}: maps must be [B,n] and not empty, got {tuple(maps.shape)}")
    eps = _finite_not_negative(what, "eps", eps)
    B = maps.shape[0]
    maps = maps.reshape(B, -1)
    maps = _dense(maps)
    n = maps.shape[1]
    if n > 1 << 20 or B > 65535:
        raise _lib.TeError(f"{what}: at most 2^20 values per map and 65535 maps, got {tuple(maps.shape)}")
    out = torch.empty((B, 2), dtype=torch.float64, device=maps.device)
    counts = torch.empty((B, 2), dtype=torch.int64, device=maps.device)
    with _on_device(maps) as lib:
        ws = _ws(lib.te_map_complexity_workspace_bytes(B, n), maps)
        _lib.check(lib.te_map_complexity_f32(_ptr(maps), _ptr(out), _ptr(counts), B, n, eps, _ptr(ws), ws.numel(),
                                             _stream(maps)), "te_map_complexity_f32")
    return out, counts


# ---------------------------------------------------------------------------------------- faithfulness (faithfulness.py)
def _grid_of(what: str, x: Tensor, grid):
    """(C, g_h, g_w, p) of x [B,C,H,W] cut into grid = g or (g_h, g_w) cells of p x p pixels."""
    if x.dim() != 4 or x.numel() == 0:
        raise _lib.TeError(f"{what}: x must be [B,C,H,W] and not empty, got {tuple(x.shape)}")
    g_h, g_w = (int(v) for v in grid) if isinstance(grid, (tuple, list)) else (int(grid), int(grid))
    _, C, H, W = x.shape
    if g_h < 1 or g_w < 1 or H % g_h or W % g_w or H // g_h != W // g_w:
        raise _lib.TeError(f"{what}: a grid of {g_h} x {g_w} does not cut x {tuple(x.shape)} into square cells")
    if g_h * g_w > _lib.TE_SUBSET_MAX_CELLS:
        raise _lib.TeError(f"{what}: at most {_lib.TE_SUBSET_MAX_CELLS} cells, got a grid of {g_h} x {g_w} for x "
                           f"{tuple(x.shape)}")
    return C, g_h, g_w, H // g_h


def subset_inputs(x: Tensor, k: int, grid, seed: int, id0: int = 0, d0: int = 0, n_draws: int = 1,
                  substrate: Optional[Tensor] = None, fill: Optional[Sequence[float]] = None, attr: Optional[Tensor] = None,
                  out_dtype: torch.dtype = torch.float32):
    """The perturbed images of the faithfulness correlation: x [B,C,H,W] fp32 (the model's normalised input), cut into
    grid = g or (g_h, g_w) square cells -> (out [B,n_draws,C,H,W] in ``out_dtype``, member uint8 [B,n_draws,G], attr_sum
    float64 [B,n_draws] or None).  Copy j of sample b is draw d0 + j of the sample with the global id id0 + b: the k cells
    with the smallest Philox keys take the substrate's value -- a [B,C,H,W] fp32 tensor in normalised space, or the
    per-channel constants ``fill`` -- and every other pixel x's, bit for bit (bfloat16: rounded once, to nearest even).
    attr [B,G] fp32, the token-level map, adds attr_sum = its sum over the chosen cells in fp64 (include/te_relprop.h,
    "faithfulness"; ``faithfulness.reference_subset_inputs``).  A sample's outputs do not depend on the batch or on the chunk
    (d0, n_draws) they are made in."""
    what = "subset_inputs"
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise _lib.TeError(f"{what}: out_dtype must be float32 or bfloat16, got {out_dtype}")
    x = _eval_tensor("robustness", what, "x", x, (torch.float32,))
    C, g_h, g_w, _ = _grid_of(what, x, grid)
    n_draws = int(n_draws)
    if n_draws < 1:
        raise _lib.TeError(f"{what}: n_draws must be at least 1, got {n_draws}")
    x = _dense(x)
    out = torch.empty((x.shape[0], n_draws) + tuple(x.shape[1:]), dtype=out_dtype, device=x.device)
    return _subset_inputs_into(x, out, k, (g_h, g_w), seed, id0, d0, substrate, fill, attr)


def _subset_inputs_into(x: Tensor, out: Tensor, k: int, grid, seed: int, id0: int = 0, d0: int = 0,
                        substrate: Optional[Tensor] = None, fill: Optional[Sequence[float]] = None,
                        attr: Optional[Tensor] = None):
    """The launches of ``subset_inputs``, into out [B,n_draws,C,H,W] fp32 or bf16, dense.  Not part of the interface: the
    tests call it to hand the kernel an output view that starts off a 16-byte boundary."""
    what = "subset_inputs"
    x = _eval_tensor("robustness", what, "x", x, (torch.float32,))
    out = _eval_tensor("robustness", what, "out", out, (torch.float32, torch.bfloat16))
    C, g_h, g_w, p = _grid_of(what, x, grid)
    if out.dim() != 5 or out.shape[0] != x.shape[0] or out.shape[2:] != x.shape[1:] or out.numel() == 0 or \
            not x.is_contiguous() or not out.is_contiguous():
        raise _lib.TeError(f"{what}: x must be a dense [B,C,H,W] and out a dense [B,n_draws,C,H,W], got {tuple(x.shape)} and "
                           f"{tuple(out.shape)}")
    B, n_draws, G = out.shape[0], out.shape[1], g_h * g_w
    k = int(k)
    if k < 1 or k > G:
        raise _lib.TeError(f"{what}: k must name 1 .. {G} of the {g_h} x {g_w} cells of x {tuple(x.shape)}, got {k}")
    if B > 65535:
        raise _lib.TeError(f"{what}: at most 65535 samples, got x {tuple(x.shape)}")
    seed, id0, d0 = _philox_args(what, seed, id0, d0, n_draws)
    if (substrate is None) == (fill is None):
        raise _lib.TeError(f"{what}: give a substrate tensor or the fill constants, one of the two")
    if substrate is not None:
        substrate = _eval_tensor("robustness", what, "substrate", substrate, (torch.float32,))
        if substrate.shape != x.shape:
            raise _lib.TeError(f"{what}: substrate {tuple(substrate.shape)} is not shaped like x {tuple(x.shape)}")
        substrate = _dense(substrate)
    elif C > _lib.TE_PERTURB_MAX_CHANNELS:
        raise _lib.TeError(f"{what}: fill constants serve at most {_lib.TE_PERTURB_MAX_CHANNELS} channels, x is "
                           f"{tuple(x.shape)}; give a substrate tensor")
    f_arr = _floats(fill, C, what, "fill")
    attr_sum = None
    if attr is not None:
        attr = _eval_tensor("robustness", what, "attr", attr, (torch.float32,))
        if attr.numel() != B * G or attr.shape[0] != B:
            raise _lib.TeError(f"{what}: attr {tuple(attr.shape)} is not a [B,G] map of the {g_h} x {g_w} cells of x "
                               f"{tuple(x.shape)}")
        attr = attr.reshape(B, G)
        attr = _dense(attr)
        attr_sum = torch.empty((B, n_draws), dtype=torch.float64, device=x.device)
    member = torch.empty((B, n_draws, G), dtype=torch.uint8, device=x.device)
    name = "te_subset_inputs_f32" if out.dtype == torch.float32 else "te_subset_inputs_bf16"
    with _on_device(x) as lib:
        _lib.check(getattr(lib, name)(_ptr(x), _ptr(substrate), f_arr, _ptr(attr), _ptr(out), _ptr(member), _ptr(attr_sum),
                                      B, C, g_h, g_w, p, k, d0, n_draws, seed, id0, _stream(x)), name)
    return out, member, attr_sum


def perturbation_dot(x: Tensor, y: Tensor, w: Tensor) -> Tensor:
    """x fp32 [B,...] of n values per sample, y fp32 or bf16 [B,D,...] with as many, w fp32 [B,...] of m values with n % m == 0
    (the pixel-level attribution, shared by the n / m channels) -> sums float64 [B,D,2] = sum_e (x_e - y_e) w_(e mod m),
    sum_e (x_e - y_e)^2, every term in fp64 from the exact upcasts, in the order of ``map_distance``; one launch, no
    synchronisation (``faithfulness.reference_dot``)."""
    what = "perturbation_dot"
    x = _eval_tensor("robustness", what, "x", x, (torch.float32,))
    y = _eval_tensor("robustness", what, "y", y, (torch.float32, torch.bfloat16))
    w = _eval_tensor("robustness", what, "w", w, (torch.float32,))
    if x.dim() < 2 or y.dim() < 3 or w.dim() < 2 or x.numel() == 0 or y.numel() == 0 or w.numel() == 0 or \
            x.shape[0] != y.shape[0] or w.shape[0] != x.shape[0] or x[0].numel() != y[0, 0].numel():
        raise _lib.TeError(f"{what}: x must be [B,n], y [B,D,n] and w [B,m] and not empty, got {tuple(x.shape)}, "
                           f"{tuple(y.shape)} and {tuple(w.shape)}")
    B, D, n, m = y.shape[0], y.shape[1], x[0].numel(), w[0].numel()
    if n % m != 0:
        raise _lib.TeError(f"{what}: the {m} weights of w {tuple(w.shape)} do not divide the {n} values of x {tuple(x.shape)}")
    x, y, w = (_dense(t) for t in (x, y, w))
    out = torch.empty((B, D, 2), dtype=torch.float64, device=x.device)
    name = "te_perturbation_dot_f32" if y.dtype == torch.float32 else "te_perturbation_dot_bf16"
    with _on_device(x) as lib:
        _lib.check(getattr(lib, name)(_ptr(x), _ptr(y), _ptr(w), _ptr(out), B, D, n, m, _stream(x)), name)
    return out


# ---------------------------------------------------------------------------------------- gradient baselines (gradients.py)
# What surrounds the forward / backward loop of Input x Gradient, SmoothGrad and Integrated Gradients (include/te_relprop.h,
# "gradient baselines"; csrc/te_gradients.hip).  The dtype of an entry is chosen from the tensor it writes or reads; on CPU
# tensors every binding runs the restatement of gradients.py.
GRAD_REDUCE = {"sum": _lib.TE_GRAD_SUM, "abs_sum": _lib.TE_GRAD_ABS_SUM, "max_abs": _lib.TE_GRAD_MAX_ABS}
_COPY_DTYPES = (torch.float32, torch.bfloat16)


def _grad_tensor(what: str, name: str, t, dtypes, like: Optional[Tensor] = None) -> Tensor:
    """A check that needs no device: a tensor of one of ``dtypes``, on the device of ``like`` (CPU or GPU alike)."""
    if not torch.is_tensor(t):
        raise _lib.TeError(f"{what}: {name} must be a tensor")
    if t.dtype not in dtypes:
        raise _lib.TeError(f"{what} takes {' or '.join(str(d) for d in dtypes)} for {name}, got {t.dtype}")
    if like is not None and t.device != like.device:
        raise _lib.TeError(f"{what}: {name} is on {t.device}, the other tensors on {like.device}")
    return t


def _copies_out(what: str, x: Tensor, n_copies: int, out_dtype, out: Optional[Tensor]) -> Tensor:
    """The dense [B,n_copies,...] output of a kernel that writes copies of x [B,...]: ``out`` itself (its dtype decides the
    entry), or a new tensor in ``out_dtype``."""
    if out is None:
        if out_dtype not in _COPY_DTYPES:
            raise _lib.TeError(f"{what}: out_dtype must be float32 or bfloat16, got {out_dtype}")
        if n_copies < 1:
            raise _lib.TeError(f"{what}: at least one copy per sample, got {n_copies}")
        return torch.empty((x.shape[0], n_copies) + tuple(x.shape[1:]), dtype=out_dtype, device=x.device)
    out = _grad_tensor(what, "out", out, _COPY_DTYPES, x)
    if out.dim() != x.dim() + 1 or out.shape[0] != x.shape[0] or out.shape[2:] != x.shape[1:] or out.numel() == 0 or \
            not out.is_contiguous():
        raise _lib.TeError(f"{what}: out must be a dense [B,copies,...] of x {tuple(x.shape)}, got {tuple(out.shape)}")
    return out


def path_inputs(x: Tensor, base: Tensor, alphas: Tensor, s0: int = 0, n_s: Optional[int] = None,
                out_dtype: torch.dtype = torch.float32, out: Optional[Tensor] = None) -> Tensor:
    """The copies of a straight path from ``base`` to ``x``, one launch: x and base [B,...] fp32, alphas [S] fp32 ->
    [B,n_s,...] in ``out_dtype`` (or into ``out``, a dense [B,n_s,...] fp32 or bf16 tensor).  Copy j of sample b is
    base + alphas[s0 + j] (x - base), formed in fp64 and rounded once to fp32 (bfloat16: once more, to nearest even)
    (include/te_relprop.h, "gradient baselines"; ``gradients.reference_path_inputs`` gives the same bits)."""
    what = "path_inputs"
    x = _grad_tensor(what, "x", x, (torch.float32,))
    base = _grad_tensor(what, "base", base, (torch.float32,), x)
    alphas = _grad_tensor(what, "alphas", alphas, (torch.float32,), x)
    if x.dim() < 2 or x.numel() == 0 or base.shape != x.shape or alphas.dim() != 1 or alphas.numel() == 0:
        raise _lib.TeError(f"{what}: x and base must be [B,...] alike and not empty and alphas [S], got {tuple(x.shape)}, "
                           f"{tuple(base.shape)} and {tuple(alphas.shape)}")
    S, s0 = alphas.numel(), int(s0)
    n_s = (out.shape[1] if torch.is_tensor(out) and out.dim() > 1 else S - s0) if n_s is None else int(n_s)
    if s0 < 0 or n_s < 1 or s0 + n_s > S:
        raise _lib.TeError(f"{what}: nodes {s0} .. {s0 + n_s - 1} are not nodes of the {S} alphas")
    out = _copies_out(what, x, n_s, out_dtype, out)
    if out.shape[1] != n_s:
        raise _lib.TeError(f"{what}: out {tuple(out.shape)} does not hold {n_s} copies per sample")
    if not x.is_cuda:
        from .gradients import reference_path_inputs
        return out.copy_(reference_path_inputs(x, base, alphas, s0, n_s, out.dtype))
    x, base, alphas = _dense(x), _dense(base), _dense(alphas)
    name = "te_path_inputs_f32" if out.dtype == torch.float32 else "te_path_inputs_bf16"
    with _on_device(x) as lib:
        _lib.check(getattr(lib, name)(_ptr(x), _ptr(base), _ptr(alphas), _ptr(out), x.shape[0], x[0].numel(), S, s0, n_s,
                                      _stream(x)), name)
    return out


def gauss_inputs(x: Tensor, n_draws: int, sigma: float, seed: int, id0: int = 0, d0: int = 0,
                 out_dtype: torch.dtype = torch.float32, out: Optional[Tensor] = None) -> Tensor:
    """SmoothGrad's noisy copies, one launch: x [B,...] fp32 -> [B,n_draws,...] in ``out_dtype`` (or into ``out``, a dense
    [B,n_draws,...] fp32 or bf16 tensor, whose second dimension then is n_draws).  Copy j of sample b is draw d0 + j of the
    sample with the global id id0 + b: x + sigma z in fp64, rounded once, z standard normal by Box-Muller from Philox4x32-10
    keyed by ``seed`` (include/te_relprop.h, "gradient baselines"; ``gradients.reference_gauss_inputs`` agrees within one
    step of the result's format).  The bits of a sample's copies do not depend on the batch or on the chunk (d0, n_draws)."""
    what = "gauss_inputs"
    x = _grad_tensor(what, "x", x, (torch.float32,))
    if x.dim() < 2 or x.numel() == 0:
        raise _lib.TeError(f"{what}: x must be [B,...] and not empty, got {tuple(x.shape)}")
    n_draws = int(n_draws)
    out = _copies_out(what, x, n_draws, out_dtype, out)
    if out.shape[1] != n_draws:
        raise _lib.TeError(f"{what}: out {tuple(out.shape)} does not hold {n_draws} copies per sample")
    sigma = _finite_not_negative(what, "sigma", sigma)
    seed, id0, d0 = _philox_args(what, seed, id0, d0, n_draws)
    if not x.is_cuda:
        from .gradients import reference_gauss_inputs
        return out.copy_(reference_gauss_inputs(x, n_draws, sigma, seed, id0, d0, out.dtype))
    x = _dense(x)
    name = "te_gauss_inputs_f32" if out.dtype == torch.float32 else "te_gauss_inputs_bf16"
    with _on_device(x) as lib:
        _lib.check(getattr(lib, name)(_ptr(x), _ptr(out), x.shape[0], x[0].numel(), d0, n_draws, sigma, seed, id0,
                                      _stream(x)), name)
    return out


def grad_accumulate(g: Tensor, w: Tensor, acc: Tensor, s0: int = 0, square: bool = False) -> Tensor:
    """acc[b] += sum_j w[s0 + j] t(g[b, j]) in place, j ascending, one fp64 multiply and one fp64 add per step: g [B,n_s,...]
    fp32 or bf16 (the input gradients of a pass of copies), w fp64 [S], acc fp64 [B,...] dense, zeroed by the caller;
    t = g, or g g with ``square``.  The bits do not depend on how S is cut into passes
    (``gradients.reference_accumulate`` gives the same bits).  Returns acc."""
    what = "grad_accumulate"
    g = _grad_tensor(what, "g", g, _COPY_DTYPES)
    w = _grad_tensor(what, "w", w, (torch.float64,), g)
    acc = _grad_tensor(what, "acc", acc, (torch.float64,), g)
    if g.dim() < 3 or g.numel() == 0 or acc.dim() < 2 or acc.shape[0] != g.shape[0] or acc[0].numel() != g[0, 0].numel() or \
            w.dim() != 1 or not acc.is_contiguous():
        raise _lib.TeError(f"{what}: g must be [B,n_s,...], acc a dense [B,...] with as many values per sample and w [S], got "
                           f"{tuple(g.shape)}, {tuple(acc.shape)} and {tuple(w.shape)}")
    B, n_s, s0 = g.shape[0], g.shape[1], int(s0)
    if s0 < 0 or s0 + n_s > w.numel():
        raise _lib.TeError(f"{what}: copies {s0} .. {s0 + n_s - 1} are not among the {w.numel()} weights")
    if not g.is_cuda:
        from .gradients import reference_accumulate
        return reference_accumulate(g, w, acc, s0, square)
    g, w = _dense(g), _dense(w)
    name = "te_grad_accumulate_f32" if g.dtype == torch.float32 else "te_grad_accumulate_bf16"
    with _on_device(g) as lib:
        _lib.check(getattr(lib, name)(_ptr(g), _ptr(w), _ptr(acc), B, acc[0].numel(), n_s, s0, 1 if square else 0,
                                      _stream(g)), name)
    return acc


def grad_finish(acc: Tensor, m: Optional[Tensor] = None, reduce: str = "sum", with_sums: bool = True):
    """acc fp64 [B,C,...] (``grad_accumulate``), m fp32 shaped like acc or None -> (map fp32 [B,...], sums fp64 [B] or None):
    per pixel v = the ``reduce`` ("sum", "abs_sum", "max_abs") over the channels, in order, of the fp64 terms m acc (acc
    itself without m); the map is v rounded once, sums its per-sample total in fp64 in a fixed order, one launch, no
    synchronisation (``gradients.reference_finish``)."""
    what = "grad_finish"
    if reduce not in GRAD_REDUCE:
        raise _lib.TeError(f"{what}: reduce must be one of {tuple(GRAD_REDUCE)}, got {reduce!r}")
    acc = _grad_tensor(what, "acc", acc, (torch.float64,))
    if acc.dim() < 3 or acc.numel() == 0:
        raise _lib.TeError(f"{what}: acc must be [B,C,...] and not empty, got {tuple(acc.shape)}")
    if m is not None:
        m = _grad_tensor(what, "m", m, (torch.float32,), acc)
        if m.shape != acc.shape:
            raise _lib.TeError(f"{what}: m {tuple(m.shape)} is not shaped like acc {tuple(acc.shape)}")
    if not acc.is_cuda:
        from .gradients import reference_finish
        out, sums = reference_finish(acc, m, reduce)
        return out, (sums if with_sums else None)
    acc = _dense(acc)
    m = None if m is None else _dense(m)
    B, C = acc.shape[0], acc.shape[1]
    out = torch.empty((B,) + tuple(acc.shape[2:]), dtype=torch.float32, device=acc.device)
    sums = torch.empty((B,), dtype=torch.float64, device=acc.device) if with_sums else None
    with _on_device(acc) as lib:
        _lib.check(lib.te_grad_finish_f64(_ptr(acc), _ptr(m), _ptr(out), _ptr(sums), B, C, acc[0, 0].numel(), GRAD_REDUCE[reduce],
                                          _stream(acc)), "te_grad_finish_f64")
    return out, sums


# ---------------------------------------------------------------------------------------- bf16 operands
# A bf16 model's rules: the reference's algorithm evaluated in fp32 on the model's own bf16 tensors (read exactly: bf16 ->
# fp32 is exact).  Relevance, safe_divide, per-sample sums and the rollout stay fp32; Linear's Z is X+ W+^T + X- W-^T from
# the bf16 X and W (never from the cached bf16 output), the attention rules take Z from the cached bf16 product.  The GEMM-
# shaped rules run on bf16 MFMAs (csrc/te_bf16.hip); shapes those kernels do not tile take the FP32-UPCAST route: exact fp32
# copies of the bf16 operands on the fp32 kernels, on the GPU (linear_bf16_route / attention_bf16_route say which).
def linear_bf16_route(T: int, in_f: int, out_f: int) -> str:
    """'bf16' (te_linear_relprop_bf16) or 'fp32-upcast' (te_linear_relprop_f32 on fp32 copies of X and W)."""
    return "bf16" if _lib.load().te_linear_relprop_bf16_supported(int(T), int(in_f), int(out_f)) else "fp32-upcast"


def attention_bf16_route(N: int, D: int) -> str:
    """'bf16' (te_matmul_relprop_av_bf16 / _qk_bf16: head dim 64) or 'fp32-upcast' (the fp32 attention kernels)."""
    return "bf16" if _lib.load().te_matmul_relprop_bf16_supported(int(N), int(D)) else "fp32-upcast"


def conv_bf16_route(C: int, E: int, p: int) -> str:
    """'bf16' (te_conv2d_zb_relprop_bf16: 3 channels, E and 3 p p multiples of 128) or 'fp32-upcast'
    (te_conv2d_zb_relprop_f32 on fp32 copies of X and W, with their fp32 convolution as Y)."""
    return "bf16" if _lib.load().te_conv2d_zb_relprop_bf16_supported(int(C), int(E), int(p)) else "fp32-upcast"


def bf16_weight_planes(W: Tensor, cache: Optional[dict] = None) -> Tensor:
    """W+, W- and their transposes for te_linear_relprop_bf16; cached like x6_weight_planes."""
    out_f, in_f = W.shape
    return _cached_planes(W, cache, "bf16_planes", lambda Wd: (_prepare_planes(
        _c16(Wd), "te_linear_bf16_weight_planes_bytes", "te_linear_bf16_prepare_weights", (in_f, out_f)),))[0]


def _rows(X: Tensor, K: int) -> Tuple[Tensor, int]:
    """[..., K] bf16 activation -> ([T, K] view, row stride), copying only if its rows are not uniformly strided."""
    X2 = _prep_bf16(X).reshape(-1, K)
    if X2.stride(1) != 1 or (X2.shape[0] > 1 and X2.stride(0) < K):
        X2 = X2.contiguous()
    return X2, (X2.stride(0) if X2.shape[0] > 1 else K)


def linear_relprop_bf16(R, X: Tensor, W: Tensor, alpha: float = 1.0, variant="ours",
                        cache: Optional[dict] = None) -> Tensor:
    """Linear.relprop of a bf16 layer: R [..., out] fp32 (or ``Deferred``), X [..., in] and W [out, in] bf16 -> fp32
    [..., in].  X may be a strided view (Block.relprop_cls_only's cls rows are read in place)."""
    _bf16_rule(variant, alpha, "Linear.relprop")
    if not (_is_bf16(X) and _is_bf16(W)):
        raise _lib.TeError(f"Linear.relprop: X ({X.dtype}) and W ({W.dtype}) must both be bf16 on the bf16 path")
    out_f, in_f = W.shape
    lead = X.shape[:-1]
    R, r_scale = _split_deferred(R)
    Rc = _c(R).reshape(-1, out_f)
    T = Rc.shape[0]
    if X.numel() // in_f != T:
        raise _lib.TeError(f"Linear.relprop: R has {T} rows, X has {X.numel() // in_f}")
    if linear_bf16_route(T, in_f, out_f) != "bf16":
        Rd = R if r_scale is None else Deferred(R, r_scale)
        return linear_relprop(Rd, X.float(), W.detach().float(), alpha=alpha, variant=variant)
    X2, x_ld = _rows(X, in_f)
    planes = bf16_weight_planes(W, cache)
    out = torch.empty((T, in_f), dtype=torch.float32, device=X.device)
    rs_ptr, rs_stride, rps = None, 0, 1
    if r_scale is not None:
        rs_ptr, rs_stride, rps = r_scale.data_ptr(), r_scale.stride(0), T // r_scale.shape[0]
    gemm = 2.0 * T * in_f * out_f
    with _on_device(X2) as lib, _timed("linear_bf16", 8.0 * gemm,
                                       2.0 * T * in_f + 8.0 * in_f * out_f + 4.0 * T * out_f + 6.0 * 2 * T * out_f
                                       + 2.0 * T * in_f + 4.0 * T * in_f):
        ws = _ws(lib.te_linear_relprop_bf16_workspace_bytes(T, in_f, out_f), X2)
        _lib.check(lib.te_linear_relprop_bf16(_ptr(Rc), out_f, rs_ptr, rs_stride, rps, _ptr(X2), x_ld, _ptr(planes),
                                              _ptr(out), T, in_f, out_f, _ptr(ws), ws.numel(), _stream(X2)),
                   "te_linear_relprop_bf16")
    return out.reshape(*lead, in_f)


def _bhnd16(t: Tensor) -> Tuple[Tensor, int, int, int]:
    t = _prep_bf16(t)
    if t.stride(-1) != 1 or min(t.stride()[:3]) < 0:
        t = t.contiguous()
    sb, sh, sn, _ = t.stride()
    return t, sb, sh, sn


def matmul_relprop_av_bf16(R: Tensor, attn: Tensor, v: Tensor, out_scale: float = 1.0,
                           cam_v_out: Optional[Tensor] = None, variant="ours", z: Optional[Tensor] = None):
    """AV rule with bf16 attn / v (and bf16 cached product z); R and the results fp32 (matmul_relprop_av)."""
    _bf16_rule(variant, 1.0, "the attention AV rule")
    B, H, N, D = v.shape
    if attention_bf16_route(N, D) != "bf16":
        return matmul_relprop_av(R, attn.float(), v.float(), out_scale, cam_v_out, variant,
                                 None if z is None else z.detach().float())
    zc, z_str = None, (0, 0, 0)
    if z is not None and USE_FORWARD_PRODUCTS and tuple(z.shape) == (B, H, N, D):
        zc, zsb, zsh, zsn = _bhnd16(z.detach())
        z_str = (zsb, zsh, zsn)
    R, r_sb, r_sh, r_sn = _bhnd(R)
    v, v_sb, v_sh, v_sn = _bhnd16(v)
    attn = _c16(attn)
    cam_attn = torch.empty((B, H, N, N), dtype=torch.float32, device=attn.device)
    cam_v = cam_v_out if cam_v_out is not None else torch.empty((B, H, N, D), dtype=torch.float32, device=attn.device)
    if cam_v.stride(-1) != 1 or cam_v.dtype != torch.float32:
        raise _lib.TeError("cam_v_out must be fp32 with a contiguous last dim")
    cv_sb, cv_sh, cv_sn, _ = cam_v.stride()
    with _on_device(attn) as lib, _timed("attention_av_rule_bf16", 12.0 * B * H * N * N * D,
                                         B * H * (6.0 * N * N + 16.0 * N * D)):
        ws = _ws(lib.te_matmul_relprop_av_bf16_workspace_bytes(B, H, N, D), attn)
        _lib.check(lib.te_matmul_relprop_av_bf16(_ptr(R), r_sb, r_sh, r_sn, _ptr(attn), _ptr(v), v_sb, v_sh, v_sn,
                                                 _ptr(zc), *z_str, _ptr(cam_attn), _ptr(cam_v), cv_sb, cv_sh, cv_sn,
                                                 B, H, N, D, float(out_scale), _variant(variant), _ptr(ws), ws.numel(),
                                                 _stream(attn)), "te_matmul_relprop_av_bf16")
    return cam_attn, cam_v


def matmul_relprop_qk_bf16(R, q: Tensor, k: Tensor, out_scale: float = 1.0, cam_q_out: Optional[Tensor] = None,
                           cam_k_out: Optional[Tensor] = None, variant="ours", z: Optional[Tensor] = None):
    """QK rule with bf16 q / k (and bf16 cached unscaled product z); R (fp32 or ``Deferred``) and the results fp32."""
    _bf16_rule(variant, 1.0, "the attention QK rule")
    B, H, N, D = q.shape
    if attention_bf16_route(N, D) != "bf16":
        return matmul_relprop_qk(R, q.float(), k.float(), out_scale, cam_q_out, cam_k_out, variant,
                                 None if z is None else z.detach().float())
    zc = None
    if z is not None and USE_FORWARD_PRODUCTS and tuple(z.shape) == (B, H, N, N):
        zc = _c16(z.detach())
    q, q_sb, q_sh, q_sn = _bhnd16(q)
    k, k_sb, k_sh, k_sn = _bhnd16(k)
    R, r_scale = _split_deferred(R)
    R = _c(R)
    dev = R.device
    cam_q = cam_q_out if cam_q_out is not None else torch.empty((B, H, N, D), dtype=torch.float32, device=dev)
    cam_k = cam_k_out if cam_k_out is not None else torch.empty((B, H, N, D), dtype=torch.float32, device=dev)
    if cam_q.stride(-1) != 1 or cam_k.stride(-1) != 1 or cam_q.dtype != torch.float32 or cam_k.dtype != torch.float32:
        raise _lib.TeError("cam_q_out / cam_k_out must be fp32 with a contiguous last dim")
    cq, ck = cam_q.stride(), cam_k.stride()
    with _on_device(q) as lib, _timed("attention_qk_rule_bf16", 12.0 * B * H * N * N * D,
                                      B * H * (12.0 * N * N + 12.0 * N * D)):
        ws = _ws(lib.te_matmul_relprop_qk_bf16_workspace_bytes(B, H, N, D), q)
        _lib.check(lib.te_matmul_relprop_qk_bf16(_ptr(R), _ptr(r_scale), 0 if r_scale is None else r_scale.stride(0),
                                                 _ptr(q), q_sb, q_sh, q_sn, _ptr(k), k_sb, k_sh, k_sn, _ptr(zc),
                                                 _ptr(cam_q), cq[0], cq[1], cq[2], _ptr(cam_k), ck[0], ck[1], ck[2],
                                                 B, H, N, D, float(out_scale), _variant(variant), _ptr(ws), ws.numel(),
                                                 _stream(q)), "te_matmul_relprop_qk_bf16")
    return cam_q, cam_k


def add_relprop_bf16(R: Tensor, X0: Tensor, X1: Tensor, variant="ours", deferred: bool = False):
    """Add.relprop with bf16 operands (same shape, X1 of batch 1, or the BERT broadcast mask [B,1,1,N] / [1,1,1,N]
    against X0 [B,H,N,N]); R and the results fp32, returned as add_relprop returns them."""
    _bf16_rule(variant, 1.0, "Add.relprop")
    X0, X1 = _c16(X0), _c16(X1)
    R = _c(R)
    B = X0.shape[0]
    n = X0[0].numel()
    if _is_bcast_mask(X0, X1):
        H, N = X0.shape[1], X0.shape[3]
        if X0.shape[2] != N or X1.shape[3] != N or X1.shape[0] not in (1, B) or R.numel() != X0.numel():
            raise _lib.TeError(f"Add.relprop (bf16): mask {tuple(X1.shape)} against scores {tuple(X0.shape)} with "
                               f"relevance {tuple(R.shape)}: expected [B|1,1,1,N], [B,H,N,N], [B,H,N,N]")
        mask = X1.reshape(X1.shape[0], N)
        if mask.shape[0] == 1 and B > 1:
            mask = mask.expand(B, N).contiguous()
        out0 = torch.empty(X0.shape, dtype=torch.float32, device=X0.device)
        out1 = torch.empty((B, 1, 1, N), dtype=torch.float32, device=X0.device)
        nb = B * (10.0 * H * N * N + 6.0 * N)
        if deferred:
            fac = torch.empty((B, 2), dtype=torch.float32, device=X0.device)
            with _on_device(X0) as lib, _timed("add_bcast_mask_deferred_bf16", 0.0, nb):
                ws = _ws(lib.te_add_bcast_relprop_workspace_bytes(B, H, N), X0)
                _lib.check(lib.te_add_bcast_relprop_deferred_bf16(_ptr(R), _ptr(X0), _ptr(mask), _ptr(out0), _ptr(out1),
                                                                  _ptr(fac), B, H, N, _ptr(ws), ws.numel(), _stream(X0)),
                           "te_add_bcast_relprop_deferred_bf16")
            return Deferred(out0, fac[:, 0]), out1
        with _on_device(X0) as lib, _timed("add_bcast_mask_bf16", 0.0, nb):
            ws = _ws(lib.te_add_bcast_relprop_workspace_bytes(B, H, N), X0)
            _lib.check(lib.te_add_bcast_relprop_bf16(_ptr(R), _ptr(X0), _ptr(mask), _ptr(out0), _ptr(out1), B, H, N,
                                                     _variant(variant), _ptr(ws), ws.numel(), _stream(X0)),
                       "te_add_bcast_relprop_bf16")
        return out0, out1
    if X1.shape == X0.shape:
        x1_bs = n
    elif X1.shape[0] == 1 and X1.shape[1:] == X0.shape[1:]:
        x1_bs = 0
    else:
        raise _lib.TeError(f"Add.relprop (bf16): unsupported operand shapes {tuple(X0.shape)} + {tuple(X1.shape)}")
    if R.numel() != X0.numel():
        raise _lib.TeError("Add.relprop: relevance / input size mismatch")
    out0 = torch.empty(X0.shape, dtype=torch.float32, device=X0.device)
    out1 = torch.empty(X0.shape, dtype=torch.float32, device=X0.device)
    x1_elems = n if x1_bs else n / B
    if deferred:
        fac = torch.empty((B, 2), dtype=torch.float32, device=X0.device)
        with _on_device(X0) as lib, _timed("add_deferred_bf16", 0.0, B * (14.0 * n + 2.0 * x1_elems)):
            ws = _ws(lib.te_add_relprop_deferred_workspace_bytes(B, n), X0)
            _lib.check(lib.te_add_relprop_deferred_bf16(_ptr(R), _ptr(X0), _ptr(X1), _ptr(out0), _ptr(out1), _ptr(fac),
                                                        B, n, x1_bs, _ptr(ws), ws.numel(), _stream(X0)),
                       "te_add_relprop_deferred_bf16")
        return Deferred(out0, fac[:, 0]), Deferred(out1, fac[:, 1])
    with _on_device(X0) as lib, _timed("add_bf16", 0.0, B * (14.0 * n + 2.0 * x1_elems)):
        ws = _ws(lib.te_add_relprop_workspace_bytes(B, n), X0)
        _lib.check(lib.te_add_relprop_bf16(_ptr(R), _ptr(X0), _ptr(X1), _ptr(out0), _ptr(out1), B, n, x1_bs,
                                           _variant(variant), _ptr(ws), ws.numel(), _stream(X0)), "te_add_relprop_bf16")
    return out0, out1


def conv_bf16_weight_planes(W: Tensor, cache: Optional[dict] = None) -> Tuple[Tensor, Tensor]:
    """(the contiguous 16-byte aligned W [E,C,p,p], its planes: W+^T, W-^T and the two channel sums) for
    te_conv2d_zb_relprop_bf16; cached like x6_weight_planes."""
    E, C, p, _ = W.shape

    def build(Wd):
        Wc = _c16(Wd)
        if Wc.data_ptr() % 16:
            Wc = Wc.clone()
        return Wc, _prepare_planes(Wc, "te_conv2d_zb_bf16_weight_planes_bytes", "te_conv2d_zb_bf16_prepare_weights", (C, E, p))
    return _cached_planes(W, cache, "conv_bf16_planes", build)


def conv2d_zb_relprop_bf16(R: Tensor, X: Tensor, W: Tensor, cache: Optional[dict] = None) -> Tensor:
    """The z^B rule of a bf16 patch embedding: R [B,E,Hp,Wp] fp32 (any strides; the token-major view of cam[:, 1:] is read
    in place), X [B,C,H,W] and W [E,C,p,p] bf16 -> fp32 [B,C,H,W].  conv(X, W) is recomputed from the bf16 operands -- on
    bf16 MFMAs (csrc/te_conv_bf16.hip), or, for a geometry that kernel does not tile (conv_bf16_route), as the fp32
    convolution of exact fp32 copies handed to the fp32 kernel; the layer's bf16 output is never the denominator."""
    for t in (X, W):                                     # mixed dtypes, bf16 relevance, then CPU tensors, are refused
        if not _is_bf16(t):
            raise _lib.TeError(f"{DTYPES_MSG}; this bf16 rule got a {t.dtype} operand")
    _prep(R), _prep_bf16(X), _prep_bf16(W)
    B, C, H, Wd = X.shape
    E, p = W.shape[0], W.shape[2]
    if W.shape[1] != C or W.shape[3] != p or H % p or Wd % p:
        raise _lib.TeError(f"conv2d_zb_relprop: not a patch convolution: X {tuple(X.shape)}, W {tuple(W.shape)}")
    Hp, Wp = H // p, Wd // p
    P = Hp * Wp
    if tuple(R.shape) != (B, E, Hp, Wp):
        raise _lib.TeError(f"conv2d_zb_relprop: R {tuple(R.shape)} does not match [B,E,H/p,W/p]")
    if conv_bf16_route(C, E, p) != "bf16":
        Xf, Wf = X.float(), W.detach().float()
        return conv2d_zb_relprop(R, Xf, Wf, torch.nn.functional.conv2d(Xf, Wf, stride=p))
    Rt = R.permute(0, 2, 3, 1)                       # [B,Hp,Wp,E]
    st = Rt.stride()
    if not (st[3] == 1 and st[2] == E and st[1] == Wp * E and st[0] >= P * E):
        Rt = Rt.contiguous()
        st = Rt.stride()
    X = _c16(X)
    if X.data_ptr() % 16:
        X = X.clone()
    Wc, planes = conv_bf16_weight_planes(W, cache)
    out = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    T, K = B * P, C * p * p
    # flops = the bf16 MFMA work executed (one product in the Z-pass, six in the C-pass); bytes = algorithmic traffic
    with _on_device(X) as lib, _timed("conv2d_zb_bf16", 14.0 * T * K * E,
                                      4.0 * T * K + 6.0 * K * E + 4.0 * T * E + 12.0 * T * E + 4.0 * T * K):
        ws = _ws(lib.te_conv2d_zb_relprop_bf16_workspace_bytes(B, C, H, Wd, E, p), X)
        _lib.check(lib.te_conv2d_zb_relprop_bf16(_ptr(Rt), st[0], _ptr(X), _ptr(Wc), _ptr(planes), _ptr(out), B, C, H, Wd,
                                                 E, p, _ptr(ws), ws.numel(), _stream(X)), "te_conv2d_zb_relprop_bf16")
    return out


# ---------------------------------------------------------------------------------------- fp64 models
# An fp64 model (model.double()) is explained in double throughout: the rules below (variant ours, alpha = 1) take fp64
# operands AND fp64 relevance, and return fp64 (csrc/te_f64.hip; include/te_relprop.h, "fp64 operands").  One GEMM loop on
# the fp64 MFMA serves every shape, so there is no route to choose and nothing to fall back to; Linear recomputes Z from X
# and W (the cached forward output is an fp32 economy), the attention rules take Z from the cached product or form it with
# torch.matmul in fp64.  A ``Deferred`` relevance is materialised first; deferred=True returns plain tensors.
def _plain(R):
    return R.materialise() if isinstance(R, Deferred) else R


def _rows64(X: Tensor, K: int) -> Tuple[Tensor, int]:
    """[..., K] fp64 tensor -> ([T, K] view, row stride), copying only if its rows are not uniformly strided."""
    X2 = X.reshape(-1, K)
    if X2.stride(1) != 1 or (X2.shape[0] > 1 and X2.stride(0) < K):
        X2 = X2.contiguous()
    return X2, (X2.stride(0) if X2.shape[0] > 1 else K)


def _bhnd64(t: Tensor) -> Tuple[Tensor, int, int, int]:
    if t.stride(-1) != 1 or min(t.stride()[:3]) < 0:
        t = t.contiguous()
    sb, sh, sn, _ = t.stride()
    return t, sb, sh, sn


def linear_relprop_f64(R, X: Tensor, W: Tensor, alpha: float = 1.0, variant="ours") -> Tensor:
    """Linear.relprop in double: R [..., out], X [..., in] (a strided view is read in place), W [out, in] -> fp64 [..., in]."""
    R = _plain(R)
    _f64_rule(variant, alpha, "Linear.relprop", R=R, X=X, W=W)
    out_f, in_f = W.shape
    lead = X.shape[:-1]
    R2, r_ld = _rows64(R, out_f)
    X2, x_ld = _rows64(X, in_f)
    W2, w_ld = _rows64(W, in_f)
    T = X2.shape[0]
    if R2.shape[0] != T:
        raise _lib.TeError(f"Linear.relprop: R has {R2.shape[0]} rows, X has {T}")
    out = torch.empty((T, in_f), dtype=torch.float64, device=X.device)
    gemm = 2.0 * T * in_f * out_f
    with _on_device(X2) as lib, _timed("linear_f64", 4.0 * gemm, 8.0 * (2 * T * in_f + 2 * in_f * out_f + 3 * T * out_f + T * in_f)):
        ws = _ws(lib.te_linear_relprop_f64_workspace_bytes(T, in_f, out_f), X2)
        _lib.check(lib.te_linear_relprop_f64(_ptr(R2), r_ld, _ptr(X2), x_ld, _ptr(W2), w_ld, _ptr(out), T, in_f, out_f,
                                             _ptr(ws), ws.numel(), _stream(X2)), "te_linear_relprop_f64")
    return out.reshape(*lead, in_f)


def _out64(t: Optional[Tensor], shape, device, what: str) -> Tensor:
    if t is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if t.dtype != torch.float64 or t.stride(-1) != 1 or tuple(t.shape) != tuple(shape):
        raise _lib.TeError(f"{what} must be torch.float64 {tuple(shape)} with a contiguous last dim (got {t.dtype} "
                           f"{tuple(t.shape)})")
    return t


def matmul_relprop_av_f64(R: Tensor, attn: Tensor, v: Tensor, out_scale: float = 1.0, cam_v_out: Optional[Tensor] = None,
                          variant="ours", z: Optional[Tensor] = None):
    """AV rule in double (matmul_relprop_av): every tensor fp64; z = attn @ v as cached, else formed here in fp64."""
    R = _plain(R)
    z = None if z is None or tuple(z.shape) != tuple(v.shape) else z.detach()
    _f64_rule(variant, 1.0, "the attention AV rule", R=R, attn=attn, v=v, z=z)
    B, H, N, D = v.shape
    if z is None:
        z = torch.matmul(attn, v)
    zc, z_sb, z_sh, z_sn = _bhnd64(z)
    R, r_sb, r_sh, r_sn = _bhnd64(R)
    v, v_sb, v_sh, v_sn = _bhnd64(v)
    attn = attn.contiguous()
    cam_attn = torch.empty((B, H, N, N), dtype=torch.float64, device=attn.device)
    cam_v = _out64(cam_v_out, (B, H, N, D), attn.device, "cam_v_out")
    cv_sb, cv_sh, cv_sn, _ = cam_v.stride()
    with _on_device(attn) as lib, _timed("attention_av_rule_f64", 4.0 * B * H * N * N * D, 8.0 * B * H * (2 * N * N + 6 * N * D)):
        ws = _ws(lib.te_matmul_relprop_av_f64_workspace_bytes(B, H, N, D), attn)
        _lib.check(lib.te_matmul_relprop_av_f64(_ptr(R), r_sb, r_sh, r_sn, _ptr(attn), _ptr(v), v_sb, v_sh, v_sn, _ptr(zc),
                                                z_sb, z_sh, z_sn, _ptr(cam_attn), _ptr(cam_v), cv_sb, cv_sh, cv_sn, B, H, N,
                                                D, float(out_scale), _ptr(ws), ws.numel(), _stream(attn)),
                   "te_matmul_relprop_av_f64")
    return cam_attn, cam_v


def matmul_relprop_qk_f64(R, q: Tensor, k: Tensor, out_scale: float = 1.0, cam_q_out: Optional[Tensor] = None,
                          cam_k_out: Optional[Tensor] = None, variant="ours", z: Optional[Tensor] = None):
    """QK rule in double (matmul_relprop_qk): every tensor fp64; z = the unscaled q @ k^T as cached, else formed here."""
    R = _plain(R)
    B, H, N, D = q.shape
    z = None if z is None or tuple(z.shape) != (B, H, N, N) else z.detach()
    _f64_rule(variant, 1.0, "the attention QK rule", R=R, q=q, k=k, z=z)
    if z is None:
        z = torch.matmul(q, k.transpose(-1, -2))
    z, R = z.contiguous(), R.contiguous()
    q, q_sb, q_sh, q_sn = _bhnd64(q)
    k, k_sb, k_sh, k_sn = _bhnd64(k)
    cam_q = _out64(cam_q_out, (B, H, N, D), q.device, "cam_q_out")
    cam_k = _out64(cam_k_out, (B, H, N, D), q.device, "cam_k_out")
    cq, ck = cam_q.stride(), cam_k.stride()
    with _on_device(q) as lib, _timed("attention_qk_rule_f64", 4.0 * B * H * N * N * D, 8.0 * B * H * (4 * N * N + 6 * N * D)):
        ws = _ws(lib.te_matmul_relprop_qk_f64_workspace_bytes(B, H, N, D), q)
        _lib.check(lib.te_matmul_relprop_qk_f64(_ptr(R), _ptr(q), q_sb, q_sh, q_sn, _ptr(k), k_sb, k_sh, k_sn, _ptr(z),
                                                _ptr(cam_q), cq[0], cq[1], cq[2], _ptr(cam_k), ck[0], ck[1], ck[2], B, H, N,
                                                D, float(out_scale), _ptr(ws), ws.numel(), _stream(q)),
                   "te_matmul_relprop_qk_f64")
    return cam_q, cam_k


def add_relprop_f64(R, X0: Tensor, X1: Tensor, variant="ours", deferred: bool = False):
    """Add.relprop (ours) in double: X1 of X0's shape, of batch 1, or the BERT mask [B|1,1,1,N] against X0 [B,H,N,N].
    Plain fp64 tensors whatever `deferred` says (there is no deferred fp64 kernel)."""
    R = _plain(R)
    _f64_rule(variant, 1.0, "Add.relprop", R=R, X0=X0, X1=X1)
    B = X0.shape[0]
    R, X0, X1 = R.contiguous(), X0.contiguous(), X1.contiguous()
    n = X0[0].numel()
    if R.numel() != X0.numel():
        raise _lib.TeError("Add.relprop: relevance / input size mismatch")
    out0 = torch.empty_like(X0)
    if _is_bcast_mask(X0, X1):
        H, N = X0.shape[1], X0.shape[3]
        if X0.shape[2] != N or X1.shape[3] != N or X1.shape[0] not in (1, B):
            raise _lib.TeError(f"Add.relprop (fp64): mask {tuple(X1.shape)} against scores {tuple(X0.shape)}: expected "
                               "[B|1,1,1,N] and [B,H,N,N]")
        out1 = torch.empty((B, 1, 1, N), dtype=torch.float64, device=X0.device)
        with _on_device(X0) as lib, _timed("add_bcast_mask_f64", 0.0, 8.0 * B * (5 * H * N * N + 3 * N)):
            ws = _ws(lib.te_add_bcast_relprop_f64_workspace_bytes(B, H, N), X0)
            _lib.check(lib.te_add_bcast_relprop_f64(_ptr(R), _ptr(X0), _ptr(X1), N if X1.shape[0] == B and B > 1 else 0,
                                                    _ptr(out0), _ptr(out1), B, H, N, _ptr(ws), ws.numel(), _stream(X0)),
                       "te_add_bcast_relprop_f64")
        return out0, out1
    if X1.shape == X0.shape:
        x1_bs = n
    elif X1.shape[0] == 1 and X1.shape[1:] == X0.shape[1:]:
        x1_bs = 0
    else:
        raise _lib.TeError(f"Add.relprop (fp64): unsupported operand shapes {tuple(X0.shape)} + {tuple(X1.shape)}")
    out1 = torch.empty_like(X0)
    with _on_device(X0) as lib, _timed("add_f64", 0.0, 8.0 * B * (7 * n + (n if x1_bs else n / B))):
        ws = _ws(lib.te_add_relprop_f64_workspace_bytes(B, n), X0)
        _lib.check(lib.te_add_relprop_f64(_ptr(R), _ptr(X0), _ptr(X1), _ptr(out0), _ptr(out1), B, n, x1_bs, _ptr(ws),
                                          ws.numel(), _stream(X0)), "te_add_relprop_f64")
    return out0, out1


def clone_relprop_f64(Rs: Sequence, X: Tensor) -> Tensor:
    """Clone.relprop in double: 2 or 3 fp64 relevance aliases (``Deferred`` ones are materialised) of the fp64 X."""
    Rs = [_plain(r) for r in Rs]
    _f64_rule("ours", 1.0, "Clone.relprop", X=X, **{f"R{i}": r for i, r in enumerate(Rs)})
    X = X.contiguous()
    Rs = [r.contiguous() for r in Rs]
    for r in Rs:
        if r.numel() != X.numel():
            raise _lib.TeError("Clone.relprop: relevance / input size mismatch")
    out = torch.empty_like(X)
    with _on_device(X) as lib, _timed("clone_f64", 0.0, 8.0 * X.numel() * (len(Rs) + 2)):
        _lib.check(lib.te_clone_relprop_f64(_ptr(Rs[0]), _ptr(Rs[1]), _ptr(Rs[2]) if len(Rs) == 3 else None, _ptr(X),
                                            _ptr(out), X.numel(), _stream(X)), "te_clone_relprop_f64")
    return out


def index_select_relprop_f64(R: Tensor, X: Tensor, index: int) -> Tensor:
    """IndexSelect.relprop (dim 1, one index) in double."""
    _f64_rule("ours", 1.0, "IndexSelect.relprop", R=R, X=X)
    X = X.contiguous()
    B, N, C = X.shape
    R = R.contiguous().reshape(B, C)
    out = torch.empty_like(X)
    with _on_device(X) as lib, _timed("index_select_f64", 0.0, 8.0 * (2 * X.numel() + B * C)):
        _lib.check(lib.te_index_select_relprop_f64(_ptr(R), _ptr(X), _ptr(out), B, N, C, int(index), _stream(X)),
                   "te_index_select_relprop_f64")
    return out


def gradcam_headmean_f64(grad: Tensor, cam: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """mean_h max(grad * cam, 0) in double: heads added in index order, one division."""
    _f64_rule("ours", 1.0, "the gradient x relevance head mean", grad=grad, cam=cam, out=out)
    grad, cam = grad.contiguous(), cam.contiguous()
    B, H, N, _ = cam.shape
    if out is None:
        out = torch.empty((B, N, N), dtype=torch.float64, device=cam.device)
    elif not out.is_contiguous() or tuple(out.shape) != (B, N, N):
        raise _lib.TeError(f"gradcam_headmean: out must be a contiguous float64 {(B, N, N)}")
    with _on_device(cam) as lib, _timed("headmean_f64", 0.0, 8.0 * (2 * B * H * N * N + B * N * N)):
        _lib.check(lib.te_gradcam_headmean_f64(_ptr(grad), _ptr(cam), _ptr(out), B, H, N, _stream(cam)),
                   "te_gradcam_headmean_f64")
    return out


def rollout_f64(cams: Tensor, start_layer: int = 0, normalise: bool = False, cls_fixup: bool = False,
                row0_only: bool = False) -> Tensor:
    """The rollout tail of an fp64 explanation: the reference's own torch expressions (ViT_LRP.py:38-49,
    ExplanationGenerator.py:7-18,58) on the fp64 [L,B,N,N] stack -- 58 us per step in fp32, not the hot path."""
    L, B, N, _ = cams.shape
    eye = torch.eye(N, dtype=cams.dtype, device=cams.device).expand(B, N, N)
    mats = [cams[i] + eye for i in range(L)]
    if normalise:
        mats = [m / m.sum(dim=-1, keepdim=True) for m in mats]
    joint = mats[start_layer]
    for i in range(start_layer + 1, L):
        joint = mats[i].bmm(joint)
    if cls_fixup:
        joint = joint.clone()
        joint[:, 0, 0] = joint[:, 0].min(dim=-1).values
    return joint[:, 0] if row0_only else joint


# ---------------------------------------------------------------------------------------- head_mask
def _head_mask_rows(m: Tensor, B: int, H: int) -> Tuple[Tensor, int]:
    """The mask operand of Mul.relprop, anything that broadcasts as [B or 1, H, 1, 1] -> (contiguous [B or 1, H], the
    batch stride the kernel takes: 0 = one mask for the whole batch)."""
    if m.numel() == H and (m.dim() < 2 or m.shape[-3:] == (H, 1, 1) or m.shape[-1] == H):
        return m.reshape(1, H).contiguous(), 0
    if m.numel() == B * H and m.shape[0] == B and (tuple(m.shape[1:]) in ((H,), (H, 1, 1))):
        return m.reshape(B, H).contiguous(), H
    raise _lib.TeError(f"Mul.relprop: a head mask must broadcast as [B or 1, H, 1, 1] = [{B} or 1, {H}, 1, 1], got "
                       f"{tuple(m.shape)}")


def mul_head_relprop(R: Tensor, P: Tensor, m: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """Mul.relprop for [attention_probs, head_mask] (BERT.py:375-377): R, P [B,H,rows,cols], m one value per head
    ([H], [1|B,H] or [1|B,H,1,1]) -> P . (sd(R, P . m) . m), the relevance of P; the mask's relevance is discarded.
    Dispatch on the operand dtype as the other rules: fp32 throughout, bf16 P and m with fp32 relevance, fp64 throughout.
    ``out``: a contiguous destination of R's shape and dtype; ``out is R`` is allowed.  Never synchronises."""
    if R.dim() != 4 or tuple(P.shape) != tuple(R.shape):
        raise _lib.TeError(f"Mul.relprop: relevance {tuple(R.shape)} and operand {tuple(P.shape)} must both be [B,H,rows,cols]")
    B, H, rows, cols = R.shape
    if _any_f64(R, P, m, out):
        _f64_rule("ours", 1.0, "Mul.relprop", R=R, P=P, m=m, out=out)
        R, P, sfx = R.contiguous(), P.contiguous(), "f64"
    else:
        bf = _is_bf16(P) or _is_bf16(m)
        want = (torch.float32, torch.bfloat16, torch.bfloat16) if bf else (torch.float32,) * 3
        if (R.dtype, P.dtype, m.dtype) != want:      # (the dtypes before the device: a mixed call is refused as such)
            raise _lib.TeError(f"{DTYPES_MSG}; Mul.relprop got relevance {R.dtype}, operand {P.dtype}, mask {m.dtype}")
        R, P, m, sfx = _c(R), (_c16(P) if bf else _c(P)), (_prep_bf16(m) if bf else _prep(m)), ("bf16" if bf else "f32")
    m2, m_sb = _head_mask_rows(m, B, H)
    if out is None:
        out = torch.empty_like(R)
    elif out.dtype != R.dtype or tuple(out.shape) != tuple(R.shape) or not out.is_contiguous() or out.device != R.device:
        raise _lib.TeError(f"Mul.relprop: out must be a contiguous {R.dtype} {tuple(R.shape)} on {R.device}")
    nb = float(R.numel()) * (2 * R.element_size() + P.element_size())
    with _on_device(P) as lib, _timed("mul_head_" + sfx, 0.0, nb):
        _lib.check(getattr(lib, "te_mul_head_relprop_" + sfx)(_ptr(R), _ptr(P), _ptr(m2), m_sb, _ptr(out), B, H, rows, cols,
                                                              _stream(P)), "te_mul_head_relprop_" + sfx)
    return out


def head_relevance(R_heads: Tensor) -> Tensor:
    """R_heads [B,H,N,D], any strided view with a contiguous last dim (fp32 or fp64 relevance) -> fp64 [B,H], the sum over
    (n, d) per head in a fixed order (te_head_relevance_*): the relevance that arrives at each head's slice of the context
    layer."""
    if R_heads.dim() != 4:
        raise _lib.TeError(f"head_relevance: expected a [B,H,N,D] view of the relevance, got {tuple(R_heads.shape)}")
    if _is_f64(R_heads):
        _f64_rule("ours", 1.0, "head_relevance", R=R_heads)
        sfx = "f64"
    else:
        _prep(R_heads)
        sfx = "f32"
    R, sb, sh, sn = _bhnd64(R_heads)
    B, H, N, D = R.shape
    out = torch.empty((B, H), dtype=torch.float64, device=R.device)
    with _on_device(R) as lib, _timed("head_relevance", 0.0, float(R.numel()) * R.element_size()):
        _lib.check(getattr(lib, "te_head_relevance_" + sfx)(_ptr(R), sb, sh, sn, _ptr(out), B, H, N, D, _stream(R)),
                   "te_head_relevance_" + sfx)
    return out


# ---------------------------------------------------------------------------------------- class targets
def relevance_dtype(dtype) -> torch.dtype:
    """The dtype of a model's relevance (seeds, scores, maps): fp32 for fp32 and bf16 models, fp64 for fp64 models."""
    return torch.float32 if dtype == torch.bfloat16 else dtype


def host_classes(classes, B: int, C: int, device) -> Tensor:
    """``classes`` ([B,K] or, for every sample alike, [K]; a tensor, an array or a list) as an int64 [B,K] tensor on
    ``device``.  Host data is checked here -- a class outside [0, C) is a ValueError, before anything is launched; a device
    tensor is not read back (te_class_targets_* marks such a class: -1, NaN score, all-zero seed)."""
    on_device = torch.is_tensor(classes) and classes.device.type != "cpu"
    idx = classes if torch.is_tensor(classes) else torch.as_tensor(classes)
    if idx.is_floating_point() or idx.dtype == torch.bool or idx.dim() not in (1, 2) or idx.numel() == 0:
        raise ValueError(f"classes must be integers of shape [B,K] or [K], got {idx.dtype} {tuple(idx.shape)}")
    if idx.dim() == 1:
        idx = idx.view(1, -1).expand(B, -1)
    if idx.shape[0] != B:
        raise ValueError(f"classes has {idx.shape[0]} rows, the batch has {B}")
    if not on_device and (int(idx.min()) < 0 or int(idx.max()) >= C):
        raise ValueError(f"classes must lie in [0, {C}), got values from {int(idx.min())} to {int(idx.max())}")
    return idx.to(device=device, dtype=torch.int64).contiguous()


def class_targets(logits: Tensor, classes: Optional[Tensor] = None, topk: Optional[int] = None, with_seeds: bool = True,
                  out: Optional[tuple] = None):
    """logits [B,C] (fp32 / bf16 / fp64, rows ``stride(0) >= C`` apart, read in place) -> (classes int64 [B,K], scores [B,K],
    seeds [K,B,C] or None) on te_class_targets_*: the ``topk`` largest logits per sample (descending; ties in ascending class
    index; NaN largest), or the given ``classes`` (a device int64 [B,K]; one outside [0, C) comes back as -1 / NaN / a zero
    row) with their logits and one-hot seeds in the relevance dtype.  ``out``: (classes, scores, seeds) to write into
    (contiguous, of those shapes and dtypes; seeds may be None).  One kernel; never synchronises; graph-capturable."""
    if logits.dim() != 2 or logits.numel() == 0 or logits.stride(1) != 1:
        raise _lib.TeError(f"class_targets: logits must be [B,C] with a contiguous last dimension, got {tuple(logits.shape)} "
                           f"strides {tuple(logits.stride())}")
    sfx = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float64: "f64"}.get(logits.dtype)
    if sfx is None:
        raise _lib.TeError(f"{DTYPES_MSG}; class_targets got {logits.dtype} logits")
    if (classes is None) == (topk is None):
        raise ValueError("class_targets: give exactly one of classes / topk")
    B, C = logits.shape
    ld = logits.stride(0) if B > 1 else C
    if topk is not None:
        K = int(topk)
        if not 1 <= K <= C:
            raise ValueError(f"topk must lie in [1, {C}] (the number of classes), got {topk}")
    else:
        if (not torch.is_tensor(classes) or classes.dtype != torch.int64 or classes.dim() != 2 or classes.shape[0] != B
                or classes.device != logits.device or not classes.is_contiguous() or classes.shape[1] == 0):
            raise _lib.TeError(f"class_targets: classes must be a contiguous int64 [{B},K] tensor on {logits.device} "
                               "(ops.host_classes makes one)")
        K = classes.shape[1]
    rel = relevance_dtype(logits.dtype)
    if out is None:
        cls_out = torch.empty((B, K), dtype=torch.int64, device=logits.device)
        scores = torch.empty((B, K), dtype=rel, device=logits.device)
        seeds = torch.empty((K, B, C), dtype=rel, device=logits.device) if with_seeds else None
    else:
        cls_out, scores, seeds = out
        for t, shape, dt, name in ((cls_out, (B, K), torch.int64, "classes"), (scores, (B, K), rel, "scores"),
                                   (seeds, (K, B, C), rel, "seeds")):
            if t is None and name == "seeds":
                continue
            if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous()
                    or t.device != logits.device):
                raise _lib.TeError(f"class_targets: out {name} must be a contiguous {dt} {shape} on {logits.device}")
    if not logits.is_cuda:
        raise _lib.TeError("relprop kernels need tensors on the MI355X (got a CPU tensor); there is no CPU fallback")
    with _on_device(logits) as lib, _timed("class_targets", 0.0, float(logits.numel()) * logits.element_size()
                                               + (0.0 if seeds is None else float(seeds.numel()) * seeds.element_size())):
        _lib.check(getattr(lib, "te_class_targets_" + sfx)(_ptr(logits.detach()), ld, B, C, K, _ptr(classes), _ptr(cls_out),
                                                           _ptr(scores), _ptr(seeds), _stream(logits)),
                   "te_class_targets_" + sfx)
    return cls_out, scores, seeds


# ---------------------------------------------------------------------------------------- AttnLRP
# The rule kernels of csrc/te_attnlrp.hip (te_relprop.h, section "AttnLRP": the specification of the method).  G and every
# result are fp32 device tensors; the cached operand of a rule (Y, x, gamma, x0) is fp32, or bf16 on a bf16 model (the
# te_attnlrp_*_bf16 entry: the _f32 entry's bits on an exact fp32 copy).  Every binding refuses anything else with DTYPES_MSG before a launch.
_ALRP_KINDS = {"gelu": _lib.TE_ALRP_ACT_GELU, "tanh": _lib.TE_ALRP_ACT_TANH}


def _alrp_operand(t: Tensor, rule: str, classes: bool = False) -> Tuple[Tensor, str]:
    """The cached operand of a rule, contiguous, and the name of the entry that reads it: te_alrp_<rule>_f32, or, a bf16
    operand, te_attnlrp_<rule>_bf16.  classes: the entry that takes G with a class axis, te_alrpk_<rule>_f32 / _bf16."""
    if classes:
        return (_c16(t), f"te_alrpk_{rule}_bf16") if _is_bf16(t) else (_c(t), f"te_alrpk_{rule}_f32")
    return (_c16(t), f"te_attnlrp_{rule}_bf16") if _is_bf16(t) else (_c(t), f"te_alrp_{rule}_f32")


def _alrp_classes(G: Tensor, operand: Tensor) -> bool:
    """G [K, *shape] against a cached operand of ``shape`` (te_relprop.h, "AttnLRP, a class axis"): one more dimension."""
    return G.dim() == operand.dim() + 1


def _alrp_out(out: Optional[Tensor], like: Tensor, what: str) -> Tensor:
    if out is None:
        return torch.empty(like.shape, dtype=torch.float32, device=like.device)
    if _prep(out).shape != like.shape or not out.is_contiguous():
        raise _lib.TeError(f"{what}: out must be a contiguous float32 tensor of shape {tuple(like.shape)}")
    return out


def alrp_damp(G: Tensor, Y: Tensor, eps: float = 1e-6, out: Optional[Tensor] = None) -> Tensor:
    """damp(G, Y) = G Y / stab(Y), stab(y) = y + eps sgn(y) with sgn(0) = +1; eps = 0: G itself.  ``out`` may be G.
    G [K, *Y.shape]: K classes on one read of Y (te_alrpk_damp_*), slice k the bits of this call on (G[k], Y)."""
    classes = _alrp_classes(G, Y)
    G, (Y, name) = _c(G), _alrp_operand(Y, "damp", classes)
    if (G.shape[1:] if classes else G.shape) != Y.shape:
        raise _lib.TeError(f"alrp_damp: G {tuple(G.shape)} and Y {tuple(Y.shape)} differ in shape")
    out = _alrp_out(out, G, "alrp_damp")
    size = (G.shape[0], Y.numel()) if classes else (G.numel(),)
    with _on_device(G) as lib, _timed("alrp_damp", 0.0, 8.0 * G.numel() + Y.element_size() * Y.numel()):
        _lib.check(getattr(lib, name)(_ptr(G), _ptr(Y), _ptr(out), *size, float(eps), _stream(G)), name)
    return out


def alrp_act(G: Tensor, x: Tensor, kind: str = "gelu", out: Optional[Tensor] = None) -> Tensor:
    """The identity rule through y = f(x), f = GELU (te_gelu) or tanh: G (f(x) / x), f'(0) at x == 0.  ``out`` may be G."""
    if kind not in _ALRP_KINDS:
        raise ValueError(f"alrp_act: kind must be one of {sorted(_ALRP_KINDS)}, got {kind!r}")
    classes = _alrp_classes(G, x)      # G [K, *x.shape]: te_alrpk_act_*, f(x) / x formed once for the K classes
    G, (x, name) = _c(G), _alrp_operand(x, "act", classes)
    if (G.shape[1:] if classes else G.shape) != x.shape:
        raise _lib.TeError(f"alrp_act: G {tuple(G.shape)} and x {tuple(x.shape)} differ in shape")
    out = _alrp_out(out, G, "alrp_act")
    size = (G.shape[0], x.numel()) if classes else (G.numel(),)
    with _on_device(G) as lib, _timed("alrp_act", 0.0, 8.0 * G.numel() + x.element_size() * x.numel()):
        _lib.check(getattr(lib, name)(_ptr(G), _ptr(x), _ptr(out), *size, _ALRP_KINDS[kind], _stream(G)), name)
    return out


def alrp_scale3(q: Tensor, k: Optional[Tensor] = None, v: Optional[Tensor] = None):
    """IN PLACE: the uniform rule's exact factors on the gradients of an attention block.  One argument: a fused [..., 3C]
    gradient whose thirds are multiplied by 1/4, 1/4, 1/2 (returned).  Three: the gradients of q, k, v, each [..., C]."""
    ts = (q,) if k is None and v is None else (q, k, v)
    if any(t is None for t in ts):
        raise ValueError("alrp_scale3: give the fused gradient alone, or all of q, k, v")
    for t in ts:
        if not _prep(t).is_contiguous() or t.shape != ts[0].shape or t.dim() < 1:
            raise _lib.TeError("alrp_scale3 works in place: contiguous float32 tensors of one shape")
    if len(ts) == 1:
        C3 = q.shape[-1]
        if C3 % 3:
            raise _lib.TeError(f"alrp_scale3: the last dimension of a fused gradient is 3C, got {C3}")
        C, ld, T = C3 // 3, C3, q.numel() // C3
        ptrs = [q.data_ptr() + 4 * i * C for i in range(3)]
    else:
        C = q.shape[-1]
        ld, T = C, q.numel() // C
        ptrs = [t.data_ptr() for t in ts]
    with _on_device(q) as lib, _timed("alrp_scale3", 0.0, 24.0 * T * C):
        _lib.check(lib.te_alrp_scale3_f32(*ptrs, ld, T, C, _stream(q)), "te_alrp_scale3_f32")
    return q if len(ts) == 1 else ts


def alrp_row_rstd(x: Tensor, eps: float) -> Tensor:
    """x [..., C] -> fp32 [...]: 1 / sqrt(biased variance of the row + eps), the constant of the LayerNorm rule."""
    x, name = _alrp_operand(x, "row_rstd")
    C = x.shape[-1]
    rstd = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    with _on_device(x) as lib, _timed("alrp_row_rstd", 0.0, float(x.element_size()) * x.numel()):
        _lib.check(getattr(lib, name)(_ptr(x), _ptr(rstd), x.numel() // C, C, float(eps), _stream(x)), name)
    return rstd


def alrp_layernorm(G: Tensor, gamma: Tensor, rstd: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """The LayerNorm rule with rstd held constant: G [..., C], gamma [C], rstd [...] -> rstd (gamma G - mean(gamma G)).
    G [K, ..., C] with rstd [...] of the operand's rows (one more dimension than rstd's + 1): K classes on one rstd
    (te_alrpk_layernorm_*), slice k the bits of this call on (G[k], gamma, rstd)."""
    classes = G.dim() == rstd.dim() + 2
    G, (gamma, name), rstd = _c(G), _alrp_operand(gamma.detach(), "layernorm", classes), _c(rstd)
    C = G.shape[-1]
    rows = G.numel() // C // (G.shape[0] if classes else 1)
    if tuple(gamma.shape) != (C,) or rstd.numel() != rows:
        raise _lib.TeError(f"alrp_layernorm: G {tuple(G.shape)} needs gamma [{C}] and one rstd per row, got "
                           f"{tuple(gamma.shape)} and {tuple(rstd.shape)}")
    out = _alrp_out(out, G, "alrp_layernorm")
    size = (G.shape[0], rows, C) if classes else (rows, C)
    with _on_device(G) as lib, _timed("alrp_layernorm", 0.0, 8.0 * G.numel()):
        _lib.check(getattr(lib, name)(_ptr(G), _ptr(gamma), _ptr(rstd), _ptr(out), *size, _stream(G)), name)
    return out


def alrp_token_relevance(x0: Tensor, G: Tensor, skip_first: bool = False) -> Tensor:
    """x0, G [B,N,C] -> fp32 [B, N - skip_first]: sum_c x0 G per token in fp64, rounded once; skip_first drops token 0.
    G [K,B,N,C]: K classes on one x0 (te_alrpk_token_relevance_*) -> fp32 [B, K, N - skip_first], batch-major; [:, k] has the
    bits of this call on (x0, G[k])."""
    classes = _alrp_classes(G, x0)
    (x0, name), G = _alrp_operand(x0, "token_relevance", classes), _c(G)
    if x0.dim() != 3 or x0.shape != (G.shape[1:] if classes else G.shape):
        raise _lib.TeError(f"alrp_token_relevance: x0 and G must both be [B,N,C] (G: or [K,B,N,C]), got {tuple(x0.shape)} and "
                           f"{tuple(G.shape)}")
    B, N, C = x0.shape
    skip = int(bool(skip_first))
    K = (G.shape[0],) if classes else ()
    out = torch.empty((B, *K, N - skip), dtype=torch.float32, device=x0.device)
    with _on_device(x0) as lib, _timed("alrp_token_relevance", 0.0, 4.0 * G.numel() + x0.element_size() * x0.numel()):
        _lib.check(getattr(lib, name)(_ptr(x0), _ptr(G), _ptr(out), *K, B, N, C, skip, _stream(x0)), name)
    return out


def alrp_patch_route(C: int, E: int, p: int) -> str:
    """'tiled' (the fp32-MFMA kernel of csrc/te_attnlrp_patch.hip: E a multiple of 32, p a multiple of 8) or 'simple' (one
    thread per pixel, any shape).  The same bits either way."""
    return "tiled" if _lib.load().te_patch_alrp_relevance_supported(int(C), int(E), int(p)) else "simple"


def alrp_patch_relevance(G: Tensor, x0: Tensor, X: Tensor, W: Tensor, eps: float = 1e-6, simple: bool = False) -> Tensor:
    """The eps-rule through a patch-embedding convolution, then input x G per pixel (te_relprop.h, "AttnLRP, pixel level"):
    G fp32 and x0 [B, P+1, E] (the chain's G at x0 and the cached patch embedding, class token in row 0, which is skipped),
    X [B,C,H,W] the image, W [E,C,p,p] the weight -> fp32 [B,H,W].  x0, X, W are all fp32 or all bf16 (read exactly: the
    fp32 call's bits on exact copies); ``simple`` forces the one-thread-per-pixel kernel (the same bits)."""
    dtypes = {"x0": x0.dtype, "X": X.dtype, "W": W.dtype}
    if len(set(dtypes.values())) != 1:
        raise _lib.TeError("alrp_patch_relevance: x0, X and W must share one dtype (all float32 or all bfloat16), got "
                           + ", ".join(f"{n}: {d}" for n, d in dtypes.items()))
    bf16 = _is_bf16(W)
    prep = _prep_bf16 if bf16 else _prep
    G, x0, X, W = _prep(G), prep(x0), _c16(X) if bf16 else _c(X), _c16(W.detach()) if bf16 else _c(W.detach())
    if X.dim() != 4 or W.dim() != 4 or W.shape[2] != W.shape[3] or W.shape[1] != X.shape[1]:
        raise _lib.TeError(f"alrp_patch_relevance: not a patch convolution: X {tuple(X.shape)}, W {tuple(W.shape)}")
    (B, C, H, Wd), (E, p) = X.shape, (W.shape[0], W.shape[2])
    if H % p or Wd % p:
        raise _lib.TeError(f"alrp_patch_relevance: the image {H} x {Wd} is not a whole number of {p} x {p} patches")
    P = (H // p) * (Wd // p)
    if tuple(G.shape) != (B, P + 1, E) or tuple(x0.shape) != (B, P + 1, E):
        raise _lib.TeError(f"alrp_patch_relevance: G {tuple(G.shape)} and x0 {tuple(x0.shape)} must both be [B, P+1, E] = "
                           f"{(B, P + 1, E)}")
    # token-major rows read in place behind the class token; any batch stride
    rows = lambda t: t if (t.stride(2) == 1 and t.stride(1) == E and t.stride(0) >= (P + 1) * E) else t.contiguous()  # noqa: E731
    G, x0 = rows(G), rows(x0)
    name = "te_patch_attnlrp_relevance_bf16" if bf16 else "te_patch_alrp_relevance_f32"
    out = torch.empty((B, H, Wd), dtype=torch.float32, device=X.device)
    T, K, es = B * P, C * p * p, X.element_size()
    with _on_device(X) as lib, _timed("alrp_patch_relevance", 2.0 * T * E * K + 2.0 * T * K,
                                      (4.0 + es) * T * E + es * (E * K + T * K) + 4.0 * T * p * p):
        _lib.check(getattr(lib, name)(G.data_ptr() + 4 * E, G.stride(0), x0.data_ptr() + es * E, x0.stride(0), _ptr(X), _ptr(W),
                                      _ptr(out), B, C, H, Wd, E, p, float(eps),
                                      TE_IMPL_SIMPLE if (simple or FORCE_SIMPLE) else 0, _stream(X)), name)
    return out


def alrp_linear_bf16_route(T: int, in_f: int, out_f: int) -> str:
    """'bf16' (te_attnlrp_linear_bf16: in_f and out_f multiples of 128) or 'fp32-upcast' (the fp32 chain's damp and product on
    exact fp32 copies of Y and W, on the GPU)."""
    return "bf16" if _lib.load().te_attnlrp_linear_bf16_supported(int(T), int(in_f), int(out_f)) else "fp32-upcast"


def alrp_attention_bf16_route(N: int, D: int) -> str:
    """'bf16' (te_attnlrp_attention_bf16: head dim 64, N <= 1024) or 'fp32-upcast' (rules.attention_attnlrp's fp32 route on exact
    fp32 copies of q, k, v and the probabilities, on the GPU)."""
    return "bf16" if _lib.load().te_attnlrp_attention_bf16_supported(int(N), int(D)) else "fp32-upcast"


# The weight side of te_attnlrp_linear_bf16: True: a contiguous bf16 W^T per layer, cached under the _weight_key scheme
# (2 B per weight element, read along k in 16-byte pieces); False: W read in place through the transposing staging of the
# GEMM loop (no extra memory).  The same bits either way; DESIGN.md section 3 "AttnLRP" has the measurement behind the default.
ALRP_WEIGHT_T = True


def alrp_weight_t(W: Tensor, cache: Optional[dict] = None) -> Tensor:
    """The contiguous transpose [in, out] of a bf16 Linear weight [out, in]; cached like x6_weight_planes."""
    return _cached_planes(W, cache, "alrp_weight_t", lambda Wd: (_c16(Wd).t().contiguous(),))[0]


def alrp_linear(G: Tensor, W: Tensor, cache: Optional[dict] = None, Y: Optional[Tensor] = None, eps: float = 0.0) -> Tensor:
    """The Linear rule's product G [..., out] . W [out, in] -> [..., in].
    fp32 W (``G`` is damp(G_y, y) already; Y is not given): te_gemm_x6_f32 on the cached planes of W^T wherever it takes the
    shape (gemm_x6_supported; X6_GEMM = "off" switches it off), the stock fp32 GEMM elsewhere -- the two routes of the
    package's own input-gradient product (producers._Linear.backward).
    bf16 W, with the layer's cached bf16 output Y and eps: damp(G, Y) W in one call -- te_attnlrp_linear_bf16 where
    alrp_linear_bf16_route says 'bf16', else the fp32 route above on exact fp32 copies of Y and W.  G [K, *Y.shape] (a class
    axis): K launches on the slices G[k] with the same Y, W and workspace, into the slices of one [K, ..., in] result.
    Whatever USE_FUSED_PRODUCERS says."""
    G = _prep(G)
    out_f, in_f = W.shape
    T = G.numel() // out_f
    if _is_bf16(W):
        classes = Y is not None and G.dim() == Y.dim() + 1
        slices = list(G) if classes else [G]
        if not _is_bf16(Y) or Y.shape != slices[0].shape:
            raise _lib.TeError("alrp_linear: a bf16 W needs the layer's cached bf16 output Y, of G's shape "
                               f"(got {None if Y is None else (Y.dtype, tuple(Y.shape))} for G {tuple(G.shape)})")
        T = slices[0].numel() // out_f
        if alrp_linear_bf16_route(T, in_f, out_f) != "bf16":
            if classes:      # per slice, like the kernel route: a stock product's order may depend on the number of rows
                return torch.stack([alrp_linear(g, W, cache, Y=Y, eps=eps) for g in slices])
            return alrp_linear(alrp_damp(G, Y.float(), eps), W.detach().float())
        W2 = alrp_weight_t(W, cache) if ALRP_WEIGHT_T else _c16(W.detach())
        Y2, y_ld = _rows(Y, out_f)
        out = torch.empty((len(slices), T, in_f), dtype=torch.float32, device=G.device)
        with _on_device(G) as lib:
            ws = _ws(lib.te_attnlrp_linear_bf16_workspace_bytes(T, in_f, out_f), G)
            for g, o in zip(slices, out):
                G2 = g.reshape(T, out_f)         # G and Y: rows at a uniform stride are read in place
                if G2.stride(1) != 1 or (T > 1 and G2.stride(0) < out_f):
                    G2 = G2.contiguous()
                g_ld = G2.stride(0) if T > 1 else out_f
                with _timed("alrp_linear_bf16", 6.0 * T * in_f * out_f,
                            6.0 * T * out_f + 12.0 * T * out_f + 2.0 * in_f * out_f + 4.0 * T * in_f):
                    _lib.check(lib.te_attnlrp_linear_bf16(_ptr(G2), g_ld, _ptr(Y2), y_ld, _ptr(W2), int(ALRP_WEIGHT_T), _ptr(o), T, in_f,
                                                       out_f, float(eps), _ptr(ws), ws.numel(), _stream(G)), "te_attnlrp_linear_bf16")
        return out.reshape(*G.shape[:-1], in_f)
    if Y is not None:
        raise _lib.TeError("alrp_linear: Y is an argument of the bf16 route; with an fp32 W pass damp(G, Y) as G")
    if X6_GEMM != "off" and gemm_x6_supported(T, out_f, in_f):
        return gemm_x6(G, x6_matrix_planes(W, True, cache), None, in_f, "alrp_linear_x6")
    return torch.matmul(G, W.detach())


def alrp_attention_bf16(G_o: Tensor, q: Tensor, k: Tensor, v: Tensor, attn: Tensor, num_heads: int, scale: float,
                        d_q: Tensor, d_k: Tensor, d_v: Tensor) -> None:
    """te_attnlrp_attention_bf16: the attention block's backward for d_out = G_o [B,N,C] fp32 on the bf16 q / k / v ([B,N,C]
    views, read in place) and probabilities attn [B,H,N,N], written into the fp32 [B,N,C] views d_q / d_k / d_v."""
    B, N, C = G_o.shape
    H, D = int(num_heads), C // int(num_heads)

    def view(t, bf16):
        t = _prep_bf16(t) if bf16 else _prep(t)
        if tuple(t.shape) != (B, N, C) or t.stride(2) != 1 or t.stride(0) < 0 or t.stride(1) < 0:
            raise _lib.TeError(f"alrp_attention_bf16: operands and outputs are [B,N,C] views with a contiguous last dimension, "
                               f"got shape {tuple(t.shape)}, strides {t.stride()}")
        return t.data_ptr(), t.stride(0), D, t.stride(1)

    G_o = _c(G_o)
    attn = _c16(attn)
    if tuple(attn.shape) != (B, H, N, N):
        raise _lib.TeError(f"alrp_attention_bf16: attn must be [B,H,N,N] = {(B, H, N, N)}, got {tuple(attn.shape)}")
    args = [*view(G_o, False), *view(q, True), *view(k, True), *view(v, True), _ptr(attn), float(scale),
            *view(d_q, False), *view(d_k, False), *view(d_v, False)]
    with _on_device(G_o) as lib, _timed("alrp_attention_bf16", 24.0 * B * H * N * N * D,
                                        B * H * (22.0 * N * N + 44.0 * N * D)):
        ws = _ws(lib.te_attnlrp_attention_bf16_workspace_bytes(B, H, N, D), G_o)
        _lib.check(lib.te_attnlrp_attention_bf16(*args, B, H, N, D, _ptr(ws), ws.numel(), _stream(G_o)), "te_attnlrp_attention_bf16")
