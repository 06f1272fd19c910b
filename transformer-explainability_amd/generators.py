"""Explanation generators: mirrors of baselines/ViT/ViT_explanation_generator.py (LRP) and
BERT_explainability/modules/BERT/ExplanationGenerator.py (Generator) of the reference.

Same method names and arguments; differences (results identical at batch 1):
  * a batch of B inputs is explained in one pass (B independent samples) -> [B, N-1] / [B, N]
  * the class index defaults to the per-sample argmax, computed on the device (no D2H round trip)
  * the attention gradients are obtained with torch.autograd.grad w.r.t. the attention tensors only,
    so no weight gradients are computed (the reference's loss.backward() computes and discards them)
"""
from __future__ import annotations

import contextlib
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import methods as M
from . import ops
from .rules import StopRelprop, stop_after_attn_cam
from .vit import relprop_tail


def _one_hot(output: torch.Tensor, index) -> torch.Tensor:
    B, K = output.shape
    if index is None:
        idx = output.detach().argmax(dim=-1)
    else:
        idx = torch.as_tensor(np.asarray(index) if not torch.is_tensor(index) else index, device=output.device)
        idx = idx.reshape(-1).long()
        if idx.numel() == 1 and B > 1:
            idx = idx.expand(B)
    # a bf16 model's relevance is fp32 from the seed on (ops: bf16 operands, fp32 relevance)
    dtype = torch.float32 if output.dtype == torch.bfloat16 else output.dtype
    one_hot = torch.zeros((B, K), dtype=dtype, device=output.device)
    one_hot.scatter_(1, idx.view(B, 1), 1.0)
    return one_hot


def _headmean_stack(attns):
    """Per-layer head means of the attention probabilities as the fp32 [L,B,N,N] stack ops.rollout reads.  A bf16 model:
    te_attn_headmean_bf16 writes every layer's fp32 mean straight into its slice (heads summed in fp32 on the exact
    upcast; the probabilities are read once, as bf16).  fp32: the reference's own expression."""
    if ops._is_bf16(attns[0]):
        B, _, N, _ = attns[0].shape
        stack = torch.empty((len(attns), B, N, N), dtype=torch.float32, device=attns[0].device)
        for i, a in enumerate(attns):
            ops.attn_headmean(a, out=stack[i])
        return stack
    return torch.stack([a.mean(dim=1) for a in attns], 0)


def _attention_gradients(loss, attn_modules, retain_graph=False):
    """Attention gradients of the listed modules (lowest block first), nothing else: no weight gradients, nothing below
    the lowest listed block.  retain_graph: another backward pass over the same forward pass follows (_class_pass)."""
    anchors = [getattr(m, "_fused_anchor", None) for m in attn_modules]
    if anchors and all(a is not None for a in anchors):
        # producer kernels (vit._FusedAttention): the gradient w.r.t. the probabilities is formed inside the block's
        # own backward and handed to save_attn_gradients; drive autograd down to the lowest block's qkv activation and
        # tell that block that nothing consumes its d_qkv
        lowest = attn_modules[0]
        lowest._fused_stop_backward = True
        try:
            torch.autograd.grad(loss, [anchors[0]], retain_graph=retain_graph, allow_unused=True)
        finally:
            lowest._fused_stop_backward = False
        return
    if any(a is not None for a in anchors):
        raise ops._lib.TeError("attention gradients: some of the listed blocks ran on the producer kernels and some on "
                               "stock PyTorch (a frozen qkv layer, or a block in train mode?); the gradient driver "
                               "handles one kind per pass -- set ops.USE_FUSED_PRODUCERS = False for this model")
    attns = [m.get_attn() for m in attn_modules]
    grads = torch.autograd.grad(loss, attns, retain_graph=retain_graph, allow_unused=False)
    for m, g in zip(attn_modules, grads):
        m.save_attn_gradients(g)


# ----------------------------------------------------------------------------------------------------------------------
# The tails of the two attention baselines as functions of the model with its populated caches (Baselines calls them; so
# does LRP.generate_all, which serves them from the forward / backward pass it runs anyway).
def cam_attn_tail(model):
    """ViT_explanation_generator.py:57-72 on the last block's attention and attention gradient."""
    last = model.blocks[-1].attn
    grad = last.get_attn_gradients()
    B, H, N, _ = grad.shape
    side = int(round((N - 1) ** 0.5))
    # (a bf16 model: evaluated in fp32 on its attention and gradient, like the relprop maps; a no-op for fp32)
    cam = last.get_attention_map().detach()[:, :, 0, 1:].float().reshape(B, H, side, side)
    g = grad[:, :, 0, 1:].float().reshape(B, H, side, side).mean(dim=[2, 3], keepdim=True)
    cam = (cam * g).mean(1).clamp(min=0)
    lo = cam.amin(dim=(1, 2), keepdim=True)
    hi = cam.amax(dim=(1, 2), keepdim=True)
    cam = (cam - lo) / (hi - lo)
    return cam[0] if B == 1 else cam


def attn_rollout_tail(model, start_layer=0):
    """ViT_explanation_generator.py:76-83 on the attention probabilities of every block."""
    stack = _headmean_stack([blk.attn.get_attention_map().detach() for blk in model.blocks])
    joint = ops.rollout(stack, start_layer=start_layer, normalise=True)
    return joint[:, 0, 1:]


def _masked(head_mask) -> dict:
    """The keyword a model call takes for a head mask -- nothing at all without one, so that models whose forward knows no
    ``head_mask`` keep working."""
    return {} if head_mask is None else {"head_mask": head_mask}


def _head_relevance_chain(attn_modules, chain):
    """Run ``chain()`` (one relprop chain) with every listed attention module storing ops.head_relevance of the relevance it
    receives -> fp64 [B, L, H], layer 0 first."""
    for m in attn_modules:
        m.save_head_relevance, m.head_relevance = True, None
    try:
        chain()
    finally:
        for m in attn_modules:
            m.save_head_relevance = False
    return torch.stack([m.head_relevance for m in attn_modules], 1)


def _refuse_before_forward(input, wanted):
    """The dtype refusals of the single-method calls, raised before the forward pass."""
    if "full" in wanted and ops._is_f64(input):
        # (refused before the forward pass: the z^B patch rule has no fp64 kernel, and no part of an fp64 map is
        # computed in a narrower format)
        raise ops._lib.TeError(f"{ops.DTYPES_MSG}; method='full' (the z^B patch rule) is not implemented for a "
                               "torch.float64 model: run it on a float32 or bfloat16 model")


def _refuse_attnlrp(model, eps, head_mask, *inputs, cast=()):
    """The refusals of generate_attnlrp, raised before the forward pass: AttnLRP (te_relprop.h, section "AttnLRP") is
    implemented for float32 models, and for bfloat16 models on the GPU, in eval mode without a head mask.  ``inputs`` share
    the parameters' dtype; ``cast`` are inputs a bfloat16 model casts to its own dtype itself (BERT's attention_mask, which
    generate_LRP takes in any dtype): they only have to be on the GPU."""
    if head_mask is not None:
        raise ops._lib.TeError("generate_attnlrp: head_mask is not implemented for AttnLRP (the chain has no Mul rule); "
                               "pass head_mask=None")
    if model.training:
        raise ops._lib.TeError("generate_attnlrp: the model is in train mode; AttnLRP reads the caches of an eval-mode "
                               "forward pass (dropout is the identity): call model.eval()")
    floats = lambda ts: [t for t in ts if torch.is_tensor(t) and t.is_floating_point()]      # noqa: E731
    params = list(model.parameters())
    bf16_model = bool(params) and all(p.dtype == torch.bfloat16 for p in params)
    strict = params + floats(inputs) + ([] if bf16_model else floats(cast))
    dtypes = [t.dtype for t in strict]
    for dt in dtypes:
        if dt not in (torch.float32, torch.bfloat16):
            raise ops._lib.TeError(f"generate_attnlrp: AttnLRP is implemented for torch.float32 and torch.bfloat16 models "
                                   f"and inputs only, got {dt}: run it on a float32 or bfloat16 copy of the model")
    if torch.bfloat16 in dtypes:
        if torch.float32 in dtypes:
            raise ops._lib.TeError("generate_attnlrp: torch.bfloat16 mixed with torch.float32 among the model's parameters and "
                                   "its inputs; the chain reads the caches of ONE format: convert the model and its inputs "
                                   "alike (model.to(torch.bfloat16), input.to(torch.bfloat16))")
        if any(not t.is_cuda for t in strict + [t for t in list(inputs) + list(cast) if torch.is_tensor(t)]):
            raise ops._lib.TeError("generate_attnlrp: a torch.bfloat16 model and its inputs must be on the GPU -- the chain on "
                                   "bf16 operands runs in the HIP kernels only, there is no host chain")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < float("inf"):
        raise ValueError(f"generate_attnlrp: eps must be a finite number >= 0, got {eps!r}")


def _drop_rule_planes(model):
    """The operand planes the x6 forward products left for the relprop rules of their layers (ops.post_x_abs_planes: 6 B per
    input element) have no reader in a call that runs no such rule: drop them with the forward pass behind."""
    for m in model.modules():
        cache = m.__dict__.get("_te_cache")
        if cache:
            ops.drop_x_planes(cache, with_abs=True)


@contextlib.contextmanager
def _x6_bracket(t):
    """Around a public call on the batch ``t``: a lost x6 hand-over of an EARLIER call is raised before it, once, without
    synchronising (ops.x6_poll; NaN in a map means exactly that -- check() asks about the calls made so far, and
    synchronises); the status word is posted to the host after it (ops.x6_post), not after a call that raised."""
    if t.is_cuda:
        ops.x6_poll(t.device)
    yield
    if t.is_cuda:
        ops.x6_post(t.device)


@contextlib.contextmanager
def _prune_flag(model, value):
    """The model's prune_below_start_layer flag is ``value`` for THIS call only: a user's own setting of it (and direct
    model.relprop calls afterwards) are unaffected."""
    user_flag = model.prune_below_start_layer
    model.prune_below_start_layer = value
    try:
        yield
    finally:
        model.prune_below_start_layer = user_flag


class ClassMaps(NamedTuple):
    """What generate_classes returns.  classes: int64 [B,K] on the device, None when ``seeds`` was given; scores [B,K]: the
    logits of those classes (for ``seeds``: sum(seed * logits)), fp32 for fp32 and bf16 models, fp64 for fp64 models;
    maps: {method: [B,K,...]} in the caller's order of methods, ``maps[m][:, k]`` the single call's map for ``classes[:, k]``
    (always with the batch dimension, also at B = 1)."""
    classes: Optional[torch.Tensor]
    scores: torch.Tensor
    maps: dict


def _num_classes(model):
    """The width of the model's logits where the model says it (ViT: num_classes; BERT: num_labels), else None: the class
    requests are then checked after the forward pass instead of before it."""
    for name in ("num_classes", "num_labels"):
        n = getattr(model, name, None)
        if isinstance(n, int) and n > 0:
            return n
    return None


class TopAnd:
    """A ``classes=`` argument of generate_classes: per sample its TOP class (the device argmax: te_class_targets, top-1)
    next to the given ``classes`` [B] or [B,K'] -- e.g. the predicted class and the label of the perturbation protocol.  The
    two are merged on the device after the forward pass; nothing is read back.  top_first: the top class is column 0."""

    def __init__(self, classes, top_first=True):
        self.classes, self.top_first = classes, bool(top_first)


class _ClassRequest:
    """Exactly one of classes / topk / seeds of a generate_classes call, validated as far as the host can see (``check`` runs
    before the forward pass when the model states its number of classes, and again on the logits)."""

    def __init__(self, classes, topk, seeds):
        if sum(a is not None for a in (classes, topk, seeds)) != 1:
            raise ValueError("generate_classes: give exactly one of classes / topk / seeds")
        self.classes, self.topk, self.seeds = classes, topk, seeds

    def check(self, B, C, rel_dtype, device):
        if self.topk is not None:
            k = self.topk
            if isinstance(k, bool) or int(k) != k or k < 1 or (C is not None and k > C):
                raise ValueError(f"topk must be an integer in [1, {C if C is not None else 'num_classes'}], got {self.topk!r}")
        elif isinstance(self.classes, TopAnd):
            given = self.classes.classes
            given = given.reshape(B, -1) if torch.is_tensor(given) else np.asarray(given).reshape(B, -1)
            if C is not None:
                self.classes = TopAnd(ops.host_classes(given, B, C, device), self.classes.top_first)
        elif self.classes is not None:
            if C is not None:
                self.classes = ops.host_classes(self.classes, B, C, device)
        else:
            t = self.seeds
            if not torch.is_tensor(t):
                raise ValueError("seeds must be a tensor of shape [B,C] or [B,K,C]")
            if t.dtype != rel_dtype:
                raise ops._lib.TeError(f"{ops.DTYPES_MSG}; the seeds of this model are {rel_dtype} (its relevance dtype), "
                                       f"got {t.dtype}")
            if t.dim() not in (2, 3) or t.shape[0] != B or t.numel() == 0 or (C is not None and t.shape[-1] != C):
                raise ValueError(f"seeds must have shape [B,C] or [B,K,C] = [{B},{'K,' if t.dim() == 3 else ''}"
                                 f"{C if C is not None else 'num_classes'}], got {tuple(t.shape)}")

    def targets(self, output):
        """On the logits [B,C] -> (classes [B,K] or None, scores [B,K], seeds [K,B,C]): ops.class_targets for classes / topk
        (nothing is read back), the caller's own seeds otherwise."""
        B, C = output.shape
        logits = output.detach()
        rel = ops.relevance_dtype(logits.dtype)
        self.check(B, C, rel, logits.device)
        if isinstance(self.classes, TopAnd):
            top = ops.class_targets(logits, topk=1, with_seeds=False)[0]
            cols = [top, self.classes.classes] if self.classes.top_first else [self.classes.classes, top]
            return ops.class_targets(logits, classes=torch.cat(cols, 1))
        if self.seeds is None:
            return ops.class_targets(logits, classes=self.classes, topk=self.topk)
        seeds = self.seeds.to(logits.device).reshape(B, -1, C).permute(1, 0, 2).contiguous()
        scores = (seeds * logits.to(rel)).sum(dim=-1).t().contiguous()
        return None, scores, seeds


def _check_chunk(chunk):
    """``chunk`` of generate_attnlrp_classes: None (all classes in one chain pass) or an integer >= 1."""
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
        raise ValueError(f"generate_attnlrp_classes: chunk must be None or an integer >= 1, got {chunk!r}")


def _attnlrp_class_chain(chain, seeds, chunk):
    """``chain`` (model.attnlrp on the caches of one forward pass) over the seeds [K,B,C], ``chunk`` classes per pass -> [B,K,...].
    A pass of several classes carries them as a class axis (te_relprop.h, "AttnLRP, a class axis"); chunk == 1 runs K chains
    without one, on the kernels of generate_attnlrp.  Slice k has the same bits either way."""
    K = seeds.shape[0]
    if chunk == 1:
        return torch.stack([chain(seeds[k]) for k in range(K)], 1)
    if chunk is None or chunk >= K:
        return chain(seeds)
    return torch.cat([chain(seeds[k0:k0 + chunk]) for k0 in range(0, K, chunk)], 1)


def _stack_classes(per_class, names):
    """[{name: map of class k}] -> {name: [B,K,...]}."""
    return {m: torch.stack([d[m] for d in per_class], 1) for m in names}


class _PassDriver:
    """What LRP and Generator share: the options, check() and the one implementation of "attention gradients, then -- or,
    with overlap_backward, beside them -- the relprop chain"."""

    def __init__(self, model, overlap_backward, prune):
        self.model = model
        self.model.eval()
        # (extension) the relprop chain reads only forward caches; the attention gradients are needed by the tail
        # alone.  With overlap_backward the backward pass (main stream) and the relprop rules (side stream) run
        # concurrently and join before the head-mean / rollout tail: the memory-bound backward kernels and the tails
        # of the MFMA-bound Linear.relprop launches fill each other's idle CUs.  Same kernels, same results, bit for bit.
        self.overlap_backward = bool(overlap_backward)
        self._relprop_stream = None
        # (extension, off by default) serve only the blocks / layers a method reads: see LRP and Generator
        self.prune = bool(prune)

    def check(self):
        """Raise TeError if any x6 Linear kernel since the last check lost a stream-K hand-over (the affected maps carry
        NaN).  Synchronises the device: call it where the maps are read back anyway, never inside a step."""
        ops.x6_raise_if_failed(next(self.model.parameters()).device)

    def _class_pass(self, output, seeds, attn_modules, chain_of, tails, tail_owner=None):
        """The backward passes and relprop chains of SEVERAL classes over ONE forward pass, one class after another in the
        order of ``seeds`` [K,B,C]: per class the attention gradients of ``attn_modules`` on sum(seed * output) (none: no
        backward pass), then ``chain_of(seed)()`` (chain_of(seed) None: no chain), then ``tails(what the chain returned)``
        -> [{name: map}] * K.  Every backward pass but the last retains the graph; the planes of |X| the forward products
        left for their rules stay in the layers' scratch dicts until the last class's rules have read them and are gone
        when this returns or raises (ops.x_abs_planes_kept).  Afterwards the model's accessors hold the LAST class's
        gradients and attn_cam."""
        K = seeds.shape[0]
        caches = [m.__dict__["_te_cache"] for m in self.model.modules() if m.__dict__.get("_te_cache") is not None]
        per_class = []
        with ops.x_abs_planes_kept(caches) as kept:
            for k in range(K):
                kept.last = k == K - 1
                seed = seeds[k]
                loss = torch.sum(seed * output)
                out = self._gradients_and_chain(loss, attn_modules, chain_of(seed), tail_owner=tail_owner,
                                                retain_graph=not kept.last)
                per_class.append(tails(out))
        return per_class

    def _gradients_and_chain(self, loss, attn_modules, chain, tail_owner=None, retain_graph=False):
        """The attention gradients of ``attn_modules`` (none: no backward pass), then what ``chain()`` returns (None: no
        chain).  tail_owner: a model whose relprop runs the tail itself (ViT) and calls ``_before_tail`` in front of it.
        retain_graph: the forward pass is differentiated again afterwards (_class_pass)."""
        if chain is None or not (self.overlap_backward and loss.is_cuda):
            if attn_modules:
                _attention_gradients(loss, attn_modules, retain_graph)
            return None if chain is None else chain()
        dev = loss.device
        main = torch.cuda.current_stream(dev)
        if self._relprop_stream is None:
            self._relprop_stream = torch.cuda.Stream(device=dev)
        side = self._relprop_stream
        side.wait_stream(main)                      # forward caches + one-hot are complete
        # backward on the main stream (autograd runs each node on its forward op's stream)
        if attn_modules:
            _attention_gradients(loss, attn_modules, retain_graph)
        if tail_owner is not None:
            # (only then: every other caller runs its tail after the join below, and an event nobody waits on is one more
            # node in a captured graph)
            grads_ready = main.record_event()
            tail_owner._before_tail = lambda: torch.cuda.current_stream(dev).wait_event(grads_ready)
        try:
            with torch.cuda.stream(side):
                out = chain()
        finally:
            if tail_owner is not None:
                tail_owner._before_tail = None
            main.wait_stream(side)                  # whatever follows (head-mean, rollout) reads both streams' results
        if not torch.cuda.is_current_stream_capturing():
            for t in (out.values() if isinstance(out, dict) else (out,)):
                if t is not None:
                    t.record_stream(main)
        return out


class LRP(_PassDriver):
    """baselines/ViT/ViT_explanation_generator.py:20-41.  Batched: B inputs -> B maps (B = 1 is the reference's call).

    (The round-1 ``streams`` extension -- micro-batches on separate HIP streams -- is gone: it stopped making progress at
    batch 64 for reasons never diagnosed, and since round 3 the Linear rules run on persistent whole-chip kernels that
    two streams could only serialise.)"""

    # what every single-method call runs, as the reference does: every attention gradient and the whole chain
    _SINGLE_CALL_NEED = M.Needs(all_grads=True, relprop=True)

    def __init__(self, model, overlap_backward=False, prune=False):
        # prune: only the blocks >= start_layer contribute to a transformer_attribution map: skip the relprop rules and
        # the attention-gradient backward below them (model.prune_below_start_layer)
        super().__init__(model, overlap_backward, prune)

    def generate_LRP(self, input, index=None, method="transformer_attribution", is_ablation=False, start_layer=0,
                     head_mask=None):
        # head_mask (extension): one value per head, [H], [L,H] or [L,B,H] (VisionTransformer.get_head_mask)
        with _x6_bracket(input):
            return self._single(input, index, method, is_ablation, start_layer, head_mask)

    def _single(self, input, index, method="transformer_attribution", is_ablation=False, start_layer=0, head_mask=None):
        """generate_LRP without the x6 bracket (what GraphedLRP captures).  Not planned from the needs table: a single call
        does the reference's work whatever its tail reads, and honours ``prune`` for methods.SINGLE_CALL_PRUNED alone."""
        _refuse_before_forward(input, (method,))
        pruned = bool((self.prune or self.model.prune_below_start_layer) and method in M.SINGLE_CALL_PRUNED)
        name = self.model.default_method if method is None else method
        return self._pass(input, (name,), index, is_ablation, start_layer, head_mask, self._SINGLE_CALL_NEED, pruned)[name]

    def generate_attnlrp(self, input, index=None, eps=1e-6, head_mask=None, method="tokens"):
        """(extension) AttnLRP (Achtibat et al., ICML 2024; the rules: te_relprop.h, section "AttnLRP") -> fp32 [B, N-1],
        the shape of generate_LRP: the relevance of the patch tokens for the class ``index`` (None: the per-sample argmax).
        One forward pass, no backward pass, one chain; ``eps`` (>= 0) stabilises the Linear and residual-Add rules.  float32
        models, and bfloat16 models with bfloat16 images on the GPU (the chain in fp32 on the cached bf16 tensors), in eval
        mode; fp16 / fp64 models, a mix of bf16 and fp32, train mode and ``head_mask`` raise TeError before the forward
        pass.  The x6 status poll / post as in generate_LRP; capturable by GraphedCall.
        method="full": the same chain, then the eps-rule through the patch embedding and input x G per pixel (te_relprop.h,
        "AttnLRP, pixel level") -> fp32 [B, H, W], the shape of generate_LRP(method="full").  Any other name than "tokens" /
        "full" is a ValueError before the forward pass."""
        with _x6_bracket(input):
            return self._attnlrp(input, index, eps, head_mask, method)

    def _attnlrp(self, input, index=None, eps=1e-6, head_mask=None, method="tokens"):
        """generate_attnlrp without the x6 bracket."""
        if method not in ("tokens", "full"):
            raise ValueError(f"generate_attnlrp: method must be 'tokens' (patch tokens, [B, N-1]) or 'full' (pixels, [B,H,W]), "
                             f"got {method!r}")
        _refuse_attnlrp(self.model, eps, head_mask, input)
        with torch.no_grad():
            output = self.model(input)
            _drop_rule_planes(self.model)
            seed = _one_hot(output, index)
            return self._gradients_and_chain(output, [], lambda: self.model.attnlrp(seed, eps=eps, method=method))

    def generate_attnlrp_classes(self, input, classes=None, topk=None, seeds=None, eps=1e-6, method="tokens",
                                 chunk=None) -> ClassMaps:
        """(extension) AttnLRP for several CLASSES of the same batch from ONE forward pass and one chain with a class axis
        (te_relprop.h, "AttnLRP, a class axis": the chain is linear in the seed and its cached operands do not depend on the
        class).  Exactly one of ``classes`` / ``topk`` / ``seeds``, as in generate_classes (``TopAnd``, [K] for all samples,
        duplicates; device tensors are not read back, an out-of-range class in one yields class -1, score NaN and the map of
        an all-zero seed); ``seeds`` [B,C] or [B,K,C] are float32, for bf16 models too (G is fp32), e.g. onehot(c) - onehot(c')
        for a contrastive map.  Returns ClassMaps(classes [B,K] or None, scores [B,K], {"attnlrp": M}), M fp32 [B,K,N-1]
        (method="tokens") or [B,K,H,W] (method="full").  ``M[:, k]`` has the bits of generate_attnlrp(input,
        index=classes[:, k], eps, method) on a fresh forward pass wherever a batch equals its samples for that call: every
        product on the package's kernels, and one-hot seeds at a stock head product; general seeds at a stock head product
        and models whose Linear products run on the stock GEMM agree to rounding.  ``chunk``: classes per chain pass (default:
        all K; bounds the memory of G, K times a single chain's); the same bits for every chunk; chunk=1 runs K chains on
        the kernels of generate_attnlrp after the one forward pass.  The refusals of generate_attnlrp (there is no
        ``head_mask`` argument), a bad ``method`` / ``chunk`` (ValueError) and a bad class request are raised before the
        forward pass.  The x6 status poll / post happens once; capturable by GraphedCall."""
        with _x6_bracket(input):
            if method not in ("tokens", "full"):
                raise ValueError(f"generate_attnlrp_classes: method must be 'tokens' (patch tokens, [B,K,N-1]) or 'full' (pixels, "
                                 f"[B,K,H,W]), got {method!r}")
            _check_chunk(chunk)
            _refuse_attnlrp(self.model, eps, None, input)
            request = _ClassRequest(classes, topk, seeds)
            request.check(input.shape[0], _num_classes(self.model), torch.float32, input.device)
            with torch.no_grad():
                output = self.model(input)
                _drop_rule_planes(self.model)
                cls, scores, seed_stack = request.targets(output)
                chain = lambda seed: self.model.attnlrp(seed, eps=eps, method=method)      # noqa: E731
                maps = self._gradients_and_chain(output, [], lambda: _attnlrp_class_chain(chain, seed_stack, chunk))
            return ClassMaps(cls, scores, {"attnlrp": maps})

    def generate_all(self, input, methods, index=None, is_ablation=False, start_layer=0, head_mask=None):
        """(extension) The maps of several methods of the SAME batch from one pass: ``methods`` is any subset of the
        ``method=`` names of generate_LRP plus the two baselines as "attn_rollout" / "attn_gradcam" (served from this
        model: ``Baselines(self.model)``); returns {name: map}, each entry the shape, dtype and bits of the single call
        (``generate_LRP(input, index, method=name, is_ablation, start_layer)``, ``Baselines.generate_rollout(input,
        start_layer)``, ``Baselines.generate_cam_attn(input, index)``).

        One forward pass, then only what the union of the methods needs (methods.LRP_NEEDS): no backward pass and no
        relprop for {"last_layer_attn", "attn_rollout"}, the last block's attention gradient alone for "attn_gradcam",
        one relprop chain for all relprop methods, which "full" continues below the blocks.  ``prune`` is honoured only
        when every requested method reads the blocks >= start_layer alone (methods.prunable); ``overlap_backward``, the
        x6 status poll / post, the GELU-backward plane hand-off and ``head_mask`` behave as in generate_LRP.  An unknown name raises
        ValueError, the dtype refusals of the single calls raise their TeError, both before the forward pass."""
        wanted = M.check(methods, M.LRP_NEEDS)
        _refuse_before_forward(input, wanted)
        if input.dtype == torch.float16:
            raise ops._lib.TeError(f"{ops.DTYPES_MSG}; got {input.dtype} here")
        need = M.needs(wanted, M.LRP_NEEDS, is_ablation, M.LRP_ABLATION_NEEDS)
        pruned = bool((self.prune or self.model.prune_below_start_layer) and need.relprop
                      and M.prunable(wanted, M.LRP_NEEDS))
        ours = tuple(m for m in wanted if m not in M.BASELINE_METHODS)       # the tails of model.relprop
        with _x6_bracket(input):
            maps = self._pass(input, ours, index, is_ablation, start_layer, head_mask, need, pruned)
            # the two baselines are tails of the same forward / backward pass (here only: to a single call they are unknown
            # names like any other)
            if "attn_rollout" in wanted:
                maps["attn_rollout"] = attn_rollout_tail(self.model, start_layer)
            if "attn_gradcam" in wanted:
                maps["attn_gradcam"] = cam_attn_tail(self.model)
            return {m: maps[m] for m in wanted}

    def generate_classes(self, input, classes=None, topk=None, seeds=None, methods=("transformer_attribution",),
                         is_ablation=False, start_layer=0, head_mask=None) -> ClassMaps:
        """(extension) The maps of several CLASSES (and several methods) of the same batch from ONE forward pass.  Exactly one
        of: ``classes`` [B,K] (or [K] for every sample alike; tensor, array or list; duplicates allowed), ``topk`` = K (the K
        largest logits per sample, chosen on the device: no device-to-host copy), ``seeds`` [B,C] or [B,K,C] in the model's
        relevance dtype (the relevance put on the logits instead of a one-hot, e.g. onehot(c) - onehot(c') for a contrastive
        map; the backward pass differentiates sum(seed * logits)).  ``classes`` may also be a ``TopAnd(given)``: the per-sample
        top class next to given ones, merged on the device.  ``methods``: as in generate_all, with its refusals.
        Returns ClassMaps(classes, scores, maps): ``maps[m][:, k]`` has the bits of the single call on a fresh forward pass
        with ``index=classes[:, k]`` (generate_LRP, Baselines.generate_rollout / generate_cam_attn).

        One forward pass; then per class, in order, the attention gradients and the relprop chain the union of the methods
        needs (methods.LRP_NEEDS) and every tail; methods that read the forward pass alone are computed once and returned K
        times, and a request of such methods only runs no backward pass and no chain.  ``prune``, ``overlap_backward``,
        ``head_mask``, ``is_ablation`` and ``start_layer`` act per class as they do per call; the x6 status poll / post happens
        once.  Afterwards the model's accessors (get_attn_cam(), get_attn_gradients()) hold the LAST class's state.  A class
        outside [0, num_classes) in a list, an array or a CPU tensor is a ValueError before the forward pass; in a device
        tensor (which is not read back) it yields classes -1, score NaN and maps of an all-zero seed."""
        wanted = M.check(methods, M.LRP_NEEDS)
        _refuse_before_forward(input, wanted)
        if input.dtype == torch.float16:
            raise ops._lib.TeError(f"{ops.DTYPES_MSG}; got {input.dtype} here")
        request = _ClassRequest(classes, topk, seeds)
        request.check(input.shape[0], _num_classes(self.model), ops.relevance_dtype(input.dtype), input.device)
        model = self.model

        def row(m):
            return M.needs((m,), M.LRP_NEEDS, is_ablation, M.LRP_ABLATION_NEEDS)
        once = tuple(m for m in wanted if row(m).forward_only)               # read the forward pass alone
        per_class = tuple(m for m in wanted if m not in once)
        need = M.needs(per_class, M.LRP_NEEDS, is_ablation, M.LRP_ABLATION_NEEDS)
        pruned = bool((self.prune or model.prune_below_start_layer) and need.relprop and M.prunable(wanted, M.LRP_NEEDS))
        ours = tuple(m for m in per_class if m not in M.BASELINE_METHODS)    # the tails of model.relprop
        with _x6_bracket(input):
            with ops.gelu_backward_plane_handoff():  # this call drives the backward passes itself (attention tensors only)
                output = model(input, **_masked(head_mask))
            cls, scores, seed_stack = request.targets(output)
            B, K = scores.shape
            shared = {m: attn_rollout_tail(model, start_layer) if m == "attn_rollout"
                      else relprop_tail(model, m, None, is_ablation, start_layer) for m in once}
            blocks = list(model.blocks)
            grad_blocks = blocks[start_layer if pruned else 0:] if need.all_grads else blocks[-1:] if need.last_grad else []

            def chain_of(seed):
                if not need.relprop:
                    return None
                return lambda: model.relprop(seed, method=ours, is_ablation=is_ablation, start_layer=start_layer, alpha=1)

            def tails(maps):
                maps = dict(maps or {})
                if "attn_gradcam" in per_class:
                    cam = cam_attn_tail(model)
                    maps["attn_gradcam"] = cam.unsqueeze(0) if B == 1 else cam
                return maps
            stacked = {}
            if per_class:
                with _prune_flag(model, pruned):
                    stacked = _stack_classes(self._class_pass(output, seed_stack, [blk.attn for blk in grad_blocks],
                                                              chain_of, tails, tail_owner=model), per_class)
            for m, t in shared.items():
                stacked[m] = t.unsqueeze(1).expand(-1, K, *t.shape[1:])
            return ClassMaps(cls, scores, {m: stacked[m] for m in wanted})

    def _pass(self, input, wanted, index, is_ablation, start_layer, head_mask, need, pruned):
        """One pass for the ``method=`` names ``wanted`` of model.relprop -> {name: map, None for a name it does not know}:
        forward; the attention gradients and the relprop chain ``need`` (a methods.Needs) asks for, from block start_layer up
        if ``pruned``; every tail."""
        model = self.model
        with ops.gelu_backward_plane_handoff():      # this call drives the backward pass itself (attention tensors only)
            output = model(input, **_masked(head_mask))
        maps = {}
        if not need.forward_only:
            one_hot = _one_hot(output, index)
            loss = torch.sum(one_hot * output)
            blocks = list(model.blocks)
            grad_blocks = blocks[start_layer if pruned else 0:] if need.all_grads else blocks[-1:] if need.last_grad else []

            def chain():            # (always a tuple of names: the model's rule for several methods, under the flag set here)
                return model.relprop(one_hot, method=wanted, is_ablation=is_ablation, start_layer=start_layer, alpha=1)
            with _prune_flag(model, pruned):
                maps = self._gradients_and_chain(loss, [blk.attn for blk in grad_blocks],
                                                 chain if need.relprop else None, tail_owner=model) or {}
        if not need.relprop:                         # ("last_layer_attn": the forward pass has produced all it reads)
            maps = {m: relprop_tail(model, m, None, is_ablation, start_layer) for m in wanted}
        return maps

    def generate_head_relevance(self, input, index=None, head_mask=None):
        """(extension) Per-head relevance in the sense of Voita et al. 2019: fp64 [B, L, H], entry (b, l, h) the sum of the
        relevance that arrives at head h's slice of block l's context layer (the argument of Attention.relprop_after_proj).
        One forward pass and one relprop chain; no backward pass, no map.  ``head_mask`` as in generate_LRP: the scores of
        the masked model."""
        model = self.model
        with torch.no_grad():
            output = model(input, **_masked(head_mask))
        one_hot = _one_hot(output, index)
        with _prune_flag(model, False):              # the whole chain runs, whatever the model's prune flag says
            return _head_relevance_chain([blk.attn for blk in model.blocks],
                                         lambda: model.relprop(one_hot, method=(), alpha=1))


class Baselines:
    """baselines/ViT/ViT_explanation_generator.py:44-83: the two attention-only baselines (no relprop; off the
    accelerated path, here so that the evaluation scripts' ``from ViT_explanation_generator import Baselines, LRP``
    resolves).  Batched: B inputs -> B maps."""

    def __init__(self, model):
        self.model = model
        self.model.eval()

    def generate_cam_attn(self, input, index=None):
        """attention GradCAM of the last block (:50-72): per-head gradient mean x attention, class-token row."""
        with ops.gelu_backward_plane_handoff():      # this call drives the backward pass itself (attention tensors only)
            output = self.model(input, register_hook=True)
        one_hot = _one_hot(output, index)
        # (the last block's gradient only; through the driver, so that a block on the producer kernels is served too)
        _attention_gradients(torch.sum(one_hot * output), [self.model.blocks[-1].attn])
        return cam_attn_tail(self.model)

    def generate_rollout(self, input, start_layer=0):
        """attention rollout (:74-83): head-averaged attention, identity added, rows normalised, chained."""
        self.model(input)
        return attn_rollout_tail(self.model, start_layer)


def _jet_bgr(mask01: np.ndarray) -> np.ndarray:
    """COLORMAP_JET as a formula (cv2 is not a dependency here): the standard piecewise-linear jet, returned in
    OpenCV's BGR channel order like cv2.applyColorMap(np.uint8(255 * mask), cv2.COLORMAP_JET) / 255.
    (Parity with cv2's 256-entry LUT is not pinned: no cv2 in the build image.)"""
    x = np.floor(255.0 * mask01) / 255.0                      # np.uint8(255 * mask) quantisation
    r = np.clip(1.5 - np.abs(4.0 * x - 3.0), 0.0, 1.0)
    g = np.clip(1.5 - np.abs(4.0 * x - 2.0), 0.0, 1.0)
    b = np.clip(1.5 - np.abs(4.0 * x - 1.0), 0.0, 1.0)
    return np.stack([b, g, r], axis=-1).astype(np.float32)


def generate_visualization(attribution_generator, original_image, class_index=None, method="transformer_attribution",
                           start_layer=0):
    """The notebooks' helper (example.ipynb:55-66, Transformer_explainability.ipynb:1149): relevance map of one image
    [3,H,W] -> bilinear x16 -> min-max -> JET overlay, uint8 [H,W,3].  The reference closes over a global
    ``attribution_generator``; here it is the first argument.  Up-sampling + normalisation run on the device
    (te_heatmap_f32)."""
    par = next(attribution_generator.model.parameters())
    image = original_image.unsqueeze(0).to(device=par.device, dtype=par.dtype)      # (a bf16 model takes a bf16 image)
    maps = attribution_generator.generate_LRP(image, method=method, index=class_index,
                                              start_layer=start_layer).detach()
    patch = attribution_generator.model.patch_embed.patch_size[0]
    heat = ops.heatmap(maps, scale=patch, normalise=True)[0, 0].cpu().numpy()
    img = original_image.permute(1, 2, 0).detach().cpu().numpy()
    img = (img - img.min()) / (img.max() - img.min())
    cam = _jet_bgr(heat) + np.float32(img)                     # show_cam_on_image (example.ipynb:47-52)
    cam = cam / np.max(cam)
    vis = np.uint8(255 * cam)
    return np.ascontiguousarray(vis[..., ::-1])                # cv2.cvtColor(vis, cv2.COLOR_RGB2BGR)


class GraphedCall:
    """``fn(*inputs)`` for FIXED input shapes captured in a HIP graph and replayed per call: inputs are copied into the
    graph's static buffers, the result lives in the graph's static output (clone it to keep it past the next call).
    Used for whole explanation passes (GraphedLRP for ViT; ``GraphedCall(lambda ids, mask: gen.generate_LRP(ids, mask,
    start_layer=0), (ids, mask))`` for BERT): ~1100 launches whose host-side enqueue time replay removes."""

    def __init__(self, fn, example_inputs, warmup=2):
        example_inputs = tuple(example_inputs)
        if not all(t.is_cuda for t in example_inputs):
            raise RuntimeError("GraphedCall needs inputs on the MI355X")
        dev = example_inputs[0].device
        self.fn = fn
        self.static_in = [t.clone() for t in example_inputs]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):          # warm-up off the capture: library handles, MIOpen find, allocator
            for _ in range(max(1, warmup)):
                fn(*self.static_in)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()               # the capture allocates from its own pool: hand the warm-up's blocks back
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_out = fn(*self.static_in)

    def __call__(self, *inputs):
        if len(inputs) != len(self.static_in):
            raise RuntimeError(f"GraphedCall was captured for {len(self.static_in)} inputs, got {len(inputs)}")
        for dst, src in zip(self.static_in, inputs):
            if src.shape != dst.shape:
                raise RuntimeError(f"GraphedCall was captured for {tuple(dst.shape)}, got {tuple(src.shape)}")
            dst.copy_(src)
        self.graph.replay()
        return self.static_out


class GraphedLRP:
    """One ``LRP.generate_LRP`` pass for a FIXED input shape captured in a HIP graph (forward, attention-gradient
    backward and every relprop kernel: ~1100 launches for ViT-B) and replayed per batch.  The pass is launch-latency
    bound between its many short kernels (stream gaps add up to ~10 % of a ViT-B/16 batch-64 step on MI355X);
    replay removes the host from the loop.  Inputs are copied into the graph's static buffer; the returned maps
    live in the graph's static output buffer (clone them to keep them past the next call).  The per-module caches
    (``get_attn_cam()`` ...) alias graph memory and are refreshed by every replay.

        glrp = GraphedLRP(LRP(model), images[:64], method="transformer_attribution", start_layer=1)
        maps = glrp(next_batch)"""

    def __init__(self, lrp, example_input, index=None, method="transformer_attribution", is_ablation=False,
                 start_layer=0, warmup=2):
        if not example_input.is_cuda:
            raise RuntimeError("GraphedLRP needs inputs on the MI355X")
        self.lrp = lrp
        statics = (example_input,)
        if index is not None:       # the class indices are the graph's second static input
            statics += (torch.as_tensor(index if torch.is_tensor(index) else np.asarray(index), device=example_input.device),)
        # (lrp._single: the pass without the x6 status poll / post, which belong to calls the host makes, not to a replay)
        self._call = GraphedCall(lambda x, idx=None: lrp._single(x, idx, method, is_ablation, start_layer), statics, warmup)

    def __call__(self, input, index=None):
        static_in, *static_index = self._call.static_in
        if input.shape != static_in.shape:
            raise RuntimeError(f"GraphedLRP was captured for {tuple(static_in.shape)}, got {tuple(input.shape)}")
        if not static_index:
            return self._call(input)
        if index is None:           # the class indices of the last call stay in force (copying a tensor onto itself is free:
            # torch returns at once, no kernel is launched)
            return self._call(input, static_index[0])
        return self._call(input, torch.as_tensor(index, device=input.device).reshape(static_index[0].shape))


class Generator(_PassDriver):
    """BERT_explainability/modules/BERT/ExplanationGenerator.py:20-59 (generate_LRP)."""

    def __init__(self, model, prune=False, overlap_backward=False):
        # prune: generate_LRP reads attn_cam / attention gradients of the layers >= start_layer only
        # (ExplanationGenerator.py:47-57) -- with the reference's default start_layer = 11 that is the LAST layer alone,
        # yet relevance and gradients are propagated through all twelve.  prune=True stops the relprop right after layer
        # start_layer's attn_cam is stored and asks autograd for the gradients of those layers only: the same vector bit
        # for bit; get_attn_cam() of the layers below is then not refreshed.
        super().__init__(model, overlap_backward, prune)

    def forward(self, input_ids, attention_mask):
        return self.model(input_ids, attention_mask)

    def _pass(self, input_ids, attention_mask, index, lowest_layer=0, grads="all", relprop=True, prune=None,
              head_mask=None):
        """One pass: forward; the attention gradients of ``grads`` ("all": the layers served, "last": the last layer
        alone, None: no backward pass); the relprop chain if ``relprop``.  prune (default: self.prune): only the layers
        >= lowest_layer are served.  -> (the encoder layers, what model.relprop returned or None)."""
        prune = self.prune if prune is None else bool(prune)
        layers = self.model.bert.encoder.layer
        if grads is None and not relprop:            # forward only: as generate_attn_last_layer / generate_rollout
            with torch.no_grad():
                self.model(input_ids=input_ids, attention_mask=attention_mask, **_masked(head_mask))
            return layers, None
        with ops.gelu_backward_plane_handoff():      # this call drives the backward pass itself (attention tensors only)
            output = self.model(input_ids=input_ids, attention_mask=attention_mask, **_masked(head_mask))[0]
        one_hot = _one_hot(output, index)
        loss = torch.sum(one_hot * output)
        first = lowest_layer if prune else 0
        grad_layers = list(layers)[first:] if grads == "all" else list(layers)[-1:] if grads == "last" else []

        return layers, self._gradients_and_chain(loss, [lay.attention.self for lay in grad_layers],
                                                 self._chain(one_hot, first, prune) if relprop else None)

    def _chain(self, seed, first, prune):
        """The relprop chain of ``seed``.  prune: layer ``first`` ends it once its attn_cam is stored; nothing is returned."""
        layers = self.model.bert.encoder.layer

        def chain():
            with stop_after_attn_cam(layers[first].attention.self if prune else None):
                try:
                    return self.model.relprop(seed, alpha=1)
                except StopRelprop:
                    return None
        return chain

    def generate_classes(self, input_ids, attention_mask, classes=None, topk=None, seeds=None, methods=("LRP",),
                         start_layer=11, rollout_start_layer=0, head_mask=None) -> ClassMaps:
        """(extension) The vectors of several CLASSES (and several methods) of the same batch from ONE forward pass: the
        class arguments, the result and the order of the work as in LRP.generate_classes, the methods and ``start_layer`` /
        ``rollout_start_layer`` as in generate_all.  ``maps[m][:, k]`` has the bits of the generate_* method of that name on a
        fresh forward pass with ``index=classes[:, k]``.  Afterwards the model's accessors hold the LAST class's state."""
        wanted = M.check(methods, M.GENERATOR_NEEDS)
        request = _ClassRequest(classes, topk, seeds)
        par = next(self.model.parameters(), None)
        rel = ops.relevance_dtype(par.dtype) if par is not None else torch.float32
        request.check(input_ids.shape[0], _num_classes(self.model), rel, input_ids.device)
        once = tuple(m for m in wanted if M.GENERATOR_NEEDS[m].forward_only)
        per_class = tuple(m for m in wanted if m not in once)
        need = M.needs(per_class, M.GENERATOR_NEEDS)
        pruned = bool(self.prune and M.prunable(wanted, M.GENERATOR_NEEDS))
        model = self.model
        with _x6_bracket(input_ids):
            with ops.gelu_backward_plane_handoff():  # this call drives the backward passes itself (attention tensors only)
                output = model(input_ids=input_ids, attention_mask=attention_mask, **_masked(head_mask))[0]
            layers = model.bert.encoder.layer
            lowest = start_layer if "LRP" in wanted else self._last_layer()
            cls, scores, seed_stack = request.targets(output)
            K = scores.shape[1]
            shared = {m: attn_last_layer_tail(model) if m == "attn_last_layer" else rollout_tail(model, rollout_start_layer)
                      for m in once}
            first = lowest if pruned else 0
            grad_layers = list(layers)[first:] if need.all_grads else list(layers)[-1:] if need.last_grad else []
            tail_of = {"LRP": lambda cam: lrp_tail(model, start_layer, pruned),
                       "LRP_last_layer": lambda cam: lrp_last_layer_tail(model),
                       "full_lrp": full_lrp_tail,
                       "attn_gradcam": lambda cam: attn_gradcam_tail(model)}
            stacked = {}
            if per_class:
                stacked = _stack_classes(self._class_pass(
                    output, seed_stack, [lay.attention.self for lay in grad_layers],
                    lambda seed: self._chain(seed, first, pruned) if need.relprop else None,
                    lambda cam: {m: tail_of[m](cam) for m in per_class}), per_class)
            for m, t in shared.items():
                stacked[m] = t.unsqueeze(1).expand(-1, K, *t.shape[1:])
            return ClassMaps(cls, scores, {m: stacked[m] for m in wanted})

    def generate_all(self, input_ids, attention_mask, methods, index=None, start_layer=11, rollout_start_layer=0,
                     head_mask=None):
        """(extension) The vectors of several methods of the SAME batch from one pass: ``methods`` is any subset of
        "LRP", "LRP_last_layer", "full_lrp", "attn_last_layer", "rollout", "attn_gradcam" (the generate_* methods);
        returns {name: vector}, each entry the shape, dtype and bits of the single call (generate_LRP with
        ``start_layer``, generate_rollout with ``rollout_start_layer``).  One forward pass and at most one backward
        pass and one relprop chain, only as far as the union of the methods needs (methods.GENERATOR_NEEDS); "full_lrp"
        keeps what model.relprop returns.  ``prune`` is honoured only when every requested method reads the layers it
        serves alone (methods.prunable).  An unknown name raises ValueError before the forward pass.  ``head_mask``: as in
        the single calls."""
        wanted = M.check(methods, M.GENERATOR_NEEDS)
        need = M.needs(wanted, M.GENERATOR_NEEDS)
        pruned = bool(self.prune and M.prunable(wanted, M.GENERATOR_NEEDS))
        lowest = start_layer if "LRP" in wanted else self._last_layer()
        with _x6_bracket(input_ids):
            _, cam = self._pass(input_ids, attention_mask, index, lowest_layer=lowest,
                                grads="all" if need.all_grads else "last" if need.last_grad else None,
                                relprop=need.relprop, prune=pruned, head_mask=head_mask)
            tails = {"LRP": lambda: lrp_tail(self.model, start_layer, pruned),
                     "LRP_last_layer": lambda: lrp_last_layer_tail(self.model),
                     "full_lrp": lambda: full_lrp_tail(cam),
                     "attn_last_layer": lambda: attn_last_layer_tail(self.model),
                     "rollout": lambda: rollout_tail(self.model, rollout_start_layer),
                     "attn_gradcam": lambda: attn_gradcam_tail(self.model)}
            return {m: tails[m]() for m in wanted}

    def _last_layer(self):
        return len(self.model.bert.encoder.layer) - 1

    def generate_LRP(self, input_ids, attention_mask, index=None, start_layer=11, head_mask=None):
        # head_mask (the model's own argument, BERT.py:556-625): one value per head, [H], [L,H] or, per sample, [L,B,H]
        with _x6_bracket(input_ids):
            self._pass(input_ids, attention_mask, index, lowest_layer=start_layer, head_mask=head_mask)
            return self.attribution_tail(start_layer)

    def generate_attnlrp(self, input_ids, attention_mask, index=None, eps=1e-6, head_mask=None):
        """(extension) AttnLRP (Achtibat et al., ICML 2024; the rules: te_relprop.h, section "AttnLRP") -> fp32 [B, N]: the
        relevance of every token (the sum over the hidden dimension of x0 (.) G at the input of the embedding LayerNorm) for
        the class ``index`` (None: the per-sample argmax).  One forward pass, no backward pass, one chain.  float32 models, and
        bfloat16 models on the GPU (attention_mask in any dtype, as for generate_LRP), in eval mode; fp16 / fp64 models, a mix
        of bf16 and fp32 parameters, train mode and ``head_mask`` raise TeError before the forward pass."""
        with _x6_bracket(input_ids):
            _refuse_attnlrp(self.model, eps, head_mask, input_ids, cast=(attention_mask,))
            with torch.no_grad():
                output = self.model(input_ids=input_ids, attention_mask=attention_mask)[0]
                _drop_rule_planes(self.model)
                seed = _one_hot(output, index)
                return self._gradients_and_chain(output, [], lambda: self.model.attnlrp(seed, eps=eps))

    def generate_attnlrp_classes(self, input_ids, attention_mask, classes=None, topk=None, seeds=None, eps=1e-6,
                                 chunk=None) -> ClassMaps:
        """(extension) AttnLRP for several CLASSES of the same batch from ONE forward pass and one chain with a class axis: the
        class arguments, ``chunk``, the result and its bit-for-bit statement as in LRP.generate_attnlrp_classes; the map is
        fp32 [B,K,N], ``maps["attnlrp"][:, k]`` the bits of generate_attnlrp(input_ids, attention_mask, index=classes[:, k],
        eps).  The refusals of generate_attnlrp (there is no ``head_mask`` argument), a bad ``chunk`` and a bad class request
        are raised before the forward pass."""
        with _x6_bracket(input_ids):
            _check_chunk(chunk)
            _refuse_attnlrp(self.model, eps, None, input_ids, cast=(attention_mask,))
            request = _ClassRequest(classes, topk, seeds)
            request.check(input_ids.shape[0], _num_classes(self.model), torch.float32, input_ids.device)
            with torch.no_grad():
                output = self.model(input_ids=input_ids, attention_mask=attention_mask)[0]
                _drop_rule_planes(self.model)
                cls, scores, seed_stack = request.targets(output)
                chain = lambda seed: self.model.attnlrp(seed, eps=eps)      # noqa: E731
                maps = self._gradients_and_chain(output, [], lambda: _attnlrp_class_chain(chain, seed_stack, chunk))
            return ClassMaps(cls, scores, {"attnlrp": maps})

    def attribution_tail(self, start_layer=11):
        """ExplanationGenerator.py:47-59 on the attn_cam / attention gradients cached by relprop + backward."""
        return lrp_tail(self.model, start_layer, self.prune)

    def generate_LRP_last_layer(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:62-84: head-mean of the last layer's attn_cam, CLS row, CLS slot zeroed."""
        self._pass(input_ids, attention_mask, index, lowest_layer=self._last_layer(), head_mask=head_mask)
        return lrp_last_layer_tail(self.model)

    def generate_full_lrp(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:86-106: relevance propagated to the encoder input, summed over the hidden
        dimension, CLS slot zeroed.  Never pruned: it reads the relevance below the lowest layer."""
        # relprop reads the attention gradients nowhere, but the reference runs the backward first (:100-101) and the
        # accessors are part of the boundary: keep them populated
        return full_lrp_tail(self._pass(input_ids, attention_mask, index, prune=False, head_mask=head_mask)[1])

    def generate_attn_last_layer(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:108-114: head-mean of the last layer's attention probabilities, CLS row."""
        self._pass(input_ids, attention_mask, index, grads=None, relprop=False, head_mask=head_mask)
        return attn_last_layer_tail(self.model)

    def generate_rollout(self, input_ids, attention_mask, start_layer=0, index=None, head_mask=None):
        """ExplanationGenerator.py:116-127: row-normalised rollout of the head-averaged attention probabilities."""
        self._pass(input_ids, attention_mask, index, grads=None, relprop=False, head_mask=head_mask)
        return rollout_tail(self.model, start_layer)

    def generate_attn_gradcam(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:129-155: last layer's attention x its per-head mean gradient, head-mean, clamped,
        min-max normalised over the whole [N, N] map, CLS row with the CLS slot zeroed."""
        self._pass(input_ids, attention_mask, index, lowest_layer=self._last_layer(), head_mask=head_mask)
        return attn_gradcam_tail(self.model)

    def generate_head_relevance(self, input_ids, attention_mask, index=None, head_mask=None):
        """(extension) Per-head relevance in the sense of Voita et al. 2019: fp64 [B, L, H], entry (b, l, h) the sum of the
        relevance that arrives at head h's slice of layer l's context layer (``cam`` at the top of
        BertSelfAttention.relprop).  One forward pass and one relprop chain; no backward pass.  ``head_mask``: the scores of
        the masked model."""
        with torch.no_grad():
            output = self.model(input_ids=input_ids, attention_mask=attention_mask, **_masked(head_mask))[0]
        one_hot = _one_hot(output, index)
        return _head_relevance_chain([lay.attention.self for lay in self.model.bert.encoder.layer],
                                     lambda: self.model.relprop(one_hot, alpha=1))


# ----------------------------------------------------------------------------------------------------------------------
# The tails of the Generator methods as functions of the BERT model with its populated caches (the generate_* methods
# call them; Generator.generate_all serves several from one pass).
def lrp_tail(model, start_layer=11, pruned=False):
    """ExplanationGenerator.py:47-59 on the attn_cam / attention gradients cached by relprop + backward.  pruned: the
    pass served the layers >= start_layer only."""
    layers = model.bert.encoder.layer
    first = layers[-1].attention.self.get_attn_cam()
    B, _, N, _ = first.shape
    stack = torch.empty((len(layers), B, N, N), dtype=first.dtype, device=first.device)
    for i, lay in enumerate(layers):
        sa = lay.attention.self
        if i >= start_layer or not pruned:            # (the rollout reads layers >= start_layer only)
            ops.gradcam_headmean(sa.get_attn_gradients(), sa.get_attn_cam(), out=stack[i])
    # ExplanationGenerator.py:7-18 (row-normalised rollout) + :58 (CLS fix-up) -> row 0
    return ops.rollout(stack, start_layer=start_layer, normalise=True, cls_fixup=True, row0_only=True)


def lrp_last_layer_tail(model):
    cam = model.bert.encoder.layer[-1].attention.self.get_attn_cam().clamp(min=0).mean(dim=1)[:, 0].clone()
    cam[:, 0] = 0
    return cam


def full_lrp_tail(cam):
    """``cam``: what model.relprop returned (the relevance of the encoder input)."""
    cam = cam.sum(dim=2)
    cam[:, 0] = 0
    return cam


def attn_last_layer_tail(model):
    with torch.no_grad():
        attn = model.bert.encoder.layer[-1].attention.self.get_attn()
        if ops._is_bf16(attn):           # fp32 map of a bf16 model: the class-token row's head mean, summed in fp32
            cam = ops.attn_headmean(attn, row0=True)
        else:
            cam = attn.mean(dim=1)[:, 0].clone()
    cam[:, 0] = 0
    return cam


def rollout_tail(model, start_layer=0):
    with torch.no_grad():
        stack = _headmean_stack([lay.attention.self.get_attn() for lay in model.bert.encoder.layer])
        joint = ops.rollout(stack, start_layer=start_layer, normalise=True)
    out = joint[:, 0].clone()
    out[:, 0] = 0
    return out


def attn_gradcam_tail(model):
    sa = model.bert.encoder.layer[-1].attention.self
    # (a bf16 model: evaluated in fp32 on its attention and gradient, like the relprop maps; a no-op for fp32)
    cam = sa.get_attn().detach().float()
    grad = sa.get_attn_gradients().float().mean(dim=[2, 3], keepdim=True)
    cam = (cam * grad).mean(dim=1).clamp(min=0)
    lo = cam.amin(dim=(1, 2), keepdim=True)
    hi = cam.amax(dim=(1, 2), keepdim=True)
    cam = ((cam - lo) / (hi - lo))[:, 0].clone()
    cam[:, 0] = 0
    return cam
