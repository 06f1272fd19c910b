"""Explanation generators: mirrors of baselines/ViT/ViT_explanation_generator.py (LRP) and
BERT_explainability/modules/BERT/ExplanationGenerator.py (Generator) of the reference.

Same method names and arguments; differences (results identical at batch 1):
  * a batch of B inputs is explained in one pass (B independent samples) -> [B, N-1] / [B, N]
  * the class index defaults to the per-sample argmax, computed on the device (no D2H round trip)
  * the attention gradients are obtained with torch.autograd.grad w.r.t. the attention tensors only,
    so no weight gradients are computed (the reference's loss.backward() computes and discards them)
"""
from __future__ import annotations

import numpy as np
import torch

from . import methods as M
from . import ops
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


def _attention_gradients(loss, attn_modules):
    """Attention gradients of the listed modules (lowest block first), nothing else: no weight gradients, nothing below
    the lowest listed block."""
    anchors = [getattr(m, "_fused_anchor", None) for m in attn_modules]
    if anchors and all(a is not None for a in anchors):
        # producer kernels (vit._FusedAttention): the gradient w.r.t. the probabilities is formed inside the block's
        # own backward and handed to save_attn_gradients; drive autograd down to the lowest block's qkv activation and
        # tell that block that nothing consumes its d_qkv
        lowest = attn_modules[0]
        lowest._fused_stop_backward = True
        try:
            torch.autograd.grad(loss, [anchors[0]], retain_graph=False, allow_unused=True)
        finally:
            lowest._fused_stop_backward = False
        return
    if any(a is not None for a in anchors):
        raise ops._lib.TeError("attention gradients: some of the listed blocks ran on the producer kernels and some on "
                               "stock PyTorch (a frozen qkv layer, or a block in train mode?); the gradient driver "
                               "handles one kind per pass -- set ops.USE_FUSED_PRODUCERS = False for this model")
    attns = [m.get_attn() for m in attn_modules]
    grads = torch.autograd.grad(loss, attns, retain_graph=False, allow_unused=False)
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


class LRP:
    """baselines/ViT/ViT_explanation_generator.py:20-41.  Batched: B inputs -> B maps (B = 1 is the reference's call).

    (The round-1 ``streams`` extension -- micro-batches on separate HIP streams -- is gone: it stopped making progress at
    batch 64 for reasons never diagnosed, and since round 3 the Linear rules run on persistent whole-chip kernels that
    two streams could only serialise.)"""

    def __init__(self, model, overlap_backward=False, prune=False):
        self.model = model
        self.model.eval()
        # (extension) the relprop chain reads only forward caches; the attention gradients are needed by the tail
        # alone.  With overlap_backward the backward pass (main stream) and the relprop rules (side stream) run
        # concurrently and join before the head-mean / rollout tail: the memory-bound backward kernels and the tails
        # of the MFMA-bound Linear.relprop launches fill each other's idle CUs.  Same kernels, same results.
        self.overlap_backward = bool(overlap_backward)
        self._relprop_stream = None
        # (extension, off by default) only the blocks >= start_layer contribute to a transformer_attribution map: skip
        # the relprop rules and the attention-gradient backward below them (model.prune_below_start_layer)
        self.prune = bool(prune)

    def generate_LRP(self, input, index=None, method="transformer_attribution", is_ablation=False, start_layer=0,
                     head_mask=None):
        # head_mask (extension): one value per head, [H], [L,H] or [L,B,H] (VisionTransformer.get_head_mask)
        # a lost x6 hand-over of an EARLIER call is raised here, once, without synchronising (ops.x6_poll); NaN in a map
        # means exactly that -- check() asks about the calls made so far (and synchronises)
        if input.is_cuda:
            ops.x6_poll(input.device)
        out = self._generate(input, index, method, is_ablation, start_layer, head_mask)
        if input.is_cuda:
            ops.x6_post(input.device)
        return out

    def check(self):
        """Raise TeError if any x6 Linear kernel since the last check lost a stream-K hand-over (the affected maps carry
        NaN).  Synchronises the device: call it where the maps are read back anyway, never inside a step."""
        ops.x6_raise_if_failed(next(self.model.parameters()).device)

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
        if input.is_cuda:
            ops.x6_poll(input.device)
        out = self._generate_all(input, wanted, index, is_ablation, start_layer, head_mask)
        if input.is_cuda:
            ops.x6_post(input.device)
        return out

    def _generate_all(self, input, wanted, index, is_ablation, start_layer, head_mask=None):
        need = M.needs(wanted, M.LRP_NEEDS, is_ablation, M.LRP_ABLATION_NEEDS)
        model = self.model
        with ops.gelu_backward_plane_handoff():      # this call drives the backward pass itself (attention tensors only)
            output = model(input, **_masked(head_mask))
        ours = tuple(m for m in wanted if m not in M.BASELINE_METHODS)       # the tails of model.relprop
        maps = {}
        if not need.forward_only:
            kwargs = {"alpha": 1}
            one_hot = _one_hot(output, index)
            loss = torch.sum(one_hot * output)
            # as in _generate: the flag is set for THIS call only
            user_flag = model.prune_below_start_layer
            pruned = bool((self.prune or user_flag) and need.relprop and M.prunable(wanted, M.LRP_NEEDS))
            model.prune_below_start_layer = pruned
            blocks = list(model.blocks)
            grad_blocks = blocks[start_layer if pruned else 0:] if need.all_grads else blocks[-1:] if need.last_grad else []
            try:
                if need.relprop and self.overlap_backward and input.is_cuda:
                    maps = self._relprop_beside_backward(loss, one_hot, ours, is_ablation, start_layer, kwargs, grad_blocks)
                else:
                    if grad_blocks:
                        _attention_gradients(loss, [blk.attn for blk in grad_blocks])
                    if need.relprop:
                        maps = model.relprop(one_hot, method=ours, is_ablation=is_ablation, start_layer=start_layer,
                                             **kwargs)
            finally:
                model.prune_below_start_layer = user_flag
        if not need.relprop:                         # ("last_layer_attn": the forward pass has produced all it reads)
            maps = {m: relprop_tail(model, m, None, is_ablation, start_layer) for m in ours}
        if "attn_rollout" in wanted:
            maps["attn_rollout"] = attn_rollout_tail(model, start_layer)
        if "attn_gradcam" in wanted:
            maps["attn_gradcam"] = cam_attn_tail(model)
        return {m: maps[m] for m in wanted}

    def generate_head_relevance(self, input, index=None, head_mask=None):
        """(extension) Per-head relevance in the sense of Voita et al. 2019: fp64 [B, L, H], entry (b, l, h) the sum of the
        relevance that arrives at head h's slice of block l's context layer (the argument of Attention.relprop_after_proj).
        One forward pass and one relprop chain; no backward pass, no map.  ``head_mask`` as in generate_LRP: the scores of
        the masked model."""
        model = self.model
        with torch.no_grad():
            output = model(input, **_masked(head_mask))
        one_hot = _one_hot(output, index)
        user_flag = model.prune_below_start_layer      # the whole chain runs, whatever the model's prune flag says
        model.prune_below_start_layer = False
        try:
            return _head_relevance_chain([blk.attn for blk in model.blocks],
                                         lambda: model.relprop(one_hot, method=(), alpha=1))
        finally:
            model.prune_below_start_layer = user_flag

    def _generate(self, input, index, method, is_ablation, start_layer, head_mask=None):
        _refuse_before_forward(input, (method,))
        with ops.gelu_backward_plane_handoff():      # this call drives the backward pass itself (attention tensors only)
            output = self.model(input, **_masked(head_mask))
        kwargs = {"alpha": 1}
        one_hot = _one_hot(output, index)
        loss = torch.sum(one_hot * output)
        prune = self.prune and method in ("transformer_attribution", "grad")
        # the flag is set for THIS call only: a user's own setting of model.prune_below_start_layer (and direct
        # model.relprop calls afterwards) are unaffected
        user_flag = self.model.prune_below_start_layer
        self.model.prune_below_start_layer = prune or (user_flag and method in ("transformer_attribution", "grad"))
        grad_blocks = list(self.model.blocks)[start_layer if self.model.prune_below_start_layer else 0:]
        try:
            if self.overlap_backward and input.is_cuda:
                return self._relprop_beside_backward(loss, one_hot, method, is_ablation, start_layer, kwargs, grad_blocks)
            _attention_gradients(loss, [blk.attn for blk in grad_blocks])
            return self.model.relprop(one_hot, method=method, is_ablation=is_ablation, start_layer=start_layer,
                                      **kwargs)
        finally:
            self.model.prune_below_start_layer = user_flag

    def _relprop_beside_backward(self, loss, one_hot, method, is_ablation, start_layer, kwargs, grad_blocks):
        dev = one_hot.device
        main = torch.cuda.current_stream(dev)
        if self._relprop_stream is None:
            self._relprop_stream = torch.cuda.Stream(device=dev)
        side = self._relprop_stream
        side.wait_stream(main)                      # forward caches + one-hot are complete
        # backward on the main stream (autograd runs each node on its forward op's stream)
        if grad_blocks:
            _attention_gradients(loss, [blk.attn for blk in grad_blocks])
        grads_ready = main.record_event()
        self.model._before_tail = lambda: torch.cuda.current_stream(dev).wait_event(grads_ready)
        try:
            with torch.cuda.stream(side):
                out = self.model.relprop(one_hot, method=method, is_ablation=is_ablation, start_layer=start_layer,
                                         **kwargs)
        finally:
            self.model._before_tail = None
        main.wait_stream(side)
        if not torch.cuda.is_current_stream_capturing():
            for t in (out.values() if isinstance(out, dict) else (out,)):     # (generate_all: a dict of maps)
                if t is not None:
                    t.record_stream(main)
        return out


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
        if index is not None and not torch.is_tensor(index):
            index = torch.as_tensor(np.asarray(index), device=example_input.device)
        self.lrp = lrp
        self.static_in = example_input.clone()
        self.static_index = None if index is None else index.clone()
        args = (self.static_in, self.static_index, method, is_ablation, start_layer)
        side = torch.cuda.Stream(device=example_input.device)
        side.wait_stream(torch.cuda.current_stream(example_input.device))
        with torch.cuda.stream(side):          # warm-up off the capture: library handles, MIOpen find, allocator
            for _ in range(max(1, warmup)):
                lrp._generate(*args)
        torch.cuda.current_stream(example_input.device).wait_stream(side)
        torch.cuda.synchronize(example_input.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_out = lrp._generate(*args)

    def __call__(self, input, index=None):
        if input.shape != self.static_in.shape:
            raise RuntimeError(f"GraphedLRP was captured for {tuple(self.static_in.shape)}, got {tuple(input.shape)}")
        self.static_in.copy_(input)
        if self.static_index is not None and index is not None:
            self.static_index.copy_(torch.as_tensor(index, device=self.static_index.device).reshape(self.static_index.shape))
        self.graph.replay()
        return self.static_out


class Generator:
    """BERT_explainability/modules/BERT/ExplanationGenerator.py:20-59 (generate_LRP)."""

    def __init__(self, model, prune=False, overlap_backward=False):
        self.model = model
        self.model.eval()
        # (extension, as LRP.overlap_backward) the relprop rules read forward caches only: run them on a side stream beside
        # the attention-gradient backward pass; both streams join before anything reads attn_cam / the gradients.  Same
        # kernels, same results, bit for bit.
        self.overlap_backward = bool(overlap_backward)
        self._relprop_stream = None
        # (extension, off by default) generate_LRP reads attn_cam / attention gradients of the layers >= start_layer
        # only (ExplanationGenerator.py:47-57) -- with the reference's default start_layer = 11 that is the LAST layer
        # alone, yet relevance and gradients are propagated through all twelve.  prune=True stops the relprop right
        # after layer start_layer's attn_cam is stored and asks autograd for the gradients of those layers only: the
        # same vector bit for bit; get_attn_cam() of the layers below is then not refreshed.
        self.prune = bool(prune)

    def forward(self, input_ids, attention_mask):
        return self.model(input_ids, attention_mask)

    def check(self):
        """As LRP.check(): raise if an x6 Linear kernel lost a hand-over since the last check (synchronises)."""
        ops.x6_raise_if_failed(next(self.model.parameters()).device)

    def _explain(self, input_ids, attention_mask, index, lowest_layer=0, head_mask=None):
        """forward, attention-gradient backward, relprop.  With prune=True only the layers >= lowest_layer are served."""
        return self._pass(input_ids, attention_mask, index, lowest_layer, head_mask=head_mask)[0]

    def _pass(self, input_ids, attention_mask, index, lowest_layer=0, grads="all", relprop=True, prune=None,
              head_mask=None):
        """One pass: forward; the attention gradients of ``grads`` ("all": the layers served, "last": the last layer
        alone, None: no backward pass); the relprop chain if ``relprop``.  prune (default: self.prune): only the layers
        >= lowest_layer are served.  -> (the encoder layers, what model.relprop returned or None)."""
        from .rules import StopRelprop
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
        side = main = None
        if relprop and self.overlap_backward and one_hot.is_cuda:
            main = torch.cuda.current_stream(one_hot.device)
            if self._relprop_stream is None:
                self._relprop_stream = torch.cuda.Stream(device=one_hot.device)
            side = self._relprop_stream
            side.wait_stream(main)                  # forward caches + one-hot are complete
        grad_layers = list(layers)[first:] if grads == "all" else list(layers)[-1:] if grads == "last" else []
        if grad_layers:
            _attention_gradients(loss, [lay.attention.self for lay in grad_layers])      # main stream
        if not relprop:
            return layers, None
        stop_at = layers[first].attention.self if prune else None
        if stop_at is not None:
            stop_at._stop_after_attn_cam = True
        cam = None
        try:
            if side is not None:
                with torch.cuda.stream(side):
                    cam = self.model.relprop(one_hot, alpha=1)
            else:
                cam = self.model.relprop(one_hot, alpha=1)
        except StopRelprop:
            pass
        finally:
            if stop_at is not None:
                stop_at._stop_after_attn_cam = False
            if side is not None:
                main.wait_stream(side)              # the tail (head-mean, rollout) reads both streams' results
        if cam is not None and side is not None and not torch.cuda.is_current_stream_capturing():
            cam.record_stream(main)
        return layers, cam

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
        if input_ids.is_cuda:
            ops.x6_poll(input_ids.device)        # a lost x6 hand-over of an earlier call: raised once, no synchronisation
        n_layers = len(self.model.bert.encoder.layer)
        pruned = bool(self.prune and M.prunable(wanted, M.GENERATOR_NEEDS))
        lowest = start_layer if "LRP" in wanted else n_layers - 1
        _, cam = self._pass(input_ids, attention_mask, index, lowest_layer=lowest,
                            grads="all" if need.all_grads else "last" if need.last_grad else None,
                            relprop=need.relprop, prune=pruned, head_mask=head_mask)
        tails = {"LRP": lambda: lrp_tail(self.model, start_layer, pruned),
                 "LRP_last_layer": lambda: lrp_last_layer_tail(self.model),
                 "full_lrp": lambda: full_lrp_tail(cam),
                 "attn_last_layer": lambda: attn_last_layer_tail(self.model),
                 "rollout": lambda: rollout_tail(self.model, rollout_start_layer),
                 "attn_gradcam": lambda: attn_gradcam_tail(self.model)}
        out = {m: tails[m]() for m in wanted}
        if input_ids.is_cuda:
            ops.x6_post(input_ids.device)
        return out

    def generate_LRP(self, input_ids, attention_mask, index=None, start_layer=11, head_mask=None):
        # head_mask (the model's own argument, BERT.py:556-625): one value per head, [H], [L,H] or, per sample, [L,B,H]
        if input_ids.is_cuda:
            ops.x6_poll(input_ids.device)        # a lost x6 hand-over of an earlier call: raised once, no synchronisation
        self._explain(input_ids, attention_mask, index, lowest_layer=start_layer, head_mask=head_mask)
        out = self.attribution_tail(start_layer)
        if input_ids.is_cuda:
            ops.x6_post(input_ids.device)
        return out

    def attribution_tail(self, start_layer=11):
        """ExplanationGenerator.py:47-59 on the attn_cam / attention gradients cached by relprop + backward."""
        return lrp_tail(self.model, start_layer, self.prune)

    def generate_LRP_last_layer(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:62-84: head-mean of the last layer's attn_cam, CLS row, CLS slot zeroed."""
        self._explain(input_ids, attention_mask, index, lowest_layer=len(self.model.bert.encoder.layer) - 1,
                      head_mask=head_mask)
        return lrp_last_layer_tail(self.model)

    def generate_full_lrp(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:86-106: relevance propagated to the encoder input, summed over the hidden
        dimension, CLS slot zeroed."""
        with ops.gelu_backward_plane_handoff():      # this call drives the backward pass itself (attention tensors only)
            output = self.model(input_ids=input_ids, attention_mask=attention_mask, **_masked(head_mask))[0]
        one_hot = _one_hot(output, index)
        layers = self.model.bert.encoder.layer
        # relprop reads the attention gradients nowhere, but the reference runs the backward first (:100-101) and the
        # accessors are part of the boundary: keep them populated
        _attention_gradients(torch.sum(one_hot * output), [lay.attention.self for lay in layers])
        return full_lrp_tail(self.model.relprop(one_hot, alpha=1))

    def generate_attn_last_layer(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:108-114: head-mean of the last layer's attention probabilities, CLS row."""
        with torch.no_grad():
            self.model(input_ids=input_ids, attention_mask=attention_mask, **_masked(head_mask))
        return attn_last_layer_tail(self.model)

    def generate_rollout(self, input_ids, attention_mask, start_layer=0, index=None, head_mask=None):
        """ExplanationGenerator.py:116-127: row-normalised rollout of the head-averaged attention probabilities."""
        with torch.no_grad():
            self.model(input_ids=input_ids, attention_mask=attention_mask, **_masked(head_mask))
        return rollout_tail(self.model, start_layer)

    def generate_attn_gradcam(self, input_ids, attention_mask, index=None, head_mask=None):
        """ExplanationGenerator.py:129-155: last layer's attention x its per-head mean gradient, head-mean, clamped,
        min-max normalised over the whole [N, N] map, CLS row with the CLS slot zeroed."""
        self._explain(input_ids, attention_mask, index, lowest_layer=len(self.model.bert.encoder.layer) - 1,
                      head_mask=head_mask)
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
