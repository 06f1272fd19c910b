"""Relprop rule classes -- host-side mirror of the reference's rule library, backed by HIP kernels.

Same class names, constructor signatures, ``forward`` behaviour, ``self.X`` / ``self.Y`` state
convention and ``relprop(R, alpha)`` signature as modules/layers_ours.py (variant "ours") and
modules/layers_lrp.py (variant "lrp") of the reference, and their BERT copies
(BERT_explainability/modules/layers_ours.py, layers_lrp.py: + MatMul, Mul, Tanh).  The reference
evaluates each rule with ``torch.autograd.grad`` on a re-built micro-graph (layers_ours.py:41-43);
here ``relprop`` calls one fused closed-form kernel through the C ABI (include/te_relprop.h).

Batch semantics: the reference is batch-1 only; a batch of B samples is B independent batch-1
problems (Add's "whole tensor" sums are per sample).  With B = 1 the results match the reference.

Off the accelerated hot path ("API surface"): BatchNorm2d / pools / Cat / AddEye keep their
forward so models build and run, but their relprop raises NotImplementedError here; so does Mul for every product other
than the head mask of an attention layer (csrc/te_headmask.hip).
Conv2d.relprop (method="full": the patch embedding's z^B rule, layers_ours.py:256-286) is implemented
(csrc/te_conv.hip).
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn

from . import ops

__all__ = ['forward_hook', 'Clone', 'Add', 'Cat', 'ReLU', 'GELU', 'Dropout', 'BatchNorm2d', 'Linear', 'MaxPool2d',
           'AdaptiveAvgPool2d', 'AvgPool2d', 'Conv2d', 'Sequential', 'safe_divide', 'einsum', 'Softmax',
           'IndexSelect', 'LayerNorm', 'AddEye', 'Tanh', 'MatMul', 'Mul']


def safe_divide(a, b):
    """modules/layers_ours.py:10-13 (plain torch; host-side helper, not used by the kernels)."""
    den = b.clamp(min=1e-9) + b.clamp(max=1e-9)
    den = den + den.eq(0).type(den.type()) * 1e-9
    return a / den * b.ne(0).type(b.type())


def forward_hook(self, input, output):
    """Capture the detached input(s) as self.X and the output as self.Y (layers_ours.py:16-27).
    No copy is made: detach() aliases the activation the forward pass produced."""
    if type(input[0]) in (list, tuple):
        self.X = [i.detach() for i in input[0]]
    else:
        self.X = input[0].detach()
    self.Y = output
    # the rules that take Z from the cached forward output (Linear, einsum, MatMul) only do so while that tensor
    # -- and the weight that produced it -- are exactly what the forward pass wrote (see _cached_y)
    self._y_version = output._version if torch.is_tensor(output) else None
    w = getattr(self, "weight", None)
    b = getattr(self, "bias", None)
    self._w_version = (w._version if torch.is_tensor(w) else None, b._version if torch.is_tensor(b) else None)


class StopRelprop(Exception):
    """Raised by an attention module whose ``_stop_after_attn_cam`` flag is set, right after it stored its attn_cam:
    the model-level relprop loop catches it (extension: ``prune_below_start_layer``, see vit.VisionTransformer)."""


@contextlib.contextmanager
def stop_after_attn_cam(attn_module):
    """While open, ``attn_module`` raises StopRelprop once its attn_cam is stored (None: no module does).  The flag is reset
    however the chain ends; catching StopRelprop stays with the caller, who knows what a stopped chain returns."""
    if attn_module is not None:
        attn_module._stop_after_attn_cam = True
    try:
        yield
    finally:
        if attn_module is not None:
            attn_module._stop_after_attn_cam = False


def _cached_y(module):
    """The forward output forward_hook stored (the product whose rule is being evaluated), or None.

    self.Y is the LIVE output tensor (an alias, like the reference's), so an in-place op after the layer
    (``ReLU(inplace=True)``, ``x += ...``) or an optimizer step on the weight would silently change what Z is derived
    from, whereas the reference recomputes Z from X and W.  forward_hook records the tensors' version counters; a
    mismatch means "modified since the forward pass" and the rule falls back to recomputing Z itself."""
    y = getattr(module, "Y", None)
    if not torch.is_tensor(y) or getattr(module, "_y_version", None) != y._version:
        return None
    w = getattr(module, "weight", None)
    b = getattr(module, "bias", None)
    now = (w._version if torch.is_tensor(w) else None, b._version if torch.is_tensor(b) else None)
    if getattr(module, "_w_version", now) != now:
        return None
    return y


class RelProp(nn.Module):
    variant = "ours"

    def __init__(self):
        super(RelProp, self).__init__()
        self.register_forward_hook(forward_hook)

    def relprop(self, R, alpha):
        return R

    def attnlrp(self, G, eps):
        """(extension) The module's AttnLRP rule (te_relprop.h, section "AttnLRP") on G, the relevance per unit of this
        module's output, from the tensors forward_hook cached -> G of its input."""
        raise NotImplementedError(f"{type(self).__name__}.attnlrp: AttnLRP has no rule for this module")


class _Identity(RelProp):
    """Rules that pass relevance through unchanged (layers_ours.py:67-80,86-87) need no cached input."""


def _no_cache_hook(self, input, output):
    self.Y = output


class ReLU(nn.ReLU, RelProp):
    pass


class GELU(nn.GELU, RelProp):
    def feeds(self, linear):
        """Model code may name the Linear layer this activation's output goes to (vit.Mlp, bert.BertLayer): the producer
        then emits that layer's operand planes itself (producers._Gelu).  A hint only -- the consumer checks that the planes
        belong to the tensor it received.  Kept in a tuple: not a registered submodule, and copy / pickle follow it."""
        self.__dict__["_te_feeds"] = (linear,)
        return self

    def forward(self, x):
        from . import producers                      # 8f.1: csrc/te_norm_act.hip behind ops.USE_FUSED_PRODUCERS
        if getattr(self, "approximate", "none") == "none" and not self.training and producers.gelu_usable(x):
            nxt = self.__dict__.get("_te_feeds", (None,))[0]
            return producers.gelu(x, nxt, x6_cache(nxt) if isinstance(nxt, Linear) else None)
        return super().forward(x)

    def attnlrp(self, G, eps):
        if getattr(self, "approximate", "none") != "none":
            raise NotImplementedError("GELU.attnlrp: the identity rule is implemented for the exact (erf) GELU")
        return ops.alrp_act(G, self.X, "gelu")


class Softmax(nn.Softmax, RelProp):
    pass


class LayerNorm(nn.LayerNorm, RelProp):
    def forward(self, x):
        from . import producers
        if producers.norm_usable(x, self):
            return producers.layer_norm(x, self)
        return super().forward(x)

    def attnlrp(self, G, eps):
        """rstd held constant (from the cached input and the layer's own eps); no damping: ``eps`` is not read."""
        if len(self.normalized_shape) != 1:
            raise NotImplementedError("LayerNorm.attnlrp: normalisation over the last dimension only")
        gamma = self.weight if self.weight is not None else torch.ones(self.normalized_shape, device=G.device)
        return ops.alrp_layernorm(G, gamma, ops.alrp_row_rstd(self.X, self.eps))


class Dropout(nn.Dropout, RelProp):
    pass


class Tanh(nn.Tanh, RelProp):
    def attnlrp(self, G, eps):
        return ops.alrp_act(G, self.X, "tanh")


# ------------------------------------------------------------------------------------------ hot path
def x6_cache(module) -> dict:
    """Per-layer store of derived operands that outlive one relprop call (the bf16 planes of the weight,
    ops.x6_weight_planes); not part of the state dict."""
    c = module.__dict__.get("_te_cache")
    if c is None:
        c = module.__dict__["_te_cache"] = {}
    return c


class _ScratchCache:
    """Mixin of the layers that keep derived weight planes (Linear, Conv2d)."""

    # The derived operand planes (x6_cache) are device scratch, not state: they are rebuilt on demand, so they are kept out of
    # pickling / deepcopy / torch.save(model), and dropped whenever the parameters are replaced wholesale.
    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_te_cache", None)
        return state

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        ops.x6_invalidate(self)

    def _apply(self, fn, *args, **kwargs):
        ops.x6_invalidate(self)
        return super()._apply(fn, *args, **kwargs)


class Linear(_ScratchCache, nn.Linear, RelProp):
    """layers_ours.py:207-230 / layers_lrp.py:188-211 -> te_linear_relprop_f32."""

    def forward(self, x):
        from . import producers                      # 8f.1: forward and / or input gradient on te_gemm_x6_f32
        plan = producers.linear_plan(x, self)
        if not plan[0]:      # no x6 forward product of THIS input: nothing may wait for it, nothing for the rule to reuse
            ops.drop_x_planes(x6_cache(self), with_abs=True)
        if plan[0] or plan[1]:
            return producers.linear(x, self, x6_cache(self), plan)
        return super().forward(x)

    def relprop(self, R, alpha):
        return linear_rule(self, R, alpha)

    def attnlrp(self, G, eps):
        """G_x = damp(G_y, y) W on the cached output y (bias included).  G [K, *y.shape] (a class axis): fp32, one damp with
        classes and ONE product over the K T rows; bf16, K calls of the fused damp-and-product on the slices."""
        Y = self.Y.detach()
        classes = G.dim() == Y.dim() + 1
        if (G.shape[1:] if classes else G.shape) != Y.shape:
            raise ops._lib.TeError(f"Linear.attnlrp: G {tuple(G.shape)} does not have the shape of the cached output "
                                   f"{tuple(Y.shape)}")
        if ops._is_bf16(self.weight):      # damp and product in one call: the damped G goes to the product as bf16 planes
            return ops.alrp_linear(G, self.weight, x6_cache(self), Y=Y, eps=eps)
        return ops.alrp_linear(ops.alrp_damp(G, Y, eps), self.weight, x6_cache(self))


def linear_rule(m, R, alpha, rows=None, variant=None):
    """The one route from a Linear layer `m` to ops.linear_relprop.  m.Y (the forward output, cached by forward_hook like
    the reference does) lets the kernel derive Z = X+ W+^T + X- W-^T from one product instead of two -- while it is what
    the forward pass wrote (_cached_y) and has X's rows.  rows: a selector applied to X and Y (``t[:, :1]``: the cls slice
    of Block.relprop_cls_only / BertLayer.relprop_cls_only, which also pass the variant their other rules run under).
    The layer's scratch dict carries the operand planes its forward product left for this rule: the signed planes of X, which
    ops.linear_relprop hands to the kernel with TE_X6_X_PLANES_SIGNED (or, ops.X6_SIGNED_PLANES off, the planes of |X|)."""
    X, Y = m.X, _cached_y(m)
    if Y is not None and Y.shape[:-1] != X.shape[:-1]:
        Y = None
    if rows is not None:
        X, Y = rows(X), None if Y is None else rows(Y)
    return ops.linear_relprop(R, X, m.weight.detach(), alpha=alpha, variant=variant or m.variant, Y=Y, bias=m.bias,
                              cache=x6_cache(m))


class Add(RelProp):
    """layers_ours.py:97-120 (ours) / layers_lrp.py:98-100 (lrp) -> te_add_relprop_f32 /
    te_add_bcast_relprop_f32 (broadcast mask operand of BERT self-attention)."""

    def forward(self, inputs):
        return torch.add(*inputs)

    def relprop(self, R, alpha, deferred=False):
        # deferred=True (model-internal call sites only): the per-sample rescale of layers_ours.py:117-118 travels with
        # the two outputs as an ``ops.Deferred`` and is applied inside the consuming Clone / Linear kernels -- the
        # rule then streams its operands once instead of twice; ``.materialise()`` is bitwise the plain result
        x0, x1 = self.X
        bcast_mask = x0.dim() == 4 and x1.dim() == 4 and x1.shape[1] == 1 and x1.shape[2] == 1       # BERT.py:386-388
        a, b = ops.add_relprop(R, x0, x1, variant=self.variant,
                               deferred=deferred and ops.USE_DEFERRED_ADD and (x0.shape == x1.shape or bcast_mask))
        return [a, b]

    def attnlrp(self, G, eps):
        """A residual Add o = a + b: both operands receive damp(G_o, o) -- ONE tensor is returned."""
        return ops.alrp_damp(G, self.Y.detach(), eps)


class einsum(RelProp):
    """layers_ours.py:122-127 (RelPropSimple) for the two attention products."""

    def __init__(self, equation):
        super().__init__()
        self.equation = equation

    def forward(self, *operands):
        ops_ = operands[0] if (len(operands) == 1 and isinstance(operands[0], (list, tuple))) else operands
        eq = self.equation.replace(" ", "")
        # the two attention products as plain batched matmuls: torch.einsum materialises k^T first (a [B,H,D,N] copy
        # per block); matmul hands the transposed strides to the BLAS
        if eq == 'bhid,bhjd->bhij' and len(ops_) == 2:
            return torch.matmul(ops_[0], ops_[1].transpose(-1, -2))
        if eq == 'bhij,bhjd->bhid' and len(ops_) == 2:
            return torch.matmul(ops_[0], ops_[1])
        return torch.einsum(self.equation, *operands)

    def relprop(self, R, alpha):
        eq = self.equation.replace(" ", "")
        if eq == 'bhij,bhjd->bhid':
            cam_attn, cam_v = ops.matmul_relprop_av(R, self.X[0], self.X[1], variant=self.variant, z=_cached_y(self))
            return [cam_attn, cam_v]
        if eq == 'bhid,bhjd->bhij':
            cam_q, cam_k = ops.matmul_relprop_qk(R, self.X[0], self.X[1], variant=self.variant, z=_cached_y(self))
            return [cam_q, cam_k]
        raise NotImplementedError(f"einsum.relprop: equation {self.equation!r} is not on the accelerated path")


class MatMul(RelProp):
    """BERT_explainability/modules/layers_ours.py:89-91: [probs, V] and [Q, K^T] products."""

    def forward(self, inputs):
        return torch.matmul(*inputs)

    def relprop(self, R, alpha):
        x0, x1 = self.X
        if x0.dim() != 4 or x1.dim() != 4:
            raise NotImplementedError("MatMul.relprop: only [B,H,.,.] attention products are accelerated")
        if x1.stride(-1) != 1 and x1.stride(-2) == 1:          # [Q, K^T] with K^T a transposed view
            k = x1.transpose(-1, -2)
            cam_q, cam_k = ops.matmul_relprop_qk(R, x0, k, variant=self.variant, z=_cached_y(self))
            return [cam_q, cam_k.transpose(-1, -2)]
        if x0.shape[-1] == x0.shape[-2] == x1.shape[-2]:       # [probs, V]
            cam_attn, cam_v = ops.matmul_relprop_av(R, x0, x1, variant=self.variant, z=_cached_y(self))
            return [cam_attn, cam_v]
        if x0.shape[-1] == x1.shape[-2]:                        # [Q, K^T] materialised contiguously
            k = x1.transpose(-1, -2).contiguous()
            cam_q, cam_k = ops.matmul_relprop_qk(R, x0, k, variant=self.variant, z=_cached_y(self))
            return [cam_q, cam_k.transpose(-1, -2)]
        raise NotImplementedError("MatMul.relprop: operand shapes are not an attention product")


def attention_attnlrp(G_o, q, k, v, attn, num_heads, scale, d_q, d_k, d_v):
    """The AttnLRP rule of o = softmax(scale q k^T (+ mask)) v for G_o [B,N,C] ('b n (h d)'): the block's own backward for
    d_out = G_o, written into d_q / d_k / d_v ([B,N,C] views, like q / k / v), which the caller then scales by 1/4, 1/4, 1/2
    (ops.alrp_scale3: the uniform rule).  On te_attention_backward_strided_f32 where it takes the shape, else the torch
    expression of the same backward.  bf16 q / k / v / attn (a bf16 model; G_o and the results stay fp32):
    te_attnlrp_attention_bf16 where ops.alrp_attention_bf16_route says 'bf16', else this function's fp32 routes on exact fp32
    copies of the operands.  Reads cached tensors only: ops.USE_FUSED_PRODUCERS plays no part."""
    B, N, C = G_o.shape
    H, D = num_heads, C // num_heads
    if any(ops._is_bf16(t) for t in (q, k, v, attn)):
        if not all(ops._is_bf16(t) for t in (q, k, v, attn)):
            raise ops._lib.TeError(f"attention_attnlrp: q, k, v and attn must share one dtype, got "
                                   f"{[t.dtype for t in (q, k, v, attn)]}")
        if ops.alrp_attention_bf16_route(N, D) == "bf16":
            ops.alrp_attention_bf16(G_o, q, k, v, attn, H, scale, d_q, d_k, d_v)
        else:
            attention_attnlrp(G_o, q.float(), k.float(), v.float(), attn.float(), H, scale, d_q, d_k, d_v)
        return
    if ops._lib.load().te_attention_strided_supported(N, D):
        ops.attention_backward_qkv(G_o, q, k, v, attn, H, scale, d_q, d_k, d_v, need_qk=True)
        return
    heads = lambda t: t.view(B, N, H, D).permute(0, 2, 1, 3)      # noqa: E731
    go = heads(ops._c(G_o))
    d_attn = torch.matmul(go, heads(v).transpose(-1, -2))
    heads(d_v).copy_(torch.matmul(attn.transpose(-1, -2), go))
    d_s = attn * (d_attn - (d_attn * attn).sum(dim=-1, keepdim=True))
    heads(d_q).copy_(torch.matmul(d_s, heads(k)) * scale)
    heads(d_k).copy_(torch.matmul(d_s.transpose(-1, -2), heads(q)) * scale)


class Clone(RelProp):
    """layers_ours.py:151-169 -> te_clone_relprop_f32."""

    def forward(self, input, num):
        self.__setattr__('num', num)
        return [input for _ in range(num)]

    def relprop(self, R, alpha):
        return ops.clone_relprop(list(R), self.X)

    def attnlrp(self, G, eps):
        """The paths that met at the cloned tensor add their G."""
        G = list(G)
        out = G[0] + G[1]
        for g in G[2:]:
            out += g
        return out


class IndexSelect(RelProp):
    """layers_ours.py:129-147 -> te_index_select_relprop_f32 (dim 1, one index)."""

    def forward(self, inputs, dim, indices):
        self.__setattr__('dim', dim)
        self.__setattr__('indices', indices)
        # a host copy of a single index, taken where it is free: python ints and CPU tensors here, a device tensor
        # once per tensor object (models pass the same buffer every call) -- relprop then never synchronises and is
        # capturable in a HIP graph
        if not torch.is_tensor(indices):
            self._index_host = int(indices)
        elif indices.numel() == 1 and (not indices.is_cuda or getattr(self, "_index_src", None) is not indices
                                       or getattr(self, "_index_version", None) != indices._version):
            # (identity AND version counter: an in-place edit of the index buffer, ``idx.fill_(k)``, refreshes the copy)
            if not (indices.is_cuda and torch.cuda.is_current_stream_capturing()):
                self._index_host = int(indices)
                self._index_src = indices
                self._index_version = indices._version
        return torch.index_select(inputs, dim, indices.reshape(-1) if torch.is_tensor(indices) else indices)

    def relprop(self, R, alpha):
        idx = self.indices
        if self.dim != 1 or self.X.dim() != 3 or (torch.is_tensor(idx) and idx.numel() != 1):
            raise NotImplementedError("IndexSelect.relprop: only dim=1 with a single index is accelerated")
        host = getattr(self, "_index_host", None)
        if host is None or (torch.is_tensor(idx) and (getattr(self, "_index_src", idx) is not idx
                                                      or getattr(self, "_index_version", idx._version) != idx._version)):
            host = int(idx)                                        # (device sync; not capturable)
        return ops.index_select_relprop(R, self.X, host)

    def attnlrp(self, G, eps):
        """Plain gradient of the class-token select: G [B,C] of the selected token -> [B,N,C], zero elsewhere.  G [K,B,C] (a class
        axis: three dimensions, the second the batch) -> [K,B,N,C]."""
        idx = self.indices
        if self.dim != 1 or self.X.dim() != 3 or (torch.is_tensor(idx) and idx.numel() != 1):
            raise NotImplementedError("IndexSelect.attnlrp: only dim=1 with a single index")
        if G.dim() == 3 and G.shape[1] == self.X.shape[0]:
            out = torch.zeros((G.shape[0], *self.X.shape), dtype=G.dtype, device=G.device)
            out.index_copy_(2, idx.reshape(1) if torch.is_tensor(idx) else torch.tensor([int(idx)], device=G.device),
                            G.unsqueeze(2))
            return out
        out = torch.zeros(self.X.shape, dtype=G.dtype, device=G.device)
        out.index_copy_(1, idx.reshape(1) if torch.is_tensor(idx) else torch.tensor([int(idx)], device=G.device),
                        G.reshape(G.shape[0], 1, -1))
        return out


class Sequential(nn.Sequential):
    def relprop(self, R, alpha):
        for m in reversed(self._modules.values()):
            R = m.relprop(R, alpha)
        return R


# ------------------------------------------------------------------------- API surface, off the hot path
class _OffPath(RelProp):
    def relprop(self, R, alpha):
        raise NotImplementedError(f"{type(self).__name__}.relprop is off the accelerated transformer_attribution path")


class Mul(_OffPath):
    """BERT_explainability/modules/layers_ours.py:77-79 (RelPropSimple).  Accelerated: the head mask of BertSelfAttention,
    operands [tensor [B,H,rows,cols], mask broadcastable to [B or 1, H, 1, 1]] (BERT.py:356,375-377) ->
    te_mul_head_relprop_*; returns [relevance of the tensor, None]: the reference discards the mask's relevance, and it
    is not computed here.  Any other product is off the transformer path."""

    def forward(self, inputs):
        return torch.mul(*inputs)

    @staticmethod
    def is_head_mask(x0, x1) -> bool:
        if not (torch.is_tensor(x0) and torch.is_tensor(x1)) or x0.dim() != 4 or x1.dim() != 4:
            return False
        B, H = x0.shape[:2]
        return x1.shape[0] in (1, B) and tuple(x1.shape[1:]) == (H, 1, 1)

    def relprop(self, R, alpha):
        X = getattr(self, "X", None)
        if not isinstance(X, (list, tuple)) or len(X) != 2 or not self.is_head_mask(*X):
            return super().relprop(R, alpha)
        return ops.mul_head_relprop(R, X[0], X[1]), None


def expand_head_mask(head_mask, num_layers: int, num_heads: int, dtype=None, batch_size=None, device=None):
    """``get_head_mask`` of Hugging Face's ModuleUtilsMixin (called at BERT.py:612-616), for the masks the kernels take: one
    value per head.  [H] (every layer alike), [L,H], or -- an extension -- per sample [L,B,H]; any finite values.  Returns
    ``[None] * L`` for None, else a [L, 1 or B, H, 1, 1] tensor in ``dtype`` on ``device`` (Hugging Face casts the mask to the
    model's dtype as well), so that ``mask[i]`` broadcasts against layer i's [B,H,N,N] probabilities.  Any other shape -- the [..,N,N]
    expansion of Hugging Face included -- is a ValueError, raised here, before the forward pass."""
    if head_mask is None:
        return [None] * num_layers
    m = torch.as_tensor(head_mask)
    L, H = num_layers, num_heads
    if m.dim() == 1 and m.shape[0] == H:
        m = m.view(1, 1, H).expand(L, 1, H)
    elif m.dim() == 2 and tuple(m.shape) == (L, H):
        m = m.view(L, 1, H)
    elif m.dim() == 3 and m.shape[0] == L and m.shape[2] == H and (batch_size is None or m.shape[1] in (1, batch_size)):
        pass
    else:
        per_sample = f"[{L},B,{H}]" if batch_size is None else f"[{L},{batch_size},{H}]"
        raise ValueError(f"head_mask must have one value per head: shape [{H}], [{L},{H}] or {per_sample} "
                         f"(layers, samples, heads); got {tuple(m.shape)}")
    if dtype is None:
        dtype = m.dtype if m.is_floating_point() else torch.float32
    return m.to(device=device, dtype=dtype)[..., None, None]


class AddEye(_OffPath):
    def forward(self, input):
        return input + torch.eye(input.shape[2], device=input.device).expand_as(input)


class Cat(_OffPath):
    def forward(self, inputs, dim):
        self.__setattr__('dim', dim)
        return torch.cat(inputs, dim)


class MaxPool2d(nn.MaxPool2d, _OffPath):
    pass


class AdaptiveAvgPool2d(nn.AdaptiveAvgPool2d, _OffPath):
    pass


class AvgPool2d(nn.AvgPool2d, _OffPath):
    pass


class BatchNorm2d(nn.BatchNorm2d, _OffPath):
    pass


class Conv2d(_ScratchCache, nn.Conv2d, RelProp):
    """layers_ours.py:232-279.  Accelerated: the z^B rule of an image-input (3-channel) convolution whose stride
    equals its kernel with no padding -- the ViT patch embedding, reached by method="full" (ViT_LRP.py:337-343) ->
    te_conv2d_zb_relprop_f32, or te_conv2d_zb_relprop_bf16 on a bf16 layer (its weight planes live in x6_cache).  Other
    geometries are off the transformer path."""

    def relprop(self, R, alpha):
        k = self.kernel_size
        patch = (self.X.shape[1] == 3 and k[0] == k[1] and tuple(self.stride) == tuple(k)
                 and tuple(self.padding) == (0, 0) and tuple(self.dilation) == (1, 1) and self.groups == 1)
        if not patch:
            raise NotImplementedError("Conv2d.relprop: only the z^B rule of a patch-embedding convolution "
                                      "(3 input channels, stride == kernel, no padding) is accelerated")
        if self.X.dtype == torch.bfloat16 or self.weight.dtype == torch.bfloat16:
            # a bf16 layer: conv(X, W) is recomputed from the bf16 operands; its rounded output self.Y is not read
            return ops.conv2d_zb_relprop_bf16(R, self.X, self.weight.detach(), cache=x6_cache(self))
        return ops.conv2d_zb_relprop(R, self.X, self.weight, self.Y, self.bias)

    def attnlrp(self, G_tokens, x0, eps):
        """AttnLRP through the patch embedding, then input x G per pixel (te_relprop.h, "AttnLRP, pixel level"): G_tokens and
        x0 [B, P+1, E] (the chain's G at x0 and the cached patch embedding, the class token in row 0) -> fp32 [B,H,W].  The
        geometry test of relprop without the 3-channel condition; reads the layer's cached input X."""
        k = self.kernel_size
        patch = (k[0] == k[1] and tuple(self.stride) == tuple(k) and tuple(self.padding) == (0, 0)
                 and tuple(self.dilation) == (1, 1) and self.groups == 1)
        if not patch:
            raise NotImplementedError(f"Conv2d.attnlrp: only a patch-embedding convolution (square kernel, stride == kernel, no "
                                      f"padding, no dilation, one group) has a pixel rule; got kernel {tuple(k)}, stride "
                                      f"{tuple(self.stride)}, padding {tuple(self.padding)}, dilation {tuple(self.dilation)}, "
                                      f"groups {self.groups}")
        return ops.alrp_patch_relevance(G_tokens, x0, self.X.detach(), self.weight.detach(), eps)
