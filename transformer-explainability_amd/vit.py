"""ViT / DeiT with relevance propagation on MI355X kernels.

Host-side mirror of baselines/ViT/ViT_LRP.py (rule variant "ours", default method
"transformer_attribution") and baselines/ViT/ViT_orig_LRP.py (variant "lrp", method "grad") of the
reference: same constructor arguments, parameter names (timm / reference checkpoints load
unchanged), accessors (``blk.attn.get_attn()/get_attn_cam()/get_attn_gradients()/get_v()/
get_v_cam()``) and ``model.relprop(cam, method=..., is_ablation=..., start_layer=..., alpha=1)``.

What differs from the reference (by design, results identical at batch 1):
  * forward + backward stay on stock PyTorch-ROCm; every ``relprop`` below is HIP kernels via the C ABI
  * batch B >= 1 = B independent samples: relprop(one_hot[B,K]) returns [B, N-1]
  * q/k/v are consumed in place from the fused qkv activation and cam_q/cam_k/cam_v are written in
    place into the 'b n (qkv h d)' relevance buffer -- no rearrange copies (ViT_LRP.py:135,157,175)
  * the /2 of ViT_LRP.py:161-162,172-173 is folded into the kernels' store (exact: power of two)
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import methods, ops, producers
from . import rules as R_ours

__all__ = ["VisionTransformer", "vit_base_patch16_224", "vit_large_patch16_224", "deit_base_patch16_224",
           "compute_rollout_attention", "make_vit_module"]


def compute_rollout_attention(all_layer_matrices, start_layer=0):
    """ViT_LRP.py:38-49 (identity added, NO row normalisation).  list of L [B,N,N] -> [B,N,N]."""
    return ops.rollout(torch.stack(list(all_layer_matrices), 0), start_layer=start_layer, normalise=False)


# --------------------------------------------------------------------------------------------------------------------
# The per-method tails of VisionTransformer.relprop (ViT_LRP.py:337-398) as functions of the model with its populated
# caches: ``model.relprop`` calls them, and one relprop chain can serve several of them (methods.py says what each reads).
def tail_full(model, cam, **kwargs):
    """ViT_LRP.py:337-343: position-embedding Add, drop the class token, z^B rule of the patch embedding, sum over the
    colour channels -> [B, H, W].  ``cam``: the relevance the chain returned below block 0."""
    cam, _ = model.add.relprop(cam, **kwargs)
    cam = model.patch_embed.relprop(cam[:, 1:], **kwargs)
    return cam.sum(dim=1)


def tail_rollout(model, start_layer=0):
    mats = [blk.attn.get_attn_cam().clamp(min=0).mean(dim=1) for blk in model.blocks]
    return compute_rollout_attention(mats, start_layer=start_layer)[:, 0, 1:]


def tail_attribution(model, start_layer=0, pruned=False):
    """ViT_LRP.py:357-369: per block mean_h max(grad * attn_cam, 0), then rollout, row 0.  pruned: the chain and the
    backward pass stopped at block start_layer, the blocks below hold nothing current."""
    first = model.blocks[-1].attn.get_attn_cam()
    Bn, _, N, _ = first.shape
    stack = torch.empty((len(model.blocks), Bn, N, N), dtype=first.dtype, device=first.device)
    for i, blk in enumerate(model.blocks):
        if i >= start_layer or not pruned:       # (the rollout reads layers >= start_layer only)
            ops.gradcam_headmean(blk.attn.get_attn_gradients(), blk.attn.get_attn_cam(), out=stack[i])
    return ops.rollout(stack, start_layer=start_layer, normalise=False, row0_only=True)[:, 1:]


def tail_layer(model, method, is_ablation=False):
    blk = model.blocks[-1] if method == "last_layer" else model.blocks[1]
    c = blk.attn.get_attn_cam()
    if is_ablation:
        c = blk.attn.get_attn_gradients() * c
    return c.clamp(min=0).mean(dim=1)[:, 0, 1:]


def tail_last_layer_attn(model):
    attn = model.blocks[-1].attn.get_attn()
    if ops._is_bf16(attn):       # fp32 map of a bf16 model: clamp, then the head mean summed in fp32
        return ops.attn_headmean(attn.detach(), clamp=True, row0=True)[:, 1:]
    return attn.clamp(min=0).mean(dim=1)[:, 0, 1:]


def relprop_tail(model, method, cam=None, is_ablation=False, start_layer=0, pruned=False, **kwargs):
    """The map of ``method`` from the caches a forward pass, the backward pass and the relprop chain left on ``model``
    (``cam``: what the chain returned; only "full" reads it)."""
    if method == "full":
        return tail_full(model, cam, **kwargs)
    if method == "rollout":
        return tail_rollout(model, start_layer)
    if method in ("transformer_attribution", "grad"):
        return tail_attribution(model, start_layer, pruned)
    if method in ("last_layer", "second_layer"):
        return tail_layer(model, method, is_ablation)
    if method == "last_layer_attn":
        return tail_last_layer_attn(model)
    return None   # unknown method: the reference falls through silently


def _trunc_normal_(t, std=.02):
    with torch.no_grad():
        return nn.init.trunc_normal_(t, mean=0., std=std, a=-2., b=2.)


class _SplitQKV(torch.autograd.Function):
    """'b n (qkv h d) -> qkv b h n d' as three contiguous [B,H,N,D] tensors.  Same values as the permuted views the
    reference slices (ViT_LRP.py:135-136); the batched products need contiguous operands anyway, and the backward
    writes dq / dk / dv straight into one [B,N,3C] gradient (three strided copies) where autograd's select_backward
    would zero-fill a [3,B,H,N,D] buffer per operand and sum the three (1.6 ms per ViT-B/16 batch-64 step)."""

    @staticmethod
    def forward(ctx, qkv, num_heads):
        B, N, C3 = qkv.shape
        parts = qkv.view(B, N, 3, num_heads, C3 // (3 * num_heads)).permute(2, 0, 3, 1, 4)
        return parts[0].contiguous(), parts[1].contiguous(), parts[2].contiguous()

    @staticmethod
    def backward(ctx, dq, dk, dv):
        ref = next(g for g in (dq, dk, dv) if g is not None)
        B, H, N, D = ref.shape
        grad = torch.empty((B, N, 3, H, D), dtype=ref.dtype, device=ref.device)
        slots = grad.permute(2, 0, 3, 1, 4)
        for slot, g in zip(slots, (dq, dk, dv)):
            if g is None:
                slot.zero_()
            else:
                slot.copy_(g)
        return grad.view(B, N, 3 * H * D), None


def split_qkv(qkv, num_heads):
    return _SplitQKV.apply(qkv, num_heads)


class _FusedAttention(torch.autograd.Function):
    """the attention block of ViT_LRP.py:132-152 on the hand-written producer kernels
    (te_attention_forward_f32 / te_attention_backward_f32) instead of ~10 stock launches per direction.

    forward : qkv [B,N,3C] -> out [B,N,C]; the probabilities and the unscaled scores (the tensors the relprop rules and
              the accessors read) come back as non-differentiable by-products.
    backward: computes d_attn -- the attention gradient the explanation needs -- and hands it to the module
              (save_attn_gradients, what the reference's register_hook does, ViT_LRP.py:144-145), then d_qkv for the
              layers below; a module whose ``_fused_stop_backward`` is set is the lowest block whose gradient is
              wanted: nothing consumes d_qkv there, so only d_attn is formed."""

    @staticmethod
    def forward(ctx, qkv, num_heads, scale, module, feeds=None):
        # feeds: the scratch dict of the projection layer if that layer takes the operand planes of `out` from this node
        # (producers.takes_producer_planes; DESIGN.md "The layer's scratch dict")
        if feeds is not None:
            out, attn, zqk, xs, xa = ops.attention_forward(qkv, num_heads, scale, planes=True, planes_abs=not ops.X6_SIGNED_PLANES)
            ops.post_x_planes(feeds, out, xs, xa)
        else:
            out, attn, zqk = ops.attention_forward(qkv, num_heads, scale)
        ctx.save_for_backward(qkv, attn, out)      # (out: the projection's input, alive anyway; the backward's row sums come from it)
        ctx.num_heads, ctx.scale, ctx.module = num_heads, scale, module
        ctx.mark_non_differentiable(attn, zqk)
        # (round 6) no zero gradients for the two by-products: autograd otherwise fills a [B,H,N,N] zero tensor for each of them
        # in front of every backward call -- 24 x 119 MB of stores per ViT-B/16 batch-64 step that nobody reads
        ctx.set_materialize_grads(False)
        return out, attn, zqk

    @staticmethod
    def backward(ctx, d_out, _d_attn_unused, _d_zqk_unused):
        qkv, attn, out = ctx.saved_tensors
        if d_out is None:          # (nothing downstream of `out` reached the loss: with unmaterialised gradients that is a None)
            return None, None, None, None, None
        stop = bool(getattr(ctx.module, "_fused_stop_backward", False))
        d_attn, d_qkv = ops.attention_backward(d_out, qkv, attn, ctx.num_heads, ctx.scale, need_qk=not stop, out=out)
        ctx.module.save_attn_gradients(d_attn)
        return (None if stop else d_qkv), None, None, None, None


# the checkpoints the reference's factories fetch (ViT_LRP.py:24-36, 428-435 -- the same URLs in ViT_new.py / ViT_orig_LRP.py)
PRETRAINED_URLS = {
    "vit_base_patch16_224": "https://github.com/rwightman/pytorch-image-models/releases/download/v0.1-vitjx/"
                            "jx_vit_base_p16_224-80ecf9dd.pth",
    "vit_large_patch16_224": "https://github.com/rwightman/pytorch-image-models/releases/download/v0.1-vitjx/"
                             "jx_vit_large_p16_224-4ee7a4dc.pth",
    "deit_base_patch16_224": "https://dl.fbaipublicfiles.com/deit/deit_base_patch16_224-b5f2ef4d.pth",
}


def load_pretrained_weights(model, url, patch_size=16, key=None):
    """``pretrained=True`` of the reference's factories (helpers.py:87-150 ``load_pretrained`` -> ``model_zoo.load_url``;
    DeiT: ``torch.hub.load_state_dict_from_url``, ViT_LRP.py:432): the checkpoint comes from the torch hub cache
    (``$TORCH_HOME/hub/checkpoints/<file name of the URL>``) and is downloaded only if it is not there -- on a host without
    a network that means: put the file there once.  Same post-processing as the reference: a linear patch-embedding
    weight is reshaped to the convolution's [C, 3, p, p] (``_conv_filter``, ViT_LRP.py:399-406); a classifier of another
    width than the model's is dropped and the rest loaded non-strictly (helpers.py:143-147)."""
    import os
    name = os.path.basename(url)
    try:
        state = torch.hub.load_state_dict_from_url(url, map_location="cpu", progress=False)
    except Exception as exc:       # urllib's errors on a host without a network
        where = os.path.join(torch.hub.get_dir(), "checkpoints", name)
        raise RuntimeError(f"pretrained=True: {name} is not in the torch hub cache and could not be downloaded "
                           f"({type(exc).__name__}: {exc}); place the checkpoint at {where}") from exc
    if key is not None:
        state = state[key]
    state = dict(state)
    w = state.get("patch_embed.proj.weight")
    if w is not None and w.dim() == 2:
        state["patch_embed.proj.weight"] = w.reshape(w.shape[0], 3, patch_size, patch_size)
    strict = True
    if "head.weight" in state and state["head.weight"].shape[0] != model.head.weight.shape[0]:
        del state["head.weight"], state["head.bias"]
        strict = False
    model.load_state_dict(state, strict=strict)
    return model


def make_vit_module(L):
    """Build the model classes over a rule namespace ``L`` (rules for 'ours', rules_lrp for 'lrp')."""

    class Mlp(nn.Module):
        def __init__(self, in_features, hidden_features=None, out_features=None, drop=0.):
            super().__init__()
            out_features = out_features or in_features
            hidden_features = hidden_features or in_features
            self.fc1 = L.Linear(in_features, hidden_features)
            self.act = L.GELU()
            self.fc2 = L.Linear(hidden_features, out_features)
            self.drop = L.Dropout(drop)
            if hasattr(self.act, "feeds"):
                self.act.feeds(self.fc2)      # (a hint for the producers: the activation may emit fc2's operand planes)

        def forward(self, x):
            return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))

        def relprop(self, cam, **kwargs):
            # ViT_LRP.py:69-74 -- dropout / GELU rules are the identity
            cam = self.fc2.relprop(cam, **kwargs)
            return self.fc1.relprop(cam, **kwargs)

        def attnlrp(self, G, eps):
            """(extension) AttnLRP: epsilon rule on both layers, identity rule through the activation, dropout plain."""
            G = self.act.attnlrp(self.fc2.attnlrp(G, eps), eps)
            return self.fc1.attnlrp(G, eps)

    class Attention(nn.Module):
        def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
            super().__init__()
            self.num_heads = num_heads
            self.scale = (dim // num_heads) ** -0.5
            self.matmul1 = L.einsum('bhid,bhjd->bhij')      # A = Q K^T
            self.matmul2 = L.einsum('bhij,bhjd->bhid')      # out = A V
            self.qkv = L.Linear(dim, dim * 3, bias=qkv_bias)
            self.attn_drop = L.Dropout(attn_drop)
            self.proj = L.Linear(dim, dim)
            self.proj_drop = L.Dropout(proj_drop)
            self.softmax = L.Softmax(dim=-1)
            self.mul = L.Mul()                              # (extension: the head mask, as BertSelfAttention.mul)
            self.attn_cam = self.attn = self.v = self.v_cam = self.attn_gradients = None
            self.head_mask = None
            # (extension, off by default) relprop_after_proj stores ops.head_relevance of the relevance it receives: fp64
            # [B,H] (LRP.generate_head_relevance)
            self.save_head_relevance = False
            self.head_relevance = None

        # accessors of ViT_LRP.py:102-130
        def get_attn(self): return self.attn
        def save_attn(self, attn): self.attn = attn
        # accessor names of the plain (non-LRP) model, baselines/ViT/ViT_new.py:78-88
        def get_attention_map(self): return self.attn
        def save_attention_map(self, attn): self.attn = attn
        def save_attn_cam(self, cam): self.attn_cam = cam
        def get_attn_cam(self): return self.attn_cam
        def get_v(self): return self.v
        def save_v(self, v): self.v = v
        def save_v_cam(self, cam): self.v_cam = cam
        def get_v_cam(self): return self.v_cam
        def save_attn_gradients(self, g): self.attn_gradients = g
        def get_attn_gradients(self): return self.attn_gradients

        def forward(self, x, head_mask=None):
            """head_mask (extension; the reference ViT has none): [B or 1, H, 1, 1], one value per head, with the semantics of
            BertSelfAttention (BERT.py:345-358): the probabilities are multiplied by it after the accessor and the gradient hook
            took the unmasked ones.  Rewritten on every call; a masked block always takes the stock branch."""
            B, N, C = x.shape
            H = self.num_heads
            self._fused_anchor = None
            self.head_mask = head_mask
            if head_mask is None and ops.USE_FUSED_PRODUCERS and x.is_cuda and not self.training and (
                    (x.dtype == torch.float32 and ops.attention_forward_supported(N, C // H))
                    or (x.dtype == torch.bfloat16 and ops.attention_forward_bf16_supported(N, C // H))):
                return self._forward_fused(x)
            q, k, v = split_qkv(self.qkv(x), H)                                 # 'b n (qkv h d) -> qkv b h n d'
            self.save_v(v)
            attn = self.attn_drop(self.softmax(self.matmul1([q, k]) * self.scale))
            self.save_attn(attn)
            if attn.requires_grad:
                attn.register_hook(self.save_attn_gradients)
            if head_mask is not None:
                attn = self.mul([attn, head_mask])
            out = self.matmul2([attn, v]).permute(0, 2, 1, 3).reshape(B, N, C)  # 'b h n d -> b n (h d)'
            return self.proj_drop(self.proj(out))

        def _forward_fused(self, x):
            """ViT_LRP.py:132-152 on the producer kernels.  q / k / v are never copied out of the fused activation: the
            rule modules' caches (matmul1.X / .Y, matmul2.X / .Y) are strided views of it and of the 'b n (h d)'
            output, which the relprop kernels read in place."""
            B, N, C = x.shape
            H, D = self.num_heads, C // self.num_heads
            qkv = self.qkv(x)
            feeds = None
            if (isinstance(self.proj, L.Linear) and ops.attention_forward_planes_supported(qkv, H)
                    and producers.takes_producer_planes(self.proj, B * N, C)):
                feeds = R_ours.x6_cache(self.proj)
            out, attn, zqk = _FusedAttention.apply(qkv, H, self.scale, self, feeds)
            self._fused_anchor = qkv if qkv.requires_grad else None
            q, k, v = qkv.detach().view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
            self.save_v(v)
            self.save_attn(attn)
            zav = out.detach().view(B, N, H, D).permute(0, 2, 1, 3)
            for mod, X, Y in ((self.matmul1, [q, k], zqk), (self.matmul2, [attn, v], zav)):
                mod.X, mod.Y = X, Y
                mod._y_version, mod._w_version = Y._version, (None, None)
            return self.proj_drop(self.proj(out))

        def relprop(self, cam, **kwargs):
            """ViT_LRP.py:154-177."""
            return self.relprop_after_proj(self.proj.relprop(cam, **kwargs), **kwargs)

        def relprop_after_proj(self, cam, **kwargs):
            """ViT_LRP.py:157-177: everything below proj.relprop (the two attention rules and qkv.relprop)."""
            B, N, C = cam.shape
            H = self.num_heads
            D = C // H
            r_heads = cam.view(B, N, H, D).permute(0, 2, 1, 3)                  # strided view, no copy
            if self.save_head_relevance:
                self.head_relevance = ops.head_relevance(r_heads)
            attn, v = self.matmul2.X
            q, k = self.matmul1.X
            cam_qkv = torch.empty((B, N, 3 * C), dtype=cam.dtype, device=cam.device)
            slots = cam_qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)          # [3][B,H,N,D] views
            var = self.matmul2.variant
            cam1, cam_v = ops.matmul_relprop_av(r_heads, attn, v, out_scale=0.5, cam_v_out=slots[2], variant=var,
                                                z=R_ours._cached_y(self.matmul2))
            self.save_v_cam(cam_v)
            if self.head_mask is not None:
                cam1, _ = self.mul.relprop(cam1, **kwargs)                      # the Mul rule of BERT.py:375-377
            self.save_attn_cam(cam1)
            if getattr(self, "_stop_after_attn_cam", False):
                raise L.StopRelprop()
            ops.matmul_relprop_qk(cam1, q, k, out_scale=0.5, cam_q_out=slots[0], cam_k_out=slots[1], variant=var,
                                  z=R_ours._cached_y(self.matmul1))
            return self.qkv.relprop(cam_qkv, **kwargs)

        def attnlrp(self, G, eps):
            """(extension) AttnLRP through proj, the attention block (its own backward for d_out = G_o, then the uniform
            rule's 1/4, 1/4, 1/2) and qkv.  q / k / v are the thirds of the cached qkv activation, read in place; the
            probabilities are the ones the accessor holds: the same tensors whichever forward produced them."""
            if self.head_mask is not None:
                raise ops._lib.TeError("Attention.attnlrp: head_mask is not implemented for AttnLRP")
            G_o = self.proj.attnlrp(G, eps)
            C = G_o.shape[-1]
            qkv = self.qkv.Y.detach()
            classes = G_o.dim() == qkv.dim() + 1      # [K,B,N,C]: the rule per class into the slices of a [K,B,N,3C] gradient
            d_qkv = torch.empty(G_o.shape[:-1] + (3 * C,), dtype=torch.float32, device=G_o.device)      # (fp32 on a bf16 model too)
            third = lambda t, i: t[..., i * C:(i + 1) * C]      # noqa: E731
            for g_o, d in (zip(G_o, d_qkv) if classes else ((G_o, d_qkv),)):
                R_ours.attention_attnlrp(g_o, third(qkv, 0), third(qkv, 1), third(qkv, 2), self.get_attn().detach(),
                                         self.num_heads, self.scale, third(d, 0), third(d, 1), third(d, 2))
            return self.qkv.attnlrp(ops.alrp_scale3(d_qkv), eps)

    class Block(nn.Module):
        def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., norm_eps=1e-6):
            super().__init__()
            self.norm1 = L.LayerNorm(dim, eps=norm_eps)
            self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
            self.norm2 = L.LayerNorm(dim, eps=norm_eps)
            self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), drop=drop)
            self.add1 = L.Add()
            self.add2 = L.Add()
            self.clone1 = L.Clone()
            self.clone2 = L.Clone()

        def forward(self, x, head_mask=None):
            x1, n = self._clone_norm(self.clone1, self.norm1, x)
            x = self.add1([x1, self.attn(n) if head_mask is None else self.attn(n, head_mask)])
            x1, n = self._clone_norm(self.clone2, self.norm2, x)
            return self.add2([x1, self.mlp(n)])

        @staticmethod
        def _clone_norm(clone, norm, x):
            """``x1, x2 = clone(x, 2); n = norm(x2)`` (ViT_LRP.py:203-205).  With the producer kernels on, the pair is one
            autograd node whose backward kernel also adds the bypass gradient (producers._ResidualLayerNorm); the two
            modules' caches are filled as their forward hooks would."""
            if producers.norm_usable(x, norm):
                x1, n = producers.residual_layer_norm(x, norm)
                clone.X, clone.num = x.detach(), 2
                norm.X, norm.Y = clone.X, n
                return x1, n
            x1, x2 = clone(x, 2)
            return x1, norm(x2)

        def relprop(self, cam, **kwargs):
            """ViT_LRP.py:203-213 (LayerNorm rules are the identity)."""
            cam1, cam2 = self.add2.relprop(cam, deferred=True, **kwargs)
            cam2 = self.mlp.relprop(cam2, **kwargs)
            cam = self.clone2.relprop((cam1, cam2), **kwargs)
            cam1, cam2 = self.add1.relprop(cam, deferred=True, **kwargs)
            cam2 = self.attn.relprop(cam2, **kwargs)
            return self.clone1.relprop((cam1, cam2), **kwargs)

        def attnlrp(self, G, eps):
            """(extension) AttnLRP: each residual Add damps once and feeds both paths; the paths add up at the Clone."""
            Gd = self.add2.attnlrp(G, eps)
            G = self.clone2.attnlrp((Gd, self.norm2.attnlrp(self.mlp.attnlrp(Gd, eps), eps)), eps)
            Gd = self.add1.attnlrp(G, eps)
            return self.clone1.attnlrp((Gd, self.norm1.attnlrp(self.attn.attnlrp(Gd, eps), eps)), eps)

        def relprop_cls_only(self, cam_cls, **kwargs):
            """Block.relprop for relevance that lives on token 0 only (cam_cls [B,1,C]) -- the state right after
            pool.relprop (ViT_LRP.py:329), i.e. the LAST block.  Every rule from add2 down to proj maps a zero
            relevance row to an exact zero row (S = safe_divide(0, Z) = 0), and Add's per-sample sums gain only
            zeros from those rows, so the six rules are evaluated on the [B,1,C] slice of their cached inputs and
            the result is scattered into a zero [B,N,C] tensor before the attention rules, which spread relevance
            to all tokens.  Bitwise equal to the dense evaluation at 1/N of its Linear work."""
            alpha = kwargs.get("alpha", 1)
            var = self.add2.variant
            cls = lambda t: t[:, :1]                                             # noqa: E731
            dfr = ops.USE_DEFERRED_ADD
            c1, c2 = ops.add_relprop(cam_cls, cls(self.add2.X[0]), cls(self.add2.X[1]), variant=var, deferred=dfr)
            c2 = R_ours.linear_rule(self.mlp.fc2, c2, alpha, cls, var)
            c2 = R_ours.linear_rule(self.mlp.fc1, c2, alpha, cls, var)
            cam = ops.clone_relprop((c1, c2), cls(self.clone2.X))
            c1, c2 = ops.add_relprop(cam, cls(self.add1.X[0]), cls(self.add1.X[1]), variant=var, deferred=dfr)
            c2 = R_ours.linear_rule(self.attn.proj, c2, alpha, cls, var)
            if isinstance(c1, ops.Deferred):
                c1 = c1.materialise()
            B, N, C = self.clone1.X.shape
            dense = torch.zeros((2, B, N, C), dtype=c2.dtype, device=c2.device)
            dense[0, :, 0] = c1[:, 0]
            dense[1, :, 0] = c2[:, 0]
            cam2 = self.attn.relprop_after_proj(dense[1], **kwargs)
            return self.clone1.relprop((dense[0], cam2), **kwargs)

    class PatchEmbed(nn.Module):
        def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
            super().__init__()
            img_size = (img_size, img_size) if isinstance(img_size, int) else tuple(img_size)
            patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
            self.img_size, self.patch_size = img_size, patch_size
            self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0])
            self.proj = L.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)

        def forward(self, x):
            B, C, Hh, Ww = x.shape
            assert Hh == self.img_size[0] and Ww == self.img_size[1], \
                f"Input image size ({Hh}*{Ww}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
            return self.proj(x).flatten(2).transpose(1, 2)

        def relprop(self, cam, **kwargs):
            # ViT_LRP.py:238-242: [B,P,E] -> [B,E,Hp,Wp]; built as a VIEW so the kernel reads the token-major memory
            # in place (the reference's transpose + reshape copies)
            cam = cam.unflatten(1, (self.img_size[0] // self.patch_size[0], self.img_size[1] // self.patch_size[1]))
            return self.proj.relprop(cam.permute(0, 3, 1, 2), **kwargs)

        def attnlrp(self, G, x0, eps):
            """G, x0 [B, P+1, E] token-major (class token first) -> fp32 [B,H,W]: the kernel reads the token rows in place."""
            return self.proj.attnlrp(G, x0, eps)

    class VisionTransformer(nn.Module):
        default_method = "transformer_attribution" if L.RelProp.variant == "ours" else "grad"

        def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                     num_heads=12, mlp_ratio=4., qkv_bias=False, mlp_head=False, drop_rate=0., attn_drop_rate=0.,
                     block_norm_eps=1e-6, final_norm_eps=1e-5):
            # (the LayerNorm epsilons are ViT_LRP.py:184,187,266; ViT_new.py uses other values -- see the drop-in)
            super().__init__()
            self.num_classes = num_classes
            self.num_features = self.embed_dim = embed_dim
            self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans,
                                          embed_dim=embed_dim)
            num_patches = self.patch_embed.num_patches
            self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
            self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
            self.blocks = nn.ModuleList([
                Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                      attn_drop=attn_drop_rate, norm_eps=block_norm_eps) for _ in range(depth)])
            self.norm = L.LayerNorm(embed_dim, eps=final_norm_eps)
            self.head = Mlp(embed_dim, int(embed_dim * mlp_ratio), num_classes) if mlp_head \
                else L.Linear(embed_dim, num_classes)
            _trunc_normal_(self.pos_embed, std=.02)
            _trunc_normal_(self.cls_token, std=.02)
            self.apply(self._init_weights)
            self.pool = L.IndexSelect()
            self.add = L.Add()
            self.inp_grad = None
            self.exploit_cls_sparsity = True     # exact; set False to evaluate the last block densely
            # (extension, off by default) "transformer_attribution" / "grad" read attn_cam of blocks >= start_layer only
            # (ViT_LRP.py:357-369), yet the reference propagates relevance through every block.  With this flag the
            # loop stops right after block start_layer's AV rule stored its attn_cam: same map bit for bit, 1/L of the
            # relprop work less per skipped block -- but get_attn_cam() of blocks < start_layer is no longer refreshed.
            self.prune_below_start_layer = False
            self.register_buffer("_cls_index", torch.zeros((), dtype=torch.long), persistent=False)

        def save_inp_grad(self, grad): self.inp_grad = grad
        def get_inp_grad(self): return self.inp_grad

        def _init_weights(self, m):
            if isinstance(m, nn.Linear):
                _trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

        @property
        def no_weight_decay(self):
            return {'pos_embed', 'cls_token'}

        def get_head_mask(self, head_mask, batch_size=None):
            """[H], [L,H] or, per sample, [L,B,H] -> [L, 1 or B, H, 1, 1] in the model's dtype on its device; None ->
            [None] * L; any other shape is a ValueError (rules.expand_head_mask, as BertModel.get_head_mask)."""
            return R_ours.expand_head_mask(head_mask, len(self.blocks), self.blocks[0].attn.num_heads, self.pos_embed.dtype,
                                           batch_size, self.pos_embed.device)

        def forward(self, x, register_hook=False, head_mask=None):
            # register_hook (ViT_new.py:195): the attention-gradient hook is always registered when a graph is built
            # head_mask (extension): one value per head, see get_head_mask; refused here, before anything runs, if misshapen
            B = x.shape[0]
            head_mask = self.get_head_mask(head_mask, B)
            # a masked pass is a stock-forward pass, for every layer: the same bits whatever ops.USE_FUSED_PRODUCERS says
            with (ops.stock_forward() if torch.is_tensor(head_mask) else ops._NULL):
                x = self.patch_embed(x)
                x = torch.cat((self.cls_token.expand(B, -1, -1), x), dim=1)
                x = self.add([x, self.pos_embed])
                if x.requires_grad:
                    x.register_hook(self.save_inp_grad)
                for blk, hm in zip(self.blocks, head_mask):
                    x = blk(x) if hm is None else blk(x, hm)
                x = self.norm(x)
                x = self.pool(x, dim=1, indices=self._cls_index).squeeze(1)   # (a device tensor made once: graph-capturable)
                return self.head(x)

        # ------------------------------------------------------------------------------------------
        def relprop(self, cam=None, method=None, is_ablation=False, start_layer=0, **kwargs):
            """ViT_LRP.py:324-398.  cam: one-hot [B, num_classes]; returns per-sample maps.
            (extension) ``method`` may be a tuple / list of names: ONE chain then serves every tail and the result is a
            dict name -> map, each entry what the single-method call returns (LRP.generate_all)."""
            if method is None:
                method = self.default_method
            several = not isinstance(method, str)
            wanted = tuple(method) if several else (method,)
            if "full" in wanted and ops._is_f64(cam):       # before any rule runs: Conv2d's z^B rule has no fp64 kernel
                raise ops._lib.TeError(f"{ops.DTYPES_MSG}; method='full' (the z^B patch rule) is not implemented for "
                                       "torch.float64 relevance: run it on a float32 or bfloat16 model")
            if several:     # the prune rule of methods.py: every requested tail reads the blocks >= start_layer alone
                prune = self.prune_below_start_layer and methods.prunable(wanted, methods.LRP_NEEDS)
            else:
                prune = self.prune_below_start_layer and method in methods.SINGLE_CALL_PRUNED
            try:
                with L.stop_after_attn_cam(self.blocks[start_layer].attn if prune else None):
                    cam = self.head.relprop(cam, **kwargs)
                    if self.exploit_cls_sparsity and isinstance(self.head, nn.Linear):
                        # pool.relprop puts relevance on the class token only: keep it as a [B,1,C] row through the last
                        # block's dense rules instead of a [B,N,C] tensor that is zero everywhere else
                        cam = ops.index_select_relprop(cam.unsqueeze(1), self.pool.X[:, :1], 0)
                        cam = self.blocks[-1].relprop_cls_only(cam, **kwargs)
                        rest = list(self.blocks)[:-1]
                    else:
                        cam = self.pool.relprop(cam.unsqueeze(1), **kwargs)
                        rest = list(self.blocks)
                    for blk in reversed(rest):
                        cam = blk.relprop(cam, **kwargs)
            except L.StopRelprop:
                cam = None

            hook = getattr(self, "_before_tail", None)    # LRP(overlap_backward=True): join with the backward pass here
            if hook is not None:
                hook()

            maps = {m: relprop_tail(self, m, cam, is_ablation, start_layer, prune, **kwargs) for m in wanted}
            return maps if several else maps[method]

        def attnlrp(self, seed, eps=1e-6, method="tokens"):
            """(extension) AttnLRP (te_relprop.h, section "AttnLRP"): ``seed`` [B, num_classes] (the one-hot of the class) ->
            fp32 [B, N-1], the relevance of the patch tokens.  One chain over the caches of the last forward pass; no
            backward pass.  The position-embedding Add is a parameter Add: plain.  method="full": the same chain, then the
            eps-rule through the patch embedding and input x G per pixel ("AttnLRP, pixel level") -> fp32 [B,H,W].
            ``seed`` [K, B, num_classes] (te_relprop.h, "AttnLRP, a class axis"): K seeds through one chain, every cached operand
            read once -> fp32 [B, K, N-1] / [B, K, H, W]; [:, k] has the bits of the call on seed[k]."""
            if method not in ("tokens", "full"):
                raise ValueError(f"attnlrp: method must be 'tokens' or 'full', got {method!r}")
            G = self.head.attnlrp(seed, eps)
            G = self.norm.attnlrp(self.pool.attnlrp(G, eps), eps)
            for blk in reversed(self.blocks):
                G = blk.attnlrp(G, eps)
            x0 = self.add.X[0]
            if method == "full":
                if G.dim() == x0.dim() + 1:
                    return torch.stack([self.patch_embed.attnlrp(g, x0, eps) for g in G], 1)
                return self.patch_embed.attnlrp(G, x0, eps)
            return ops.alrp_token_relevance(x0, G, skip_first=True)

    def vit_base_patch16_224(pretrained=False, **kwargs):
        model = VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                  **kwargs)
        if pretrained:
            load_pretrained_weights(model, PRETRAINED_URLS["vit_base_patch16_224"], patch_size=16)
        return model

    def vit_large_patch16_224(pretrained=False, **kwargs):
        model = VisionTransformer(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True,
                                  **kwargs)
        if pretrained:
            load_pretrained_weights(model, PRETRAINED_URLS["vit_large_patch16_224"], patch_size=16)
        return model

    def deit_base_patch16_224(pretrained=False, **kwargs):
        model = VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                                  **kwargs)
        if pretrained:
            load_pretrained_weights(model, PRETRAINED_URLS["deit_base_patch16_224"], patch_size=16, key="model")
        return model

    ns = dict(Mlp=Mlp, Attention=Attention, Block=Block, PatchEmbed=PatchEmbed, VisionTransformer=VisionTransformer,
              vit_base_patch16_224=vit_base_patch16_224, vit_large_patch16_224=vit_large_patch16_224,
              deit_base_patch16_224=deit_base_patch16_224)
    return ns


_ns = make_vit_module(R_ours)
Mlp, Attention, Block, PatchEmbed = _ns["Mlp"], _ns["Attention"], _ns["Block"], _ns["PatchEmbed"]
VisionTransformer = _ns["VisionTransformer"]
vit_base_patch16_224 = _ns["vit_base_patch16_224"]
vit_large_patch16_224 = _ns["vit_large_patch16_224"]
deit_base_patch16_224 = _ns["deit_base_patch16_224"]
