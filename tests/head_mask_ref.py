"""CPU restatement of the reference's attention relprop WITH the head-mask rule (tests/test_head_mask_host.py,
tests/test_gpu_head_mask.py).

The reference cannot produce a fixture: its forward multiplies ``attention_probs * head_mask`` directly (BERT.py:356), so
``self.mul.X`` is never set and ``self.mul.relprop`` (BERT.py:375-377) has nothing to read.  The rule itself is unambiguous --
Mul is RelPropSimple (BERT_explainability/modules/layers_ours.py:49-61,77-79) -- and is restated here from the oracle's
primitives: BERT.py:367-409 and ViT_LRP.py:154-177 as oracle.relprop_oracle writes them, plus the Mul step.

The oracle's own cache (oracle.model_cache) holds the UNMASKED probabilities and has no Mul step, so two more tensors per
layer come from the modules: ``matmul2.X[0]`` (P' = P . m, the AV rule's operand) and ``mul.X[1]`` (m, [B or 1, H, 1, 1]).
Every function computes in the dtype of its arguments (fp32 or fp64), on the CPU."""
import torch

from oracle import relprop_oracle as O


def mul_head_relprop(R, P, m):
    """RelPropSimple on Z = P . m, relevance of the first operand: Z = P m ; S = safe_divide(R, Z) ; P (S m)."""
    Z = P * m
    S = O.safe_divide(R, Z)
    return P * (S * m)


def head_relevance(cam, num_heads):
    """cam [B,N,C], the relevance entering an attention layer's rules -> (fp64 [B,H]: its sum over each head's slice, fp64
    [B,H]: the sum of its absolute values there -- the scale an error of that sum is measured against)."""
    heads = O._heads(cam, num_heads).double()
    return heads.sum(dim=(2, 3)), heads.abs().sum(dim=(2, 3))


def bert_self_attention_relprop(c1, lay, num_heads, p_masked, m, alpha=1.0, variant="ours"):
    """BertSelfAttention.relprop (BERT.py:367-409) on c1 [B,N,C] -> (relevance of hidden_states, attn_cam, the q / k / v
    relevance [B,H,N,D] as they enter the three Linear rules).  m is None: the unmasked layer, as oracle.bert_layer_relprop."""
    q, k, v = (O._heads(lay[n], num_heads) for n in ("q", "k", "v"))
    probs = lay["probs"] if m is None else p_masked
    cam1, cam_v = O.matmul_relprop(O._heads(c1, num_heads), probs, v, lay.get("z_av"))       # :371
    cam1 = cam1 / 2
    cam_v = cam_v / 2
    if m is not None:
        cam1 = mul_head_relprop(cam1, lay["probs"], m)                                        # :375-377
    attn_cam = cam1                                                                           # :380
    if lay.get("ext_mask") is not None:
        cam1, _ = O.add_relprop(cam1, lay["mask_add_x0"], lay["ext_mask"], variant)           # :386-388
    cq, ckt = O.matmul_relprop(cam1, q, k.transpose(-1, -2), lay.get("z_qk"))                 # :391
    cq = cq / 2
    ck = (ckt / 2).transpose(-1, -2)
    rq = O.linear_relprop(O._unheads(cq), lay["q_x"], lay["q_w"], alpha, variant)
    rk = O.linear_relprop(O._unheads(ck), lay["k_x"], lay["k_w"], alpha, variant)
    rv = O.linear_relprop(O._unheads(cam_v), lay["v_x"], lay["v_w"], alpha, variant)
    return O.clone_relprop([rq, rk, rv], lay["self_clone_x"]), attn_cam, (cq, ck, cam_v)      # :407


def bert_layer_relprop(cam, lay, num_heads, p_masked, m, alpha=1.0, variant="ours"):
    """oracle.bert_layer_relprop with the masked self-attention -> (cam, attn_cam, head_relevance(...), (cq, ck, cv))."""
    c1, c2 = O.add_relprop(cam, lay["out_add_x0"], lay["out_add_x1"], variant)
    c1 = O.linear_relprop(c1, lay["out_dense_x"], lay["out_dense_w"], alpha, variant)
    c1 = O.linear_relprop(c1, lay["inter_x"], lay["inter_w"], alpha, variant)
    cam = O.clone_relprop([c1, c2], lay["clone_x"])
    c1, c2 = O.add_relprop(cam, lay["att_add_x0"], lay["att_add_x1"], variant)
    c1 = O.linear_relprop(c1, lay["att_dense_x"], lay["att_dense_w"], alpha, variant)
    hr = head_relevance(c1, num_heads)
    c1, attn_cam, qkv = bert_self_attention_relprop(c1, lay, num_heads, p_masked, m, alpha, variant)
    return O.clone_relprop([c1, c2], lay["att_clone_x"]), attn_cam, hr, qkv


def bert_relprop(one_hot, cache, num_heads, p_masked, masks, start_layer=11, alpha=1.0, variant="ours"):
    """oracle.bert_relprop with per-layer masks.  p_masked / masks: one entry per layer (None: that layer is unmasked).
    -> map, cam, attn_cams, head_relevance and head_relevance_abs fp64 [B,L,H], qkv_cams."""
    cam = O.linear_relprop(one_hot, cache["cls_x"], cache["cls_w"], alpha, variant)
    cam = O.linear_relprop(cam, cache["pool_dense_x"], cache["pool_dense_w"], alpha, variant)
    cam = O.index_select_relprop(cam.unsqueeze(1), cache["pool_x"], 1, 0)
    L = len(cache["layers"])
    attn_cams, hrs, qkvs = [None] * L, [None] * L, [None] * L
    for i in reversed(range(L)):
        cam, attn_cams[i], hrs[i], qkvs[i] = bert_layer_relprop(cam, cache["layers"][i], num_heads, p_masked[i], masks[i],
                                                                alpha, variant)
    grads = [lay["attn_grad"] for lay in cache["layers"]]
    out = O.bert_attribution_tail(grads, attn_cams, start_layer) if all(g is not None for g in grads) else None
    return {"map": out, "cam": cam, "attn_cams": attn_cams, "head_relevance": torch.stack([h[0] for h in hrs], 1),
            "head_relevance_abs": torch.stack([h[1] for h in hrs], 1), "qkv_cams": qkvs}


def vit_block_relprop(cam, blk, num_heads, p_masked, m, alpha=1.0, variant="ours"):
    """oracle.vit_block_relprop (ViT_LRP.py:203-213,154-177) with the Mul step after the AV rule -> (cam, attn_cam,
    head_relevance(...), (c_q, c_k, c_v))."""
    cam1, cam2 = O.add_relprop(cam, blk["add2_x0"], blk["add2_x1"], variant)
    cam2 = O.linear_relprop(cam2, blk["fc2_x"], blk["fc2_w"], alpha, variant)
    cam2 = O.linear_relprop(cam2, blk["fc1_x"], blk["fc1_w"], alpha, variant)
    cam = O.clone_relprop([cam1, cam2], blk["clone2_x"])
    cam1, cam2 = O.add_relprop(cam, blk["add1_x0"], blk["add1_x1"], variant)
    cam2 = O.linear_relprop(cam2, blk["proj_x"], blk["proj_w"], alpha, variant)
    hr = head_relevance(cam2, num_heads)
    B, N, C = cam2.shape
    qkv = blk["qkv_out"].reshape(B, N, 3, num_heads, C // num_heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    attn = blk["attn"] if m is None else p_masked
    c_attn, c_v = O.einsum_av_relprop(O._heads(cam2, num_heads), attn, v, blk.get("z_av"))
    c_attn = c_attn / 2
    c_v = c_v / 2
    if m is not None:
        c_attn = mul_head_relprop(c_attn, blk["attn"], m)
    attn_cam = c_attn
    c_q, c_k = O.einsum_qk_relprop(c_attn, q, k, blk.get("z_qk"))
    c_q = c_q / 2
    c_k = c_k / 2
    cam_qkv = torch.cat([O._unheads(c_q), O._unheads(c_k), O._unheads(c_v)], dim=-1)
    cam2 = O.linear_relprop(cam_qkv, blk["qkv_x"], blk["qkv_w"], alpha, variant)
    return O.clone_relprop([cam1, cam2], blk["clone1_x"]), attn_cam, hr, (c_q, c_k, c_v)


def vit_relprop(one_hot, cache, num_heads, p_masked, masks, start_layer=0, alpha=1.0, variant="ours"):
    """oracle.vit_relprop with per-block masks -> map, cam, attn_cams, head_relevance and head_relevance_abs fp64 [B,L,H], qkv_cams."""
    cam = O.linear_relprop(one_hot, cache["head_x"], cache["head_w"], alpha, variant)
    cam = O.index_select_relprop(cam.unsqueeze(1), cache["pool_x"], 1, 0)
    L = len(cache["blocks"])
    attn_cams, hrs, qkvs = [None] * L, [None] * L, [None] * L
    for i in reversed(range(L)):
        cam, attn_cams[i], hrs[i], qkvs[i] = vit_block_relprop(cam, cache["blocks"][i], num_heads, p_masked[i], masks[i],
                                                               alpha, variant)
    grads = [b["attn_grad"] for b in cache["blocks"]]
    out = O.vit_attribution_tail(grads, attn_cams, start_layer) if all(g is not None for g in grads) else None
    return {"map": out, "cam": cam, "attn_cams": attn_cams, "head_relevance": torch.stack([h[0] for h in hrs], 1),
            "head_relevance_abs": torch.stack([h[1] for h in hrs], 1), "qkv_cams": qkvs}


def masked_operands(attn_modules, conv):
    """(p_masked, masks) per layer from OUR attention modules after a forward pass: matmul2.X[0] and mul.X[1] of a layer
    whose forward was masked, (None, None) otherwise.  conv: the cache's own tensor conversion (``.float().cpu()`` ...)."""
    pm, ms = [], []
    for a in attn_modules:
        if a.head_mask is None:
            pm.append(None)
            ms.append(None)
        else:
            pm.append(conv(a.matmul2.X[0]))
            ms.append(conv(a.mul.X[1]))
    return pm, ms
