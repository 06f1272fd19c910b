"""AttnLRP restated on the model's OWN caches (a test helper; the specification is include/te_relprop.h, section "AttnLRP").

tests/attnlrp_ref.py recomputes its own forward pass, which is the right yardstick for an fp32 model and the wrong one for a
bf16 model: its forward pass in fp64 differs from the model's by the bf16 rounding of every activation (2e-3 to 1e-2 relative
L2 per sample on the toy ViT), which is not the chain's error.  Here the header's rules are written out explicitly in torch --
no autograd, no kernel of the package -- on the same cached tensors the kernel chain reads (the outputs of Linears and Adds,
the inputs of LayerNorms, GELU and tanh, qkv.Y / query.Y, key.Y, value.Y, the probabilities the accessor holds, gamma, W, x0),
each upcast EXACTLY to ``dtype`` (torch.float64: the yardstick; torch.float32: the scale an fp32 evaluation of the same
formulas reaches).  Call it after a forward pass of the model, with the seed that chain gets."""
import math

import torch
import torch.nn.functional as F


def _up(t, dtype):
    return t.detach().to(dtype)


def damp(G, y, eps):
    if eps == 0:
        return G
    sgn = torch.where(y >= 0, torch.ones_like(y), -torch.ones_like(y))
    return G * y / (y + eps * sgn)


def linear(lin, G, eps, dtype):
    return torch.matmul(damp(G, _up(lin.Y, dtype), eps), _up(lin.weight, dtype))


def layer_norm(norm, G, dtype):
    x = _up(norm.X, dtype)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + norm.eps)
    t = _up(norm.weight, dtype) * G
    return rstd * (t - t.mean(-1, keepdim=True))


def identity_rule(act, G, f, slope_at_zero, dtype):
    x = _up(act.X, dtype)
    safe = torch.where(x == 0, torch.ones_like(x), x)
    return G * torch.where(x == 0, torch.full_like(x, slope_at_zero), f(x) / safe)


def attention(G_o, q, k, v, p, scale):
    """The block's backward for d_out = G_o on [B,H,N,D] operands and probabilities p, then the uniform rule's factors ->
    (G_q, G_k, G_v)."""
    d_attn = torch.matmul(G_o, v.transpose(-1, -2))
    d_v = torch.matmul(p.transpose(-1, -2), G_o)
    d_s = p * (d_attn - (d_attn * p).sum(-1, keepdim=True))
    d_q = torch.matmul(d_s, k) * scale
    d_k = torch.matmul(d_s.transpose(-1, -2), q) * scale
    return d_q / 4, d_k / 4, d_v / 2


def _heads(t, H):
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H).permute(0, 2, 1, 3)


def _merge(t):
    B, H, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * D)


def vit_chain(model, seed, eps=1e-6, dtype=torch.float64):
    """-> [B, N-1] in ``dtype`` from the caches of the last forward pass of a vit.VisionTransformer; seed [B, classes]."""
    m = model
    G = linear(m.head, seed.to(dtype), eps, dtype)
    full = torch.zeros(m.pool.X.shape, dtype=dtype, device=G.device)
    full[:, 0] = G.reshape(G.shape[0], -1)
    G = layer_norm(m.norm, full, dtype)
    for blk in reversed(m.blocks):
        Gd = damp(G, _up(blk.add2.Y, dtype), eps)
        mlp = blk.mlp
        G_mlp = linear(mlp.fc1, identity_rule(mlp.act, linear(mlp.fc2, Gd, eps, dtype), F.gelu, 0.5, dtype), eps, dtype)
        G = Gd + layer_norm(blk.norm2, G_mlp, dtype)
        Gd = damp(G, _up(blk.add1.Y, dtype), eps)
        a = blk.attn
        G_o = linear(a.proj, Gd, eps, dtype)
        C, H = G_o.shape[-1], a.num_heads
        qkv = _up(a.qkv.Y, dtype)
        q, k, v = (_heads(qkv[..., i * C:(i + 1) * C], H) for i in range(3))
        G_q, G_k, G_v = attention(_heads(G_o, H), q, k, v, _up(a.get_attn(), dtype), a.scale)
        G_qkv = torch.cat((_merge(G_q), _merge(G_k), _merge(G_v)), -1)
        G = Gd + layer_norm(blk.norm1, linear(a.qkv, G_qkv, eps, dtype), dtype)
    return (_up(m.add.X[0], dtype) * G).sum(-1)[:, 1:]


def bert_chain(model, seed, eps=1e-6, dtype=torch.float64):
    """-> [B, N] in ``dtype`` from the caches of the last forward pass of a bert.BertForSequenceClassification."""
    bert = model.bert
    G = linear(model.classifier, seed.to(dtype), eps, dtype)
    pooler = bert.pooler
    G = linear(pooler.dense, identity_rule(pooler.activation, G, torch.tanh, 1.0, dtype), eps, dtype)
    full = torch.zeros(pooler.pool.X.shape, dtype=dtype, device=G.device)
    full[:, 0] = G.reshape(G.shape[0], -1)
    G = full
    for layer in reversed(bert.encoder.layer):
        out = layer.output
        Gd = damp(layer_norm(out.LayerNorm, G, dtype), _up(out.add.Y, dtype), eps)
        inter = layer.intermediate
        G1 = linear(inter.dense, identity_rule(inter.intermediate_act_fn, linear(out.dense, Gd, eps, dtype), F.gelu, 0.5, dtype),
                    eps, dtype)
        G = G1 + Gd
        so, sa = layer.attention.output, layer.attention.self
        Gd = damp(layer_norm(so.LayerNorm, G, dtype), _up(so.add.Y, dtype), eps)
        G_o = linear(so.dense, Gd, eps, dtype)
        H, D = sa.num_attention_heads, sa.attention_head_size
        q, k, v = (_heads(_up(lin.Y, dtype), H) for lin in (sa.query, sa.key, sa.value))
        G_q, G_k, G_v = attention(_heads(G_o, H), q, k, v, _up(sa.get_attn(), dtype), 1.0 / math.sqrt(D))
        G_self = (linear(sa.query, _merge(G_q), eps, dtype) + linear(sa.key, _merge(G_k), eps, dtype)) \
            + linear(sa.value, _merge(G_v), eps, dtype)
        G = G_self + Gd
    norm = bert.embeddings.LayerNorm
    return (_up(norm.X, dtype) * layer_norm(norm, G, dtype)).sum(-1)


def one_hot(logits, index=None):
    """The seed the chain gets: fp32 [B, classes], the one-hot of ``index`` (None: the per-sample argmax)."""
    B = logits.shape[0]
    idx = logits.detach().float().argmax(-1) if index is None else torch.as_tensor(index, device=logits.device).reshape(-1).long()
    if idx.numel() == 1 and B > 1:
        idx = idx.expand(B)
    seed = torch.zeros(logits.shape, dtype=torch.float32, device=logits.device)
    return seed.scatter_(1, idx.view(B, 1), 1.0), idx
