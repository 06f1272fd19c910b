"""AttnLRP restated with torch autograd (a test helper; the specification is include/te_relprop.h, section "AttnLRP").

The same rules as the kernel chain, written as autograd tricks on a functional forward pass over the parameters of a deep
copy of the model, so that ONE backward pass of the class logit leaves G = x0.grad and the result is x0 * x0.grad summed
over the hidden dimension.  Hand it a deep copy of the model under test, in eval mode (``copy.deepcopy(model).double()``
for the fp64 yardstick): the patch embedding is called as a module and overwrites that copy's caches.

  damp          a custom autograd.Function on the output of every Linear and every residual Add: identity forward,
                backward G -> G y / stab(y), stab(y) = y + eps sgn(y), sgn(0) = +1 (eps = 0: G itself)
  uniform rule  A B  ->  (A B.detach() + A.detach() B) / 2 for both attention products
  LayerNorm     rstd.detach()
  identity rule x * (f(x) / x).detach(), the factor f'(0) at x == 0 (GELU, tanh)
  softmax, the class-token select, the position-embedding Add, the additive mask: plain autograd

Runs in the dtype and on the device of the model it is given (fp64 / fp32, CPU / GPU).  ``softmax`` is a module attribute
so that a test can replace it (tests/test_attnlrp_host.py proves conservation with the identity in its place)."""
import math

import torch
import torch.nn.functional as F

softmax = torch.softmax


class _Damp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, eps):
        ctx.save_for_backward(y)
        ctx.eps = eps
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        if ctx.eps == 0:
            return g, None
        sgn = torch.where(y >= 0, torch.ones_like(y), -torch.ones_like(y))
        return g * y / (y + ctx.eps * sgn), None


def damp(y, eps):
    return _Damp.apply(y, eps)


def linear(x, lin, eps):
    return damp(F.linear(x, lin.weight, lin.bias), eps)


def add(a, b, eps):
    return damp(a + b, eps)


def layer_norm(x, norm):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(var + norm.eps).detach()
    y = (x - mu) * rstd
    if norm.weight is not None:
        y = y * norm.weight
    return y if norm.bias is None else y + norm.bias


def identity_rule(x, f, slope_at_zero):
    xd = x.detach()
    safe = torch.where(xd == 0, torch.ones_like(xd), xd)
    ratio = torch.where(xd == 0, torch.full_like(xd, slope_at_zero), f(xd) / safe)
    return x * ratio


def gelu(x):
    return identity_rule(x, F.gelu, 0.5)


def tanh(x):
    return identity_rule(x, torch.tanh, 1.0)


def uniform_matmul(a, b):
    return 0.5 * (torch.matmul(a, b.detach()) + torch.matmul(a.detach(), b))


def _finish(x0, logits, index):
    B = logits.shape[0]
    if index is None:
        idx = logits.detach().argmax(dim=-1)
    else:
        idx = torch.as_tensor(index, device=logits.device).reshape(-1).long()
        if idx.numel() == 1 and B > 1:
            idx = idx.expand(B)
    seed = torch.zeros_like(logits)
    seed.scatter_(1, idx.view(B, 1), 1.0)
    (g,) = torch.autograd.grad((seed * logits).sum(), x0)
    return (x0.detach() * g).sum(dim=-1), logits.detach()


def vit_attnlrp(model, x, index=None, eps=1e-6, keep_cls=False):
    """-> (R [B, N-1] (keep_cls: [B, N], the class token first), logits [B, classes]) for a vit.VisionTransformer."""
    m = model
    B = x.shape[0]
    with torch.no_grad():
        patches = m.patch_embed(x)
        x0 = torch.cat((m.cls_token.expand(B, -1, -1), patches), dim=1)
    x0 = x0.detach().clone().requires_grad_(True)
    h = x0 + m.pos_embed
    N, C = h.shape[1:]
    for blk in m.blocks:
        H = blk.attn.num_heads
        qkv = linear(layer_norm(h, blk.norm1), blk.attn.qkv, eps)
        q, k, v = qkv.view(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
        p = softmax(uniform_matmul(q, k.transpose(-1, -2)) * blk.attn.scale, dim=-1)
        o = uniform_matmul(p, v).permute(0, 2, 1, 3).reshape(B, N, C)
        h = add(h, linear(o, blk.attn.proj, eps), eps)
        mlp = blk.mlp
        h = add(h, linear(gelu(linear(layer_norm(h, blk.norm2), mlp.fc1, eps)), mlp.fc2, eps), eps)
    logits = linear(layer_norm(h, m.norm)[:, 0], m.head, eps)
    R, logits = _finish(x0, logits, index)
    return (R if keep_cls else R[:, 1:]), logits


def bert_attnlrp(model, input_ids, attention_mask=None, index=None, eps=1e-6):
    """-> (R [B, N], logits [B, labels]) for a bert.BertForSequenceClassification."""
    m = model
    bert = m.bert
    emb = bert.embeddings
    B, N = input_ids.shape
    dtype = emb.word_embeddings.weight.dtype
    with torch.no_grad():
        pos = emb.position_embeddings(emb.position_ids[:, :N]).expand(B, -1, -1)
        typ = emb.token_type_embeddings(torch.zeros_like(input_ids))
        x0 = (typ + pos) + emb.word_embeddings(input_ids)
    x0 = x0.detach().clone().requires_grad_(True)
    if attention_mask is None:
        attention_mask = torch.ones((B, N), device=input_ids.device)
    ext = (1.0 - attention_mask[:, None, None, :].to(dtype)) * -10000.0
    h = layer_norm(x0, emb.LayerNorm)
    for layer in bert.encoder.layer:
        sa = layer.attention.self
        H, D = sa.num_attention_heads, sa.attention_head_size
        heads = lambda t: t.view(B, N, H, D).permute(0, 2, 1, 3)      # noqa: E731
        q, k, v = (heads(linear(h, lin, eps)) for lin in (sa.query, sa.key, sa.value))
        p = softmax(uniform_matmul(q, k.transpose(-1, -2)) / math.sqrt(D) + ext, dim=-1)
        ctx = uniform_matmul(p, v).permute(0, 2, 1, 3).reshape(B, N, H * D)
        so = layer.attention.output
        a = layer_norm(add(linear(ctx, so.dense, eps), h, eps), so.LayerNorm)
        inter = gelu(linear(a, layer.intermediate.dense, eps))
        h = layer_norm(add(linear(inter, layer.output.dense, eps), a, eps), layer.output.LayerNorm)
    pooled = tanh(linear(h[:, 0], bert.pooler.dense, eps))
    return _finish(x0, linear(pooled, m.classifier, eps), index)
