"""AttnLRP at pixel level restated with torch autograd (a test helper; the specification is include/te_relprop.h, section
"AttnLRP, pixel level").

The restatement of tests/attnlrp_ref.py (imported, its rules are used as they are) with the patch-embedding convolution
INSIDE the graph: the image is the leaf, the convolution's output -- as tokens, bias included -- goes through ``damp``
like the output of every Linear, and ONE backward pass of the class logit leaves both x.grad (pixels) and x0.grad (tokens):

    pixels [B,H,W]  = (x * x.grad).sum(1)            input x G per pixel, summed over the channels
    tokens [B,N-1]  = (x0 * x0.grad).sum(-1)[:, 1:]  the token map of attnlrp_ref.vit_attnlrp

The convolution is evaluated with F.conv2d on the parameters of the model it is given: no cache of that model is written.
Runs in the dtype and on the device of the model (fp64 / fp32, CPU / GPU)."""
import torch
import torch.nn.functional as F

import attnlrp_ref as ref


def vit_attnlrp_pixels(model, x, index=None, eps=1e-6):
    """-> (pixels [B,H,W], tokens [B,N-1], logits [B,classes]) for a vit.VisionTransformer."""
    m = model
    B = x.shape[0]
    proj = m.patch_embed.proj
    x = x.detach().clone().requires_grad_(True)
    y = F.conv2d(x, proj.weight, proj.bias, stride=proj.stride)              # [B,E,Hp,Wp], with the bias
    patches = ref.damp(y.flatten(2).transpose(1, 2), eps)
    x0 = torch.cat((m.cls_token.expand(B, -1, -1), patches), dim=1)
    h = x0 + m.pos_embed
    N, C = h.shape[1:]
    for blk in m.blocks:
        H = blk.attn.num_heads
        qkv = ref.linear(ref.layer_norm(h, blk.norm1), blk.attn.qkv, eps)
        q, k, v = qkv.view(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
        p = ref.softmax(ref.uniform_matmul(q, k.transpose(-1, -2)) * blk.attn.scale, dim=-1)
        o = ref.uniform_matmul(p, v).permute(0, 2, 1, 3).reshape(B, N, C)
        h = ref.add(h, ref.linear(o, blk.attn.proj, eps), eps)
        mlp = blk.mlp
        h = ref.add(h, ref.linear(ref.gelu(ref.linear(ref.layer_norm(h, blk.norm2), mlp.fc1, eps)), mlp.fc2, eps), eps)
    logits = ref.linear(ref.layer_norm(h, m.norm)[:, 0], m.head, eps)
    if index is None:
        idx = logits.detach().argmax(dim=-1)
    else:
        idx = torch.as_tensor(index, device=logits.device).reshape(-1).long()
        if idx.numel() == 1 and B > 1:
            idx = idx.expand(B)
    seed = torch.zeros_like(logits)
    seed.scatter_(1, idx.view(B, 1), 1.0)
    gx, g0 = torch.autograd.grad((seed * logits).sum(), (x, x0))
    pixels = (x.detach() * gx).sum(dim=1)
    tokens = (x0.detach() * g0).sum(dim=-1)[:, 1:]
    return pixels, tokens, logits.detach()


def patch_sums(pixels, p):
    """[B,H,W] -> [B, (H/p)(W/p)]: the sum over the pixels of every p x p patch, patches in token order"""
    B, H, W = pixels.shape
    return pixels.view(B, H // p, p, W // p, p).sum(dim=(2, 4)).flatten(1)
