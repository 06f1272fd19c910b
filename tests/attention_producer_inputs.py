"""Seeded operands for the attention PRODUCERS (the kernels that make attn, out, d_attn, d_q, d_k and d_v): heads that differ
by 2^-40, softmax rows from near uniform to one-hot inside one head, scores that carry +-200, a key whose score lifts the
running maximum at a chosen position, and the additive masks a BERT model can meet.  No device needed.

q, k, v and g_out are [B,H,N,64] fp32 draws of dynamic_range_inputs.rnd; every scale is a power of two, so scaling is exact
and kernel(2^-k v) == 2^-k kernel(v) must hold bit for bit while no value leaves the normal range.  The x6 kernels keep an
operand as three bf16 planes, the third 2^-16 below the value (the note in dynamic_range_inputs.attention_case): the smallest
head here is 2^-40, the homogeneity checks scale by a further 2^-24, and a Gaussian draw of a million is ~2^-20 at its
smallest -- the third plane of the smallest value is still ~2^-100, normal.  v and g_out are scaled in separate cases because
d_q and d_k carry their product.

Shared by tests/test_attention_producer_range_host.py (the bound is fair: an independently ordered fp32 restatement stays
within 3/4 of it; three mutants fail it) and tests/test_gpu_attention_producer_range.py (the kernels)."""
import torch

from dynamic_range_inputs import pow2, rnd

B, H, D = 2, 3, 64
SCALE = D ** -0.5          # 2^-3: exact
HOMOGENEITY_K = (1, 24)
MASKED_AWAY = -10000.0     # (1 - 0) * -10000 of BERT's extended attention mask; -9984 in bf16

UNMASKED_CASES = ["v_scaled", "g_scaled", "temperature", "offset_pos", "offset_neg", "dominant_key_0", "dominant_chunk0_last",
                  "dominant_last_chunk_first", "dominant_key_last"]
MASK_CASES = ["first_chunk", "stripes", "all_but_one", "all_masked", "soft", "per_sample", "fmin", "all_fmin"]
LARGEST_N_CASES = ["temperature", "offset_pos", "first_chunk"]      # what the largest N of every entry takes
# masks whose masked keys sit beside an unmasked key of the same sample: attn, d_v rows and d_k rows of those keys are exactly 0
EXACT_ZERO_CASES = ["first_chunk", "stripes", "all_but_one", "per_sample", "fmin"]


def head_scale():
    """(b, h) x 2^-(8 (b H + h)): 2^0 ... 2^-40."""
    return pow2(-8 * torch.arange(B * H)).view(B, H, 1, 1)


def dominant_position(case, N, chunk):
    """The key that is scaled by 6: where the running maximum of an online softmax over `chunk` keys rises."""
    return {"dominant_key_0": 0, "dominant_chunk0_last": min(chunk, N) - 1, "dominant_last_chunk_first": chunk * ((N - 1) // chunk),
            "dominant_key_last": N - 1}[case]


def first_chunk_keys(N):
    return min(64, N - 1)


def mask_of(case, N, bf16=False):
    """Additive mask [B,1,1,N] fp32 (bf16: the bf16 value of every entry, as fp32), or None."""
    if case not in MASK_CASES:
        return None
    away = float(torch.tensor(MASKED_AWAY).bfloat16()) if bf16 else MASKED_AWAY
    m = torch.zeros(B, 1, 1, N)
    if case == "first_chunk":
        m[..., :first_chunk_keys(N)] = away
    elif case == "stripes":
        m[..., ::3] = away
    elif case == "all_but_one":
        m[...] = away
        m[..., N // 2] = 0.0
    elif case == "all_masked":
        m[0] = away                                  # sample 0: every key; sample 1: none
    elif case == "soft":
        m[..., 1::3] = -1.0
        m[..., 2::3] = -3.0
    elif case == "per_sample":
        m[1, ..., :first_chunk_keys(N)] = away       # sample 0 unmasked
    elif case == "fmin":                             # what current HF models export
        m[..., ::3] = torch.finfo(torch.bfloat16 if bf16 else torch.float32).min
    elif case == "all_fmin":                         # sample 0: every key at finfo.min -- x + mask = finfo.min for every key, in
        m[0] = torch.finfo(torch.bfloat16 if bf16 else torch.float32).min      # fp64 too (ulp 7.5e22): a uniform row, never NaN
    return m


def producer_case(case, N, chunk=32, bf16=False, seed=1200):
    """{q, k, v, g: [B,H,N,64] fp32, mask: [B,1,1,N] fp32 or None}; bf16: every operand holds bf16 values (widened exactly).
      v_scaled / g_scaled : v / g_out of head (b, h) x 2^-(8 (b H + h))
      temperature         : query row n of q x 2^((n // 8) mod 7 - 1): 0.5 ... 32, near uniform to one-hot inside one head
      offset_pos / _neg   : q[..., 0] = 40, k[..., 0] = +-40: every scaled score carries +-200
      dominant_*          : one key x 6 (dominant_position)
      mask cases          : unit-scale operands under mask_of(case)"""
    q, k, v, g = (rnd((B, H, N, D), seed + i) for i in range(4))
    if case == "v_scaled":
        v = v * head_scale()
    elif case == "g_scaled":
        g = g * head_scale()
    elif case == "temperature":
        n = torch.arange(N)
        q = q * pow2((n // 8) % 7 - 1).view(1, 1, N, 1)
    elif case in ("offset_pos", "offset_neg"):
        q[..., 0] = 40.0
        k[..., 0] = 40.0 if case == "offset_pos" else -40.0
    elif case.startswith("dominant_"):
        k[:, :, dominant_position(case, N, chunk)] *= 6.0
    elif case not in MASK_CASES:
        raise ValueError(case)
    if bf16:
        q, k, v, g = (t.bfloat16().float() for t in (q, k, v, g))
    return {"q": q, "k": k, "v": v, "g": g, "mask": mask_of(case, N, bf16)}


def merge_heads(t):
    """[B,H,N,D] -> 'b n (h d)'"""
    b, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, n, h * d)


def split_heads(t, heads=H):
    """'b n (h d)' -> [B,H,N,D] (a view)"""
    b, n, c = t.shape
    return t.view(b, n, heads, c // heads).permute(0, 2, 1, 3)


def fused_layout(c):
    """(qkv [B,N,3C] 'b n (qkv h d)', g_out [B,N,C]) of a case."""
    return torch.cat([merge_heads(c[n]) for n in ("q", "k", "v")], -1).contiguous(), merge_heads(c["g"]).contiguous()


def split_fused(qkv, heads=H):
    """[B,N,3C] -> q, k, v [B,H,N,D] views"""
    b, n, c3 = qkv.shape
    return qkv.view(b, n, 3, heads, c3 // 3 // heads).permute(2, 0, 3, 1, 4)


def three_layout(c):
    """(q, k, v, g_out), each [B,N,C] 'b n (h d)' and contiguous."""
    return tuple(merge_heads(c[n]).contiguous() for n in ("q", "k", "v", "g"))


NAMES = ("z_qk", "attn", "out", "d_attn", "d_q", "d_k", "d_v")


def chain(q, k, v, g, mask, scale=SCALE):
    """The attention block with stock torch ops in the dtype and on the device of its operands ([B,H,N,D]), gradients by
    autograd: z_qk, x (scaled scores before the mask), attn, out, d_attn, d_q, d_k, d_v."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    z = q @ k.transpose(-1, -2)
    x = z * scale
    s = x if mask is None else x + mask.to(device=x.device, dtype=x.dtype)
    attn = torch.softmax(s, dim=-1)
    attn.retain_grad()
    out = attn @ v
    out.backward(g.to(out.dtype))
    return {"z_qk": z.detach(), "x": x.detach(), "attn": attn.detach(), "out": out.detach(), "d_attn": attn.grad,
            "d_q": q.grad, "d_k": k.grad, "d_v": v.grad}


def chain64(c, scale=SCALE):
    """The fp64 chain on the exactly widened operands of a case: the reference of every comparison."""
    return chain(c["q"].double(), c["k"].double(), c["v"].double(), c["g"].double(),
                 None if c["mask"] is None else c["mask"].double(), scale)


# ------------------------------------------------------------------------------------------------ the bound
TOL = {"attn": 3e-6, "out": 3e-6, "d_attn": 3e-6, "d_v": 3e-6, "d_q": 1e-5, "d_k": 1e-5}      # the bars of test_gpu_producers.py
BF16_TOL = 2.0 ** -7                     # one bf16 ulp of the group's maximum
GROUP_DIMS = {"attn": -1, "out": -1, "d_attn": -1, "d_q": -1, "d_k": (-2, -1), "d_v": (-2, -1)}      # per query row / per (b, h)
ROW_SUM_TOL, BF16_ROW_SUM_TOL = 1e-5, 2e-2


def score_magnitude(ref64):
    """[B,H,N]: per query row, the largest |scaled score| BEFORE the mask.  (A sample with every key masked rounds its
    scores at ulp(10000), far above ulp(|x|); the stock chain does the same, and 2 x err_stock carries that case:
    tests/test_attention_producer_range_host.py holds the restatement to 3/4 of the bound there too.)"""
    return ref64["x"].abs().amax(-1)


def bound_terms(name, c, ref64, scale=SCALE):
    """(xmax_g, scale_floor_g) of output `name`, shaped like its groups (or None): the score term 4 x 2^-24 xmax_g stands for
    four roundings of a score at half an ulp each (product, scaling, mask addition, max subtraction) and is absent for
    d_attn = d_out v^T, which no score enters; d_q and d_k are judged against at least the magnitude of the terms that
    cancel in d_s = p (d_attn - rowsum): scale max|d_attn| max(|q|, |k|) of the (b, h), as tests/test_gpu_producers.py does."""
    rows = score_magnitude(ref64)                       # [B,H,N]
    per_row = GROUP_DIMS[name] == -1
    xmax = None if name == "d_attn" else (rows if per_row else rows.amax(-1))
    floor = None
    if name in ("d_q", "d_k"):
        nat = scale * ref64["d_attn"].abs().amax((-2, -1)) * torch.maximum(c["q"].abs().amax((-2, -1)), c["k"].abs().amax((-2, -1))).double()
        floor = nat[..., None].expand_as(rows) if per_row else nat
    return xmax, floor
