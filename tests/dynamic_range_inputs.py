"""Seeded operands whose independent problems (rows, heads, samples) differ by many orders of magnitude -- what real
relevance looks like (only the CLS row non-zero at the last block, rows spanning decades further down, outlier channels
and biases in the activations), and what a unit-scale Gaussian never shows.  No device needed.

Every scale is a power of two, so scaling is exact: the oracle's result on a scaled operand is known, and
rule(2^-k R) == 2^-k rule(R) must hold bit for bit as long as no value leaves the normal range (the smallest relevance
built here is 0.01 x 2^-40 x a Gaussian draw, ~2^-60; the homogeneity checks scale by a further 2^-48 at most).

The cases are shared by tests/test_dynamic_range_host.py (the fp32 oracle meets a quarter of every bar on them: the
inputs are fair; three mutants of it fail: the checks bite) and tests/test_gpu_dynamic_range.py (the kernels)."""
import torch

HOMOGENEITY_K = (1, 24, 48)

LINEAR_FWD_SHAPES = [(140, 256, 192), (140, 256, 256), (300, 768, 768)]      # fp32-MFMA, x6 128-wide tiles, x6 256 x 256
LINEAR_NOY_SHAPES = [(140, 256, 192), (7, 10, 2)]
LINEAR_BF16_SHAPE = (130, 128, 256)      # the smallest the bf16-operand MFMA route takes with two row tiles
LINEAR_F64_SHAPE = (130, 72, 40)
LINEAR_CASES = ["r_scaled", "x_scaled", "xr_scaled", "bias_scaled", "cls_only"]
ATTN_SHAPES = [(2, 3, 65, 64), (1, 2, 130, 64)]
ATTN_CASES = ["head_scaled", "row_scaled", "cls_only"]
ADD_SHAPES = [(3, 9, 16), (2, 5, 3)]
ADD_MASK_SHAPE = (2, 3, 33)
LN_ROWS = 9
LN_WIDTHS = [4, 260, 1028, 1540, 2048]      # 1028, 1540: the half-empty NV = 6 and NV = 8 instantiations


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def pow2(e):
    """2^e as an exact fp32 tensor (e: integer tensor or int)."""
    return torch.ldexp(torch.ones((), dtype=torch.float32), torch.as_tensor(e, dtype=torch.int32))


def row_scale(T):
    """Row t scaled by 2^-(8 (t // 16 mod 6)): 2^0 ... 2^-40 in runs of 16 rows."""
    t = torch.arange(T)
    return pow2(-8 * ((t // 16) % 6))


def samples_of(T):
    """(B, N) with B N = T for the CLS-only variant: samples of N tokens."""
    for B in (3, 2):
        if T % B == 0 and T // B >= 7:
            return B, T // B
    return 1, T


def linear_case(case, T, in_f, out_f, seed=500):
    """X [T,in], W [out,in], bias [out], R [T,out] of one Linear layer.
      r_scaled    : row t of R x 2^-(8 (t // 16 mod 6)); row 5 of R all zero
      x_scaled    : every 8th row of X x 2^-(2 (t // 8 mod 16)) (2^0 ... 2^-30; 7 of 8 rows keep unit scale, so no tile
                    is made of small rows only), four outlier channels x 2^6, an all-zero row of X; unit-scale bias
      xr_scaled   : x_scaled, and the scaled rows of X carry relevance x 2^-24 (a token that is small in the activations and
                    in the relevance: the whole-tensor metric cannot see these rows at all)
      bias_scaled : every 8th bias element x 2^14 (X at unit scale)
      cls_only    : R non-zero on row 0 of each sample only"""
    X, W, R = rnd((T, in_f), seed), rnd((out_f, in_f), seed + 1, 0.05), rnd((T, out_f), seed + 2, 0.01)
    bias = rnd((out_f,), seed + 3, 0.3)
    if case == "r_scaled":
        R = R * row_scale(T)[:, None]
        R[min(5, T - 1)] = 0.0
    elif case in ("x_scaled", "xr_scaled"):
        t = torch.arange(T)
        s = torch.where(t % 8 == 3, pow2(-2 * ((t // 8) % 16)), torch.ones(T))
        X = X * s[:, None]
        X[:, [1, in_f // 3, in_f // 2 + 1, in_f - 2]] *= 64.0
        if T > 12:
            X[12] = 0.0
        if case == "xr_scaled":
            R = R * torch.where(t % 8 == 3, pow2(-24), torch.ones(()))[:, None]
    elif case == "bias_scaled":
        bias[::8] *= 16384.0
    elif case == "cls_only":
        B, N = samples_of(T)
        keep = torch.zeros(T, 1)
        keep[::N] = 1.0
        R = R * keep
    else:
        raise ValueError(case)
    return {"X": X, "W": W, "bias": bias, "R": R}


def attention_case(case, B, H, N, D, seed=600):
    """Positive q, k, v (every Z a sum of positive products: well conditioned), fused 'b n (qkv h d)' layout as the model
    holds it, and R [B,H,N,D]:
      head_scaled : (b,h) x 2^-(8 (b H + h))
      row_scaled  : query row n x 2^-(8 (n // 16 mod 6)) inside every head; row 3 all zero
      cls_only    : only query row 0 of every head non-zero"""
    C = H * D
    qkv = rnd((B, N, 3 * C), seed).abs() + 0.05
    # R at unit scale: the kernels keep R / Z as three bf16 planes, the third 2^-16 below the value.  With the 2^-40 of the
    # smallest head and the 2^-48 of the homogeneity check, a value 2^-16 below its row's typical size still has a normal
    # third plane (2^-120); with R ~ 0.01 such planes went subnormal and the bitwise equality was lost to their flushing.
    R = rnd((B, H, N, D), seed + 1)
    if case == "head_scaled":
        R = R * pow2(-8 * torch.arange(B * H)).view(B, H, 1, 1)
    elif case == "row_scaled":
        R = R * row_scale(N).view(1, 1, N, 1)
        R[:, :, 3] = 0.0
    elif case == "cls_only":
        R[:, :, 1:] = 0.0
    else:
        raise ValueError(case)
    return {"qkv": qkv, "R": R}


def sample_scale(B):
    """Sample b x 2^-(40 b / (B - 1)): 2^0 ... 2^-40."""
    return pow2(-(40 * torch.arange(B)) // max(B - 1, 1))


def add_case(shape, seed=700):
    """Add / Clone operands with samples at 2^0 ... 2^-40.  X0 and X1 share a random sign per element and R > 0, so
    Z = X0 + X1 takes both signs while every per-sample sum of the rescaling (layers_ours.py:109-116) is a sum of
    positive terms: the fp32 oracle is then accurate ELEMENT-wise and an element-wise bound is fair."""
    sgn = torch.where(rnd(shape, seed) < 0, -1.0, 1.0)
    X0, X1 = sgn * (rnd(shape, seed + 1).abs() + 0.05), sgn * (rnd(shape, seed + 2).abs() + 0.05)
    s = sample_scale(shape[0]).view(-1, *([1] * (len(shape) - 1)))
    R = (rnd(shape, seed + 3, 0.01).abs() + 1e-4) * s
    R2 = (rnd(shape, seed + 4, 0.01).abs() + 1e-4) * s
    R3 = (rnd(shape, seed + 5, 0.01).abs() + 1e-4) * s
    return {"X0": X0, "X1": X1, "R": R, "R2": R2, "R3": R3}


def add_mask_case(B, H, N, seed=720):
    """Broadcast-mask Add (BERT: scores [B,H,N,N] + mask [B,1,1,N]); masked keys carry no relevance, as in the model."""
    X0 = rnd((B, H, N, N), seed).abs() + 0.05
    R = (rnd((B, H, N, N), seed + 1, 0.01).abs() + 1e-4) * sample_scale(B).view(B, 1, 1, 1)
    mask = torch.zeros(B, 1, 1, N)
    m = max(1, N // 5)
    mask[..., N - m:] = -10000.0
    R[..., N - m:] = 0.0
    return {"X0": X0, "mask": mask, "R": R}


def layernorm_case(C, seed=800):
    """T = 9 rows: row r = (offset_r + N(0,1)) x 2^(3 r - 14), offset 0 / 64 / 4096 in turn -- mean / std up to 2^12, row
    scales 2^-14 ... 2^10 (variance from far below to far above eps = 1e-6)."""
    T = LN_ROWS
    off = torch.tensor([0.0, 64.0, 4096.0]).repeat(3)[:, None]
    x = (off + rnd((T, C), seed)) * pow2(3 * torch.arange(T) - 14)[:, None]
    w = rnd((C,), seed + 1) * 0.5 + 1.0
    b = rnd((C,), seed + 2)
    dy = rnd((T, C), seed + 3)
    return {"x": x, "w": w, "b": b, "dy": dy}


def gelu_case(seed=900):
    """x on [-9, 9]: a regular grid (the negative tail, where |gelu(x)| < 1e-5, included) plus Gaussian draws."""
    grid = torch.linspace(-9.0, 9.0, 36001, dtype=torch.float64).float()
    x = torch.cat([grid, rnd((27999,), seed) * 3.0]).clamp(-9.0, 9.0)      # 64000 elements, a multiple of 4
    dy = rnd(tuple(x.shape), seed + 1)
    return {"x": x, "dy": dy}


def ulp_distance(a, b):
    """Distance of two fp32 tensors in units in the last place (monotone integer image of the floats)."""
    def key(t):
        i = t.detach().cpu().contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    return (key(a) - key(b)).abs()


def attention_operands(qkv, B, H, N, D):
    """q, k, v [B,H,N,D] as views of the fused activation, and the softmax probabilities the forward pass would cache."""
    q, k, v = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    attn = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1).contiguous()
    return q, k, v, attn


def elementwise_excess(got, ref64, rel):
    """(worst |got - ref64| / |ref64| over the non-zero elements of ref64 in units of `rel`, got is zero wherever ref64
    is): the element-wise bound of the streaming rules."""
    got, ref64 = got.detach().cpu().double(), ref64.detach().cpu().double()
    nz = ref64 != 0
    worst = float(((got - ref64).abs()[nz] / ref64.abs()[nz]).max()) / rel if bool(nz.any()) else 0.0
    return worst, bool((got[~nz] == 0).all()) and bool(torch.isfinite(got).all())
