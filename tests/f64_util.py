"""Helpers of the fp64 tests (tests/test_f64_host.py, tests/test_gpu_f64.py): fp64 cache adapters, fp64 statistics and the
a-priori rounding bounds of the rules.

gpu_util.map_stats and oracle.model_cache._cpu cast to float32 and are useless for an fp64 model; the adapters here are the
oracle's own (same dict layout) with that one cast replaced by ``.double()``.

Bounds.  u = 2^-53 is the unit roundoff of fp64.  A sum of n terms t_k evaluated in ANY order errs by at most
(n - 1) u sum|t_k| (to first order), a product or quotient by u relative; the bound of an output is u times (the
contraction lengths on its path + a small constant for the element-wise steps) times the sum of the absolute values of the
terms of its expression, taken from the oracle's intermediates.  Both the kernels and the oracle round in fp64, so the tests
assert |got - oracle| <= 2 bound.  No constant is fitted to a measurement."""
import os
import sys
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import model_cache  # noqa: E402
from oracle import relprop_oracle as O  # noqa: E402

U = 2.0 ** -53
F64 = torch.float64


def cpu64(t):
    return None if t is None else t.detach().double().cpu()


def vit_cache_f64(model):
    """oracle.model_cache.vit_cache_from_model with every tensor upcast / kept in double."""
    with mock.patch.object(model_cache, "_cpu", cpu64):
        return model_cache.vit_cache_from_model(model)


def bert_cache_f64(model):
    with mock.patch.object(model_cache, "_cpu", cpu64):
        return model_cache.bert_cache_from_model(model)


def rnd64(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64) * scale


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def minmax64(m):
    flat = m.detach().double().cpu().reshape(m.shape[0], -1)
    lo, hi = flat.min(1, keepdim=True).values, flat.max(1, keepdim=True).values
    return (flat - lo) / (hi - lo)


def norm_err(got, ref):
    """The project's parity statistic, evaluated in double: max |minmax(got) - minmax(ref)| over the batch."""
    return float((minmax64(got) - minmax64(ref)).abs().max())


def ratio_to_bound(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf)."""
    err = (got.detach().double().cpu() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


# ------------------------------------------------------------------------------------------------ bounds
def linear_bound(R, X, W):
    """(in_f + out_f + 6) u |x_i| (|S| |W^{sign x_i}|)_i.  Z = X+ W+^T + X- W-^T is a sum of in_f non-negative terms (no
    cancellation: relative error <= (in_f + 1) u), S = sd(R, Z) adds three roundings, the C-pass a sum of out_f terms S_o
    W_oi of either sign (error <= out_f u sum_o |S_o| |W_oi|) and the product with x_i and the final sum two more."""
    out_f, in_f = W.shape
    pw, nw, px, nx = W.clamp(min=0), W.clamp(max=0), X.clamp(min=0), X.clamp(max=0)
    S = O.safe_divide(R, px.matmul(pw.t()) + nx.matmul(nw.t())).abs()
    terms = px * S.matmul(pw) + nx.abs() * S.matmul(nw.abs())
    return (in_f + out_f + 6) * U * terms


def matmul_rule_bounds(R, X0, X1, z):
    """Generic RelPropSimple rule with Z an operand: out0 = X0 . (S X1^T) contracts X1's columns (n1 terms), out1 =
    X1 . (X0^T S) contracts X0's rows (n0 terms); S = sd(R, Z) is two roundings of exact inputs, the gate and the sum's
    own last step two more: (n + 4) u |X| (|S| |X'|)."""
    S = O.safe_divide(R, z).abs()
    n1, n0 = X1.shape[-1], X0.shape[-2]
    b0 = (n1 + 4) * U * X0.abs() * S.matmul(X1.abs().transpose(-1, -2))
    b1 = (n0 + 4) * U * X1.abs() * X0.abs().transpose(-1, -2).matmul(S)
    return b0, b1


def add_bounds(R, X0, X1):
    """Add 'ours' per sample b (dim 0): a = X0 S, b = X1 red(S) with S = sd(R, X0 + X1) (four roundings: 4 u relative),
    sums A = sum a, Bs = sum b, Rs = sum R over n elements in some order: each errs by <= (n + 4) u sum|terms|.  The factors
    are fa = +- Rs / (|A| + |Bs|) up to six roundings (the |A| / A of the expression cancels to a sign), so
        d = (n + 4) u [ (sum|a| + sum|b|) / (|A| + |Bs|) + sum|R| / |Rs| ] + 8 u
    bounds their relative error -- the condition numbers of the three sums are in it -- and
        |out0 - ref| <= |a| |fa| (d + 6 u),   |out1 - ref| <= |X1| red(|S|) |fb| (d + (m + 6) u)
    where red sums S over the m positions a broadcast X1 element serves (m = 1 for same-shape operands) and sum|b| uses
    |X1| red(|S|): the conditioning of the column sums is included."""
    B = R.shape[0]
    n = X0[0].numel()
    b0s, b1s = [], []
    for i in range(B):
        r, x0 = R[i:i + 1], X0[i:i + 1]
        x1 = X1[i:i + 1] if X1.shape[0] == B else X1
        S = O.safe_divide(r, x0 + x1)
        a, b = x0 * S, x1 * O._reduce_to(S, x1.shape)
        b_abs = x1.abs() * O._reduce_to(S.abs(), x1.shape)
        m = S.numel() // x1.numel()
        A, Bs, Rs = a.sum(), b.sum(), r.sum()
        den = A.abs() + Bs.abs()
        fa = O.safe_divide(O.safe_divide(A.abs(), den) * Rs, A).abs()
        fb = O.safe_divide(O.safe_divide(Bs.abs(), den) * Rs, Bs).abs()
        if float(den) == 0.0 or float(Rs) == 0.0:
            d = torch.tensor(0.0, dtype=F64)            # (both factors are exactly zero on either side)
        else:
            d = (n + 4) * U * ((a.abs().sum() + b_abs.sum()) / den + r.abs().sum() / Rs.abs()) + 8 * U
        b0s.append(a.abs() * fa * (d + 6 * U))
        b1s.append(b_abs * fb * (d + (m + 6) * U))
    return torch.cat(b0s, 0), torch.cat(b1s, 0)


def headmean_bound(grad, cam):
    """(H + 2) u mean_h |g c|: one product, a sum of H terms, one division."""
    H = grad.shape[1]
    return (H + 2) * U * (grad * cam).abs().mean(dim=1)
