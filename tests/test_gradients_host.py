"""CPU: the restatement of the gradient baselines (gradients.py) against independent definitions -- brute-force loops in
Python's own doubles, Philox's known answers, the quadrature's closed forms, Integrated Gradients of a linear model in closed
form -- the refusals of GradientBaselines (all before the forward pass), and the header's new entries through the binding.
captum is not installed where this suite runs: parity with it is not claimed and nothing here imports it."""
import math
import os
import struct

import numpy as np
import pytest
import torch

from host_util import header_args, lib, same_bits  # noqa: F401
from robustness_inputs import KNOWN_ANSWERS, inputs

U = 2.0 ** -53
BF = torch.bfloat16


def te():
    from transformer_explainability_amd import gradients, ops
    return ops, gradients


def f32(v):
    """the double v rounded once to fp32 (struct packs with IEEE round-to-nearest-even), as a double"""
    return struct.unpack("f", struct.pack("f", v))[0]


# ------------------------------------------------------------------------------------------------ the restatement
def test_path_restatement_equals_a_brute_force_loop():
    ops, G = te()
    x, base = inputs(2, 35, seed=1), inputs(2, 35, seed=2)
    alphas = torch.tensor([0.0, 0.3, 0.77, 1.0])
    got = G.reference_path_inputs(x, base, alphas, s0=1, n_s=3)
    assert got.shape == (2, 3, 35) and got.dtype == torch.float32
    for b in range(2):
        for j in range(3):
            for i in range(35):
                a, xv, bv = float(alphas[1 + j]), float(x[b, i]), float(base[b, i])        # exact upcasts to double
                assert float(got[b, j, i]) == f32(bv + a * (xv - bv)), (b, j, i)
    # the ops run the restatement on CPU tensors; bf16 is the fp32 value rounded once more
    assert same_bits(ops.path_inputs(x, base, alphas, 1, 3), got)
    assert same_bits(ops.path_inputs(x, base, alphas, 1, 3, out_dtype=BF), got.to(BF))
    ends = ops.path_inputs(x.reshape(2, 1, 5, 7), base.reshape(2, 1, 5, 7), torch.tensor([0.0, 1.0]))
    assert ends.shape == (2, 2, 1, 5, 7) and same_bits(ends[:, 0], base.reshape(2, 1, 5, 7)) and same_bits(ends[:, 1], x.reshape(2, 1, 5, 7))


@pytest.mark.parametrize("square", [False, True])
def test_accumulate_restatement_equals_a_brute_force_loop(square):
    ops, G = te()
    g = torch.stack([inputs(2, 35, seed=s) for s in (3, 4, 5)], 1)                        # [2,3,35]
    w = torch.tensor([0.2, 0.5, 0.3, 0.7], dtype=torch.float64)
    start = inputs(2, 35, seed=6).double()
    got = G.reference_accumulate(g, w, start.clone(), s0=1, square=square)
    for b in range(2):
        for i in range(35):
            a = float(start[b, i])
            for j in range(3):
                t = float(g[b, j, i])
                a = a + float(w[1 + j]) * (t * t if square else t)
            assert float(got[b, i]) == a, (b, i)
    # chunks of the copies give the bits of one call; bf16 gradients are upcast exactly
    acc = start.clone()
    ops.grad_accumulate(g[:, :1], w, acc, s0=1, square=square)
    ops.grad_accumulate(g[:, 1:], w, acc, s0=2, square=square)
    assert same_bits(acc, got)
    assert same_bits(ops.grad_accumulate(g.to(BF), w, start.clone(), 1, square), G.reference_accumulate(g.to(BF).float(), w, start.clone(), 1, square))


@pytest.mark.parametrize("reduce", ["sum", "abs_sum", "max_abs"])
def test_finish_restatement_equals_a_brute_force_loop(reduce):
    ops, G = te()
    acc = inputs(2, 3 * 35, seed=7).double().reshape(2, 3, 5, 7) * 1.7
    m = inputs(2, 3 * 35, seed=8).reshape(2, 3, 5, 7)
    for mm in (m, None):
        out, sums = G.reference_finish(acc, mm, reduce)
        assert out.shape == (2, 5, 7) and out.dtype == torch.float32 and sums.shape == (2,) and sums.dtype == torch.float64
        for b in range(2):
            total = []
            for p in range(35):
                v = 0.0
                for c in range(3):
                    t = float(acc[b, c].reshape(-1)[p]) * (float(m[b, c].reshape(-1)[p]) if mm is not None else 1.0)
                    v = v + t if reduce == "sum" else v + abs(t) if reduce == "abs_sum" else max(v, abs(t))
                assert float(out[b].reshape(-1)[p]) == f32(v), (b, p)
                total.append(v)
            assert abs(float(sums[b]) - math.fsum(total)) <= 34 * U * math.fsum(abs(v) for v in total)
        got_out, got_sums = ops.grad_finish(acc, mm, reduce)
        assert same_bits(got_out, out) and same_bits(got_sums, sums) and ops.grad_finish(acc, mm, reduce, with_sums=False)[1] is None
    nan = acc.clone()
    nan[0, 1, 2, 3] = float("nan")                                      # a NaN term makes its pixel NaN in every mode, no other
    out, _ = G.reference_finish(nan, None, reduce)
    assert int(torch.isnan(out).sum()) == 1 and bool(torch.isnan(out[0, 2, 3]))


# ------------------------------------------------------------------------------------------------ Philox and the normals
def test_philox_known_answers_and_the_gauss_stream():
    _, G = te()
    for counter, key, want in KNOWN_ANSWERS:
        assert tuple(int(v) for v in G.philox4x32(counter, key)) == want
    seed, id0, d0 = 0x9e3779b97f4a7c15, (1 << 32) - 1, 5                # the ids cross 2^32: the high counter word is used
    z = G.gauss_normals(2, 10, 3, seed, id0=id0, d0=d0)
    assert z.shape == (2, 3, 10) and z.dtype == np.float64
    for b, j, e in ((0, 0, 0), (0, 2, 5), (1, 1, 9), (1, 2, 2)):
        sample = id0 + b
        w = [int(v) for v in G.philox4x32(((1 << 30) | (e >> 2), d0 + j, sample & 0xffffffff, sample >> 32),
                                          (seed & 0xffffffff, seed >> 32))]
        pair = (e & 3) // 2 * 2
        u1, u2 = (w[pair] + 0.5) * 2.0 ** -32, (w[pair + 1] + 0.5) * 2.0 ** -32
        r, t = math.sqrt(-2.0 * math.log(u1)), 2.0 * math.pi * u2
        want = r * math.cos(t) if e % 2 == 0 else r * math.sin(t)
        assert abs(z[b, j, e] - want) <= 8 * U * max(1.0, abs(want)), (b, j, e)
    # chunks of the draws and samples alone are slices of the batch's draws
    assert np.array_equal(G.gauss_normals(2, 10, 1, seed, id0=id0, d0=d0 + 2), z[:, 2:])
    assert np.array_equal(G.gauss_normals(1, 10, 3, seed, id0=id0 + 1, d0=d0), z[1:])
    # not the noise stream of the sensitivity protocol: bit 30 of the first counter word is set
    from transformer_explainability_amd import robustness
    assert not np.array_equal(robustness.noise_words(1, 4, 1, seed)[0, 0],
                              G.philox4x32(((1 << 30), 0, 0, 0), (seed & 0xffffffff, seed >> 32)))


def test_gauss_normals_are_standard_normal():
    """200000 draws: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N), |z| < 6.8 (u1 >= 2^-33), kurtosis near 3."""
    _, G = te()
    z = G.gauss_normals(2, 25000, 4, seed=11).reshape(-1)
    N = z.size
    assert abs(z.mean()) <= 5 / math.sqrt(N) and abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / N)
    assert np.abs(z).max() < 6.8 and abs((z ** 4).mean() - 3.0) <= 5 * math.sqrt(96.0 / N)
    # the four elements of a group are uncorrelated
    q = z.reshape(-1, 4)
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3)):
        assert abs((q[:, a] * q[:, b]).mean()) <= 5 / math.sqrt(q.shape[0])


def test_gauss_restatement_rounds_once_and_sigma_zero_copies():
    ops, G = te()
    x = inputs(2, 105, seed=9).reshape(2, 3, 5, 7)
    z = G.gauss_normals(2, 105, 3, seed=4, id0=7, d0=1)
    got = G.reference_gauss_inputs(x, 3, 0.25, seed=4, id0=7, d0=1)
    want = (x.reshape(2, 1, 105).double().numpy() + 0.25 * z).astype(np.float32)
    assert got.shape == (2, 3, 3, 5, 7) and np.array_equal(got.reshape(2, 3, 105).numpy(), want)
    assert same_bits(ops.gauss_inputs(x, 3, 0.25, 4, id0=7, d0=1), got)
    assert same_bits(ops.gauss_inputs(x, 3, 0.25, 4, id0=7, d0=1, out_dtype=BF), got.to(BF))
    assert same_bits(ops.gauss_inputs(x, 2, 0.0, 4), x[:, None].expand(2, 2, 3, 5, 7).contiguous())


# ------------------------------------------------------------------------------------------------ the quadrature
@pytest.mark.parametrize("rule", ["midpoint", "trapezoid", "gauss_legendre"])
@pytest.mark.parametrize("S", [2, 3, 8, 32, 128])
def test_quadrature_nodes_and_weights(rule, S):
    _, G = te()
    a, w = G.quadrature(rule, S)
    assert a.dtype == np.float64 and w.dtype == np.float64 and a.shape == (S,) == w.shape
    assert (a >= 0.0).all() and (a <= 1.0).all() and (np.diff(a) > 0).all() and (w > 0).all()
    assert abs(math.fsum(w) - 1.0) <= S * U                             # the weights sum to 1
    exact = {"midpoint": 1, "trapezoid": 1, "gauss_legendre": 2 * S - 1}[rule]
    for k in range(min(exact, 9) + 1):                                  # polynomials up to the rule's degree: 1 / (k + 1)
        assert abs(math.fsum(w * a ** k) - 1.0 / (k + 1)) <= 64 * S * U, (rule, S, k)
    if rule == "midpoint":
        assert np.array_equal(a, (np.arange(S) + 0.5) / S)
    if rule == "trapezoid":
        assert a[0] == 0.0 and a[-1] == 1.0 and w[0] == w[-1] == 0.5 / (S - 1)


def test_quadrature_refusals():
    _, G = te()
    for rule, S in (("simpson", 4), ("midpoint", 0), ("trapezoid", 1), ("gauss_legendre", -2)):
        with pytest.raises(ValueError):
            G.quadrature(rule, S)


# ------------------------------------------------------------------------------------------------ the methods on stubs
class LinearStub(torch.nn.Module):
    """logits = x . W^T: the gradient of logit k is row k of W at every input, so the methods are known in closed form"""

    def __init__(self, n, K=4, seed=0):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.randn((K, n), generator=torch.Generator().manual_seed(seed)))
        self.num_classes, self.rows = K, []

    def forward(self, x):
        self.rows.append(x.shape[0])
        return x.flatten(1) @ self.weight.t()


@pytest.mark.parametrize("rule,steps,chunk", [("midpoint", 8, None), ("trapezoid", 5, 2), ("gauss_legendre", 7, 7), ("midpoint", 12, 5)])
def test_integrated_gradients_of_a_linear_model(rule, steps, chunk):
    """logit = <w, x>: the map is sum_c w (x - base) per pixel.  With t_c = fl32(x - base) w_c exactly (what the call forms:
    x - base in fp32, the gradient w at every node) and S the number of nodes:
        |map - sum_c t_c| <= 2^-24 |v| + (C - 1 + 3 S + 1) 2^-53 sum_c |t_c|
    -- the finish bound 2^-24 |v| + (C - 1) 2^-53 sum |t| plus what precedes it in fp64: the weights sum to 1 within S 2^-53,
    the S products and S - 1 sums of the accumulation round once each (3 S in all), the product m acc once."""
    _, G = te()
    C, H, W = 3, 5, 7
    model = LinearStub(C * H * W).eval()
    x = inputs(2, C * H * W, seed=21).reshape(2, C, H, W)
    base = inputs(2, C * H * W, seed=22).reshape(2, C, H, W) * 0.1
    idx = torch.tensor([1, 3])
    gb = G.GradientBaselines(model)
    got, comp = gb.integrated_gradients(x, index=idx, steps=steps, baseline=base, rule=rule, chunk=chunk)
    assert got.shape == (2, H, W) and got.dtype == torch.float32
    n_c = min(steps, 10) if chunk is None else chunk
    passes = [2 * min(n_c, steps - s0) for s0 in range(0, steps, n_c)]
    assert model.rows == [2, 2] + passes                               # f(x), f(base), then the passes of B chunk rows
    terms = (x - base).double() * model.weight.detach()[idx].double().reshape(2, C, H, W)
    want, mag = terms.sum(1), terms.abs().sum(1)
    bound = 2.0 ** -24 * want.abs() + (C - 1 + 3 * steps + 1) * U * mag
    err = (got.double() - want).abs()
    print(f"IG linear {rule} S {steps}: worst err / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    # completeness: sum = f(x) - f(base) up to the model's own fp32 rounding of its n-term logits, (n + 2) 2^-24 sum |x w|
    assert all(t.dtype == torch.float64 and t.shape == (2,) for t in comp)
    n = C * H * W
    w = model.weight.detach()[idx].double().reshape(2, -1)
    slack = (n + 2) * 2.0 ** -24 * ((x.reshape(2, -1).double() * w).abs().sum(1) + (base.reshape(2, -1).double() * w).abs().sum(1))
    assert bool(((comp.sum - (comp.f_x - comp.f_base)).abs() <= slack).all())
    assert bool((comp.f_x - (x.reshape(2, -1).double() * w).sum(1)).abs().max() <= slack.max())


def test_baselines_resolve_like_the_curve_substrates():
    _, G = te()
    from transformer_explainability_amd import curves
    gb = G.GradientBaselines(LinearStub(3 * 8 * 8).eval(), mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.5))
    x = inputs(2, 192, seed=3).reshape(2, 3, 8, 8)
    black = gb.baseline(x, "black")
    assert black.shape == x.shape and black.dtype == torch.float32
    assert black[0, :, 0, 0].tolist() == curves.substrate_fill("black", 3, gb.mean, gb.std)
    assert float(gb.baseline(x, "zero").abs().max()) == 0.0
    assert gb.baseline(x, (1.0, 1.0, 1.0))[1, :, 3, 3].tolist() == curves.substrate_fill((1.0, 1.0, 1.0), 3, gb.mean, gb.std)
    assert same_bits(gb.baseline(x, "blur"), curves.reference_blur(x, 11, 5.0).float())
    assert same_bits(gb.baseline(x, x[:1] * 0.5), (x[:1] * 0.5).expand(2, 3, 8, 8).contiguous())


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.a, self.b = torch.nn.Linear(3 * 5 * 7, 16), torch.nn.Linear(16, 4)
        self.num_classes = 4

    def forward(self, x):
        return self.b(torch.tanh(self.a(x.flatten(1))))


@pytest.mark.parametrize("reduce", ["abs_sum", "sum", "max_abs"])
def test_smoothgrad_without_noise_is_the_plain_gradients_reduction(reduce):
    """sigma = 0: every copy is the image, so with one draw per pass every pass is the plain pass and the mean of four equal
    gradients with the weights 1/4 is that gradient exactly: the map has the bits of the reduction of the plain gradient."""
    ops, G = te()
    model = TinyNet().eval()
    x = inputs(2, 105, seed=31).reshape(2, 3, 5, 7)
    idx = torch.tensor([2, 0])
    xg = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(model(xg).gather(1, idx.view(-1, 1)).sum(), xg)
    for squared in (False, True):
        got = G.GradientBaselines(model).smoothgrad(x, index=idx, n_draws=4, sigma=0.0, squared=squared, reduce=reduce, chunk=1)
        plain = g.double() * g.double() if squared else g.double()
        assert got.shape == (2, 5, 7) and same_bits(got, ops.grad_finish(plain, None, reduce)[0]), squared
    # input x gradient on the same model: x g summed over the channels, rounded once
    ixg = G.GradientBaselines(model).input_x_gradient(x, index=idx)
    assert same_bits(ixg, ops.grad_finish(g.double(), x, "sum")[0])
    # with noise the map moves, the same seed gives the same bits, another seed another map
    gb = G.GradientBaselines(model)
    a, b, c = (gb.smoothgrad(x, index=idx, n_draws=6, sigma=0.2, seed=s, chunk=4) for s in (1, 1, 2))
    assert same_bits(a, b) and not same_bits(a, c) and not same_bits(a, gb.smoothgrad(x, index=idx, n_draws=6, sigma=0.0))


def test_the_class_is_fixed_by_one_clean_forward_pass():
    _, G = te()
    model = LinearStub(105, seed=2).eval()
    x = inputs(3, 105, seed=41).reshape(3, 3, 5, 7)
    top = (x.flatten(1) @ model.weight.detach().t()).argmax(-1)
    gb = G.GradientBaselines(model)
    assert same_bits(gb.input_x_gradient(x), gb.input_x_gradient(x, index=top))
    assert model.rows == [3, 3, 3]                                     # the clean pass, its gradient pass; the gradient pass
    assert same_bits(gb.input_x_gradient(x, index=1), gb.input_x_gradient(x, index=[1, 1, 1]))


# ------------------------------------------------------------------------------------------------ refusals
class Raises(torch.nn.Module):
    def __init__(self, dtype=torch.float32):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(4, dtype=dtype))
        self.num_classes = 4

    def forward(self, x):
        raise AssertionError("the forward pass ran")


def test_every_refusal_comes_before_the_forward_pass():
    _, G = te()
    from transformer_explainability_amd import TeError
    x = inputs(2, 105, seed=1).reshape(2, 3, 5, 7)
    calls = ("input_x_gradient", "smoothgrad", "integrated_gradients")

    def refused(model, images, match, call=None, **kw):
        for name in ([call] if call else calls):
            with pytest.raises((TeError, ValueError), match=match):
                getattr(G.GradientBaselines(model), name)(images, **kw)

    refused(Raises().train(), x, "train mode")
    refused(Raises(torch.float16).eval(), x.half(), "float16")
    refused(Raises(torch.float64).eval(), x.double(), "float64")
    refused(Raises().eval(), x.double(), "float64")
    refused(Raises(BF).eval(), x, "mixed")                              # a mix of dtypes: bf16 parameters, fp32 images
    refused(Raises().eval(), x.to(BF), "mixed")
    refused(Raises(BF).eval(), x.to(BF), "must be on the GPU")          # a bf16 model on the host
    refused(Raises().eval(), x[0], "images must be")
    refused(Raises().eval(), torch.zeros((2, 16), dtype=torch.int64), "images must be")
    refused(Raises().eval(), x, "index", index=[0, 1, 2])
    refused(Raises().eval(), x, "index", index=7)
    refused(Raises().eval(), x, "index", index=0.5)
    ok = Raises().eval()
    for bad in (0, -1, 1.5, True, None):
        refused(ok, x, "steps", "integrated_gradients", steps=bad)
    for bad in (0, 2.0, True):
        refused(ok, x, "n_draws", "smoothgrad", n_draws=bad)
        refused(ok, x, "chunk", "smoothgrad", chunk=bad)
        refused(ok, x, "chunk", "integrated_gradients", chunk=bad)
    refused(ok, x, "rule", "integrated_gradients", rule="simpson")
    refused(ok, x, "steps", "integrated_gradients", rule="trapezoid", steps=1)
    refused(ok, x, "baseline", "integrated_gradients", baseline="white")
    refused(ok, x, "values", "integrated_gradients", baseline=(0.0, 0.0))
    refused(ok, x, "reduce", "smoothgrad", reduce="mean")
    for bad in (-0.1, float("nan"), float("inf"), "0.1"):
        refused(ok, x, "sigma", "smoothgrad", sigma=bad)
    # ... and a call that is not refused does reach the forward pass
    for name in calls:
        with pytest.raises(AssertionError, match="the forward pass ran"):
            getattr(G.GradientBaselines(ok), name)(x)


def test_ops_refuse_on_the_host():
    ops, _ = te()
    from transformer_explainability_amd import TeError
    x, base = inputs(2, 8), inputs(2, 8, seed=1)
    al, w, acc = torch.tensor([0.5, 1.0]), torch.ones(2, dtype=torch.float64), torch.zeros((2, 8), dtype=torch.float64)
    for bad in (lambda: ops.path_inputs(x, base, al, s0=-1), lambda: ops.path_inputs(x, base, al, s0=1, n_s=2),
                lambda: ops.path_inputs(x, base[:1], al), lambda: ops.path_inputs(x.double(), base, al),
                lambda: ops.path_inputs(x, base, al, out_dtype=torch.float16),
                lambda: ops.path_inputs(x, base, al, out=torch.empty((2, 2, 9))),
                lambda: ops.gauss_inputs(x, 2, -1.0, 0), lambda: ops.gauss_inputs(x, 2, float("nan"), 0),
                lambda: ops.gauss_inputs(x, 0, 0.1, 0), lambda: ops.gauss_inputs(x, 2, 0.1, 0, d0=(1 << 32) - 1),
                lambda: ops.gauss_inputs(x, 1, 0.1, 1 << 64),
                lambda: ops.grad_accumulate(x[:, None], w, acc, s0=2), lambda: ops.grad_accumulate(x[:, None], w.float(), acc),
                lambda: ops.grad_accumulate(x[:, None], w, acc.float()), lambda: ops.grad_accumulate(x[:, None], w, acc[:, :7]),
                lambda: ops.grad_finish(acc.reshape(2, 2, 4), None, "mean"), lambda: ops.grad_finish(acc, None),
                lambda: ops.grad_finish(acc.reshape(2, 2, 4), x.reshape(2, 4, 2)),
                lambda: ops.grad_finish(acc.reshape(2, 2, 4).float(), None)):
        with pytest.raises(TeError):
            bad()


# ------------------------------------------------------------------------------------------------ header and binding
ENTRIES = {
    "te_path_inputs_f32": ("x", "base", "alphas", "out", "B", "n", "S", "s0", "n_s", "stream"),
    "te_gauss_inputs_f32": ("x", "out", "B", "n", "d0", "n_d", "sigma", "seed", "id0", "stream"),
    "te_grad_accumulate_f32": ("g", "w", "acc", "B", "n", "n_s", "s0", "square", "stream"),
    "te_grad_finish_f64": ("acc", "m", "out", "sums", "B", "C", "HW", "reduce", "stream"),
}


def test_header_and_binding_agree_on_the_new_entries(lib):  # noqa: F811
    """The mechanism of test_cabi.py: _lib binds what _cabi parses from the header, the library exports it."""
    from ctypes import c_double, c_int, c_int64, c_void_p
    from transformer_explainability_amd import _lib, ops
    for name, params in ENTRIES.items():
        for n in {name, name.replace("_f32", "_bf16")}:
            assert _lib.PARAMS[n] == params and header_args(n) == len(params) and hasattr(lib, n), n
            assert _lib.SIGNATURES[n][0] is c_int and len(_lib.SIGNATURES[n][1]) == len(params)
    assert "te_grad_finish_bf16" not in _lib.SIGNATURES
    assert _lib.SIGNATURES["te_gauss_inputs_bf16"][1] == [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_double, c_int64,
                                                          c_int64, c_void_p]
    assert _lib.SIGNATURES["te_grad_finish_f64"][1] == [c_void_p] * 4 + [c_int64] * 3 + [c_int, c_void_p]
    assert (_lib.TE_GRAD_SUM, _lib.TE_GRAD_ABS_SUM, _lib.TE_GRAD_MAX_ABS) == (0, 1, 2)
    assert ops.GRAD_REDUCE == {"sum": 0, "abs_sum": 1, "max_abs": 2}


def test_entry_points_reject_on_the_host(lib):  # noqa: F811
    """What every entry answers before it touches a device.  P is a fake non-null, 16-byte-aligned address that the host
    never dereferences; every call below returns before the first HIP call."""
    P, nan, inf = 4096, float("nan"), float("inf")

    def status(lib, fn, args, **changed):      # (host_util.status names its second dict `base`, as te_path_inputs does an argument)
        assert set(changed) <= set(args), changed
        return getattr(lib, fn)(*{**args, **changed}.values())

    path = dict(x=P, base=P, alphas=P, out=P, B=2, n=8, S=3, s0=0, n_s=3, stream=None)
    for f in ("te_path_inputs_f32", "te_path_inputs_bf16"):
        assert [status(lib, f, path, **{k: None}) for k in ("x", "base", "alphas", "out")] == [-1] * 4
        assert [status(lib, f, path, **c) for c in (dict(B=0), dict(n=0), dict(n_s=0), dict(S=0), dict(s0=-1), dict(s0=1),
                                                    dict(s0=3, n_s=1), dict(n_s=4))] == [-1] * 8
        assert [status(lib, f, path, **c) for c in (dict(x=P + 2), dict(base=P + 1), dict(alphas=P + 3), dict(B=65536),
                                                    dict(n=1 << 31))] == [-3] * 5
    assert status(lib, "te_path_inputs_f32", path, out=P + 2) == -3 and status(lib, "te_path_inputs_bf16", path, out=P + 1) == -3
    gauss = dict(x=P, out=P, B=2, n=8, d0=0, n_d=2, sigma=0.1, seed=0, id0=0, stream=None)
    for f in ("te_gauss_inputs_f32", "te_gauss_inputs_bf16"):
        assert [status(lib, f, gauss, **c) for c in (dict(x=None), dict(out=None), dict(n_d=0), dict(d0=-1), dict(sigma=-0.5),
                                                     dict(sigma=nan), dict(sigma=inf), dict(d0=(1 << 32) - 1))] == [-1] * 8
        assert [status(lib, f, gauss, **c) for c in (dict(x=P + 1), dict(out=P + 1), dict(B=65536), dict(n=1 << 31))] == [-3] * 4
    accum = dict(g=P, w=P, acc=P, B=2, n=8, n_s=2, s0=0, square=0, stream=None)
    for f in ("te_grad_accumulate_f32", "te_grad_accumulate_bf16"):
        assert [status(lib, f, accum, **c) for c in (dict(g=None), dict(w=None), dict(acc=None), dict(n_s=0), dict(s0=-1))] == [-1] * 5
        assert [status(lib, f, accum, **c) for c in (dict(g=P + 1), dict(w=P + 4), dict(acc=P + 4), dict(B=65536))] == [-3] * 4
    finish = dict(acc=P, m=None, out=P, sums=None, B=2, C=3, HW=8, reduce=0, stream=None)
    f = "te_grad_finish_f64"
    assert [status(lib, f, finish, **c) for c in (dict(acc=None), dict(out=None), dict(C=0), dict(HW=0), dict(reduce=3),
                                                  dict(reduce=-1))] == [-1] * 6
    assert [status(lib, f, finish, **c) for c in (dict(acc=P + 4), dict(out=P + 2), dict(m=P + 2), dict(sums=P + 4),
                                                  dict(B=65536))] == [-3] * 5


def test_the_new_kernel_file_is_built_and_shares_the_headers_primitives():
    """csrc/te_gradients.hip is a source of the library and defines none of the primitives of te_common.h a second time
    (tests/test_csrc_shared.py checks every file of csrc/; here: the file is among them and uses the shared ones)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "transformer-explainability_amd")
    spec = importlib.util.spec_from_file_location("_te_build_g", os.path.join(pkg, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "te_gradients.hip" in mod.SOURCES
    text = open(os.path.join(pkg, "csrc", "te_gradients.hip")).read()
    for used in ("philox4x32_10(", "te_pack_bf16(", "te_load4_f64<", "te_block_sum(", '#include "te_common.h"'):
        assert used in text, used
    assert "atomic" not in text.replace("no atomics", "")
