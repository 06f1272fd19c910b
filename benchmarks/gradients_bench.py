"""The gradient-baseline kernels (csrc/te_gradients.hip) beside the torch composition of the same steps, in one process on the
same device tensors, and one whole Integrated Gradients / SmoothGrad call beside the same protocol composed in torch.

    python benchmarks/gradients_bench.py [--rounds 5] [--window-ms 200] [--warmup 2] [--skip-model] [--model-rounds 2]
                                         [--chunk 4] [--out F]

Configuration: ViT-B/16 shapes, batch 64, 3 x 224 x 224 normalised inputs (n = 150528), n_s = 8 copies per sample and launch,
fp32 and bf16 copies and gradients.  Prints one JSON line (and writes it to --out, default profiles/gradients_bench.json):
  * path: one ops.path_inputs launch of 64 x 8 copies beside ``base + a (x - base)`` broadcast in torch -- in fp32 (what a
    user composes; other bits) and in fp64 with one rounding (the kernel's definition).
  * gauss: one ops.gauss_inputs launch beside ``x + sigma * randn`` of torch (another generator: only the time is comparable).
  * accumulate: one ops.grad_accumulate launch over 64 x 8 gradients beside ``acc += (g.double() * w).sum(1)``.
  * finish: one ops.grad_finish launch (map and per-sample sums) beside ``v = (m.double() * acc).sum(1)``, ``v.float()``,
    ``v.sum``.
  Each with the bytes the step must move over the kernel's time, as a share of the measured copy rate of the part, 6.29 TB/s.
  * calls: integrated_gradients(steps=32) and smoothgrad(n_draws=25) of GradientBaselines on vit_base_patch16_224, --chunk
    copies per sample and pass, beside the same passes with the copies and the sums composed in torch.  The forward and
    backward passes are the protocol and dominate both sides; ``kernels_ms`` times the call's own launches alone.
The versions alternate, --rounds timed windows each (host clock between two device synchronisations) after a warm-up;
reported: median, min and max.  The yardstick of every time is the torch composition on the device; no ratio is promised,
the result is written down whichever way it falls.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmarks._models import vit_b16  # noqa: E402
from benchmarks._timing import MEASURED_COPY_BYTES_PER_S, alternate, summary, wall_window  # noqa: E402

B, C, H, W, N_S, STEPS, DRAWS, SIGMA = 64, 3, 224, 224, 8, 32, 25, 0.15
N = C * H * W
BF = torch.bfloat16
DTYPES = (("fp32", torch.float32, 4), ("bf16", BF, 2))


def _legs(t, nbytes=None, scale=1e6, unit="us"):
    """every leg's median / min / max, each torch leg's median over the kernel's, and the kernel's rate"""
    row = {name: summary(ts, scale, unit, 3) for name, ts in t.items()}
    med = statistics.median(t["kernel"])
    for name, ts in t.items():
        if name != "kernel":
            row[f"{name}_over_kernel_medians"] = round(statistics.median(ts) / med, 2)
            row[f"kernel_range_below_{name}"] = bool(max(t["kernel"]) < min(ts))
    if nbytes is not None:
        row.update(algorithmic_bytes=nbytes, TB_per_s=round(nbytes / med / 1e12, 3),
                   share_of_measured_copy_rate_6_29TBps=round(nbytes / med / MEASURED_COPY_BYTES_PER_S, 3))
    return row


def images(seed=0):
    return torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(seed)).to("cuda:0")


def torch_path32(x, base, a, dtype):
    return (base[:, None] + a.view(1, -1, 1, 1, 1) * (x - base)[:, None]).to(dtype)


def torch_path64(x, base, a, dtype):
    b64 = base.double()
    return (b64[:, None] + a.double().view(1, -1, 1, 1, 1) * (x.double() - b64)[:, None]).float().to(dtype)


def torch_gauss(x, n_d, sigma, dtype):
    return (x[:, None] + sigma * torch.randn((x.shape[0], n_d) + tuple(x.shape[1:]), device=x.device)).to(dtype)


def torch_accumulate(g, w, acc, s0=0, square=False):
    t = g.double()
    if square:
        t = t * t
    acc += (t * w[s0:s0 + g.shape[1]].view(1, -1, 1, 1, 1)).sum(1)
    return acc


def torch_finish(acc, m, reduce="sum"):
    t = acc if m is None else m.double() * acc
    v = t.sum(1) if reduce == "sum" else t.abs().sum(1) if reduce == "abs_sum" else t.abs().amax(1)
    return v.float(), v.flatten(1).sum(1)


def bench_kernels(rounds, window, warmup):
    from transformer_explainability_amd import ops
    x, base = images(0), images(1) * 0.1
    a = torch.linspace(0.05, 0.95, N_S, device="cuda:0")
    w = torch.full((N_S,), 1.0 / N_S, dtype=torch.float64, device="cuda:0")
    res = {}
    for name, dtype, size in DTYPES:
        t = alternate({"kernel": lambda: ops.path_inputs(x, base, a, out_dtype=dtype),
                       "torch_fp32": lambda: torch_path32(x, base, a, dtype),
                       "torch_fp64": lambda: torch_path64(x, base, a, dtype)}, rounds, window, warmup)
        res[f"path_inputs.B{B}.n{N}.{N_S}nodes.{name}"] = _legs(t, B * N_S * N * size + 2 * B * N * 4)
        t = alternate({"kernel": lambda: ops.gauss_inputs(x, N_S, SIGMA, 0, out_dtype=dtype),
                       "torch": lambda: torch_gauss(x, N_S, SIGMA, dtype)}, rounds, window, warmup)
        res[f"gauss_inputs.B{B}.n{N}.{N_S}draws.{name}"] = _legs(t, B * N_S * N * size + B * N * 4)
        g = ops.gauss_inputs(x, N_S, SIGMA, 1, out_dtype=dtype)
        acc_k, acc_t = (torch.zeros((B, C, H, W), dtype=torch.float64, device="cuda:0") for _ in range(2))
        t = alternate({"kernel": lambda: ops.grad_accumulate(g, w, acc_k), "torch": lambda: torch_accumulate(g, w, acc_t)},
                      rounds, window, warmup)
        res[f"grad_accumulate.B{B}.n{N}.{N_S}copies.{name}"] = _legs(t, B * N_S * N * size + 2 * B * N * 8)
        del g
    acc = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(2), dtype=torch.float64).to("cuda:0")
    for reduce in ("sum", "abs_sum", "max_abs"):
        t = alternate({"kernel": lambda: ops.grad_finish(acc, x, reduce), "torch": lambda: torch_finish(acc, x, reduce)},
                      rounds, window, warmup)
        res[f"grad_finish.B{B}.C{C}.HW{H * W}.{reduce}"] = _legs(t, B * N * 12 + B * H * W * 4 + B * 8)
    return res


def torch_integrated_gradients(gb, x, index, steps, chunk):
    """integrated_gradients composed in torch on device tensors: the same passes, torch's broadcasts and sums"""
    from transformer_explainability_amd import gradients
    alphas, weights = gradients.quadrature("midpoint", steps)
    xf, base = x.float(), gb.baseline(x, "black")
    f_x = gb._selected(gb._logits(x), index).double()
    f_b = gb._selected(gb._logits(base.to(x.dtype)), index).double()
    a = torch.from_numpy(alphas.astype(np.float32)).to(x.device)
    w = torch.from_numpy(weights).to(x.device)
    acc = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for s0 in range(0, steps, chunk):
        n_s = min(chunk, steps - s0)
        torch_accumulate(gb._gradients(torch_path32(xf, base, a[s0:s0 + n_s], x.dtype), index), w, acc, s0)
    return torch_finish(acc, xf - base), f_x, f_b


def torch_smoothgrad(gb, x, index, n_draws, sigma, chunk):
    xf = x.float()
    scale = sigma * float(xf.max() - xf.min())
    w = torch.full((n_draws,), 1.0 / n_draws, dtype=torch.float64, device=x.device)
    acc = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    for d0 in range(0, n_draws, chunk):
        n_d = min(chunk, n_draws - d0)
        torch_accumulate(gb._gradients(torch_gauss(xf, n_d, scale, x.dtype), index), w, acc, d0)
    return torch_finish(acc, None, "abs_sum")


def bench_calls(rounds, window, warmup, chunk):
    from transformer_explainability_amd import gradients, ops
    res = {}
    for name, dtype, _ in (DTYPES[1], DTYPES[0]):
        gb = gradients.GradientBaselines(vit_b16(dtype))
        x = images(3).to(dtype)
        index = gb._logits(x).argmax(-1)
        xf, base = x.float(), gb.baseline(x, "black")
        a = torch.linspace(0.05, 0.95, STEPS, device="cuda:0")
        w = torch.full((STEPS,), 1.0 / STEPS, dtype=torch.float64, device="cuda:0")
        g = torch.randn((B, chunk, C, H, W), device="cuda:0").to(dtype)
        one = partial(wall_window, min_s=0.0)

        def launches(steps, path):      # the call's own launches alone, on tensors of the same shapes
            acc = torch.zeros(x.shape, dtype=torch.float64, device=x.device)
            for s0 in range(0, steps, chunk):
                n_s = min(chunk, steps - s0)
                if path:
                    ops.path_inputs(xf, base, a, s0, n_s, out_dtype=dtype)
                else:
                    ops.gauss_inputs(xf, n_s, SIGMA, 0, d0=s0, out_dtype=dtype)
                ops.grad_accumulate(g[:, :n_s], w, acc, s0=s0)
            ops.grad_finish(acc, xf if path else None, "sum" if path else "abs_sum")

        for call, steps, kernel, composed in (
                (f"integrated_gradients.steps{STEPS}", STEPS, lambda: gb.integrated_gradients(x, index=index, steps=STEPS, chunk=chunk),
                 lambda: torch_integrated_gradients(gb, x, index, STEPS, chunk)),
                (f"smoothgrad.draws{DRAWS}", DRAWS, lambda: gb.smoothgrad(x, index=index, n_draws=DRAWS, sigma=SIGMA, chunk=chunk),
                 lambda: torch_smoothgrad(gb, x, index, DRAWS, SIGMA, chunk))):
            t = alternate({"kernel": kernel, "torch": composed}, rounds, one, 1)
            row = _legs(t, None, 1e3, "ms")
            tk = alternate({"kernel": partial(launches, steps, call.startswith("integrated"))}, rounds, window, warmup)["kernel"]
            row["kernels_ms"] = summary(tk, 1e3, "ms", 3)
            row["kernels_share_of_call"] = round(statistics.median(tk) / statistics.median(t["kernel"]), 5)
            row["rows_per_pass"], row["passes"] = B * chunk, -(-steps // chunk)
            res[f"{call}.vit_base_patch16_224.batch{B}.chunk{chunk}.{name}"] = row
        m, comp = gb.integrated_gradients(x, index=index, steps=STEPS, chunk=chunk)
        gap = (comp.sum - (comp.f_x - comp.f_base)).abs()
        res[f"completeness.steps{STEPS}.{name}"] = {"max_gap": float(gap.max()), "max_abs_f_x_minus_f_base": float((comp.f_x - comp.f_base).abs().max())}
        del gb, g
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=200.0, help="least duration of a timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--model-rounds", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=4, help="copies per sample and pass of the whole calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradients_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "gradients", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    window = partial(wall_window, min_s=a.window_ms / 1e3)
    res["kernels"] = bench_kernels(a.rounds, window, a.warmup)
    if not a.skip_model:
        res["calls"] = bench_calls(a.model_rounds, window, a.warmup, a.chunk)
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
