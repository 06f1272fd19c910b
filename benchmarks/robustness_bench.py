"""The robustness / complexity kernels (csrc/te_robust.hip) beside the torch composition of the same protocol, in one process
on the same device tensors.

    python benchmarks/robustness_bench.py [--rounds 5] [--window-ms 200] [--warmup 2] [--skip-model] [--model-rounds 3] [--out F]

Configuration: ViT-B/16, batch 64, 3 x 224 x 224 normalised inputs (n = 150528), 10 draws at radius 0.02, fp32 and bf16
copies; maps of 196 patches and of 224 x 224 pixels.  Prints one JSON line (and writes it to --out, default
profiles/robustness_bench.json):
  * noise: one ops.noise_inputs launch of 64 x 10 copies beside ``x[:, None] + radius * (2 * rand - 1)`` of torch (another
    generator: only the time is comparable); the bytes written (and x read once) over the time, as a share of the 8 TB/s of the
    data sheet and of the measured copy rate of the part, 6.29 TB/s; and the Philox rate that time means (40 32-bit
    multiplies, each hi and lo, per 4 words).
  * distance: ops.map_distance beside robustness.reference_distance on the input pairs (n = 150528, fp32 and bf16 copies) and
    on map pairs (n = 196 and 50176).
  * complexity: ops.map_complexity beside robustness.reference_complexity at n = 196 and 50176.
  * update: one SensitivityEvaluator.update (1 + 10 explanations of 64 images) beside the same protocol composed in torch
    with the same explanations; ``kernels_ms`` times the evaluator's own launches alone (10 noise, 20 distance, 1 complexity),
    the share of an update they are.
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

import torch  # noqa: E402

from benchmarks._models import vit_b16  # noqa: E402
from benchmarks._timing import (HBM_BYTES_PER_S, MEASURED_COPY_BYTES_PER_S, alternate, summary,  # noqa: E402
                                wall_window)                                  # (the wall-window protocol)

B, C, H, W, DRAWS, RADIUS = 64, 3, 224, 224, 10, 0.02
N = C * H * W
BF = torch.bfloat16


def _pair(t, scale=1e6, unit="us"):
    return {"kernel": summary(t["kernel"], scale, unit, 3), "torch": summary(t["torch"], scale, unit, 3),
            "torch_over_kernel_medians": round(statistics.median(t["torch"]) / statistics.median(t["kernel"]), 2),
            "kernel_range_below_torch": bool(max(t["kernel"]) < min(t["torch"]))}


def images():
    return torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(0)).to("cuda:0")


def torch_noise(x, n_d, dtype):
    """captum's default perturbation composed in torch: uniform in the L-infinity ball, torch's own generator"""
    u = torch.rand((x.shape[0], n_d) + tuple(x.shape[1:]), device=x.device)
    return (x[:, None] + RADIUS * (2 * u - 1)).to(dtype)


def bench_noise(rounds, window, warmup):
    from transformer_explainability_amd import ops
    x = images()
    res = {}
    for name, dtype, size in (("fp32", torch.float32, 4), ("bf16", BF, 2)):
        t = alternate({"kernel": lambda: ops.noise_inputs(x, DRAWS, RADIUS, 0, out_dtype=dtype),
                       "torch": lambda: torch_noise(x, DRAWS, dtype)}, rounds, window, warmup)
        row = _pair(t)
        med = statistics.median(t["kernel"])
        nbytes = B * DRAWS * N * size + B * N * 4
        philox_calls = B * DRAWS * N / 4
        row.update(algorithmic_bytes=nbytes, TB_per_s=round(nbytes / med / 1e12, 3),
                   share_of_8TBps=round(nbytes / med / HBM_BYTES_PER_S, 3),
                   share_of_measured_copy_rate_6_29TBps=round(nbytes / med / MEASURED_COPY_BYTES_PER_S, 3),
                   philox_calls=int(philox_calls), T_mul32_hi_lo_per_s=round(philox_calls * 40 / med / 1e12, 3),
                   note="host clock over a window of back-to-back calls: launch and allocation of the output included")
        res[f"noise_inputs.B{B}.n{N}.{DRAWS}draws.{name}"] = row
    return res


def bench_distance(rounds, window, warmup):
    from transformer_explainability_amd import ops, robustness
    g = torch.Generator().manual_seed(1)
    res = {}
    for n, dtypes in ((N, (torch.float32, BF)), (196, (torch.float32,)), (H * W, (torch.float32,))):
        a = torch.randn((B, n), generator=g).to("cuda:0")
        for dtype in dtypes:
            b = (a[:, None] + 0.02 * torch.randn((B, DRAWS, n), generator=g).to("cuda:0")).to(dtype)
            t = alternate({"kernel": lambda: ops.map_distance(a, b), "torch": lambda: robustness.reference_distance(a, b)},
                          rounds, window, warmup)
            row = _pair(t)
            nbytes = b.numel() * b.element_size() + a.numel() * 4
            row.update(algorithmic_bytes=nbytes, TB_per_s=round(nbytes / statistics.median(t["kernel"]) / 1e12, 3))
            res[f"map_distance.B{B}.D{DRAWS}.n{n}.{'bf16' if dtype == BF else 'fp32'}"] = row
    return res


def bench_complexity(rounds, window, warmup):
    from transformer_explainability_amd import ops, robustness
    g = torch.Generator().manual_seed(2)
    res = {}
    for n in (196, H * W):
        m = torch.randn((B, n), generator=g).to("cuda:0")
        t = alternate({"kernel": lambda: ops.map_complexity(m), "torch": lambda: robustness.reference_complexity(m)},
                      rounds, window, warmup)
        res[f"map_complexity.B{B}.n{n}"] = _pair(t)
    return res


def torch_update(lrp, x, dtype):
    """SensitivityEvaluator.update composed in torch on device tensors: the same explanations, torch's noise and sums"""
    from transformer_explainability_amd import robustness
    seen = x.to(dtype)
    clean = seen.float()
    got = lrp.generate_classes(seen, topk=1)
    classes, map0 = got.classes, got.maps["transformer_attribution"][:, 0].reshape(B, -1).float().clone()
    map_sums, input_sums = [], []
    for _ in range(DRAWS):
        copies = torch_noise(clean, 1, dtype)
        maps = lrp.generate_classes(copies.reshape(B, C, H, W), classes=classes).maps["transformer_attribution"][:, 0]
        map_sums.append(robustness.reference_distance(map0, maps.reshape(B, 1, -1).float()))
        input_sums.append(robustness.reference_distance(clean.reshape(B, -1), copies.reshape(B, 1, -1)))
    scores = robustness.scores_from_sums(torch.cat(map_sums, 1), torch.cat(input_sums, 1))
    return scores, robustness.reference_complexity(map0)


def bench_update(rounds, window, warmup):
    from transformer_explainability_amd import ops, robustness
    from transformer_explainability_amd.generators import LRP
    x = images()
    res = {}
    for name, dtype in (("bf16", BF), ("fp32", torch.float32)):
        lrp = LRP(vit_b16(dtype))

        def kernel():
            ev = robustness.SensitivityEvaluator(lrp, n_draws=DRAWS, radius=RADIUS, seed=0, draws_per_pass=1)
            ev.update(x)
            return ev
        t = alternate({"kernel": kernel, "torch": lambda: torch_update(lrp, x, dtype)}, rounds,
                      partial(wall_window, min_s=0.0), 1)
        row = _pair(t, 1e3, "ms")
        # the evaluator's own launches of one update, alone, on tensors of the same shapes
        clean = x.to(dtype).float()
        maps0 = torch.randn((B, 196), device="cuda:0")
        maps1 = torch.randn((B, 1, 196), device="cuda:0")

        def launches():
            for d in range(DRAWS):
                copies = ops.noise_inputs(clean, 1, RADIUS, 0, d0=d, out_dtype=dtype)
                ops.map_distance(maps0, maps1)
                ops.map_distance(clean.reshape(B, -1), copies.reshape(B, 1, -1))
            ops.map_complexity(maps0)
        tk = alternate({"kernel": launches}, rounds, window, warmup)["kernel"]
        row["kernels_ms"] = summary(tk, 1e3, "ms", 3)
        row["kernels_share_of_update"] = round(statistics.median(tk) / statistics.median(t["kernel"]), 5)
        row["explanations_per_update"] = (1 + DRAWS) * B
        row["summary"] = kernel().summary()
        res[f"update.vit_base_patch16_224.batch{B}.{DRAWS}draws.{name}"] = row
        del lrp
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=200.0, help="least duration of a timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--model-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robustness_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "robustness", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    window = partial(wall_window, min_s=a.window_ms / 1e3)
    res["noise"] = bench_noise(a.rounds, window, a.warmup)
    res["distance"] = bench_distance(a.rounds, window, a.warmup)
    res["complexity"] = bench_complexity(a.rounds, window, a.warmup)
    if not a.skip_model:
        res["update"] = bench_update(a.model_rounds, window, a.warmup)
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
