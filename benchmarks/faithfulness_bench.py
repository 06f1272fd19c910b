"""The faithfulness kernels (csrc/te_faithful.hip) beside the torch composition of the same protocol, in one process on the
same device tensors.

    python benchmarks/faithfulness_bench.py [--rounds 5] [--window-ms 200] [--warmup 2] [--skip-model] [--model-rounds 3] [--out F]

Configuration: ViT-B/16, batch 64, 3 x 224 x 224 normalised inputs (n = 150528), a 14 x 14 grid of 16 x 16 patches, 49 patches
per subset, 50 draws in passes of 10, fp32 and bf16 copies.  Prints one JSON line (and writes it to --out, default
profiles/faithfulness_bench.json):
  * subset: one ops.subset_inputs call (two launches) of 64 x 10 copies with the constants of the "black" baseline and the
    attribution sums, beside the same definition composed in torch (``torch.rand(...).argsort`` ranks instead of Philox keys:
    another generator, only the time is comparable); the bytes written (x and the membership read) over the time, as a share
    of the 8 TB/s of the data sheet and of the measured copy rate of the part, 6.29 TB/s.  ops.noise_inputs runs in the same
    process at the same shape, for the same two shares.
  * dot: ops.perturbation_dot beside faithfulness.reference_dot on 64 x 10 pairs, fp32 and bf16 copies, a 224 x 224 weight.
  * update: one FaithfulnessEvaluator.update (1 explanation of 64 images, 6 forward passes of 640) beside the same protocol
    composed in torch with the same explanation and forward passes; ``kernels_ms`` times the evaluator's own launches alone.
The versions alternate, --rounds timed windows each (host clock between two device synchronisations) after a warm-up of every
shape; reported: median, min and max.  The yardstick of every time is the torch composition on the device; no ratio is
promised, the result is written down whichever way it falls.
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

B, C, H, W, GRID, P, K = 64, 3, 224, 224, 14, 16, 49
DRAWS, PASS, RADIUS = 50, 10, 0.02
N, G = C * H * W, GRID * GRID
FILL = [-1.0, -1.0, -1.0]                            # "black" under mean = std = 0.5
BF = torch.bfloat16


def _pair(t, scale=1e6, unit="us"):
    return {"kernel": summary(t["kernel"], scale, unit, 3), "torch": summary(t["torch"], scale, unit, 3),
            "torch_over_kernel_medians": round(statistics.median(t["torch"]) / statistics.median(t["kernel"]), 2),
            "kernel_range_below_torch": bool(max(t["kernel"]) < min(t["torch"]))}


def images():
    return torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(0)).to("cuda:0")


def torch_subsets(x, attr, n_d, dtype):
    """ops.subset_inputs composed in torch on the device: the k cells of the smallest random keys per (sample, draw)"""
    ranks = torch.rand((B, n_d, G), device=x.device).argsort(2).argsort(2)
    member = ranks < K
    pixels = member.reshape(B, n_d, 1, GRID, GRID).repeat_interleave(P, 3).repeat_interleave(P, 4)
    fill = torch.tensor(FILL, device=x.device).reshape(1, 1, C, 1, 1)
    out = torch.where(pixels, fill, x[:, None]).to(dtype)
    a = attr.reshape(B, 1, G).double()
    return out, member.to(torch.uint8), torch.where(member, a, torch.zeros_like(a)).sum(2)


def _shares(row, nbytes, med):
    row.update(algorithmic_bytes=nbytes, TB_per_s=round(nbytes / med / 1e12, 3),
               share_of_8TBps=round(nbytes / med / HBM_BYTES_PER_S, 3),
               share_of_measured_copy_rate_6_29TBps=round(nbytes / med / MEASURED_COPY_BYTES_PER_S, 3),
               note="host clock over a window of back-to-back calls: launches and allocation of the outputs included")
    return row


def bench_copies(rounds, window, warmup):
    from transformer_explainability_amd import ops
    x = images()
    attr = torch.randn((B, G), generator=torch.Generator().manual_seed(3)).to("cuda:0")
    res = {}
    for name, dtype, size in (("fp32", torch.float32, 4), ("bf16", BF, 2)):
        t = alternate({"kernel": lambda: ops.subset_inputs(x, K, GRID, 0, n_draws=PASS, fill=FILL, attr=attr, out_dtype=dtype),
                       "torch": lambda: torch_subsets(x, attr, PASS, dtype)}, rounds, window, warmup)
        nbytes = B * PASS * N * size + B * N * 4 + 2 * B * PASS * G
        res[f"subset_inputs.B{B}.n{N}.{PASS}draws.{name}"] = _shares(_pair(t), nbytes, statistics.median(t["kernel"]))
        t = alternate({"kernel": lambda: ops.noise_inputs(x, PASS, RADIUS, 0, out_dtype=dtype)}, rounds, window, warmup)
        row = {"kernel": summary(t["kernel"], digits=3)}
        res[f"noise_inputs.B{B}.n{N}.{PASS}draws.{name}"] = _shares(row, B * PASS * N * size + B * N * 4, statistics.median(t["kernel"]))
    return res


def bench_dot(rounds, window, warmup):
    from transformer_explainability_amd import faithfulness, ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn((B, N), generator=g).to("cuda:0")
    w = torch.randn((B, H * W), generator=g).to("cuda:0")
    res = {}
    for dtype in (torch.float32, BF):
        y = (x[:, None] + 0.02 * torch.randn((B, PASS, N), generator=g).to("cuda:0")).to(dtype)
        t = alternate({"kernel": lambda: ops.perturbation_dot(x, y, w), "torch": lambda: faithfulness.reference_dot(x, y, w)},
                      rounds, window, warmup)
        row = _pair(t)
        nbytes = y.numel() * y.element_size() + x.numel() * 4 + w.numel() * 4
        row.update(algorithmic_bytes=nbytes, TB_per_s=round(nbytes / statistics.median(t["kernel"]) / 1e12, 3))
        res[f"perturbation_dot.B{B}.D{PASS}.n{N}.m{H * W}.{'bf16' if dtype == BF else 'fp32'}"] = row
    return res


def torch_update(lrp, x, dtype):
    """FaithfulnessEvaluator.update (subset mode, "black", "prob") composed in torch on device tensors: the same explanation
    and forward passes, torch's subsets, up-sampling, softmax and sums"""
    from transformer_explainability_amd import curves, faithfulness
    seen = x.to(dtype)
    clean = seen.float()
    got = lrp.generate_classes(seen, topk=1)
    classes, map0 = got.classes, got.maps["transformer_attribution"][:, 0].reshape(B, -1).float().clone()
    weight = faithfulness.reference_heat(map0, P).reshape(B, H * W)
    target = classes.reshape(B).repeat_interleave(PASS, 0)
    ips, deltas, sums = [], [], []
    with torch.no_grad():
        f0 = curves.reference_scores(lrp.model(seen.repeat_interleave(PASS, 0)), target).reshape(B, PASS)
        for _ in range(0, DRAWS, PASS):
            copies, _, attr_sum = torch_subsets(clean, map0, PASS, dtype)
            f = curves.reference_scores(lrp.model(copies.reshape(B * PASS, C, H, W)), target).reshape(B, PASS)
            deltas.append(f0 - f)
            ips.append(faithfulness.reference_dot(clean.reshape(B, -1), copies.reshape(B, PASS, -1), weight)[..., 0])
            sums.append(attr_sum)
    return faithfulness.scores_from_sums(torch.cat(ips, 1), torch.cat(deltas, 1), torch.cat(sums, 1))


def bench_update(rounds, window, warmup):
    from transformer_explainability_amd import faithfulness, ops
    from transformer_explainability_amd.generators import LRP
    x = images()
    res = {}
    for name, dtype in (("bf16", BF), ("fp32", torch.float32)):
        lrp = LRP(vit_b16(dtype))

        def kernel():
            ev = faithfulness.FaithfulnessEvaluator(lrp, n_draws=DRAWS, subset_size=K, seed=0, draws_per_pass=PASS)
            ev.update(x)
            return ev
        t = alternate({"kernel": kernel, "torch": lambda: torch_update(lrp, x, dtype)}, rounds,
                      partial(wall_window, min_s=0.0), 1)
        row = _pair(t, 1e3, "ms")
        # the evaluator's own launches of one update, alone, on tensors of the same shapes
        clean = x.to(dtype).float()
        map0 = torch.randn((B, G), device="cuda:0")
        logits = torch.randn((B * PASS, 1000), device="cuda:0").to(dtype)
        target = torch.zeros((B * PASS,), dtype=torch.int64, device="cuda:0")
        prob = torch.empty((1, B * PASS), dtype=torch.float64, device="cuda:0")

        def launches():
            weight = ops.heatmap(map0, scale=P, normalise=False).reshape(B, H * W)
            ops.curve_scores(logits, target, prob, 0)
            for d0 in range(0, DRAWS, PASS):
                copies, _, _ = ops.subset_inputs(clean, K, GRID, 0, d0=d0, n_draws=PASS, fill=FILL, attr=map0, out_dtype=dtype)
                ops.curve_scores(logits, target, prob, 0)
                ops.perturbation_dot(clean.reshape(B, -1), copies.reshape(B, PASS, -1), weight)
        tk = alternate({"kernel": launches}, rounds, window, warmup)["kernel"]
        row["kernels_ms"] = summary(tk, 1e3, "ms", 3)
        row["kernels_share_of_update"] = round(statistics.median(tk) / statistics.median(t["kernel"]), 5)
        row["forward_rows_per_update"] = (1 + DRAWS // PASS) * B * PASS
        row["summary"] = kernel().summary()
        res[f"update.vit_base_patch16_224.batch{B}.{DRAWS}draws.passes_of_{PASS}.{name}"] = row
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faithfulness_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "faithfulness", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    window = partial(wall_window, min_s=a.window_ms / 1e3)
    res["copies"] = bench_copies(a.rounds, window, a.warmup)
    res["dot"] = bench_dot(a.rounds, window, a.warmup)
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
