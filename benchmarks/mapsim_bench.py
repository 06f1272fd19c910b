"""The map-similarity kernels (te_map_similarity_f32) beside the torch composition of the same definitions, in one process on the
same CUDA tensors.

    python benchmarks/mapsim_bench.py [--rounds 9] [--window-ms 50] [--warmup 3] [--skip-model] [--model-batch 64] [--model-rounds 3] [--out F]

Prints one JSON line (and writes it to --out, default profiles/mapsim_bench.json):
  * metrics: one similarity call per shape -- [64,196], [64,50176] with SSIM at 224 x 224, [1,50176] (no SSIM).  ``kernel`` is
    ops.map_similarity (two launches, nothing read back), ``torch`` is sanity.map_similarity on the same device tensors (batched
    sort / cummax / cummin / scatter for the ranks, fp64 reductions, avg_pool2d for the SSIM windows).  The versions alternate,
    --rounds timed windows each of at least --window-ms (host clock between two device synchronisations) after warming every
    shape; reported: median, min and max seconds per call, the ratio of the medians, and whether the two agree (integers
    equal, the fp64 columns within the bounds of the tests).
  * evaluator: one SanityCheckEvaluator.update of a ViT-B/16 batch (cascading, 14 stages, transformer_attribution and
    attn_rollout) with and without the similarity calls, alternating: the share of the protocol that the metrics are.
The yardstick is the torch composition on the device; no speed-up is promised, the result is written down whichever way it falls.
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
from benchmarks._timing import alternate, summary, wall_window  # noqa: E402  (the wall-window protocol)

SHAPES = ((64, 196, None), (64, 50176, (224, 224)), (1, 50176, None))


def inputs(B, n, seed=0):
    """Two batches of maps in [0, 1] that are correlated and have ties (values on a grid of 1/1024), as min-max normalised
    relevance maps do."""
    g = torch.Generator().manual_seed(seed + 7 * B + n)
    a = torch.rand((B, n), generator=g)
    b = 0.6 * a + 0.4 * torch.rand((B, n), generator=g)
    return ((a * 1024).round() / 1024).to("cuda:0"), ((b * 1024).round() / 1024).to("cuda:0")


def bench_metrics(rounds, min_s, warmup):
    from transformer_explainability_amd import ops, sanity
    res = {}
    for B, n, shape in SHAPES:
        a, b = inputs(B, n)
        got, ref = ops.map_similarity(a, b, shape), sanity.map_similarity(a, b, shape)
        t = alternate({"kernel": lambda: ops.map_similarity(a, b, shape),
                       "torch": lambda: sanity.map_similarity(a, b, shape)}, rounds, partial(wall_window, min_s=min_s), warmup)
        d = (torch.nan_to_num(got[1]) - torch.nan_to_num(ref[1])).abs().max(0).values
        res[f"B{B}.n{n}" + (".ssim" if shape else "")] = {
            "kernel": summary(t["kernel"]), "torch": summary(t["torch"]),
            "torch_over_kernel_medians": round(statistics.median(t["torch"]) / statistics.median(t["kernel"]), 2),
            "kernel_range_below_torch": bool(max(t["kernel"]) < min(t["torch"])),
            "rank_sums_equal": bool(torch.equal(got[0], ref[0])),
            "max_abs_difference_per_column": [float(v) for v in d],
            "workspace_bytes": int(ops._lib.load().te_map_similarity_workspace_bytes(B, n))}
    return res


def bench_evaluator(rounds, B):
    from transformer_explainability_amd import sanity
    from transformer_explainability_amd.generators import LRP
    from transformer_explainability_amd.sweep import normalize
    m = vit_b16()
    lrp = LRP(m)
    g = torch.Generator().manual_seed(B)
    x = normalize(torch.rand((B, 3, 224, 224), generator=g).to("cuda:0"))
    methods = ("transformer_attribution", "attn_rollout")

    real = sanity.compare_maps
    blank = (torch.zeros((B, 2, 3), dtype=torch.int64, device="cuda:0"), torch.zeros((B, 4), dtype=torch.float64, device="cuda:0"))

    def update(similarity):
        # without: the same protocol with the comparison replaced by a constant (and no image of the original map)
        ev = sanity.SanityCheckEvaluator(lrp, methods, ssim=similarity, upsample=True, start_layer=1)
        sanity.compare_maps = real if similarity else (lambda *a, **k: blank)
        try:
            ev.update(x)
        finally:
            sanity.compare_maps = real
        return ev
    t = alternate({"with_metrics": lambda: update(True), "without_metrics": lambda: update(False)}, rounds,
                  partial(wall_window, min_s=0.0), 1)
    lrp.check()
    with_m, without = statistics.median(t["with_metrics"]), statistics.median(t["without_metrics"])
    row = {k: summary(v, 1e3, "ms") for k, v in t.items()}
    row["metrics_share_of_update"] = round((with_m - without) / with_m, 4)
    row["stages"], row["methods"], row["upsample"] = len(sanity.randomization_stages(m)), methods, True
    s = update(True).summary()
    row["spearman_mean_per_stage"] = {k: [round(float(v), 4) for v in s[k]["mean"][:, 1]] for k in s}
    return {f"update.vit_base_patch16_224.batch{B}": row}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9, help="timed windows per version (the versions alternate)")
    ap.add_argument("--window-ms", type=float, default=50.0, help="least duration of a timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--model-batch", type=int, default=64)
    ap.add_argument("--model-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapsim_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    te._lib.require_device()
    res = {"bench": "mapsim", "rounds": a.rounds, "window_ms": a.window_ms, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    res["metrics"] = bench_metrics(a.rounds, a.window_ms / 1e3, a.warmup)
    if not a.skip_model:
        res["evaluator"] = bench_evaluator(a.model_rounds, a.model_batch)
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
