#!/usr/bin/env python
"""Measurement infrastructure (not product code): the head-mask rule kernel (csrc/te_headmask.hip) on one MI355X.

  1. te_mul_head_relprop_f32 / _bf16 at (B,H,N,N) = (64,12,197,197) and (32,12,512,512) against the torch composition of the
     same rule (Z = P m ; S = safe_divide(R, Z) ; P (S m)) in the same process: device events, medians of alternating windows.
     Reported with the achieved fraction of 8 TB/s on the ALGORITHMIC bytes (R in, P in, out written); Clone.relprop on the same
     element count runs beside it as the project's own streaming yardstick.
  2. The price of a mask at model level: a ViT-B/16 batch-64 explanation step with a mask on every head of every block (m = 1:
     the forward pass computes the unmasked values, the Mul rule runs in full on all 12 x 12 heads) against the unmasked
     stock-forward step, same process, alternating.  A masked pass is a stock-forward pass whatever ops.USE_FUSED_PRODUCERS
     says; the unmasked step on the producer kernels is timed as well, for the user who gives those up.

    python benchmarks/head_mask_bench.py [--windows 7] [--reps 20] [--skip-model] [--out profiles/head_mask_bench.json]   (GPU box)
"""
import argparse
import json
import os
import statistics
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmarks._models import vit_b16  # noqa: E402
from benchmarks._timing import HBM_BYTES_PER_S as PEAK_BYTES_PER_S  # noqa: E402
from benchmarks._timing import alternate, event_window  # noqa: E402  (the event-window protocol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model-windows", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from transformer_explainability_amd import _lib, ops, rules
    _lib.load()
    _lib.require_device()
    d = torch.device("cuda:0")
    res = {"build_id": _lib.build_id(), "peak_bytes_per_s": PEAK_BYTES_PER_S, "windows": args.windows, "reps": args.reps}

    def alternate_us(legs, windows, reps):
        """legs: {name: fn}; every window times each leg once, in turn -> {name: median us}"""
        times = alternate(legs, windows, partial(event_window, n=reps), 3)
        return {n: {"us": statistics.median(t) * 1e6, "us_min": min(t) * 1e6, "us_max": max(t) * 1e6} for n, t in times.items()}

    for B, H, N in ((64, 12, 197), (32, 12, 512)):
        g = torch.Generator().manual_seed(N)
        P32 = torch.softmax(torch.randn(B, H, N, N, generator=g), -1).to(d)
        R = (1e-3 * torch.randn(B, H, N, N, generator=g)).to(d)
        m32 = torch.tensor([1.0, 0.5, -2.0, 0.75] * (H // 4), device=d).view(1, H, 1, 1)      # (no head masked out: full work)
        out = torch.empty_like(R)
        n = R.numel()
        for sfx, P, m in (("f32", P32, m32), ("bf16", P32.to(torch.bfloat16), m32.to(torch.bfloat16))):
            def torch_rule(P=P, m=m):
                Pf, mf = P.float(), m.float()
                return Pf * (rules.safe_divide(R, Pf * mf) * mf)
            legs = {"kernel": lambda P=P, m=m: ops.mul_head_relprop(R, P, m, out=out), "torch": torch_rule}
            if sfx == "f32":
                legs["clone_rule"] = lambda: ops.clone_relprop([R, out], P32)
            t = alternate_us(legs, args.windows, args.reps)
            nbytes = n * (4 + P.element_size() + 4)
            t["kernel"].update(algorithmic_bytes=nbytes, fraction_of_peak=nbytes / (t["kernel"]["us"] * 1e-6) / PEAK_BYTES_PER_S)
            t["torch"]["kernel_speedup"] = t["torch"]["us"] / t["kernel"]["us"]
            if "clone_rule" in t:
                cb = 4 * n * 4
                t["clone_rule"].update(algorithmic_bytes=cb, fraction_of_peak=cb / (t["clone_rule"]["us"] * 1e-6) / PEAK_BYTES_PER_S)
            diff = (ops.mul_head_relprop(R, P, m) - torch_rule()).abs().max() / R.abs().max()      # (torch's division may round otherwise)
            t["legs_max_abs_diff_over_max_R"] = float(diff)
            assert float(diff) < 1e-5, "the two legs must compute the same rule"
            res[f"rule.{sfx}.B{B}.H{H}.N{N}"] = t
            print(f"rule {sfx} ({B},{H},{N},{N}): kernel {t['kernel']['us']:8.1f} us = {t['kernel']['fraction_of_peak']:.2f} of "
                  f"8 TB/s on {nbytes / 1e6:.0f} MB; torch {t['torch']['us']:8.1f} us ({t['torch']['kernel_speedup']:.1f}x)", flush=True)
        del P32, R, out

    if not args.skip_model:
        from oracle.ref_harness import seeded_randn
        from transformer_explainability_amd.generators import LRP
        model = vit_b16()
        x = seeded_randn((64, 3, 224, 224), 1).to(d)
        ones = torch.ones(12, 12, device=d)
        lrp = LRP(model)

        def step(mask, fused):
            def run():
                ops.USE_FUSED_PRODUCERS = fused
                try:
                    return lrp.generate_LRP(x, start_layer=1, head_mask=mask)
                finally:
                    ops.USE_FUSED_PRODUCERS = False
            return run
        legs = {"unmasked_stock_forward": step(None, False), "masked_every_head": step(ones, False),
                "masked_every_head_flag_on": step(ones, True), "unmasked_fused_producers": step(None, True)}
        t = alternate_us(legs, args.model_windows, 2)
        lrp.check()
        base = t["unmasked_stock_forward"]["us"]
        for v in t.values():
            v["ms"] = v.pop("us") / 1e3
            v["vs_unmasked_stock_forward"] = v["ms"] * 1e3 / base
        res["vit_b16_batch64_step"] = t
        for n_, v in t.items():
            print(f"ViT-B/16 batch-64 step, {n_}: {v['ms']:.1f} ms ({v['vs_unmasked_stock_forward']:.3f} x the unmasked stock step)",
                  flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
