"""AttnLRP at pixel level: what generate_attnlrp(method="full") costs, and where the time of its last rule goes.

    python benchmarks/attnlrp_full_bench.py [--dtypes fp32 bf16] [--batch 64] [--steps 5] [--rounds 5] [--warmup 2]
                                            [--out profiles/attnlrp_full_bench.json]

ViT-B/16 (224 x 224) at batch 64, an fp32 and a bf16 model; one process, windows alternating (benchmarks/_timing.py), medians
reported.  Three measurements per dtype:

  kernel       ops.alrp_patch_relevance against its composition on the SAME device tensors: ops.alrp_damp, ops.alrp_linear on
               W.view(E, -1) (bf16: the one call that damps and multiplies), then the torch expression that reads the image
               through the patch geometry, multiplies and sums the channels -- which materialises the [B P, C p p] product.
               With the kernel's distance from the nominal fp32-MFMA peak (256 CUs x 4 SIMDs x 64 FLOP per clock at 2.4 GHz:
               not measured on the part) and from the measured copy rate (the bytes of G, y, X, W and the map).
  full/tokens  generate_attnlrp(method="full") against method="tokens" on the same model, and the kernel's share of the
               call (HIP events around the binding: ops.KERNEL_TIMER).
  full/LRP     generate_attnlrp(method="full") against generate_LRP(method="full") on the same model.

No speed is claimed and there is no threshold: the change buys a capability, and the file holds what was measured.  The
result is printed as one JSON line and written to ``--out``."""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks._models import vit_b16  # noqa: E402
from benchmarks._timing import MEASURED_COPY_BYTES_PER_S, alternate, event_window, summary  # noqa: E402

FP32_MFMA_NOMINAL_FLOPS = 256 * 4 * 64 * 2.4e9      # CUs x SIMDs x FLOP per clock per SIMD x clock: nominal, not measured
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


class _OneRule:
    """ops.KERNEL_TIMER: HIP events around the calls of one binding"""

    def __init__(self, name):
        self.name, self.pending = name, []

    @contextlib.contextmanager
    def __call__(self, name, flops, nbytes):
        if name != self.name:
            yield
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        yield
        b.record()
        self.pending.append((a, b))

    def ms(self):
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in self.pending]


def _kernel_leg(dtype, batch, a):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import ops
    B, C, H, Wd, E, p = batch, 3, 224, 224, 768, 16
    P, K = (H // p) * (Wd // p), C * p * p
    dev = "cuda:0"
    G = seeded_randn((B, P + 1, E), 2).to(dev)
    x0 = seeded_randn((B, P + 1, E), 3).to(dev).to(dtype)
    X = seeded_randn((B, C, H, Wd), 4).to(dev).to(dtype)
    W = (seeded_randn((E, C, p, p), 5) * 0.05).to(dev).to(dtype)
    Gp, yp = G[:, 1:].reshape(B * P, E).contiguous(), x0[:, 1:].reshape(B * P, E).contiguous()
    W2, Xf, cache = W.view(E, K), X.float(), {}

    def composition():
        if dtype == torch.bfloat16:
            Z = ops.alrp_linear(Gp, W2, cache, Y=yp, eps=1e-6)
        else:
            Z = ops.alrp_linear(ops.alrp_damp(Gp, yp, 1e-6), W2, cache)
        Z = Z.view(B, H // p, Wd // p, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, Wd)
        return (Xf * Z).sum(1)

    modes = {"kernel": lambda: ops.alrp_patch_relevance(G, x0, X, W, 1e-6), "composition": composition}
    got, want = modes["kernel"](), modes["composition"]()
    rel = float((got - want).norm() / want.norm())
    ts = alternate(modes, a.rounds, partial(event_window, n=a.steps), a.warmup)
    out = {m: summary(v, 1e3, "ms", 3) for m, v in ts.items()}
    med = out["kernel"]["median_ms"] / 1e3
    es = X.element_size()
    flops = 2.0 * B * P * E * K + 2.0 * B * P * K
    nbytes = (4.0 + es) * B * P * E + es * (E * K + B * P * K) + 4.0 * B * H * Wd
    out.update(route=ops.alrp_patch_route(C, E, p), kernel_over_composition=round(med / (out["composition"]["median_ms"] / 1e3), 3),
               rel_l2_kernel_vs_composition=rel, algorithmic_GFLOP=round(flops / 1e9, 2), algorithmic_MB=round(nbytes / 1e6, 1),
               intermediate_MB_not_written=round(4.0 * B * P * K / 1e6, 1), kernel_TFLOP_per_s=round(flops / med / 1e12, 2),
               kernel_share_of_nominal_fp32_mfma_peak=round(flops / med / FP32_MFMA_NOMINAL_FLOPS, 4),
               kernel_GB_per_s=round(nbytes / med / 1e9, 1),
               kernel_share_of_measured_copy_rate=round(nbytes / med / MEASURED_COPY_BYTES_PER_S, 4))
    return out


def _model_leg(dtype, batch, a):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd import ops
    from transformer_explainability_amd.generators import LRP
    x = seeded_randn((batch, 3, 224, 224), 1).to("cuda:0").to(dtype)
    gen = LRP(vit_b16(dtype))
    modes = {"attnlrp_full": lambda: gen.generate_attnlrp(x, method="full"),
             "attnlrp_tokens": lambda: gen.generate_attnlrp(x, method="tokens"),
             "LRP_full": lambda: gen.generate_LRP(x, method="full", start_layer=0)}
    ts = alternate(modes, a.rounds, partial(event_window, n=a.steps), a.warmup)
    gen.check()
    out = {m: summary(v, 1e3, "ms", 3) for m, v in ts.items()}
    med = lambda m: out[m]["median_ms"]      # noqa: E731
    shapes = {m: list(fn().shape) for m, fn in modes.items()}
    timer = _OneRule("alrp_patch_relevance")
    ops.KERNEL_TIMER = timer
    try:
        for _ in range(3):
            finite = bool(torch.isfinite(modes["attnlrp_full"]()).all())
        rule_ms = sorted(timer.ms())[1]
    finally:
        ops.KERNEL_TIMER = None
    out.update(shapes=shapes, finite=finite, full_over_tokens=round(med("attnlrp_full") / med("attnlrp_tokens"), 3),
               full_minus_tokens_ms=round(med("attnlrp_full") - med("attnlrp_tokens"), 3),
               attnlrp_full_over_LRP_full=round(med("attnlrp_full") / med("LRP_full"), 3),
               patch_rule_ms=round(rule_ms, 3), patch_rule_share_of_the_call=round(rule_ms / med("attnlrp_full"), 4))
    del gen
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", nargs="+", choices=sorted(DTYPES), default=["fp32", "bf16"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per call")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attnlrp_full_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    from transformer_explainability_amd import ops
    te._lib.require_device()
    ops.USE_FUSED_PRODUCERS = True
    tuned = te.enable_tuned_gemms()
    res = {"model": "vit_base_patch16_224", "batch": a.batch, "producers": "fused", "tuned_gemms": bool(tuned),
           "steps_per_window": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "fp32_mfma_nominal_TFLOP_per_s": round(FP32_MFMA_NOMINAL_FLOPS / 1e12, 1),
           "measured_copy_GB_per_s": MEASURED_COPY_BYTES_PER_S / 1e9, "dtypes": {}}
    for name in a.dtypes:
        res["dtypes"][name] = {"kernel": _kernel_leg(DTYPES[name], a.batch, a), "model": _model_leg(DTYPES[name], a.batch, a)}
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
