"""generate_attnlrp beside generate_LRP, one process, the same model and inputs, windows alternating.

    python benchmarks/attnlrp_bench.py [--configs vit_b16 bert_base] [--steps 5] [--rounds 5] [--warmup 2]
                                       [--producers fused|stock] [--out profiles/attnlrp_bench.json]

Two configurations: ViT-B/16 (224 x 224) at batch 64 and BERT-base at 512 tokens x 32.  Per configuration both calls are
warmed up together, then timed A B A B ...: one window = ``--steps`` calls between two HIP events, ended by a synchronise;
reported are the median, minimum and maximum ms per call over the ``--rounds`` windows of each method, and the ratio of the
medians.  generate_LRP runs a forward pass, an attention-gradient backward pass and the sign-split relprop chain;
generate_attnlrp a forward pass and one chain.  No speed is claimed anywhere: the file holds what was measured.
The result is printed as one JSON line and written to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks._models import vit_b16  # noqa: E402
from benchmarks._timing import alternate, event_window, summary  # noqa: E402  (the event-window protocol)


def _vit_b16(batch):
    from oracle.ref_harness import seeded_randn
    from transformer_explainability_amd.generators import LRP
    x = seeded_randn((batch, 3, 224, 224), 1).to("cuda:0")
    gen = LRP(vit_b16())
    return gen, {"generate_LRP": lambda: gen.generate_LRP(x, start_layer=0), "generate_attnlrp": lambda: gen.generate_attnlrp(x)}


def _bert_base(batch, tokens=512):
    from transformer_explainability_amd import bert
    from transformer_explainability_amd.generators import Generator
    torch.manual_seed(0)
    model = bert.BertForSequenceClassification(bert.BertConfigLite()).eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(0.02 * torch.randn_like(p))
    model.to("cuda:0")
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30000, (batch, tokens), generator=g).to("cuda:0")
    mask = torch.ones(batch, tokens)
    mask[::2, tokens - tokens // 8:] = 0.0                     # every other sample padded
    mask = mask.to("cuda:0")
    gen = Generator(model)
    return gen, {"generate_LRP": lambda: gen.generate_LRP(ids, mask, start_layer=0),
                 "generate_attnlrp": lambda: gen.generate_attnlrp(ids, mask)}


CONFIGS = {"vit_b16": (_vit_b16, 64), "bert_base": (_bert_base, 32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=sorted(CONFIGS), default=["vit_b16", "bert_base"])
    ap.add_argument("--steps", type=int, default=5, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="windows per method")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="0: the configuration's own (64 / 32)")
    ap.add_argument("--producers", choices=["stock", "fused"], default="fused")
    ap.add_argument("--tuned-gemms", choices=["on", "off"], default="on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attnlrp_bench.json"))
    a = ap.parse_args()

    import transformer_explainability_amd as te
    from transformer_explainability_amd import ops
    te._lib.require_device()
    ops.USE_FUSED_PRODUCERS = a.producers == "fused"
    tuned = te.enable_tuned_gemms() if a.tuned_gemms == "on" else False
    res = {"producers": a.producers, "tuned_gemms": bool(tuned), "steps_per_window": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.configs:
        make, batch = CONFIGS[name]
        batch = a.batch or batch
        gen, modes = make(batch)
        for _ in range(a.warmup):
            for fn in modes.values():
                fn()
        ts = alternate(modes, a.rounds, partial(event_window, n=a.steps), 0)      # (warmed above, the two calls in turn)
        gen.check()                                            # no x6 hand-over was lost in any timed call
        finite = {m: bool(torch.isfinite(fn()).all()) for m, fn in modes.items()}
        entry = {"batch": batch, "finite": finite, **{m: summary(v, 1e3, "ms", 3) for m, v in ts.items()}}
        entry["attnlrp_over_lrp"] = round(entry["generate_attnlrp"]["median_ms"] / entry["generate_LRP"]["median_ms"], 3)
        res["configs"][name] = entry
        del gen, modes
        torch.cuda.empty_cache()
    res["build_id"] = te._lib.build_id()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
