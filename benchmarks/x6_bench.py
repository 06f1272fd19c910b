#!/usr/bin/env python
"""Microbenchmark + on-device checks of the split-operand bf16 Linear.relprop (csrc/te_linear_x6.hip) on the Linear
shapes of the three single-GPU configurations.  Per shape and tile geometry: HIP-event time of the three phases
(|X| split, Z-pass, C-pass), executed bf16 TF, fp32-equivalent TF, against the fp32-MFMA kernels of te_linear.hip on the
same operands; checks: x6 vs fp64 (error no larger than the fp32-MFMA path's), the two tile geometries bit for bit,
a half batch bit for bit (rows independent of the stream-K cut), no expired hand-over wait.

    python benchmarks/x6_bench.py [--config vit_b16|vit_l16|bert_base|all] [--iters 20] [--check-rows 1024]
    python benchmarks/x6_bench.py --zpass-ab [--config vit_b16] [--iters 40]
    python benchmarks/x6_bench.py --schedule-ab [--config vit_b16] [--iters 30] [--pin 2]
    python benchmarks/x6_bench.py --ragged-ab [--iters 30] [--pin 2]

--zpass-ab: the Z-pass alone on the planes of |X| (MODE_Z) against the Z-pass on the signed planes of X
(TE_X6_X_PLANES_SIGNED: the sign is applied while the activation blocks are staged), per shape and tile geometry, the two
variants alternating launch by launch in one process; `out` of the whole rule compared bit for bit.
--schedule-ab: every x6 launch of a layer (Z-pass, C-pass, forward and input-gradient product) under the schedule the cost rule
picks, the slack rule before it (TE_X6_SLACK_RULE), whole tiles claimed (TE_X6_WHOLE_TILES) and in static ranges
(+ TE_X6_STATIC_TILES): what te_linear_x6_schedule says each would do, us per launch, us per K16 step, CU-time.
--ragged-ab: the same four launches of every ViT-B layer at T = 12 544 (49 full tile columns of 256 rows), 12 608 (ViT-B batch 64:
the last column holds 64 live rows) and 12 800 (50 full columns), alternating launch by launch: what a ragged column costs.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import transformer_explainability_amd as te  # noqa: E402
from transformer_explainability_amd import _lib, ops  # noqa: E402

CONFIGS = {
    # (T, [(name, in_f, out_f)])
    "vit_b16": (64 * 197, [("qkv", 768, 2304), ("proj", 768, 768), ("fc1", 768, 3072), ("fc2", 3072, 768)]),
    "vit_l16": (32 * 577, [("qkv", 1024, 3072), ("proj", 1024, 1024), ("fc1", 1024, 4096), ("fc2", 4096, 1024)]),
    "bert_base": (32 * 512, [("qkv1", 768, 768), ("inter", 768, 3072), ("out", 3072, 768)]),
}


def operands(T, in_f, out_f, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn(T, in_f, generator=g)
    W = 0.03 * torch.randn(out_f, in_f, generator=g)
    b = 0.1 * torch.randn(out_f, generator=g)
    R = 1e-3 * torch.randn(T, out_f, generator=g)
    X, W, b, R = (t.to(dev) for t in (X, W, b, R))
    Y = torch.nn.functional.linear(X, W, b)
    return X, W, b, R, Y


class Timer:
    def __init__(self):
        self.rows = {}

    def __call__(self, name, flops, nbytes):
        import contextlib

        @contextlib.contextmanager
        def cm():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            yield
            b.record()
            self.rows.setdefault(name, []).append((a, b, flops, nbytes))
        return cm()

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, evs in self.rows.items():
            ts = sorted(a.elapsed_time(b) * 1e3 for a, b, _, _ in evs)
            out[name] = dict(us_med=ts[len(ts) // 2], us_min=ts[0], flops=evs[0][2], bytes=evs[0][3], n=len(ts))
        return out


def bench_shape(T, in_f, out_f, iters, dev, tile):
    X, W, b, R, Y = operands(T, in_f, out_f, 1, dev)
    cache = {}
    ops.X6_TILE = tile
    res = {}
    for use_x6 in (True, False):
        ops.USE_LINEAR_X6 = use_x6
        for _ in range(3):
            ops.linear_relprop(R, X, W, Y=Y, bias=b, cache=cache)
        torch.cuda.synchronize()
        t = Timer()
        ops.KERNEL_TIMER = t
        try:
            for _ in range(iters):
                ops.linear_relprop(R, X, W, Y=Y, bias=b, cache=cache)
        finally:
            ops.KERNEL_TIMER = None
        res["x6" if use_x6 else "fp32"] = t.summary()
    ops.USE_LINEAR_X6 = True
    # whole rule, un-instrumented (one call = memset + split + Z + C back to back)
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops.linear_relprop(R, X, W, Y=Y, bias=b, cache=cache)
    a.record()
    for _ in range(iters):
        ops.linear_relprop(R, X, W, Y=Y, bias=b, cache=cache)
    e.record()
    torch.cuda.synchronize()
    res["x6_rule_us"] = a.elapsed_time(e) * 1e3 / iters
    return res


def check_shape(T, in_f, out_f, dev):
    """x6 vs fp64 and vs the fp32-MFMA path; tile geometries and a half batch bit for bit; hand-over flags clean."""
    from oracle import relprop_oracle as O
    X, W, b, R, Y = operands(T, in_f, out_f, 7, dev)
    X[1] = 0.0
    X[2] = X[2].abs() + 0.01
    W[:5] = -W[:5].abs() - 0.001                 # row 2 against these: every product negative -> cancellation fallback
    Y = torch.nn.functional.linear(X, W, b)
    cache = {}
    ops.USE_LINEAR_X6 = False
    fp32 = ops.linear_relprop(R, X, W, Y=Y, bias=b)
    ops.USE_LINEAR_X6 = True
    ops.X6_CHECK = True
    outs = {}
    for tile in (0, 1):
        ops.X6_TILE = tile
        outs[tile] = ops.linear_relprop(R, X, W, Y=Y, bias=b, cache=cache)
    ops.X6_TILE = 0
    h = T // 2
    half = ops.linear_relprop(R[:h].contiguous(), X[:h].contiguous(), W, Y=Y[:h].contiguous(), bias=b, cache=cache)
    ops.X6_CHECK = False
    torch.cuda.synchronize()
    ref64 = O.linear_relprop(R.double().cpu(), X.double().cpu(), W.double().cpu(), 1.0, "ours")
    scale = float(ref64.abs().max())
    e6 = float((outs[0].cpu().double() - ref64).abs().max())
    e32 = float((fp32.cpu().double() - ref64).abs().max())
    return dict(T=T, in_f=in_f, out_f=out_f, finite=bool(torch.isfinite(outs[0]).all()),
                err_x6_vs_fp64=e6 / scale, err_fp32_vs_fp64=e32 / scale,
                tiles_bitwise=bool(torch.equal(outs[0], outs[1])), half_bitwise=bool(torch.equal(half, outs[0][:h])),
                max_abs_x6_vs_fp32=float((outs[0] - fp32).abs().max()) / scale)


def zpass_ab(T, in_f, out_f, iters, dev):
    """us per Z-pass launch, |X| planes against signed planes, for the geometry the library picks and the three pins."""
    lib = _lib.load()
    X, W, b, R, Y = operands(T, in_f, out_f, 1, dev)
    wp = ops.x6_weight_planes(W)
    st = torch.cuda.current_stream().cuda_stream
    nb = lib.te_linear_x6_planes_bytes(T, in_f)
    planes = {"abs": torch.empty(nb, dtype=torch.uint8, device=dev), "signed": torch.empty(nb, dtype=torch.uint8, device=dev)}
    _lib.check(lib.te_linear_x6_split_abs_f32(X.data_ptr(), T, in_f, planes["abs"].data_ptr(), nb, st), "split_abs")
    _lib.check(lib.te_linear_x6_split_matrix_f32(X.data_ptr(), T, in_f, 0, planes["signed"].data_ptr(), nb, st), "split_matrix")
    ws = torch.zeros(lib.te_linear_relprop_x6_workspace_bytes(T, in_f, out_f), dtype=torch.uint8, device=dev)
    outs = {k: torch.empty((T, in_f), dtype=torch.float32, device=dev) for k in planes}

    def call(kind, flags):
        fl = flags | (ops.TE_X6_X_PLANES_SIGNED if kind == "signed" else 0)
        _lib.check(lib.te_linear_relprop_x6_f32(R.data_ptr(), None, 0, 1, X.data_ptr(), W.data_ptr(), wp.data_ptr(),
                                                planes[kind].data_ptr(), Y.data_ptr(), b.data_ptr(), outs[kind].data_ptr(), T, in_f,
                                                out_f, fl, None, ws.data_ptr(), ws.numel(), st), "te_linear_relprop_x6_f32")

    rows = []
    for geo, pin in (("auto", 0), ("128x256", _lib.TE_X6_TILE_128), ("256x256", _lib.TE_X6_TILE_256), ("128x128", _lib.TE_X6_TILE_128x128)):
        zpin = pin << ops.TE_X6_TILE_Z_SHIFT
        for kind in planes:                                   # the whole rule once: warm-up and the bitwise comparison
            call(kind, zpin)
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["abs"], outs["signed"]))
        clean = lib.te_linear_relprop_x6_check(ws.data_ptr(), T, in_f, out_f, st) == 0
        ev = {k: [] for k in planes}
        for _ in range(iters):
            for kind in planes:
                call(kind, zpin | ops.TE_X6_PHASE_SPLIT)       # (planes given: this phase only resets the hand-over flags)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(kind, zpin | ops.TE_X6_PHASE_Z)
                e.record()
                ev[kind].append((a, e))
        torch.cuda.synchronize()
        us = {k: sorted(a.elapsed_time(e) * 1e3 for a, e in v) for k, v in ev.items()}
        rows.append(dict(T=T, in_f=in_f, out_f=out_f, geometry=geo, out_bitwise=same, check_clean=clean,
                         abs_us_med=us["abs"][iters // 2], abs_us_min=us["abs"][0], signed_us_med=us["signed"][iters // 2],
                         signed_us_min=us["signed"][0], delta_us_med=us["signed"][iters // 2] - us["abs"][iters // 2]))
    return rows


def x6_schedule(lib, T, in_f, out_f, pass_, flags):
    """te_linear_x6_schedule as a dict (no launch): what a call with these flags would do."""
    import ctypes
    out = (ctypes.c_int * 4)()
    _lib.check(lib.te_linear_x6_schedule(T, in_f, out_f, pass_, flags, out), "te_linear_x6_schedule")
    return dict(geometry={1: "128x256", 2: "256x256", 3: "128x128"}[out[0]],
                schedule={0: "stream-K", 1: "whole static", 2: "whole claimed"}[out[1]], grid=out[2], tiles=out[3])


def schedule_ab(T, lname, in_f, out_f, iters, dev, pin):
    """us per launch of the four x6 launches of a layer (Z-pass, C-pass, forward product, input-gradient product) under the
    schedule variants, alternating launch by launch in one process; results compared bit for bit.  CU-time (CU us): stream-K
    holds its whole grid for the launch; a whole-tile launch holds a CU for the tiles it computes, tiles x (launch / rounds)."""
    import math
    lib = _lib.load()
    X, W, b, R, Y = operands(T, in_f, out_f, 1, dev)
    st = torch.cuda.current_stream().cuda_stream
    wp = ops.x6_weight_planes(W)
    status = ops.x6_status(dev)
    variants = {"slack": ops.TE_X6_SLACK_RULE, "cost": 0, "whole": ops.TE_X6_WHOLE_TILES,
                "static": ops.TE_X6_WHOLE_TILES | ops.TE_X6_STATIC_TILES}

    def planes_of(A, rows, K, transposed=0):
        nb = lib.te_linear_x6_planes_bytes(rows, K)
        p = torch.empty(nb, dtype=torch.uint8, device=dev)
        _lib.check(lib.te_linear_x6_split_matrix_f32(A.data_ptr(), rows, K, transposed, p.data_ptr(), nb, st), "split_matrix")
        return p

    xs = planes_of(X, T, in_f)
    ws = torch.zeros(lib.te_linear_relprop_x6_workspace_bytes(T, in_f, out_f), dtype=torch.uint8, device=dev)
    out = {v: torch.empty((T, in_f), dtype=torch.float32, device=dev) for v in variants}

    def rule(v, phase):
        _lib.check(lib.te_linear_relprop_x6_f32(R.data_ptr(), None, 0, 1, X.data_ptr(), W.data_ptr(), wp.data_ptr(), xs.data_ptr(),
                                                Y.data_ptr(), b.data_ptr(), out[v].data_ptr(), T, in_f, out_f,
                                                pin | variants[v] | ops.TE_X6_X_PLANES_SIGNED | phase, status.data_ptr(),
                                                ws.data_ptr(), ws.numel(), st), "te_linear_relprop_x6_f32")

    # the two plain products of the layer: forward [T, in_f] -> [T, out_f], input gradient [T, out_f] -> [T, in_f]
    dY = R
    prods = {"forward": (xs, planes_of(W, out_f, in_f), in_f, out_f, b),
             "input-gradient": (planes_of(dY, T, out_f), planes_of(W, in_f, out_f, 1), out_f, in_f, None)}
    gws = {k: torch.zeros(lib.te_gemm_x6_workspace_bytes(T, K, M), dtype=torch.uint8, device=dev) for k, (_, _, K, M, _) in prods.items()}
    gout = {(k, v): torch.empty((T, M), dtype=torch.float32, device=dev) for k, (_, _, K, M, _) in prods.items() for v in variants}

    def product(k, v):
        xp, wpl, K, M, bias = prods[k]
        _lib.check(lib.te_gemm_x6_f32(None, xp.data_ptr(), wpl.data_ptr(), None if bias is None else bias.data_ptr(),
                                      gout[k, v].data_ptr(), T, K, M, pin | variants[v], status.data_ptr(), gws[k].data_ptr(),
                                      gws[k].numel(), st), "te_gemm_x6_f32")

    launches = {"Z-pass": (ops.TE_X6_PASS_Z, in_f, out_f, in_f // 16, lambda v: rule(v, ops.TE_X6_PHASE_Z)),
                "C-pass": (ops.TE_X6_PASS_C, in_f, out_f, out_f // 16, lambda v: rule(v, ops.TE_X6_PHASE_C)),
                "forward product": (ops.TE_X6_PASS_PRODUCT, in_f, out_f, in_f // 16, lambda v: product("forward", v)),
                "input-gradient product": (ops.TE_X6_PASS_PRODUCT, out_f, in_f, out_f // 16, lambda v: product("input-gradient", v))}
    rows = []
    for name, (pass_, k_in, k_out, nks, launch) in launches.items():
        ev = {v: [] for v in variants}
        for it in range(iters + 3):
            for v in variants:
                if name == "Z-pass":
                    rule(v, ops.TE_X6_PHASE_SPLIT)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(v)
                e.record()
                if it >= 3:
                    ev[v].append((a, e))
        torch.cuda.synchronize()
        ref = out["slack"] if name in ("Z-pass", "C-pass") else gout[name.split(" product")[0], "slack"]
        for v in variants:
            got = out[v] if name in ("Z-pass", "C-pass") else gout[name.split(" product")[0], v]
            us = sorted(a.elapsed_time(e) * 1e3 for a, e in ev[v])
            s = x6_schedule(lib, T, k_in, k_out, pass_, pin | variants[v])
            r = s["tiles"] / s["grid"]
            per_tile = us[len(us) // 2] / (r if s["schedule"] == "stream-K" else math.ceil(r))
            rows.append(dict(layer=lname, launch=name, variant=v, nks=nks, **s, us_med=round(us[len(us) // 2], 1), us_min=round(us[0], 1),
                             us_per_k16=round(per_tile / nks, 3), cu_us=round(s["tiles"] * per_tile),
                             bitwise=bool(name == "Z-pass" or torch.equal(got, ref))))
    return rows


RAGGED_TS = (12544, 12608, 12800)      # 49 full tile columns of 256 rows, ViT-B batch 64 (49.25), 50 full columns


def ragged_ab(lname, in_f, out_f, iters, dev, pin):
    """us per launch of the four x6 launches of a layer at 49 full tile columns, at the 49.25 of ViT-B batch 64 and at 50 full columns,
    the three row counts alternating launch by launch in one process.  `position` = (t[12608] - t[12544]) / (t[12800] - t[12544]):
    1 where the ragged column costs what a full one costs, 0.25 where it costs its live rows."""
    lib = _lib.load()
    Tmax = max(RAGGED_TS)
    assert all(T % 32 == 0 for T in RAGGED_TS)      # (the planes of the first T rows are then the first blocks of the planes of Tmax rows)
    X, W, b, R, Y = operands(Tmax, in_f, out_f, 1, dev)
    st = torch.cuda.current_stream().cuda_stream
    wp = ops.x6_weight_planes(W)
    status = ops.x6_status(dev)

    def planes_of(A, rows, K, transposed=0):
        nb = lib.te_linear_x6_planes_bytes(rows, K)
        p = torch.empty(nb, dtype=torch.uint8, device=dev)
        _lib.check(lib.te_linear_x6_split_matrix_f32(A.data_ptr(), rows, K, transposed, p.data_ptr(), nb, st), "split_matrix")
        return p

    xs = planes_of(X, Tmax, in_f)
    # (a workspace per row count: where the S planes lie depends on T, and a C-pass reads those of its own Z-pass)
    wss = {T: torch.zeros(lib.te_linear_relprop_x6_workspace_bytes(T, in_f, out_f), dtype=torch.uint8, device=dev) for T in RAGGED_TS}
    out = torch.empty((Tmax, in_f), dtype=torch.float32, device=dev)

    def rule(T, phase):
        ws = wss[T]
        _lib.check(lib.te_linear_relprop_x6_f32(R.data_ptr(), None, 0, 1, X.data_ptr(), W.data_ptr(), wp.data_ptr(), xs.data_ptr(),
                                                Y.data_ptr(), b.data_ptr(), out.data_ptr(), T, in_f, out_f,
                                                pin | ops.TE_X6_X_PLANES_SIGNED | phase, status.data_ptr(), ws.data_ptr(), ws.numel(), st),
                   "te_linear_relprop_x6_f32")

    prods = {"forward": (xs, planes_of(W, out_f, in_f), in_f, out_f, b),
             "input-gradient": (planes_of(R, Tmax, out_f), planes_of(W, in_f, out_f, 1), out_f, in_f, None)}
    gws = {k: torch.zeros(lib.te_gemm_x6_workspace_bytes(Tmax, K, M), dtype=torch.uint8, device=dev) for k, (_, _, K, M, _) in prods.items()}
    gout = {k: torch.empty((Tmax, M), dtype=torch.float32, device=dev) for k, (_, _, K, M, _) in prods.items()}

    def product(k, T):
        xp, wpl, K, M, bias = prods[k]
        _lib.check(lib.te_gemm_x6_f32(None, xp.data_ptr(), wpl.data_ptr(), None if bias is None else bias.data_ptr(), gout[k].data_ptr(),
                                      T, K, M, pin, status.data_ptr(), gws[k].data_ptr(), gws[k].numel(), st), "te_gemm_x6_f32")

    for T in RAGGED_TS:            # the whole rule once per row count: warm-up, and the S planes the C-pass launches read
        rule(T, 0)
    launches = {"Z-pass": lambda T: rule(T, ops.TE_X6_PHASE_Z), "C-pass": lambda T: rule(T, ops.TE_X6_PHASE_C),
                "forward product": lambda T: product("forward", T), "input-gradient product": lambda T: product("input-gradient", T)}
    rows = []
    for name, launch in launches.items():
        ev = {T: [] for T in RAGGED_TS}
        for it in range(iters + 3):
            for T in RAGGED_TS:
                if name == "Z-pass":
                    rule(T, ops.TE_X6_PHASE_SPLIT)           # (planes given: this phase only resets the hand-over flags)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(T)
                e.record()
                if it >= 3:
                    ev[T].append((a, e))
        torch.cuda.synchronize()
        us = {T: sorted(a.elapsed_time(e) * 1e3 for a, e in v) for T, v in ev.items()}
        med = {T: v[len(v) // 2] for T, v in us.items()}
        lo, mid, hi = (med[T] for T in RAGGED_TS)
        rows.append(dict(layer=lname, launch=name, **{f"us_med_{T}": round(med[T], 1) for T in RAGGED_TS},
                         **{f"us_spread_{T}": round(us[T][-1] - us[T][0], 1) for T in RAGGED_TS},
                         position=round((mid - lo) / (hi - lo), 2) if hi > lo else None))
    assert int(status[0].item()) == 0
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vit_b16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--check-rows", type=int, default=1100)
    ap.add_argument("--tiles", default="0,1")
    ap.add_argument("--skip-checks", action="store_true")
    ap.add_argument("--zpass-ab", action="store_true", help="Z-pass on |X| planes against signed planes, per shape and geometry")
    ap.add_argument("--schedule-ab", action="store_true",
                    help="the four x6 launches of every layer under the schedule variants (slack rule, cost rule, whole tiles claimed / static)")
    ap.add_argument("--pin", type=int, default=2, help="--schedule-ab: TE_X6_TILE_* pin (2 = what bench.py pins under concurrent streams)")
    ap.add_argument("--ragged-ab", action="store_true",
                    help="the four x6 launches of every ViT-B layer at 49, 49.25 and 50 tile columns of activation rows (--pin as --schedule-ab)")
    a = ap.parse_args()
    _lib.require_device()
    dev = torch.device("cuda:0")
    names = list(CONFIGS) if a.config == "all" else a.config.split(",")
    if a.ragged_ab:
        for (lname, in_f, out_f) in CONFIGS["vit_b16"][1]:
            for r in ragged_ab(lname, in_f, out_f, a.iters, dev, a.pin):
                print("RAGGED " + json.dumps(r), flush=True)
        return
    if a.schedule_ab:
        for name in names:
            T, shapes = CONFIGS[name]
            for (lname, in_f, out_f) in shapes:
                for r in schedule_ab(T, lname, in_f, out_f, a.iters, dev, a.pin):
                    print("SCHEDULE " + json.dumps(dict(config=name, T=T, **r)), flush=True)
        return
    if a.zpass_ab:
        for name in names:
            T, shapes = CONFIGS[name]
            for (lname, in_f, out_f) in shapes:
                for r in zpass_ab(T, in_f, out_f, a.iters, dev):
                    print("ZPASS " + json.dumps(dict(config=name, layer=lname, **r)), flush=True)
        return
    if not a.skip_checks:
        for (T, i, o) in [(a.check_rows, 768, 2304), (a.check_rows, 3072, 768), (394, 768, 768), (300, 128, 384),
                          (70, 192, 128), (2 * 197, 1024, 4096)]:
            r = check_shape(T, i, o, dev)
            ok = (r["finite"] and r["tiles_bitwise"] and r["half_bitwise"]
                  and r["err_x6_vs_fp64"] <= 2.0 * r["err_fp32_vs_fp64"] + 1e-9)
            print(("CHECK ok   " if ok else "CHECK FAIL ") + json.dumps(r), flush=True)
    for name in names:
        T, shapes = CONFIGS[name]
        tot = {}
        for (lname, in_f, out_f) in shapes:
            for tile in [int(t) for t in a.tiles.split(",")]:
                if tile == 1 and not (out_f % 256 == 0 and in_f % 128 == 0):
                    continue
                r = bench_shape(T, in_f, out_f, a.iters, dev, tile)
                x6 = r["x6"]
                gemm = 2.0 * T * in_f * out_f
                line = dict(config=name, layer=lname, T=T, in_f=in_f, out_f=out_f, tile=("256" if tile == 0 else "128"),
                            split_us=x6["linear_x6_split"]["us_med"], z_us=x6["linear_x6_zpass"]["us_med"],
                            c_us=x6["linear_x6_cpass"]["us_med"], rule_us=r["x6_rule_us"],
                            z_bf16_tf=6 * gemm / x6["linear_x6_zpass"]["us_med"] * 1e-6,
                            c_bf16_tf=12 * gemm / x6["linear_x6_cpass"]["us_med"] * 1e-6,
                            fp32_z_us=r["fp32"].get("linear_zpass_fwd", {}).get("us_med"),
                            fp32_c_us=r["fp32"].get("linear_cpass", {}).get("us_med"))
                line["rule_fp32equiv_tf"] = 3 * gemm / line["rule_us"] * 1e-6
                line["rule_bf16_tf"] = 18 * gemm / line["rule_us"] * 1e-6
                print("BENCH " + json.dumps(line), flush=True)
                tot.setdefault(tile, []).append(line["rule_us"])
        for tile, v in tot.items():
            print(f"TOTAL {name} tile={'256' if tile == 0 else '128'}: one block's four rules {sum(v):.0f} us", flush=True)
    rc = te._lib.load()
    del rc


if __name__ == "__main__":
    main()
