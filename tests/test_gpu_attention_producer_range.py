"""`-m gpu`: the attention PRODUCERS -- the kernels that make attn, out, d_attn, d_q, d_k and d_v -- on peaked, shifted, scaled
and masked scores (tests/attention_producer_inputs.py), every output judged per group against the fp64 chain on the host:
attn, out, d_attn and d_q per query row, d_k and d_v per (b, h),

    err_g <= 2 err_stock_g + (tol + 4 x 2^-24 xmax_g) scale_g            (gpu_util.check_producer_groups)

with err_stock_g the stock torch chain on the device in the operands' dtype, tol the bar the kernel already has in
tests/test_gpu_producers.py (3e-6; 1e-5 for d_q and d_k; bf16: 2^-7, one bf16 ulp of the group's maximum), xmax_g the largest
|scaled score| of the group before the mask (four roundings of a score at half an ulp each: product, scaling, mask addition,
max subtraction; absent for d_attn) and scale_g the group's own fp64 maximum -- for d_q and d_k at least the magnitude of the
terms that cancel in d_s, scale max|d_attn| max(|q|, |k|) of the (b, h).  tests/test_attention_producer_range_host.py shows
on the CPU that an independently ordered fp32 (bf16-rounded) restatement stays within 3/4 of this bound on every case and
shape below, and that three mutants of it fail it while passing gpu_util.check.

Beside the bound, bit for bit: homogeneity in v and g_out, a sample or a head alone = itself in the batch, exact zeros under
masked keys, a one-hot row when one key is left, and a NaN that stays in its row.

Which kernel each N reaches (csrc/te_attn.hip, the launchers of te_attn_fwd6 / rc / rules / long / fwd6l / bwd6l / bf16):
  fused    33   te_attn_fwd6 (two key blocks); backward: te_attn_kb AV, then te_attn_rc (N <= 160) with and without `out`
           160  the last N te_attn_rc takes without `out`
           161  without `out` the te_attn_rules BWD kernel, with `out` te_attn_rc: the seam
           224  the longest the fused entry takes (seven key blocks)
  strided  17   te_attn_long (N <= 64), forward and both backward sides; one ragged 32-row tile
           64   the last N of te_attn_long: two full tiles
           65   te_attn_fwd6l / te_attn_bwd6l, 4-wave cut, 32-key chunks: the shortest they take, one key past two chunks
           97   4-wave cut, four row blocks: every wave of the workgroup owns one; one key past three chunks
           130  8-wave cut, 64-key chunks: five row blocks, two keys past two chunks
           257  4-wave cut again (nine row blocks in three parts of a (b, h))
           640  8-wave cut, twenty row blocks in three parts: the longest
           (without `out` and with need_qk the row side is te_attn_long's at every N; the column side te_attn_bwd6l's beyond 64)
  bf16     97   attn_*_bf16_kernel<8>  (N <= 256)       289  <16> (N <= 512)       545, 640  <20>
The largest N of each entry takes temperature, offset_pos and first_chunk only."""
import functools

import pytest
import torch

import attention_producer_inputs as A
from gpu_util import check_producer_groups, dev, record

pytestmark = pytest.mark.gpu

# entry -> [(N, keys per chunk of the forward kernel that N reaches)]
SHAPES = {"fused": [(33, 32), (160, 32), (161, 32), (224, 32)],
          "strided": [(17, 32), (64, 32), (65, 32), (97, 32), (130, 64), (257, 32), (640, 64)],
          "bf16": [(97, 32), (289, 32), (545, 32), (640, 32)]}
# (need_qk, with the forward output): every pair at which a dispatcher takes another kernel or another row sum
VARIANTS = {"fused": [(True, False), (True, True), (False, False)], "strided": [(True, False), (True, True), (False, True)],
            "bf16": [(True, False), (False, False)]}      # (the bf16 backward has no `out` operand)
NAN_SHAPES = [("fused", 33), ("fused", 224), ("strided", 17), ("strided", 97), ("strided", 130), ("bf16", 97)]


def _params():
    out = []
    for entry, shapes in SHAPES.items():
        for N, chunk in shapes:
            cases = A.UNMASKED_CASES + (A.MASK_CASES if entry != "fused" else [])
            if N == shapes[-1][0]:
                cases = [c for c in A.LARGEST_N_CASES if c in cases]
            out += [pytest.param(entry, N, chunk, case, id=f"{entry}-N{N}-{case}") for case in cases]
    return out


@functools.lru_cache(maxsize=2)
def _reference(case, N, chunk, bf16):
    """The case and its fp64 chain on the host: computed once, shared, left unchanged."""
    c = A.producer_case(case, N, chunk, bf16)
    return c, A.chain64(c)


def _dtype(entry):
    return torch.bfloat16 if entry == "bf16" else torch.float32


def forward(entry, c):
    """The entry's forward on the operands of c ([B',H',N,64], any B', H'): outputs in the [B',H',N,*] layout, plus what the
    backward needs."""
    from transformer_explainability_amd import ops
    heads, dt, d = c["q"].shape[1], _dtype(entry), dev()
    if entry == "fused":
        qkv, g_out = (t.to(d) for t in A.fused_layout(c))
        out, attn, zqk = ops.attention_forward(qkv, heads, A.SCALE)
        return {"z_qk": zqk, "attn": attn, "out": A.split_heads(out, heads), "_": (qkv, g_out, out)}
    q, k, v, g_out = (t.to(d).to(dt) for t in A.three_layout(c))
    mask = None if c["mask"] is None else c["mask"].to(d).to(dt)
    out, attn, zqk, _ = ops.attention_forward_qkv(q, k, v, heads, A.SCALE, mask=mask, want_z=True)
    return {"z_qk": zqk, "attn": attn, "out": A.split_heads(out, heads), "_": (q, k, v, g_out, out)}


def backward(entry, fwd, need_qk, with_out):
    from transformer_explainability_amd import ops
    heads = fwd["attn"].shape[1]
    if entry == "fused":
        qkv, g_out, out = fwd["_"]
        d_attn, d_qkv = ops.attention_backward(g_out, qkv, fwd["attn"], heads, A.SCALE, need_qk=need_qk, out=out if with_out else None)
        d_q, d_k, d_v = A.split_fused(d_qkv, heads)
    else:
        q, k, v, g_out, out = fwd["_"]
        d_q, d_k, d_v = (torch.full_like(out, float("nan")) for _ in range(3))
        d_attn = ops.attention_backward_qkv(g_out, q, k, v, fwd["attn"], heads, A.SCALE, d_q if need_qk else None,
                                            d_k if need_qk else None, d_v, need_qk=need_qk, out=out if with_out else None)
        d_q, d_k, d_v = (A.split_heads(t, heads) for t in (d_q, d_k, d_v))
    res = {"d_attn": d_attn, "d_v": d_v}
    if need_qk:
        res.update(d_q=d_q, d_k=d_k)
    return res


def _sub(c, b=None, h=None):
    """Sample b (head h) of a case alone."""
    pick = lambda t: t[(slice(None) if b is None else slice(b, b + 1)), (slice(None) if h is None else slice(h, h + 1))]      # noqa: E731
    out = {n: pick(c[n]).contiguous() for n in ("q", "k", "v", "g")}
    out["mask"] = None if c["mask"] is None else (c["mask"] if b is None else c["mask"][b:b + 1])
    return out


def _stock(entry, c):
    dt, d = _dtype(entry), dev()
    res = A.chain(*(c[n].to(d).to(dt) for n in ("q", "k", "v", "g")), None if c["mask"] is None else c["mask"].to(d).to(dt))
    return {n: t.float().cpu() for n, t in res.items()}


def _judge(variant, got, names, c, ref, stock, bf16, fails, figures):
    for name in names:
        xmax, floor = A.bound_terms(name, c, ref)
        try:
            check_producer_groups((variant, name), got[name].float(), stock[name], ref[name], A.GROUP_DIMS[name],
                                  A.BF16_TOL if bf16 else A.TOL[name], xmax, floor, sink=figures)
        except AssertionError as e:      # (every figure of the test first, then the verdict)
            fails.append(e.args[0])


def _report(tag, figures, row_err):
    """One line per test: per tensor [the worst err / bound over the variants that make it, that variant, its worst group, the
    kernel's worst err / scale, the stock chain's worst err / scale], and the largest |row sum of attn - 1|."""
    sig = lambda x: float(f"{x:.3g}")      # noqa: E731
    worst = {}
    for (variant, name), s in figures.items():
        if name not in worst or s["worst_over_bound"] > worst[name][0]:
            worst[name] = [sig(s["worst_over_bound"]), variant, s["worst_group"], sig(s["worst_ratio"]), sig(s["stock_worst_ratio"])]
    record(tag, **worst, row_sums=sig(row_err))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                              b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


def _equal_scaled(a, base, s):
    """a == s x base bit for bit (s a power of two; -0 and 0 alike, as == has it)."""
    return torch.equal(a.float(), base.float() * s)


@pytest.mark.parametrize("entry,N,chunk,case", _params())
def test_attention_producers_per_row_and_per_head(entry, N, chunk, case):
    bf16 = entry == "bf16"
    c, ref = _reference(case, N, chunk, bf16)
    stock = _stock(entry, c)
    tag = f"apr.{entry}.{case}.N{N}"
    fails, figures = [], {}
    fwd = forward(entry, c)
    _judge("fwd", fwd, ("attn", "out"), c, ref, stock, bf16, fails, figures)
    bwd = {}
    for need_qk, with_out in VARIANTS[entry]:
        bwd[need_qk, with_out] = r = backward(entry, fwd, need_qk, with_out)
        _judge(f"{'qk' if need_qk else 'noqk'}.{'out' if with_out else 'noout'}", r, tuple(r), c, ref, stock, bf16, fails, figures)
    # finiteness and row sums
    for name, t in list(fwd.items())[:3] + [(f"{k}.{n}", t) for k, r in bwd.items() for n, t in r.items()]:
        assert bool(torch.isfinite(t.float()).all()), (tag, name)
    row_err = float((fwd["attn"].float().sum(-1) - 1).abs().max())
    _report(tag, figures, row_err)
    assert row_err < (A.BF16_ROW_SUM_TOL if bf16 else A.ROW_SUM_TOL), (tag, row_err)
    # exact zeros under masked keys that sit beside an unmasked one; exactly one-hot where one key is left
    if case in A.EXACT_ZERO_CASES:
        gone = (c["mask"].view(A.B, N) < -1000.0).to(dev())                    # [B,N]
        assert bool(gone.any())
        assert not bool(fwd["attn"].permute(0, 3, 1, 2)[gone].any()), tag      # attn[b, :, :, j]
        for key, r in bwd.items():
            assert not bool(r["d_v"].permute(0, 2, 1, 3)[gone].any()), (tag, key, "d_v")
            if "d_k" in r:
                assert not bool(r["d_k"].permute(0, 2, 1, 3)[gone].any()), (tag, key, "d_k")
    if case == "all_but_one":
        hot = torch.zeros_like(fwd["attn"])
        hot[..., N // 2] = 1.0
        assert torch.equal(fwd["attn"], hot), tag
    # a sample alone and a head alone = itself in the batch
    for b, h in [(b, None) for b in range(A.B)] + [(None, h) for h in range(A.H)]:
        one = _sub(c, b, h)
        f1 = forward(entry, one)
        pick = lambda t: t[(slice(None) if b is None else slice(b, b + 1)), (slice(None) if h is None else slice(h, h + 1))]      # noqa: E731
        for name in ("z_qk", "attn", "out"):
            assert _same_bits(f1[name], pick(fwd[name])), (tag, "alone", b, h, name)
        for key in VARIANTS[entry]:
            if key[0]:
                for name, t in backward(entry, f1, *key).items():
                    assert _same_bits(t, pick(bwd[key][name])), (tag, "alone", b, h, key, name)
    # homogeneity, on every case: powers of two, nothing leaves the normal range
    for kk in A.HOMOGENEITY_K:
        s = float(A.pow2(-kk))
        fv = forward(entry, dict(c, v=c["v"] * s))
        assert _same_bits(fv["attn"], fwd["attn"]) and _equal_scaled(fv["out"], fwd["out"], s), (tag, "v", kk, "forward")
        fg = forward(entry, dict(c, g=c["g"] * s))
        assert _same_bits(fg["out"], fwd["out"])
        for key in VARIANTS[entry]:
            bv, bg = backward(entry, fv, *key), backward(entry, fg, *key)
            assert _equal_scaled(bv["d_attn"], bwd[key]["d_attn"], s), (tag, "v", kk, key, "d_attn")
            assert _same_bits(bv["d_v"], bwd[key]["d_v"]), (tag, "v", kk, key, "d_v")
            for name, t in bg.items():
                assert _equal_scaled(t, bwd[key][name], s), (tag, "g_out", kk, key, name)
    assert not fails, fails


@pytest.mark.parametrize("entry,N", NAN_SHAPES)
def test_one_nan_stays_in_its_row(entry, N):
    """A NaN in q[0, 1, 5]: every other (b, h) keeps the bits of the clean run, every other row of that head's attn, out and
    d_attn too; z_qk row 5 is NaN and attn row 5 non-finite, as in torch."""
    c = A.producer_case("stripes", N, bf16=entry == "bf16")
    c["mask"] = None
    clean = forward(entry, c)
    key = VARIANTS[entry][1] if entry != "bf16" else VARIANTS[entry][0]
    clean.update(backward(entry, clean, *key))
    bad = dict(c, q=c["q"].clone())
    bad["q"][0, 1, 5, 7] = float("nan")
    got = forward(entry, bad)
    got.update(backward(entry, got, *key))
    others = torch.ones(A.B, A.H, dtype=torch.bool)
    others[0, 1] = False
    for name in A.NAMES:
        assert _same_bits(got[name][others.to(dev())], clean[name][others.to(dev())]), (entry, N, name)
    rows = torch.arange(N) != 5
    for name in ("z_qk", "attn", "out", "d_attn"):
        assert _same_bits(got[name][0, 1][rows], clean[name][0, 1][rows]), (entry, N, name)
    assert bool(torch.isnan(got["z_qk"][0, 1, 5].float()).all()), (entry, N, "z_qk")
    assert not bool(torch.isfinite(got["attn"][0, 1, 5].float()).any()), (entry, N, "attn")
