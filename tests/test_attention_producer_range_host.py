"""CPU side of the attention-producer range tests (tests/attention_producer_inputs.py, gpu_util.check_producer_groups; the
kernels are judged in tests/test_gpu_attention_producer_range.py):

  * the inputs are finite and normal, a third bf16 plane 2^-16 below them and the 2^-24 of the homogeneity checks included;
  * the bound is fair: an independently ordered fp32 restatement of the block -- scores as four 16-wide partial products, an
    online softmax over 32-key chunks, `out` accumulated per chunk, row sums from d_out . out -- stays within 3/4 of it per
    group against fp64 autograd, on every case and shape the GPU tests use; for bf16 the same restatement with a rounding to
    bf16 wherever csrc/te_attn_bf16.hip documents one (z, scaled score + mask, p, out, d_attn, d_s);
  * the check bites: three mutants of the restatement pass gpu_util.check at the bars of tests/test_gpu_producers.py on its
    inputs (unit Gaussians, the tail of the even samples masked) and fail here."""
import functools

import pytest
import torch

import attention_producer_inputs as A
import gpu_util
from gpu_util import check, check_producer_groups

FAIR = 0.75
# every (entry, N, chunk) the GPU file runs: (bf16?, N, keys per chunk of the kernel that N reaches)
FP32_SHAPES = [(33, 32), (160, 32), (161, 32), (224, 32), (17, 32), (64, 32), (65, 32), (97, 32), (130, 64), (257, 32), (640, 64)]
BF16_SHAPES = [(97, 32), (289, 32), (545, 32), (640, 32)]
LARGEST = {224, 640}
FUSED_N = {33, 160, 161, 224}          # the fused entry takes no mask


@pytest.fixture(autouse=True)
def _no_report(monkeypatch):
    monkeypatch.setattr(gpu_util, "record", lambda *a, **k: None)      # the parity report belongs to the device runs


def cases_of(N, masked_entry):
    if N in LARGEST:
        return [c for c in A.LARGEST_N_CASES if masked_entry or c not in A.MASK_CASES]
    return A.UNMASKED_CASES + (A.MASK_CASES if masked_entry else [])


def _rb(t, bf16):
    return t.bfloat16().float() if bf16 else t


def restatement(c, bf16=False, chunk=32, no_max=False, mask_before_scale=False, scale=A.SCALE):
    """The block in fp32 in another order than torch's: q k^T as four 16-wide partial products, one pass over key chunks with
    a running maximum m, a running sum l = l exp(m - m') + sum exp(s - m') and `out` rescaled alongside; attn from the final
    (m, l); d_attn = g v^T in four partial products; the softmax backward's row sums from d_out . out.  bf16: rounded where
    the bf16 kernel rounds.  The mutants: no_max (no maximum subtracted), mask_before_scale ((z + mask) scale)."""
    q, k, v, g, mask = c["q"], c["k"], c["v"], c["g"], c["mask"]
    N = q.shape[-2]
    z = sum(q[..., i:i + 16] @ k[..., i:i + 16].transpose(-1, -2) for i in range(0, A.D, 16))
    z = _rb(z, bf16)
    if mask_before_scale:
        s = (z + (0.0 if mask is None else mask)) * scale
    else:
        x = _rb(z * scale, bf16)
        s = _rb(x if mask is None else x + mask, bf16)
    m = torch.full(s.shape[:-1] + (1,), float("-inf"))
    l_sum = torch.zeros_like(m)
    acc = torch.zeros_like(q)
    for j in range(0, N, chunk):
        sc = s[..., j:j + chunk]
        m_new = torch.zeros_like(m) if no_max else torch.maximum(m, sc.amax(-1, keepdim=True))
        e = torch.exp(sc - m_new)
        w = torch.exp(m - m_new)
        l_sum = l_sum * w + e.sum(-1, keepdim=True)
        if not bf16:
            acc = acc * w + e @ v[..., j:j + chunk, :]
        m = m_new
    p = _rb(torch.exp(s - m) / l_sum, bf16)
    out = _rb(p @ v, True) if bf16 else acc / l_sum          # (bf16: out = bf16(attn v) with the rounded attn)
    d_attn = _rb(sum(g[..., i:i + 16] @ v[..., i:i + 16].transpose(-1, -2) for i in range(0, A.D, 16)), bf16)
    rowsum = (g * out).sum(-1, keepdim=True)
    d_s = _rb(p * (d_attn - rowsum), bf16)
    return {"z_qk": z, "attn": p, "out": out, "d_attn": d_attn, "d_q": _rb((d_s @ k) * scale, bf16),
            "d_k": _rb((d_s.transpose(-1, -2) @ q) * scale, bf16), "d_v": _rb(p.transpose(-1, -2) @ g, bf16)}


@functools.lru_cache(maxsize=4)
def _refs(case, N, chunk, bf16):
    c = A.producer_case(case, N, chunk, bf16)
    ref = A.chain64(c)
    dt = torch.bfloat16 if bf16 else torch.float32
    stock = A.chain(*(c[n].to(dt) for n in ("q", "k", "v", "g")), None if c["mask"] is None else c["mask"].to(dt))
    return c, ref, stock


def judge(tag, got, c, ref, stock, bf16, limit=1.0, names=None):
    """Every output of `got` per group at the bound the kernels are held to; returns the worst err / bound."""
    worst = 0.0
    for name in names or A.TOL:
        xmax, floor = A.bound_terms(name, c, ref)
        s = check_producer_groups(f"{tag}.{name}", got[name], stock[name].float(), ref[name], A.GROUP_DIMS[name],
                                  A.BF16_TOL if bf16 else A.TOL[name], xmax, floor)
        assert s["worst_over_bound"] <= limit, (tag, name, s)
        worst = max(worst, s["worst_over_bound"])
    return worst


# ------------------------------------------------------------------------------------------------ the comparison itself
def test_check_producer_groups_judges_every_group():
    ref = torch.tensor([[1.0, -2.0], [1e-12, 3e-12], [0.0, 0.0]], dtype=torch.float64)
    ok = ref.float()
    s = check_producer_groups("t", ok, ok, ref, -1, 1e-6)
    assert s["groups"] == 3 and s["worst_over_bound"] <= 0.1
    bad = ok.clone()
    bad[1, 1] = 0.0                              # invisible to check(), 100 % of its own row
    check("t", bad, ok, 1e-6)
    with pytest.raises(AssertionError):
        check_producer_groups("t", bad, ok, ref, -1, 1e-6)
    # ... unless the stock chain is as wrong there (2 x err_stock), the score term allows it, or the floor lifts the scale
    check_producer_groups("t", bad, bad, ref, -1, 1e-6)
    check_producer_groups("t", bad, ok, ref, -1, 1e-6, xmax=torch.tensor([0.0, 2.0 ** 22, 0.0]))
    check_producer_groups("t", bad, ok, ref, -1, 1e-6, scale_floor=torch.tensor([0.0, 1.0, 0.0]))
    dirty = ok.clone()
    dirty[2, 0] = 1e-30                          # a group whose bound is zero must be exact
    with pytest.raises(AssertionError):
        check_producer_groups("t", dirty, ok, ref, -1, 1e-6)
    nan = ok.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        check_producer_groups("t", nan, ok, ref, -1, 1e-6)


# ------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_inputs_are_finite_normal_and_scaled_by_powers_of_two(bf16):
    # 2^-16 for the third plane and 2^-24 for the homogeneity check below the smallest value: still normal
    room = torch.finfo(torch.float32).tiny * 2.0 ** 40
    for N, chunk in ((97, 32), (130, 64)):
        for case in A.UNMASKED_CASES + A.MASK_CASES:
            c = A.producer_case(case, N, chunk, bf16)
            for n in ("q", "k", "v", "g"):
                t = c[n]
                assert t.shape == (A.B, A.H, N, A.D) and torch.isfinite(t).all(), (case, n)
                assert not ((t != 0) & (t.abs() < room)).any(), (case, n)
                if bf16:
                    assert torch.equal(t, t.bfloat16().float())
            if c["mask"] is not None:
                assert c["mask"].shape == (A.B, 1, 1, N) and torch.isfinite(c["mask"]).all()
                if bf16:
                    assert torch.equal(c["mask"], c["mask"].bfloat16().float())
            qkv, g_out = A.fused_layout(c)
            for a, b in zip(A.split_fused(qkv), (c["q"], c["k"], c["v"])):
                assert torch.equal(a, b)
            assert torch.equal(A.split_heads(g_out), c["g"])
            for a, n in zip(A.three_layout(c), ("q", "k", "v", "g")):
                assert torch.equal(A.split_heads(a), c[n])
    base, c = A.producer_case("stripes", 97)["v"], A.producer_case("v_scaled", 97)
    ratio = c["v"][1, 2] / base[1, 2]
    assert torch.equal(ratio, torch.full_like(ratio, 2.0 ** -40))
    t = A.producer_case("temperature", 97)["q"] / A.producer_case("stripes", 97)["q"]
    assert float(t.min()) == 0.5 and float(t.max()) == 32.0
    x = A.chain64(A.producer_case("offset_pos", 97))["x"]
    assert float(x.min()) > 150.0 and float(A.chain64(A.producer_case("offset_neg", 97))["x"].max()) < -150.0
    assert [A.dominant_position(n, 130, 64) for n in A.UNMASKED_CASES[5:]] == [0, 63, 128, 129]
    assert [A.dominant_position(n, 17, 32) for n in A.UNMASKED_CASES[5:]] == [0, 16, 0, 16]
    m = A.mask_of("first_chunk", 17)
    assert int((m != 0).sum()) == A.B * 16 and float(m[0, 0, 0, 16]) == 0.0
    assert int((A.mask_of("all_but_one", 65) == 0).sum()) == A.B
    assert float(A.mask_of("fmin", 65, True).min()) == torch.finfo(torch.bfloat16).min
    assert float(A.mask_of("stripes", 65, True).min()) == -9984.0


# ------------------------------------------------------------------------------------------------ the bound is fair
def _fair(N, chunk, bf16):
    worst = {}
    for case in cases_of(N, bf16 or N not in FUSED_N):
        c, ref, stock = _refs(case, N, chunk, bf16)
        got = restatement(c, bf16)
        assert all(torch.isfinite(t).all() for t in got.values()), case
        worst[case] = judge(f"host.producer.{case}.{N}", got, c, ref, stock, bf16, FAIR)
    return worst


@pytest.mark.parametrize("N,chunk", FP32_SHAPES)
def test_fp32_restatement_within_three_quarters_of_the_bound(N, chunk):
    print(_fair(N, chunk, False))


@pytest.mark.parametrize("N,chunk", BF16_SHAPES)
def test_bf16_restatement_within_three_quarters_of_the_bound(N, chunk):
    print(_fair(N, chunk, True))


def test_score_term_is_needed_for_the_offset_cases():
    """Without 4 x 2^-24 xmax the offset cases are out of reach of any fp32 evaluation: every score is rounded at ulp(200)."""
    c, ref, stock = _refs("offset_pos", 130, 64, False)
    got = restatement(c)
    s = check_producer_groups("t", got["attn"], stock["attn"], ref["attn"], -1, A.TOL["attn"], A.bound_terms("attn", c, ref)[0])
    worst_without = 0.0
    err = (got["attn"].double() - ref["attn"]).abs().amax(-1)
    err_stock = (stock["attn"].double() - ref["attn"]).abs().amax(-1)
    worst_without = float((err / (2 * err_stock + A.TOL["attn"] * ref["attn"].amax(-1))).max())
    print(s["worst_over_bound"], worst_without)
    assert s["worst_over_bound"] <= FAIR < worst_without


# ------------------------------------------------------------------------------------------------ the check bites
def _todays_case(N=97, masked=True):
    """The operands of tests/test_gpu_producers.py: unit Gaussians, the tail of the even samples masked at -10000."""
    c = A.producer_case("stripes", N, seed=81)
    c["mask"] = None
    if masked:
        c["mask"] = torch.zeros(A.B, 1, 1, N)
        c["mask"][::2, ..., N - max(1, N // 8):] = A.MASKED_AWAY
    return c


def _passes_todays_check(got, c):
    stock = A.chain(c["q"], c["k"], c["v"], c["g"], c["mask"])
    for name, tol in A.TOL.items():
        check(f"today.{name}", got[name], stock[name], tol)


def _zero_small_heads(got):
    """Mutant (a): out and d_v of every head below 1e-6 of the tensor's maximum flushed to zero."""
    m = dict(got)
    for name in ("out", "d_v"):
        t = got[name].clone()
        heads = t.abs().amax((-2, -1), keepdim=True)
        m[name] = torch.where(heads < 1e-6 * heads.max(), torch.zeros_like(t), t)
    return m


def test_mutant_zeroed_small_heads_passes_the_old_check_and_fails_per_group():
    today = _todays_case()
    _passes_todays_check(_zero_small_heads(restatement(today)), today)
    failed = []
    for case, names in (("v_scaled", ("out",)), ("g_scaled", ("d_v",))):      # (d_v = attn^T d_out: v does not enter it)
        c, ref, stock = _refs(case, 97, 32, False)
        good = restatement(c)
        judge("mutant.a.good", good, c, ref, stock, False, FAIR)
        mutant = _zero_small_heads(good)
        check(f"mutant.a.{case}.out", mutant["out"], stock["out"], A.TOL["out"])          # the whole-tensor metric: blind
        check(f"mutant.a.{case}.d_v", mutant["d_v"], stock["d_v"], A.TOL["d_v"])
        for name in names:
            with pytest.raises(AssertionError):
                judge("mutant.a", mutant, c, ref, stock, False, names=(name,))
            failed.append((case, name))
    assert len(failed) == 2


def test_mutant_softmax_without_max_subtraction_passes_the_old_check_and_fails_here():
    today = _todays_case()
    _passes_todays_check(restatement(today, no_max=True), today)
    c, ref, stock = _refs("offset_pos", 97, 32, False)
    with pytest.raises(AssertionError):
        judge("mutant.b", restatement(c, no_max=True), c, ref, stock, False, names=("attn",))
    # offset_neg underflows instead: every exponential is 0 and the row is 0 / 0
    c, ref, stock = _refs("offset_neg", 97, 32, False)
    with pytest.raises(AssertionError):
        judge("mutant.b", restatement(c, no_max=True), c, ref, stock, False, names=("attn",))


def test_mutant_mask_before_scaling_passes_the_old_check_and_fails_here():
    today = _todays_case()
    _passes_todays_check(restatement(today, mask_before_scale=True), today)
    c, ref, stock = _refs("soft", 97, 32, False)
    judge("mutant.c.good", restatement(c), c, ref, stock, False, FAIR)
    for name in ("attn", "out", "d_q", "d_k", "d_v"):
        with pytest.raises(AssertionError):
            judge("mutant.c", restatement(c, mask_before_scale=True), c, ref, stock, False, names=(name,))
