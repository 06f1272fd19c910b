"""`-m gpu`: the bf16 relprop rules one at a time, at the shapes and alignments a whole bf16 model never produces.

Streaming rules (csrc/te_elementwise.hip with TX = te_bf16_t: Add two-pass and deferred, Clone plain and scaled, IndexSelect,
the grad x cam head mean), each (a) against the fp64 oracle on exact copies at the tolerance of the fp32 test of the same
rule, (b) bit for bit against the fp32 kernel on exact fp32 copies -- one template, identical arithmetic; for Add the fp32
call is built to take the same VEC form, whose fp64 sums run in the same order -- and (c) batch == samples run alone,
deferred == two-pass once materialised.  Shapes: n % 4 != 0 and a misaligned relevance (the VEC == 1 instantiations),
bf16 operands at odd element offsets of a larger buffer (ldx4 on 2-byte-aligned pointers), two chunks per sample, every
head-mean kernel including the second trip of the grid-stride one.  The inputs (bf16_rule_inputs.py) carry exact zeros,
-0.0 and exact cancellation X0 == -X1; test_bf16_host.py checks on the CPU that they leave the tolerances to the kernels.

GEMM-shaped rules (csrc/te_bf16.hip: Linear, AV, QK): every case on fresh aligned tensors and on views of the same values
whose row starts are not 16-byte aligned, with a ragged K (N = 70) -- the element-wise branches of fetch(); the results must
be the same bits, and one of them meets the fp64 bars of test_gpu_bf16.py.  Linear with a deferred factor over several
samples, an in-place weight edit against the cached planes, and N = 1 / N = 1024 of the attention rules.

Clone and IndexSelect take no variant argument, so the variant-lrp refusal is Add's alone."""
import pytest
import torch

import bf16_rule_inputs as I
from gpu_util import check, d as _d, dev, record, rms as _rms
from oracle import relprop_oracle as O

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


def _at(t, off):
    """`t` on the device as a contiguous slice that starts at element `off` of a larger buffer; what surrounds it is NaN."""
    if off == 0:
        return t.to(dev())
    n = t.numel()
    buf = torch.full((off + n + 8,), NAN, dtype=t.dtype, device=dev())
    view = buf[off:off + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.storage_offset() == off
    return view


def _same(name, got, ref):
    """Bit for bit (as values: torch.equal), recorded like every other comparison."""
    return check(name, got, ref, 0.0, exact=True)


def _ids(cases):
    def flat(c):
        return "x".join(flat(x) for x in c) if isinstance(c, tuple) else str(c)
    return ["-".join(flat(x) for x in (c if isinstance(c[0], tuple) else (c,))) for c in cases]


# ================================================================================================ Add
def _run_add(shape, layout, shared):
    from transformer_explainability_amd import ops
    tag = f"bf16rules.add{shape}.{layout}.{'shared' if shared else 'per_sample'}"
    R, X0, X1 = I.add_inputs(shape, shared)
    ra, rb = O.add_relprop(R.double(), X0.double(), X1.double())
    xo = {"x_off1": 1, "x_off3": 3}.get(layout, 0)
    Rd, X0d, X1d = _at(R, 1 if layout == "r_off1" else 0), _at(X0, xo), _at(X1, xo)
    n, B = X0[0].numel(), shape[0]
    assert Rd.data_ptr() % 16 == (4 if layout == "r_off1" else 0) and X0d.data_ptr() % 16 == 2 * xo
    # (a) fp64 oracle
    a, b = ops.add_relprop(Rd, X0d, X1d)
    check(tag + ".a", a, ra, I.ADD_TOL)
    check(tag + ".b", b, rb, I.ADD_TOL)
    # (b) the fp32 kernel on exact copies: .float() gives fresh 16-byte-aligned operands, so both calls take VEC 4 when
    # n % 4 == 0 and R is aligned, and VEC 1 otherwise (the misaligned R is the same tensor in both)
    X0f, X1f = X0d.float(), X1d.float()
    assert X0f.data_ptr() % 16 == 0 and X1f.data_ptr() % 16 == 0 and torch.equal(X0f.double(), X0d.double())
    fa, fb = ops.add_relprop(Rd, X0f, X1f)
    _same(tag + ".a_vs_f32", a, fa)
    _same(tag + ".b_vs_f32", b, fb)
    if layout == "r_off1":                  # VEC 1 at n % 4 == 0 is new for the fp32 kernel as well
        assert n % 4 == 0
        check(tag + ".f32.a", fa, ra, I.ADD_TOL)
        check(tag + ".f32.b", fb, rb, I.ADD_TOL)
    # deferred: one pass, the factor left to the consumer; materialised it is the two-pass result
    da, db = ops.add_relprop(Rd, X0d, X1d, deferred=True)
    assert isinstance(da, ops.Deferred) and isinstance(db, ops.Deferred)
    _same(tag + ".deferred.a_vs_two_pass", da.materialise(), a)
    _same(tag + ".deferred.b_vs_two_pass", db.materialise(), b)
    check(tag + ".deferred.a", da.materialise(), ra, I.ADD_TOL)
    check(tag + ".deferred.b", db.materialise(), rb, I.ADD_TOL)
    fda, fdb = ops.add_relprop(Rd, X0f, X1f, deferred=True)
    _same(tag + ".deferred.a_vs_f32", da.t, fda.t)
    _same(tag + ".deferred.b_vs_f32", db.t, fdb.t)
    _same(tag + ".deferred.fac_vs_f32", torch.stack([da.scale, db.scale]), torch.stack([fda.scale, fdb.scale]))
    # (c) a batch is its samples
    if B > 1:
        sa, sb, sda, sdb, sfac = [], [], [], [], []
        for i in range(B):
            x1 = X1d if shared else X1d[i:i + 1]
            ai, bi = ops.add_relprop(Rd[i:i + 1], X0d[i:i + 1], x1)
            dai, dbi = ops.add_relprop(Rd[i:i + 1], X0d[i:i + 1], x1, deferred=True)
            sa.append(ai), sb.append(bi), sda.append(dai.t), sdb.append(dbi.t)
            sfac.append(torch.stack([dai.scale, dbi.scale], 1))
        _same(tag + ".samples.a", torch.cat(sa), a)
        _same(tag + ".samples.b", torch.cat(sb), b)
        _same(tag + ".samples.deferred.a", torch.cat(sda), da.t)
        _same(tag + ".samples.deferred.b", torch.cat(sdb), db.t)
        _same(tag + ".samples.deferred.fac", torch.cat(sfac), torch.stack([da.scale, db.scale], 1))


@pytest.mark.parametrize("shared", [False, True], ids=["x1_per_sample", "x1_shared"])
@pytest.mark.parametrize("shape,layout", I.ADD_CASES, ids=_ids(I.ADD_CASES))
def test_bf16_add(shape, layout, shared):
    _run_add(shape, layout, shared)


def test_bf16_add_model_shape():
    _run_add(I.ADD_MODEL_SHAPE, "fresh", False)


# ================================================================================================ Clone
@pytest.mark.parametrize("num", [2, 3])
@pytest.mark.parametrize("shape,off", I.CLONE_CASES, ids=_ids(I.CLONE_CASES))
def test_bf16_clone(shape, off, num):
    from transformer_explainability_amd import ops
    tag = f"bf16rules.clone{num}{shape}.off{off}"
    Rs, X = I.clone_inputs(shape, num)
    Xd, Rd = _at(X, off), [r.to(dev()) for r in Rs]
    Xf = Xd.float()
    B = shape[0]
    assert Xd.data_ptr() % 16 == (2 * off) % 16
    got = ops.clone_relprop(Rd, Xd)
    check(tag, got, O.clone_relprop([r.double() for r in Rs], X.double()), I.CLONE_TOL)
    _same(tag + ".vs_f32", got, ops.clone_relprop(Rd, Xf))
    if B > 1:
        alone = [ops.clone_relprop([r[i:i + 1] for r in Rd], Xd[i:i + 1]) for i in range(B)]
        _same(tag + ".samples", torch.cat(alone), got)
    # relevance operands that carry a per-sample factor, in every position
    fac = I.clone_factors(B).to(dev())
    for pos in I.clone_deferred_positions(num):
        ptag = f"{tag}.scaled{''.join(map(str, pos))}"
        col = {j: I.clone_factor_column(j, pos) for j in pos}
        ins = [ops.Deferred(r, fac[:, col[j]]) if j in pos else r for j, r in enumerate(Rd)]
        mat = [r.materialise() if isinstance(r, ops.Deferred) else r for r in ins]
        gs = ops.clone_relprop(ins, Xd)
        _same(ptag + ".vs_materialised", gs, ops.clone_relprop(mat, Xd))
        check(ptag, gs, O.clone_relprop([_d(m) for m in mat], X.double()), I.CLONE_TOL)
        _same(ptag + ".vs_f32", gs, ops.clone_relprop(ins, Xf))
        if B > 1:
            alone = []
            for i in range(B):
                one = [ops.Deferred(r[i:i + 1], fac[i:i + 1, col[j]]) if j in pos else r[i:i + 1]
                       for j, r in enumerate(Rd)]
                alone.append(ops.clone_relprop(one, Xd[i:i + 1]))
            _same(ptag + ".samples", torch.cat(alone), gs)


# ================================================================================================ IndexSelect
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", I.INDEX_SHAPES, ids=_ids(I.INDEX_SHAPES))
def test_index_select_every_position(shape, dtype):
    from transformer_explainability_amd import ops
    R, X = I.index_select_inputs(shape)
    B, N, _ = shape
    Xd, Rd = X.to(dev()).to(dtype), R.to(dev())
    name = "bf16" if dtype == BF else "f32"
    for index in (0, N // 2, N - 1):
        tag = f"bf16rules.index_select{shape}.{name}.at{index}"
        got = ops.index_select_relprop(Rd, Xd, index)
        ref = O.index_select_relprop(R.double(), X.double(), 1, index)
        check(tag, got, ref, I.INDEX_TOL)
        assert float(got[:, [r for r in range(N) if r != index]].abs().max()) == 0.0
        assert float(got[:, index].abs().max()) > 0.0
        if dtype == BF:
            _same(tag + ".vs_f32", got, ops.index_select_relprop(Rd, Xd.float(), index))
        alone = [ops.index_select_relprop(Rd[i:i + 1], Xd[i:i + 1], index) for i in range(B)]
        _same(tag + ".samples", torch.cat(alone), got)


# ================================================================================================ head mean
@pytest.mark.parametrize("B,H,N,off", I.HEADMEAN_CASES, ids=_ids(I.HEADMEAN_CASES))
def test_bf16_headmean(B, H, N, off):
    """headmean_flat_kernel<12> (H <= 12), <16> (H <= 16) and the grid-stride headmean_kernel<4> (H > 16) on bf16
    gradients, N*N % 4 in {0, 1}, N*N < 4, and gradients at an odd element offset."""
    from transformer_explainability_amd import ops
    tag = f"bf16rules.headmean({B},{H},{N}).off{off}"
    g, c = I.headmean_inputs(B, H, N)
    gd, cd = _at(g, off), c.to(dev())
    got = ops.gradcam_headmean(gd, cd)
    check(tag, got, O.gradcam_headmean(g.double(), c.double()), I.HEADMEAN_TOL)
    _same(tag + ".vs_f32", got, ops.gradcam_headmean(gd.float(), cd))
    if B > 1:
        alone = [ops.gradcam_headmean(gd[i:i + 1], cd[i:i + 1]) for i in range(B)]
        _same(tag + ".samples", torch.cat(alone), got)


def test_headmean_grid_stride_second_trip():
    """B = 2048 leaves one block per sample, N*N = 1089 > 1024 elements: every block takes a second trip, whose last
    element goes through the scalar tail.  Once per dtype, against the fp32 oracle."""
    from transformer_explainability_amd import ops
    B, H, N = I.HEADMEAN_SECOND_TRIP
    assert -(-N * N // 1024) > -(-2048 // B) and H > 16
    g, c = I.headmean_inputs(B, H, N)
    ref = O.gradcam_headmean(g.float(), c)
    gd, cd = g.to(dev()), c.to(dev())
    got = ops.gradcam_headmean(gd, cd)
    got32 = ops.gradcam_headmean(gd.float(), cd)
    tag = f"bf16rules.headmean({B},{H},{N})"
    check(tag + ".bf16", got, ref, I.HEADMEAN_TOL)
    check(tag + ".f32", got32, ref, I.HEADMEAN_TOL)
    _same(tag + ".vs_f32", got, got32)


# ================================================================================================ refusals
def test_bf16_streaming_rules_refuse_what_they_do_not_implement():
    from transformer_explainability_amd import ops
    from transformer_explainability_amd._lib import TeError
    R, X0, X1 = (t.to(dev()) for t in I.add_inputs((2, 5, 4), False))
    Xi = X0.reshape(2, 5, 4)
    Ri = R[:, :1]
    # mixed bf16 / fp32 operands; bf16 relevance
    for call in (lambda: ops.add_relprop(R, X0, X1.float()), lambda: ops.add_relprop(R, X0.float(), X1),
                 lambda: ops.add_relprop(R.to(BF), X0, X1),
                 lambda: ops.clone_relprop([R, R.to(BF)], X0), lambda: ops.clone_relprop([R.to(BF), R], X0.float()),
                 lambda: ops.index_select_relprop(Ri.to(BF), Xi, 0),
                 lambda: ops.index_select_relprop(Ri.to(BF), Xi.float(), 0)):
        with pytest.raises(TeError):
            call()
    # variant lrp (Add is the one streaming rule with variants)
    for deferred in (False, True):
        with pytest.raises(TeError, match="variant"):
            ops.add_relprop(R, X0, X1, variant="lrp", deferred=deferred)
    # a CPU tensor: there is no host fallback
    for call in (lambda: ops.add_relprop(R, X0.cpu(), X1), lambda: ops.add_relprop(R, X0, X1.cpu()),
                 lambda: ops.add_relprop(R.cpu(), X0, X1),
                 lambda: ops.clone_relprop([R, R], X0.cpu()), lambda: ops.clone_relprop([R, R.cpu()], X0),
                 lambda: ops.index_select_relprop(Ri, Xi.cpu(), 0), lambda: ops.index_select_relprop(Ri.cpu(), Xi, 0)):
        with pytest.raises(TeError, match="CPU"):
            call()


# ================================================================================================ Linear
def _linear_bar(tag, got, f32, ref):
    """The bar of test_bf16_linear_rule_vs_fp64: as close to the fp64 oracle as the fp32 kernel on exact copies."""
    e_bf, e_32 = _rms(got, ref), _rms(f32, ref)
    record(tag, rms_bf16=e_bf, rms_f32=e_32, ref_rms=float(ref.pow(2).mean().sqrt()))
    assert torch.isfinite(got).all() and e_bf <= 1.1 * e_32 + 1e-12, (tag, e_bf, e_32)


def _linear_operands(lead, in_f, out_f, seed):
    X = I.signed_bf16(lead + (in_f,), seed)
    W = I.signed_bf16((out_f, in_f), seed + 1, zero_frac=0.02, scale=0.02)
    return X, W, I.relevance(lead + (out_f,), seed + 2)


def test_bf16_linear_unaligned_row_starts():
    """Two row tiles, the second ragged (T = 130); X as the first in_f columns of a [T, in_f + 3] buffer (row starts
    alternate between 16-byte aligned and not), the same at a base offset of one element, and contiguous at a base offset
    of one element (no row aligned): fetch() reads what it cannot load as 16 bytes element by element."""
    from transformer_explainability_amd import ops
    T, in_f, out_f = 130, 128, 256
    assert ops.linear_bf16_route(T, in_f, out_f) == "bf16"
    X, W, R = _linear_operands((T,), in_f, out_f, 500)
    X[T // 2] = 0.0
    Xd, Wd, Rd = X.to(dev()), W.to(dev()), R.to(dev())
    cache = {}
    got = ops.linear_relprop(Rd, Xd, Wd, cache=cache)
    pitch = in_f + 3
    wide = torch.full((T, pitch), NAN, dtype=BF, device=dev())
    wide[:, :in_f] = Xd
    flat = torch.full((1 + T * pitch + 8,), NAN, dtype=BF, device=dev())
    shifted = flat[1:1 + T * pitch].view(T, pitch)[:, :in_f]
    shifted.copy_(Xd)
    views = {"pitch": wide[:, :in_f], "pitch_off1": shifted, "contig_off1": _at(X, 1)}
    assert views["pitch"].stride() == (pitch, 1) and views["pitch_off1"].data_ptr() % 16 == 2
    for name, Xv in views.items():
        assert torch.equal(Xv, Xd) and (Xv.data_ptr() % 16 != 0 or (Xv.stride(0) * 2) % 16 != 0)
        _same(f"bf16rules.linear({T},{in_f},{out_f}).{name}", ops.linear_relprop(Rd, Xv, Wd, cache=cache), got)
    assert float(got[T // 2].abs().max()) == 0.0
    _linear_bar(f"bf16rules.linear({T},{in_f},{out_f})", got, ops.linear_relprop(Rd, Xd.float(), Wd.float()),
                O.linear_relprop(R.double(), X.double(), W.double()))


@pytest.mark.parametrize("B,N,in_f,out_f,route", [(3, 50, 128, 256, "bf16"), (3, 50, 64, 192, "fp32-upcast")])
def test_bf16_linear_deferred_factor_per_sample(B, N, in_f, out_f, route):
    """Distinct factors, sample boundaries (rows 50 and 100) inside one 128-row tile: a kernel that took another sample's
    factor, or none, gives other bits than the rule on the materialised relevance."""
    from transformer_explainability_amd import ops
    assert ops.linear_bf16_route(B * N, in_f, out_f) == route
    X, W, R = _linear_operands((B, N), in_f, out_f, 510)
    Xd, Wd, Rd = X.to(dev()), W.to(dev()), R.to(dev())
    fac = torch.tensor([[0.5, 7.0], [1.5, 7.0], [0.25, 7.0]], device=dev())
    Rdef = ops.Deferred(Rd, fac[:, 0])
    Rmat = Rdef.materialise()
    got = ops.linear_relprop(Rdef, Xd, Wd)
    tag = f"bf16rules.linear_deferred({B},{N},{in_f},{out_f})"
    _same(tag + ".vs_materialised", got, ops.linear_relprop(Rmat, Xd, Wd))
    for i in range(B):
        one = ops.linear_relprop(ops.Deferred(Rd[i:i + 1], fac[i:i + 1, 0]), Xd[i:i + 1], Wd)
        _same(f"{tag}.sample{i}", one, got[i:i + 1])
    _linear_bar(tag, got, ops.linear_relprop(Rmat, Xd.float(), Wd.float()),
                O.linear_relprop(_d(Rmat), X.double(), W.double()))


def test_bf16_linear_tracks_in_place_weight_edit():
    """ops.bf16_weight_planes keys the cached planes on W._version: after W.mul_(1.5) the rule reads the new weight.  (The
    rule is invariant under a scaling of W up to rounding; what tells stale planes from new ones is that 1.5 W is rounded to
    bf16 again, a relative 2^-9 change of about half the weights: three orders of magnitude above the bar.)"""
    from transformer_explainability_amd import ops
    T, in_f, out_f = 130, 128, 256
    X, W, R = _linear_operands((T,), in_f, out_f, 520)
    Xd, Wd, Rd = X.to(dev()), W.to(dev()), R.to(dev())
    cache = {}
    old = ops.linear_relprop(Rd, Xd, Wd, cache=cache).clone()
    planes = cache["bf16_planes"][1]
    assert ops.linear_relprop(Rd, Xd, Wd, cache=cache) is not None and cache["bf16_planes"][1] is planes   # a hit
    Wd.mul_(1.5)
    new = ops.linear_relprop(Rd, Xd, Wd, cache=cache)
    assert cache["bf16_planes"][1] is not planes
    assert not torch.equal(new, old)
    W15 = Wd.cpu()                            # 1.5 W as the bf16 tensor holds it
    assert torch.equal(W15, (W.float() * 1.5).to(BF))
    tag = f"bf16rules.linear_weight_edit({T},{in_f},{out_f})"
    _same(tag + ".vs_uncached", new, ops.linear_relprop(Rd, Xd, Wd))
    _linear_bar(tag, new, ops.linear_relprop(Rd, Xd.float(), Wd.float()),
                O.linear_relprop(R.double(), X.double(), W15.double()))


# ================================================================================================ attention rules
def _norm_rms(got, ref, den):
    """As in test_gpu_bf16.py: rms of the error relative to the componentwise condition bound of each output."""
    d = _d(den)
    m = d > 0
    return float((((_d(got) - _d(ref)) / d.clamp_min(1e-300))[m] ** 2).mean().sqrt())


def _attention_case(B, H, N, with_z, views):
    from transformer_explainability_amd import ops
    D = 64
    C = H * D
    assert ops.attention_bf16_route(N, D) == "bf16"
    g = torch.Generator().manual_seed(1000 + N)
    qkv = torch.randn(B, N, 3 * C, generator=g).to(BF)
    attn = torch.softmax(torch.randn(B, H, N, N, generator=g) * 2, -1).to(BF)
    R_av = I.relevance((B, H, N, D), 1001).to(dev())
    R_qk = I.relevance((B, H, N, N), 1002).to(dev())
    fac = torch.tensor([[1.5, 0.0], [0.25, 0.0]], device=dev())[:B]

    def heads(t):
        return t.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    qf, kf, vf = (t.contiguous() for t in heads(qkv.to(dev())))          # fresh, aligned, contiguous
    attn_f = attn.to(dev())
    z_av = torch.matmul(attn_f, vf) if with_z else None
    z_qk = torch.matmul(qf, kf.transpose(-1, -2)) if with_z else None
    up = lambda t: None if t is None else t.float()                       # noqa: E731
    rules = (("av", ops.matmul_relprop_av, R_av, attn_f, vf, z_av),
             ("qk", ops.matmul_relprop_qk, R_qk, qf, kf, z_qk),
             ("qk_scaled", ops.matmul_relprop_qk, ops.Deferred(R_qk, fac[:, 0]), qf, kf, z_qk))
    fresh = {}
    for name, fn, Rr, a, b, zz in rules:
        got = fn(Rr, a, b, out_scale=0.5, z=zz)
        fresh[name] = got
        f32 = fn(Rr, up(a), up(b), out_scale=0.5, z=up(zz))
        R64 = _d(Rr.materialise() if isinstance(Rr, ops.Deferred) else Rr)
        a64, b64 = _d(a), _d(b)
        o = O.einsum_av_relprop if name == "av" else O.einsum_qk_relprop
        z64 = _d(zz) if zz is not None else (a64 @ b64 if name == "av" else a64 @ b64.transpose(-1, -2))
        ref = o(R64, a64, b64, z64)
        den = o(R64.abs(), a64.abs(), b64.abs(), z64.abs())
        for j in range(2):
            e_bf, e_32 = _norm_rms(got[j], ref[j] * 0.5, den[j] * 0.5), _norm_rms(f32[j], ref[j] * 0.5, den[j] * 0.5)
            record(f"bf16rules.attn.{name}.B{B}H{H}N{N}.z{int(with_z)}.{j}", rms_bf16=e_bf, rms_f32=e_32)
            assert torch.isfinite(got[j]).all()
            bound = 1.1 if with_z else 4.0                                # the bars of test_bf16_attention_rules_vs_fp64
            assert e_bf <= bound * e_32 + 1e-12, (name, j, e_bf, e_32)
    if not views:
        return
    # the same values as views: q / k / v inside a fused activation that starts at element 3 of its buffer, attn and the
    # cached products at element 1, the results into the strided slots of a fused fp32 buffer
    qv, kv, vv = heads(_at(qkv, 3))
    attn_v = _at(attn, 1)
    zv_av = None if z_av is None else _at(z_av.cpu(), 1)
    zv_qk = None if z_qk is None else _at(z_qk.cpu(), 1)
    assert qv.data_ptr() % 16 == 6 and attn_v.data_ptr() % 16 == 2 and torch.equal(vv, vf)
    fused = torch.full((B, N, 3 * C), NAN, dtype=torch.float32, device=dev())
    slot_q, slot_k, slot_v = heads(fused)
    tag = f"bf16rules.attn_views.N{N}.z{int(with_z)}"
    ca, cv = ops.matmul_relprop_av(R_av, attn_v, vv, out_scale=0.5, z=zv_av, cam_v_out=slot_v)
    assert cv.data_ptr() == slot_v.data_ptr()
    _same(tag + ".av.cam_attn", ca, fresh["av"][0])
    _same(tag + ".av.cam_v", slot_v, fresh["av"][1])
    cq, ck = ops.matmul_relprop_qk(ops.Deferred(R_qk, fac[:, 0]), qv, kv, out_scale=0.5, z=zv_qk)
    _same(tag + ".qk_scaled.cam_q", cq, fresh["qk_scaled"][0])
    _same(tag + ".qk_scaled.cam_k", ck, fresh["qk_scaled"][1])
    ops.matmul_relprop_qk(R_qk, qv, kv, out_scale=0.5, z=zv_qk, cam_q_out=slot_q, cam_k_out=slot_k)
    _same(tag + ".qk.cam_q", slot_q, fresh["qk"][0])
    _same(tag + ".qk.cam_k", slot_k, fresh["qk"][1])
    assert torch.isfinite(fused).all()                                    # every slot element was written


@pytest.mark.parametrize("with_z", [True, False], ids=["cached_z", "recomputed_z"])
def test_bf16_attention_rules_on_unaligned_views(with_z):
    """N = 70: two 64-row tiles with the second ragged, K = N not a multiple of 32."""
    _attention_case(2, 2, 70, with_z, views=True)


@pytest.mark.parametrize("with_z", [True, False], ids=["cached_z", "recomputed_z"])
@pytest.mark.parametrize("N", [1, 1024])
def test_bf16_attention_rules_smallest_and_largest_n(N, with_z):
    """Both ends of te_matmul_relprop_bf16_supported."""
    _attention_case(1, 1, N, with_z, views=False)
