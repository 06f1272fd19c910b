"""`-m gpu`: the fp32 attention relprop rules (ops.matmul_relprop_av / ops.matmul_relprop_qk) at every seam of their
dispatch -- the sequence lengths at which a kernel family changes, a key block or key group is partial, or the number
of key groups changes -- from N = 2 to beyond 4096, against the fp64 oracle.

Which code a length reaches (head dim 64; csrc/te_attn.hip holds the whole dispatch, one chain per entry point):
  N <= 224        QK rule on te_attn_rc.hip (`both` = 1 up to 208, the re-staged two-phase form for 209-224)
  225 .. 4096     QK rule on qk_rule_kernel<RULE>: ng = ceil(N / 256) key groups of jg = roundup64(ceil(N / ng)) keys;
                  the last group's nj & 3 selects the tail assembly, nj < 4 the guarded loads, ng > 1 the finishing kernel
  N <= 4096       AV rule on av6_kb_kernel<RULE>: wave-owned 32-key blocks, ceil(nkb / 8) workgroups
  N > 4096        both rules on the 64 x 64-tile kernels (av_row / qk_row / col); a deferred factor is refused there and
                  ops retries on the materialised operand
  head dim != 64  the simple kernels, by dispatch

Two input modes keep every comparison well conditioned (the ill-conditioned combination -- mixed sign AND the kernel's own
Z -- stays with test_gpu_rules.py::test_attention_rules_fused_qkv_layout):
  P  every operand positive, the kernel computes Z: each output is a sum of positive terms, compared ELEMENT BY ELEMENT
     with the fp64 oracle, |got - ref| <= gamma ref, gamma = (2 N + 128) 2^-24 -- the first-order forward bound of an fp32
     evaluation in any order: the two chained contractions total at most 2 N terms; 128 covers the division, the factors,
     the scale and the truncation of the split products.  Derived, not measured.
  M  mixed sign, Z handed over as the device forward product (the model path); 3e-5 of the tensor maximum, the project's
     bar for these rules."""
import pytest
import torch

from gpu_util import check, dev, record, rnd
from oracle import relprop_oracle as O

pytestmark = pytest.mark.gpu

RC = [(2, 2, 2), (1, 3, 15), (1, 2, 16), (2, 1, 17), (1, 2, 31), (1, 2, 32), (1, 2, 208), (2, 2, 209), (1, 3, 224)]
ONE_GROUP = [(2, 2, 225), (1, 3, 250), (1, 2, 255), (1, 2, 256)]
GROUPS = [(2, 2, 257), (1, 2, 258), (1, 3, 259), (1, 2, 513), (1, 2, 641), (2, 2, 769), (1, 2, 770), (1, 3, 771), (1, 2, 772),
          (1, 2, 785), (1, 2, 1025), (1, 2, 1026), (1, 2, 2049), (1, 2, 4095), (1, 1, 4096)]
ROUND1 = [(1, 1, 4100)]
SEAMS = [(B, H, N, 64) for B, H, N in RC + ONE_GROUP + GROUPS + ROUND1]
BY_DISPATCH = [(1, 2, 257, 80), (1, 2, 50, 128), (1, 1, 300, 16)]
WEIGHTED = [(1, 3, 250, 64), (1, 3, 771, 64), (1, 2, 2049, 64)]


@pytest.fixture(autouse=True)
def _dispatch_untouched():
    """ops.FORCE_SIMPLE stays as shipped: which kernel runs is decided by N and D alone."""
    from transformer_explainability_amd import ops
    assert ops.FORCE_SIMPLE is False
    yield
    assert ops.FORCE_SIMPLE is False


def key_groups(N):
    """te_attn_rules.hip: groups_for -> (ng, jg, keys of the last group)."""
    ng = (N + 255) // 256
    jg = ((N + ng - 1) // ng + 63) & ~63
    return ng, jg, N - (ng - 1) * jg


def fused_operands(B, H, N, D, positive, seed=131):
    """The fused qkv activation [B,N,3HD] with its q / k / v head views, softmax attention, and the AV rule's relevance
    as [B,H,N,D] view of a 'b n (h d)' tensor -- all on the host, fp32."""
    C = H * D
    qkv = rnd((B, N, 3 * C), seed)
    R = rnd((B, N, C), seed + 1, 0.01)
    if positive:
        qkv = qkv.abs() + 0.05
        R = R.abs() + 1e-4
    v5 = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = v5[0], v5[1], v5[2]
    attn = torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1).contiguous()
    return qkv, q, k, v, attn, R.view(B, N, H, D).permute(0, 2, 1, 3)


def weight_query_rows(R, N):
    """x 100 on the AV rule's query rows at the 32-row block edges and the last row."""
    R = R.clone()
    for i in sorted({0, 31, 32, N - 1}):
        if i < N:
            R[:, :, i] *= 100.0
    return R


def seam_key_columns(N):
    """The key columns either side of the first group boundary, and the last min(4, nj_last) keys."""
    ng, jg, nj_last = key_groups(N)
    cols = {j for j in (jg - 1, jg) if j < N}
    cols.update(range(N - min(4, nj_last), N))
    return sorted(cols)


def check_elementwise(name, got, ref64, N):
    """Mode P: |got - ref| <= gamma ref for EVERY element (ref > 0), gamma = (2 N + 128) 2^-24."""
    gamma = (2 * N + 128) * 2.0 ** -24
    got = got.detach().cpu().double()
    assert bool((ref64 > 0).all()), name
    nonfinite = int((~torch.isfinite(got)).sum())
    worst = float(((got - ref64).abs() / ref64).max())
    record(name, max_rel_elementwise=worst, bar=gamma, ref_min=float(ref64.min()), ref_max=float(ref64.max()),
           nonfinite=nonfinite)
    assert nonfinite == 0, name
    assert bool(((got - ref64).abs() <= gamma * ref64).all()), (name, dict(worst=worst, bar=gamma))


def run_rules(B, H, N, D, mode, weighted=False):
    """Both rules on the fused layout (q / k / v read in place, outputs written in place into a NaN-filled
    'b n (qkv h d)' buffer), then the comparison of `mode` on all four outputs."""
    from transformer_explainability_amd import ops
    positive = mode == "P"
    C = H * D
    qkv, q, k, v, attn, r_heads = fused_operands(B, H, N, D, positive)
    if weighted:
        r_heads = weight_query_rows(r_heads, N)
    d = dev()
    qkv_d = qkv.to(d)
    v5d = qkv_d.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    cam_qkv = torch.full((B, N, 3 * C), float("nan"), device=d)
    slots = cam_qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    attn_d = attn.to(d)
    # M: Z handed over as the forward pass produced it on the device, as the model path does; P: the Z kernels run
    z_av = None if positive else attn_d @ v5d[2]
    z_qk = None if positive else v5d[0] @ v5d[1].transpose(-1, -2)
    # (the relevance goes to the device as the contiguous 'b n (h d)' tensor and is read through its head view)
    r_d = r_heads.permute(0, 2, 1, 3).contiguous().to(d).permute(0, 2, 1, 3)
    cam1, _ = ops.matmul_relprop_av(r_d, attn_d, v5d[2], out_scale=0.5, cam_v_out=slots[2], z=z_av)
    # each rule is compared on identical inputs: the QK rule and its oracle get the relevance the device AV rule produced
    cam1_c = cam1.cpu()
    if weighted:
        r_qk_c = cam1_c.clone()
        r_qk_c[..., seam_key_columns(N)] *= 100.0
        r_qk = r_qk_c.to(d)
    else:
        r_qk_c, r_qk = cam1_c, cam1
    ops.matmul_relprop_qk(r_qk, v5d[0], v5d[1], out_scale=0.5, cam_q_out=slots[0], cam_k_out=slots[1], z=z_qk)
    assert not torch.isnan(cam_qkv).any()       # every slot of the fused buffer was written

    zc_av = None if z_av is None else z_av.cpu().double()
    zc_qk = None if z_qk is None else z_qk.cpu().double()
    a64, v64 = O.einsum_av_relprop(r_heads.double(), attn.double(), v.double(), zc_av)
    q64, k64 = O.einsum_qk_relprop(r_qk_c.double(), q.double(), k.double(), zc_qk)
    tag = f"({B},{H},{N},{D}){mode}{'w' if weighted else ''}"
    outs = (("av.cam_attn", cam1_c, a64), ("av.cam_v", slots[2], v64), ("qk.cam_q", slots[0], q64),
            ("qk.cam_k", slots[1], k64))
    for name, got, ref in outs:
        if positive:
            check_elementwise(f"seam.{name}{tag}", got, ref * 0.5, N)
        else:
            check(f"seam.{name}{tag}", got, (ref * 0.5).float(), 3e-5)


# ------------------------------------------------------------------------------------------ 1. parity at the seams
@pytest.mark.parametrize("mode", ["P", "M"])
@pytest.mark.parametrize("B,H,N,D", SEAMS)
def test_attention_rule_seams(B, H, N, D, mode):
    run_rules(B, H, N, D, mode)


@pytest.mark.parametrize("B,H,N,D", WEIGHTED)
def test_attention_rule_seams_weighted(B, H, N, D):
    """Mode M with the relevance x 100 on the seams (query rows 0, 31, 32, N - 1 of the AV rule; the key columns at the
    first group boundary and the last min(4, nj_last) keys of the QK rule): the tensor maximum that 3e-5 is relative to
    is then set by the elements a wrong tail would touch."""
    run_rules(B, H, N, D, "M", weighted=True)


# ------------------------------------------------------------------------------------------ 2. properties
@pytest.mark.parametrize("B,H,N,D", BY_DISPATCH)
@pytest.mark.parametrize("mode", ["P", "M"])
def test_attention_rules_other_head_dims(B, H, N, D, mode):
    """Head dims other than 64 reach the simple kernels by dispatch (FORCE_SIMPLE untouched); same bars."""
    run_rules(B, H, N, D, mode)


def _device_case(B, H, N, seed):
    d = dev()
    D, C = 64, H * 64
    qkv = rnd((B, N, 3 * C), seed).to(d)
    v5 = qkv.view(B, N, 3, H, D).permute(2, 0, 3, 1, 4)
    attn = torch.softmax(v5[0] @ v5[1].transpose(-1, -2) * D ** -0.5, -1).contiguous()
    R = rnd((B, H, N, D), seed + 1, 0.01).to(d)
    return v5, attn, R


@pytest.mark.parametrize("B,H,N", [(2, 3, 250), (2, 2, 771), (2, 1, 2049)])
def test_attention_rule_seams_batch_independent(B, H, N):
    """(b,h) problems are independent at partial groups too: a batch run equals per-sample runs, bitwise."""
    from transformer_explainability_amd import ops
    v5, attn, R = _device_case(B, H, N, 141)
    cam1, cam_v = ops.matmul_relprop_av(R, attn, v5[2], out_scale=0.5)
    cam_q, cam_k = ops.matmul_relprop_qk(cam1, v5[0], v5[1], out_scale=0.5)
    for i in range(B):
        c1, cv = ops.matmul_relprop_av(R[i:i + 1], attn[i:i + 1], v5[2][i:i + 1], out_scale=0.5)
        cq, ck = ops.matmul_relprop_qk(c1, v5[0][i:i + 1], v5[1][i:i + 1], out_scale=0.5)
        assert torch.equal(c1, cam1[i:i + 1]) and torch.equal(cv, cam_v[i:i + 1])
        assert torch.equal(cq, cam_q[i:i + 1]) and torch.equal(ck, cam_k[i:i + 1])


@pytest.mark.parametrize("B,H,N", [(2, 2, 257), (1, 2, 771)])
def test_av_rule_reads_z_in_place(B, H, N):
    """Z of the AV rule as the [B,H,N,64] view of the 'b n (h d)' activation (row stride H * 64) == a contiguous copy of
    the same Z, bitwise."""
    from transformer_explainability_amd import ops
    v5, attn, R = _device_case(B, H, N, 151)
    z_bnc = (attn @ v5[2]).permute(0, 2, 1, 3).reshape(B, N, H * 64)
    z_view = z_bnc.view(B, N, H, 64).permute(0, 2, 1, 3)
    assert not z_view.is_contiguous() and z_view.stride(2) == H * 64
    a0, v0 = ops.matmul_relprop_av(R, attn, v5[2], out_scale=0.5, z=z_view)
    a1, v1 = ops.matmul_relprop_av(R, attn, v5[2], out_scale=0.5, z=z_view.contiguous())
    assert torch.isfinite(a0).all() and torch.isfinite(v0).all()
    assert torch.equal(a0, a1) and torch.equal(v0, v1)


def test_av_rule_strided_z_on_kernels_that_read_it_contiguous():
    """Head dim 32 (the simple kernels, which read Z as a contiguous [B,H,N,D] tensor): the entry point refuses the strided view
    and ops calls it again with a contiguous copy and the contiguous strides == the call on that copy, bitwise."""
    from transformer_explainability_amd import ops
    d = dev()
    B, H, N, D = 2, 2, 17, 32
    v = rnd((B, H, N, D), 171).to(d)
    attn = torch.softmax(rnd((B, H, N, N), 172).to(d), -1).contiguous()
    R = rnd((B, H, N, D), 173, 0.01).to(d)
    z_view = (attn @ v).permute(0, 2, 1, 3).reshape(B, N, H * D).view(B, N, H, D).permute(0, 2, 1, 3)
    assert not z_view.is_contiguous() and z_view.stride(2) == H * D
    a0, v0 = ops.matmul_relprop_av(R, attn, v, out_scale=0.5, z=z_view)
    a1, v1 = ops.matmul_relprop_av(R, attn, v, out_scale=0.5, z=z_view.contiguous())
    assert torch.isfinite(a0).all() and torch.isfinite(v0).all()
    assert torch.equal(a0, a1) and torch.equal(v0, v1)


@pytest.mark.parametrize("B,H,N", [(2, 2, 17), (2, 2, 65)])
def test_qk_rule_deferred_factor_without_z(B, H, N):
    """The deferred factor with no cached forward product (Z formed in the workspace first) == the QK rule on the materialised
    operand, bitwise."""
    from transformer_explainability_amd import ops
    d = dev()
    R = rnd((B, H, N, N), 181, 0.01).to(d)
    fac = (rnd((B, 2), 182).abs() + 0.5).to(d)
    q, k = rnd((B, H, N, 64), 183).to(d), rnd((B, H, N, 64), 184).to(d)
    Rd = ops.Deferred(R, fac[:, 1])
    cq, ck = ops.matmul_relprop_qk(Rd, q, k, out_scale=0.5)
    rq, rk = ops.matmul_relprop_qk(Rd.materialise(), q, k, out_scale=0.5)
    assert torch.isfinite(cq).all() and torch.isfinite(ck).all()
    assert torch.equal(cq, rq) and torch.equal(ck, rk)


@pytest.mark.parametrize("B,H,N", [(3, 2, 257), (2, 2, 771), (2, 1, 209), (2, 1, 4100)])
def test_qk_rule_deferred_factor(B, H, N):
    """The QK rule taking the deferred per-sample factor == the QK rule on the materialised operand, bitwise.  Beyond
    N = 4096 the kernel refuses the factor and ops retries on the materialised operand: the same bits as the plain call."""
    from transformer_explainability_amd import ops
    d = dev()
    R = rnd((B, H, N, N), 161, 0.01).to(d)
    fac = (rnd((B, 2), 162).abs() + 0.5).to(d)
    q, k = rnd((B, H, N, 64), 163).to(d), rnd((B, H, N, 64), 164).to(d)
    z = q @ k.transpose(-1, -2)
    Rd = ops.Deferred(R, fac[:, 1])
    cq, ck = ops.matmul_relprop_qk(Rd, q, k, out_scale=0.5, z=z)
    rq, rk = ops.matmul_relprop_qk(Rd.materialise(), q, k, out_scale=0.5, z=z)
    assert torch.isfinite(cq).all() and torch.isfinite(ck).all()
    assert torch.equal(cq, rq) and torch.equal(ck, rk)
