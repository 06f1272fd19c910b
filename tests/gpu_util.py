"""Helpers shared by the `-m gpu` parity tests (HIP path through the C ABI vs the CPU oracle).

Belongs here: what several -m gpu files use alike and what needs the device or the oracle -- the device, seeded inputs, the
comparisons that write the parity report (check*, map_stats), moving and upcasting caches (move_relprop_state, cache64), fp64
copies and their rms distance (d, rms), misaligned device views (odd_offset_view) and the seeded bf16 models that several
files build with the same weights (the vit_b16_bf16 and bert_base_bf16 fixtures, module-scoped: one model per test file).

Does not belong here: tolerances, shapes and expected values (they stay in the test files), helpers that need no device
(host_util.py: lib, status, header_args, free_port, bits, same_bits, one_hot) and fixtures that build other weights under a
shared name (the tiny_vit of test_sanity_host, test_host_logic and test_gpu_f64 are three different models).
"""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "gpurun_out", "parity_report.jsonl")


def dev():
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def d(t):
    return t.detach().double().cpu()


def rms(a, b):
    return float(((d(a) - d(b)) ** 2).mean().sqrt())


def cache64(cache, keys=None):
    """The cache (or its entries `keys`) with every tensor upcast to fp64, exactly"""
    def conv(v):
        if torch.is_tensor(v):
            return v.double()
        if isinstance(v, list):
            return [conv(x) for x in v]
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        return v
    return conv(cache if keys is None else {k: cache[k] for k in keys})


def odd_offset_view(t, dtype=None):
    """t's values (or an uninitialised tensor of t's shape in ``dtype``) in a dense device view that starts one element past a
    16-byte boundary"""
    dtype = t.dtype if dtype is None else dtype
    store = torch.empty(t.numel() + 1, dtype=dtype, device=dev())
    view = store[1:].view(t.shape)
    if dtype == t.dtype:
        view.copy_(t)
    assert view.data_ptr() % 16 == view.element_size() and view.is_contiguous()
    return view


@pytest.fixture(scope="module")
def vit_b16_bf16():
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import vit
    model = vit.vit_base_patch16_224().eval()
    synthetic_init(model, 0)
    return model.to(dev()).to(torch.bfloat16)


@pytest.fixture(scope="module")
def bert_base_bf16():
    from oracle.ref_harness import synthetic_init
    from transformer_explainability_amd import bert
    model = bert.BertForSequenceClassification(bert.BertConfigLite(num_labels=2)).eval()
    synthetic_init(model, 0)
    return model.to(dev()).to(torch.bfloat16)


def stats(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    d = (got - ref).abs()
    return {"max_abs": float(d.max()), "ref_max": float(ref.abs().max()),
            "rel": float(d.max()) / max(float(ref.abs().max()), 1e-30),
            "nonfinite": int((~torch.isfinite(got)).sum())}


def record(name, **kw):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(json.dumps({"test": name, **kw}) + "\n")


def check(name, got, ref, rel_tol, exact=False):
    s = stats(got, ref)
    s["bitwise_equal"] = bool(torch.equal(got.detach().cpu(), ref.detach().cpu()))
    record(name, **s, rel_tol=rel_tol)
    assert s["nonfinite"] == 0, (name, s)
    if exact:
        assert s["bitwise_equal"], (name, s)
    assert s["rel"] <= rel_tol, (name, s)
    return s


def check_nan_aware(name, got, ref, rel_tol):
    """check() for outputs where the reference itself yields NaN (0/0 of an all-clamped map): the NaN positions must
    agree, the rest is compared as usual."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), name
    return check(name, torch.nan_to_num(got), torch.nan_to_num(ref), rel_tol)


def check_conditioned(name, got, ref32, ref64, base_tol, k=8.0, k_max=16.0, q=0.999):
    """Conditioning-aware comparison for rules that divide by a mixed-sign sum the kernel RECOMPUTES in its own
    summation order (safe_divide(R, Z), Z = sum of products of either sign; not the model path, which hands the cached
    forward Z to the rule): the fp32 oracle itself is only as accurate as its distance from the fp64 oracle there.

      * bulk:  the q-quantile (99.9 %) of |got - ref64| <= k x the q-quantile of |ref32 - ref64| + base_tol x max|ref64|
               with k = 8 (measured over the 112 computeZ cases on the MI355X: <= 6.1; the bulk statistic is what a
               wrong kernel cannot pass) -- "as accurate as a plain fp32 evaluation in another summation order";
      * tail:  max|got - ref64| <= k_max x max|ref32 - ref64| + base_tol x max|ref64|.  The maxima are single draws
               from a heavy tail (the element with the smallest |Z| of the tensor, error ~ eps |terms| / Z^2), whose
               ratio reached 11.9 over the 112 recorded cases of round 1 -- hence k_max = 16, not 3."""
    got = got.detach().cpu().double()
    ref32, ref64 = ref32.detach().cpu().double(), ref64.detach().cpu().double()
    e_got, e_ref = (got - ref64).abs().flatten(), (ref32 - ref64).abs().flatten()
    err, floor = float(e_got.max()), float(e_ref.max())
    kth = max(1, int(q * e_got.numel()))
    err_q, floor_q = float(e_got.kthvalue(kth).values), float(e_ref.kthvalue(kth).values)
    mx = float(ref64.abs().max())
    tol = k_max * floor + base_tol * mx
    tol_q = k * floor_q + base_tol * mx
    record(name, max_abs_vs_fp64=err, oracle32_vs_fp64=floor, q_abs_vs_fp64=err_q, q_oracle32_vs_fp64=floor_q,
           ref_max=mx, rel=err / max(mx, 1e-30), tol_abs=tol, tol_q=tol_q, nonfinite=int((~torch.isfinite(got)).sum()))
    assert torch.isfinite(got).all(), name
    assert err_q <= tol_q, (name, dict(err_q=err_q, floor_q=floor_q, ref_max=mx, tol_q=tol_q))
    assert err <= tol, (name, dict(err=err, floor=floor, ref_max=mx, tol=tol))


def group_stats(got, ref32, ref64, group_dims):
    """Per independent problem (the dims in `group_dims` are reduced inside one): err_g = max|got - ref64|,
    scale_g = max|ref64|, floor_g = max|ref32 - ref64|, and whether `got` has a non-zero element in the group."""
    got, ref32, ref64 = (t.detach().cpu().double() for t in (got, ref32, ref64))
    dims = tuple(d % ref64.dim() for d in ((group_dims,) if isinstance(group_dims, int) else group_dims))
    return ((got - ref64).abs().amax(dims), ref64.abs().amax(dims), (ref32 - ref64).abs().amax(dims),
            got.abs().amax(dims) != 0)


def check_groups(name, got, ref32, ref64, group_dims, base_tol):
    """Comparison that weighs every independent problem of a tensor by its OWN magnitude (check() and check_conditioned()
    scale every error by the maximum of the whole tensor, so they only ever judge the largest row / head / sample).
    For every group g (a row of a Linear output, a (b,h) slice of cam_v, a sample of an Add ...), against the fp64 oracle:
        err_g <= base_tol x scale_g           wherever scale_g > 0,
        got is exactly zero on the group      wherever ref64 is exactly zero on it,
    and got is finite.  No group is left out.  The worst err_g / scale_g, the fp32 oracle's worst floor_g / scale_g and
    the index of the worst group go to the parity report."""
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(ref32.shape), (name, got.shape, ref32.shape, ref64.shape)
    finite = bool(torch.isfinite(got).all())
    err, scale, floor, got_nz = group_stats(torch.nan_to_num(got.detach().cpu().double(), 0.0, 0.0, 0.0), ref32, ref64,
                                            group_dims)
    live = scale > 0
    ratio = torch.where(live, err / scale.clamp_min(1e-300), torch.zeros_like(err))
    fratio = torch.where(live, floor / scale.clamp_min(1e-300), torch.zeros_like(err))
    worst = int(ratio.argmax()) if ratio.numel() else 0
    widx = [int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape)] if ratio.dim() else []
    nonzero_on_zero = int((got_nz & ~live).sum())
    s = dict(groups=int(ratio.numel()), live_groups=int(live.sum()), worst_ratio=float(ratio.max()) if ratio.numel() else 0.0,
             oracle32_worst_ratio=float(fratio.max()) if ratio.numel() else 0.0, worst_group=widx,
             worst_group_scale=float(scale.flatten()[worst]) if ratio.numel() else 0.0,
             nonzero_on_zero_groups=nonzero_on_zero, base_tol=base_tol, finite=finite)
    record(name, **s)
    assert finite, (name, s)
    assert nonzero_on_zero == 0, (name, s)
    assert s["worst_ratio"] <= base_tol, (name, s)
    return s


def check_producer_groups(name, got, stock, ref64, group_dims, tol, xmax=None, scale_floor=None, sink=None):
    """check_groups for a PRODUCER (a kernel with a stock torch counterpart), the form of test_layernorm_per_row: for every
    group g, against the fp64 chain,
        err_g <= 2 x err_stock_g + (tol + 4 x 2^-24 x xmax_g) x scale_g ,     scale_g = max(max|ref64| of g, scale_floor_g)
    with err_stock_g the error of the stock chain in the operands' dtype and xmax_g the largest score magnitude that decides
    the group (None: no score enters the output).  xmax and scale_floor are shaped like the groups.  No group is left out; a
    group whose bound is zero must be exactly right.  The worst err / bound, its group and the stock chain's worst
    err / scale go to the parity report -- as a line of their own, or into the dict `sink` under `name` for a caller that
    writes one line per test."""
    assert tuple(got.shape) == tuple(stock.shape) == tuple(ref64.shape), (name, got.shape, stock.shape, ref64.shape)
    finite = bool(torch.isfinite(got).all())
    err, scale, err_stock, _ = group_stats(torch.nan_to_num(got.detach().cpu().double(), 0.0, 0.0, 0.0), stock, ref64, group_dims)
    if scale_floor is not None:
        scale = torch.maximum(scale, scale_floor.detach().cpu().double())
    rel = torch.full_like(scale, float(tol))
    if xmax is not None:
        rel = rel + 4.0 * 2.0 ** -24 * xmax.detach().cpu().double()
    bound = 2.0 * err_stock + rel * scale
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                             torch.zeros_like(err)))
    worst = int(ratio.argmax())
    widx = [int(i) for i in torch.unravel_index(torch.tensor(worst), ratio.shape)] if ratio.dim() else []
    live = scale > 0
    sratio = torch.where(live, err_stock / scale.clamp_min(1e-300), torch.zeros_like(err))
    s = dict(groups=int(ratio.numel()), worst_over_bound=float(ratio.max()), worst_group=widx,
             worst_group_err=float(err.flatten()[worst]), worst_group_scale=float(scale.flatten()[worst]),
             worst_group_stock_err=float(err_stock.flatten()[worst]), stock_worst_ratio=float(sratio.max()),
             worst_ratio=float(torch.where(live, err / scale.clamp_min(1e-300), torch.zeros_like(err)).max()), tol=float(tol),
             finite=finite)
    if sink is None:
        record(name, **s)
    else:
        sink[name] = s
    assert finite, (name, s)
    assert s["worst_over_bound"] <= 1.0, (name, s)
    return s


from oracle.model_cache import bert_cache_from_model, vit_cache_from_model  # noqa: E402,F401


def minmax(m):
    flat = m.reshape(m.shape[0], -1)
    lo, hi = flat.min(1, keepdim=True).values, flat.max(1, keepdim=True).values
    return (flat - lo) / (hi - lo)


def map_stats(got, ref):
    """The three parity statistics of SURVEY.md section 8d: raw, min-max-normalised, relative."""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    raw = float((got - ref).abs().max())
    return {"raw_max_abs": raw, "normalised_max_abs": float((minmax(got) - minmax(ref)).abs().max()),
            "rel_linf": raw / max(float(ref.abs().max()), 1e-30), "ref_max": float(ref.abs().max())}


def _move(v, device):
    if torch.is_tensor(v):
        return v.to(device)
    if isinstance(v, (list, tuple)) and v and all(torch.is_tensor(t) for t in v):
        return type(v)(t.to(device) for t in v)
    return v


def move_relprop_state(model, device):
    """Move every tensor the relprop path reads from module attributes (self.X / self.Y of the rule
    modules, cached attention probabilities / gradients / masks) to `device`, together with the
    parameters.  Lets a test produce the caches with the CPU forward + backward (bit-comparable to the
    reference's CPU producers) and then run the HIP relprop on exactly those tensors."""
    for m in model.modules():
        for name, val in list(vars(m).items()):
            if name.startswith("_"):
                continue
            new = _move(val, device)
            if new is not val:
                setattr(m, name, new)
    model.to(device)
    return model


from oracle.model_cache import sliced_relprop_state  # noqa: E402,F401  (shared with bench.py's parity block)
