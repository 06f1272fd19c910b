"""`-m gpu`: ragged activation tiles of the x6 kernels.  A wave of a tile whose whole 64-row column lies at or beyond T stages its
weight-side block and keeps the barriers, and does nothing else (csrc/te_linear_x6.hip: `dead`).  Every output row is one k-ordered
chain that does not depend on the other rows of the call, so the check is exact:

  * operands with random rows everywhere for T' = the next multiple of 256 above T; the call on the first T rows (copied out, so
    that nothing behind them is there to be read) gives, bit for bit, rows [0, T) of the call on all T' rows;
  * the output buffer of the T-row call is followed by a tile's worth of sentinel rows, which stay untouched;
  * the x6 status word stays zero.

T: every wave-column (64) and row-block (32) boundary of a 256-row tile, one row on either side, and ragged second columns.
Calls, on buffers this file owns (the C ABI entry points ops.linear_relprop / ops.gemm_x6 bind, which allocate their outputs
themselves and so cannot carry a guard): the default rule on the planes of |X| (ops.X6_SIGNED_PLANES off) and on the signed planes,
with and without the per-row factor on R; the plain product in both directions; the general rule (variant lrp, alpha != 1).  Each on
the three tile geometries and under every schedule, the 16-workgroup grid included, which cuts a ragged tile between two
workgroups.  test_ops_calls_on_ragged_rows runs the same comparison through ops itself."""
import pytest
import torch

from gpu_util import dev, rnd

pytestmark = pytest.mark.gpu

TS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 257, 320]
FEATURES = [(256, 256), (256, 768)]
GUARD_ROWS = 256
SENTINEL = -7.25


def _up256(T):
    return T // 256 * 256 + 256          # the next multiple of 256 ABOVE T


class Dense:
    """Operands of one Linear layer on T' rows, the weight planes, and the results of every call on all T' rows (default flags)."""

    def __init__(self, Tp, in_f, out_f, seed):
        from transformer_explainability_amd import _lib, ops
        self.ops, self._lib, self.lib = ops, _lib, _lib.load()
        _lib.require_device()
        self.Tp, self.in_f, self.out_f = Tp, in_f, out_f
        X, W, b = rnd((Tp, in_f), seed), rnd((out_f, in_f), seed + 1, 0.05), rnd((out_f,), seed + 2, 0.3)
        R = rnd((Tp, out_f), seed + 3, 0.01)
        X[1] = 0.0
        self.X, self.W, self.b, self.R = (t.to(dev()) for t in (X, W, b, R))
        self.Y = torch.nn.functional.linear(self.X, self.W, self.b)
        self.rs = (0.5 + 0.01 * torch.arange(Tp, dtype=torch.float32)).to(dev())       # one factor per row
        self.wp, self.wpl = ops.x6_weight_planes(self.W), ops.x6_weight_planes_lrp(self.W)
        self.wg, self.wgT = ops.x6_matrix_planes(self.W, False), ops.x6_matrix_planes(self.W, True)
        self.status = ops.x6_status(dev())
        self.ws = {}
        self.want = {name: self.run(name, Tp, 0, self.rows(Tp))[0] for name in CALLS}
        for name, t in self.want.items():
            assert torch.isfinite(t).all(), name
        assert int(self.status[0]) == 0

    def rows(self, T):
        """The first T rows of every activation-side operand as tensors of their own, and the plane sets of X[:T]."""
        X, R, Y, rs = (t[:T].clone() for t in (self.X, self.R, self.Y, self.rs))
        nb = self.lib.te_linear_x6_planes_bytes(T, self.in_f)
        xs, xa = (torch.empty(nb, dtype=torch.uint8, device=dev()) for _ in range(2))
        st = torch.cuda.current_stream().cuda_stream
        self._lib.check(self.lib.te_linear_x6_split_matrix_f32(X.data_ptr(), T, self.in_f, 0, xs.data_ptr(), nb, st), "split")
        self._lib.check(self.lib.te_linear_x6_split_abs_f32(X.data_ptr(), T, self.in_f, xa.data_ptr(), nb, st), "split_abs")
        return dict(X=X, R=R, Y=Y, rs=rs, xs=xs, xa=xa)

    def workspace(self, kind, nbytes):
        if kind not in self.ws or self.ws[kind].numel() < nbytes:
            self.ws[kind] = torch.empty(nbytes, dtype=torch.uint8, device=dev())
        return self.ws[kind]

    def run(self, name, T, flags, o):
        """-> (rows [0, T) of the output, the guard rows behind them)"""
        lib, p = self.lib, lambda t: None if t is None else t.data_ptr()      # noqa: E731
        in_f, out_f = self.in_f, self.out_f
        st = torch.cuda.current_stream().cuda_stream
        kind, arg = CALLS[name]
        width = out_f if name == "product forward" else in_f
        buf = torch.full((T + GUARD_ROWS, width), SENTINEL, dtype=torch.float32, device=dev())
        sp = p(self.status)
        if kind == "rule":
            planes, signed, scaled = arg
            ws = self.workspace(kind, lib.te_linear_relprop_x6_workspace_bytes(self.Tp, in_f, out_f))
            fl = flags | (self.ops.TE_X6_X_PLANES_SIGNED if signed else 0)
            rc = lib.te_linear_relprop_x6_f32(p(o["R"]), p(o["rs"]) if scaled else None, 1, 1, p(o["X"]), p(self.W), p(self.wp),
                                              p(o[planes]), p(o["Y"]), p(self.b), p(buf), T, in_f, out_f, fl, sp, p(ws), ws.numel(), st)
        elif kind == "product":
            if arg == "forward":
                ws = self.workspace("gf", lib.te_gemm_x6_workspace_bytes(self.Tp, in_f, out_f))
                rc = lib.te_gemm_x6_f32(p(o["X"]), None, p(self.wg), p(self.b), p(buf), T, in_f, out_f, flags, sp, p(ws), ws.numel(), st)
            else:                                                                   # d_x = d_y W, with R as d_y
                ws = self.workspace("gb", lib.te_gemm_x6_workspace_bytes(self.Tp, out_f, in_f))
                rc = lib.te_gemm_x6_f32(p(o["R"]), None, p(self.wgT), None, p(buf), T, out_f, in_f, flags, sp, p(ws), ws.numel(), st)
        else:
            variant, alpha = arg
            ours = variant == self._lib.TE_VARIANT_OURS
            ws = self.workspace((kind, variant), lib.te_linear_relprop_x6_general_workspace_bytes(self.Tp, in_f, out_f, variant))
            rc = lib.te_linear_relprop_x6_general_f32(p(o["R"]), None, 0, 1, p(o["X"]), p(self.W), p(self.wp) if ours else None,
                                                      None if ours else p(self.wpl), None, p(o["Y"]) if ours else None,
                                                      p(self.b) if ours else None, p(buf), T, in_f, out_f, alpha, variant, flags, sp,
                                                      p(ws), ws.numel(), st)
        assert rc == 0, (name, T, hex(flags), rc)
        return buf[:T], buf[T:]


def _calls():
    from transformer_explainability_amd import _lib
    return {
        "rule on |X| planes": ("rule", ("xa", False, False)),
        "rule on |X| planes, r_scale": ("rule", ("xa", False, True)),
        "rule on signed planes": ("rule", ("xs", True, False)),
        "rule on signed planes, r_scale": ("rule", ("xs", True, True)),
        "product forward": ("product", "forward"),
        "product backward": ("product", "backward"),
        "general lrp": ("general", (_lib.TE_VARIANT_LRP, 1.0)),
        "general lrp alpha 2": ("general", (_lib.TE_VARIANT_LRP, 2.0)),
        "general ours alpha 2": ("general", (_lib.TE_VARIANT_OURS, 2.0)),
    }


CALLS = {}
_dense = {}


def dense(Tp, in_f, out_f):
    """One reference per shape, shared by the cases and never written again."""
    if not CALLS:
        CALLS.update(_calls())
    key = (Tp, in_f, out_f)
    if key not in _dense:
        _dense[key] = Dense(Tp, in_f, out_f, 900 + len(_dense) * 10)
    return _dense[key]


def _schedules(ops):
    return {"default": 0, "whole tiles": ops.TE_X6_WHOLE_TILES, "static tiles": ops.TE_X6_STATIC_TILES,
            "static whole tiles": ops.TE_X6_WHOLE_TILES | ops.TE_X6_STATIC_TILES, "small grid": ops.TE_X6_TEST_SMALL_GRID,
            "small grid, whole tiles": ops.TE_X6_TEST_SMALL_GRID | ops.TE_X6_WHOLE_TILES}


@pytest.mark.parametrize("in_f,out_f", FEATURES)
@pytest.mark.parametrize("T", TS)
def test_ragged_rows_equal_dense_rows(T, in_f, out_f):
    D = dense(_up256(T), in_f, out_f)
    ops = D.ops
    o = D.rows(T)
    for name in CALLS:
        want = D.want[name][:T]
        for pin in (ops._lib.TE_X6_TILE_256, ops._lib.TE_X6_TILE_128, ops._lib.TE_X6_TILE_128x128):
            for sched, sf in _schedules(ops).items():
                got, guard = D.run(name, T, pin | sf, o)
                assert torch.equal(got, want), (name, pin, sched)
                assert bool((guard == SENTINEL).all()), (name, pin, sched)
                assert int(D.status[0]) == 0, (name, pin, sched)


@pytest.mark.parametrize("in_f,out_f", [(768, 3072), (3072, 768)])
def test_class_token_rows_of_the_last_block(in_f, out_f):
    """T = 64 on the fc1 / fc2 shapes (Block.relprop_cls_only): every tile of every launch is ragged."""
    D = dense(256, in_f, out_f)
    o = D.rows(64)
    for name in ("rule on signed planes", "rule on |X| planes", "product forward", "product backward"):
        for flags in (0, D.ops.TE_X6_TEST_SMALL_GRID):
            got, guard = D.run(name, 64, flags, o)
            assert torch.equal(got, D.want[name][:64]), (name, flags)
            assert bool((guard == SENTINEL).all()), (name, flags)
            assert int(D.status[0]) == 0, (name, flags)


@pytest.mark.parametrize("T", TS)
def test_ops_calls_on_ragged_rows(T):
    """The same rows through ops.gemm_x6 and ops.linear_relprop: the forward product leaves the rule its planes (signed, or those of
    |X| with ops.X6_SIGNED_PLANES off), the rule with and without a deferred factor on R, variant lrp and alpha != 1."""
    in_f, out_f = FEATURES[0]
    D = dense(_up256(T), in_f, out_f)
    ops = D.ops

    def chain(n, signed):
        X, R, rs = D.X[:n].clone(), D.R[:n].clone(), D.rs[:n].clone()
        res, cache = {}, {}
        was = ops.X6_SIGNED_PLANES
        ops.X6_SIGNED_PLANES = signed
        try:
            for scaled in (False, True):
                Y = ops.gemm_x6(X, ops.x6_matrix_planes(D.W, False, cache), D.b, out_f, keep_abs=cache)
                assert ("x_abs_planes" in cache) and ops.planes_are_signed(cache["x_abs_planes"][1]) == signed
                res["forward"] = Y
                res["rule", scaled] = ops.linear_relprop(ops.Deferred(R, rs) if scaled else R, X, D.W, Y=Y, bias=D.b, cache=cache)
                assert "x_abs_planes" not in cache
            res["backward"] = ops.gemm_x6(R, ops.x6_matrix_planes(D.W, True, cache), None, in_f)
            res["lrp"] = ops.linear_relprop(R, X, D.W, variant="lrp", cache=cache)
            res["alpha 2"] = ops.linear_relprop(R, X, D.W, alpha=2.0, Y=Y, bias=D.b, cache=cache)
        finally:
            ops.X6_SIGNED_PLANES = was
        return res

    key = ("ops", D.Tp)
    if key not in _dense:
        _dense[key] = chain(D.Tp, True)
    want = _dense[key]
    assert torch.equal(want["forward"], D.want["product forward"])      # (the rules here read this Y, those above the stock product's)
    for signed in (True, False):
        got = chain(T, signed)
        for k, v in got.items():
            assert v.shape[0] == T and torch.equal(v, want[k][:T]), (k, signed)
    ops.x6_raise_if_failed()
