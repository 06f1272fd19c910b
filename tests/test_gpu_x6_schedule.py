"""`-m gpu`: every schedule of an x6 launch gives the same bits.  The Linear rule (te_linear_relprop_x6_f32) and the plain product
(te_gemm_x6_f32) through the C ABI on workspaces this file owns, on the three tile geometries: the schedule the cost rule picks,
the rule before it (TE_X6_SLACK_RULE), whole tiles in static ranges (TE_X6_WHOLE_TILES | TE_X6_STATIC_TILES) and whole tiles claimed
from the XCD's counter (TE_X6_WHOLE_TILES), each on the default grid and on the 16-workgroup grid of TE_X6_TEST_SMALL_GRID.

At 1100 rows the 16 workgroups claim several tiles each; at 257 rows an XCD has one tile or none and most workgroups find the
range empty.  Every output is one k-ordered chain whoever computes its tile, so every comparison is torch.equal."""
import pytest
import torch

from gpu_util import dev, rnd

pytestmark = pytest.mark.gpu

SHAPES = [(257, 128, 256), (700, 256, 512), (1100, 768, 2304)]


class Layer:
    """Operands of one Linear layer [T, in_f] -> [T, out_f] on the device, and the two calls on caller-owned buffers."""

    def __init__(self, T, in_f, out_f, seed):
        from transformer_explainability_amd import _lib, ops
        self.ops, self._lib, self.lib = ops, _lib, _lib.load()
        _lib.require_device()
        self.T, self.in_f, self.out_f = T, in_f, out_f
        X, W, b, R = rnd((T, in_f), seed), rnd((out_f, in_f), seed + 1, 0.05), rnd((out_f,), seed + 2, 0.3), rnd((T, out_f), seed + 3, 0.01)
        X[1] = 0.0
        self.X, self.W, self.b, self.R = (t.to(dev()) for t in (X, W, b, R))
        self.Y = torch.nn.functional.linear(self.X, self.W, self.b)
        self.rule_planes = ops.x6_weight_planes(self.W)
        self.gemm_planes = ops.x6_matrix_planes(self.W, False)
        self.status = ops.x6_status(dev())
        torch.cuda.synchronize()

    def rule_ws(self):
        return torch.empty(self.lib.te_linear_relprop_x6_workspace_bytes(self.T, self.in_f, self.out_f), dtype=torch.uint8, device=dev())

    def gemm_ws(self):
        return torch.empty(self.lib.te_gemm_x6_workspace_bytes(self.T, self.in_f, self.out_f), dtype=torch.uint8, device=dev())

    def rule(self, flags, ws, stream=None):
        st = (stream or torch.cuda.current_stream()).cuda_stream
        out = torch.full((self.T, self.in_f), float("nan"), dtype=torch.float32, device=dev())
        self._lib.check(self.lib.te_linear_relprop_x6_f32(
            self.R.data_ptr(), None, 0, 1, self.X.data_ptr(), self.W.data_ptr(), self.rule_planes.data_ptr(), None,
            self.Y.data_ptr(), self.b.data_ptr(), out.data_ptr(), self.T, self.in_f, self.out_f, flags, self.status.data_ptr(),
            ws.data_ptr(), ws.numel(), st), "te_linear_relprop_x6_f32")
        return out

    def product(self, flags, ws, stream=None):
        st = (stream or torch.cuda.current_stream()).cuda_stream
        out = torch.full((self.T, self.out_f), float("nan"), dtype=torch.float32, device=dev())
        self._lib.check(self.lib.te_gemm_x6_f32(
            self.X.data_ptr(), None, self.gemm_planes.data_ptr(), self.b.data_ptr(), out.data_ptr(), self.T, self.in_f,
            self.out_f, flags, self.status.data_ptr(), ws.data_ptr(), ws.numel(), st), "te_gemm_x6_f32")
        return out


def schedules(ops):
    return {"default": 0, "slack rule": ops.TE_X6_SLACK_RULE, "static whole tiles": ops.TE_X6_WHOLE_TILES | ops.TE_X6_STATIC_TILES,
            "claimed whole tiles": ops.TE_X6_WHOLE_TILES}


@pytest.mark.parametrize("T,in_f,out_f", SHAPES)
def test_every_schedule_gives_the_same_bits(T, in_f, out_f):
    L = Layer(T, in_f, out_f, 500)
    ops = L.ops
    ops.x6_raise_if_failed()
    rws, gws = L.rule_ws(), L.gemm_ws()
    base, gbase = L.rule(0, rws), L.product(0, gws)
    assert torch.isfinite(base).all() and torch.isfinite(gbase).all()
    assert float((gbase - L.Y).abs().max()) <= 1e-5 * float(L.Y.abs().max())        # the product is the layer's forward output
    for pin in (1, 2, 3):                                    # 128 x 256, 256 x 256, 128 x 128 tiles
        for name, st in schedules(ops).items():
            for grid in (0, ops.TE_X6_TEST_SMALL_GRID):
                got, ggot = L.rule(pin | st | grid, rws), L.product(pin | st | grid, gws)
                assert torch.equal(got, base), ("rule", pin, name, grid)
                assert torch.equal(ggot, gbase), ("product", pin, name, grid)
                assert L.lib.te_linear_relprop_x6_check(rws.data_ptr(), T, in_f, out_f, torch.cuda.current_stream().cuda_stream) == 0, \
                    (pin, name, grid)
    ops.x6_raise_if_failed()


@pytest.mark.parametrize("T,in_f,out_f", SHAPES)
def test_twice_on_one_workspace(T, in_f, out_f):
    """The tile counters start from zero in every call: the second call on the same workspace computes every tile again (a stale
    counter would leave its `out`, filled with NaN here, untouched)."""
    L = Layer(T, in_f, out_f, 510)
    ops = L.ops
    rws, gws = L.rule_ws(), L.gemm_ws()
    for grid in (0, ops.TE_X6_TEST_SMALL_GRID):
        fl = 2 | ops.TE_X6_WHOLE_TILES | grid
        first, gfirst = L.rule(fl, rws), L.product(fl, gws)
        second, gsecond = L.rule(fl, rws), L.product(fl, gws)
        assert torch.isfinite(first).all() and torch.equal(first, second), grid
        assert torch.isfinite(gfirst).all() and torch.equal(gfirst, gsecond), grid
        # ... and one phase per call, as the measurement scripts make them
        parts = None
        for ph in (ops.TE_X6_PHASE_SPLIT, ops.TE_X6_PHASE_Z, ops.TE_X6_PHASE_C):
            parts = L.rule(fl | ph, rws)
        assert torch.equal(parts, first), grid
    ops.x6_raise_if_failed()


def test_two_rules_side_by_side():
    """Two launches on two streams share the CUs: workgroups of either become resident late.  Same bits as one after the other."""
    T, in_f, out_f = 700, 256, 512
    L = Layer(T, in_f, out_f, 520)
    ops = L.ops
    ws = [L.rule_ws(), L.rule_ws()]
    serial = [L.rule(2 | ops.TE_X6_WHOLE_TILES, ws[0]), L.rule(1 | ops.TE_X6_WHOLE_TILES | ops.TE_X6_TEST_SMALL_GRID, ws[1])]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    side = []
    for _ in range(3):
        with torch.cuda.stream(streams[0]):
            a = L.rule(2 | ops.TE_X6_WHOLE_TILES, ws[0], streams[0])
        with torch.cuda.stream(streams[1]):
            b = L.rule(1 | ops.TE_X6_WHOLE_TILES | ops.TE_X6_TEST_SMALL_GRID, ws[1], streams[1])
        side.append((a, b))
    for s in streams:
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for a, b in side:
        assert torch.equal(a, serial[0]) and torch.equal(b, serial[1])
    assert torch.equal(serial[0], serial[1])
    ops.x6_raise_if_failed()
