"""The schedule of an x6 launch as te_linear_x6_schedule reports it (host arithmetic, no GPU): which launches take whole tiles and
which stream-K under the cost rule of csrc/te_linear_x6.hip (plan_x6), the grid, the forcing flags, the refusals.

The rule: r = tiles per workgroup; whole tiles where ceil(r) * t_lock(nks) <= (1 + margin) * r * t_skew(nks), with the K16 step
times t_lock = 2.27 us and t_skew = 2.60 us at nks <= 48 falling linearly to 2.00 and 2.32 us at nks >= 144; margin = 5 %, and 20 %
for a call pinned to 256 x 256 tiles (the caller packs kernels of several streams: CU-time counts).  On 256 x 256 tiles a launch has
256 workgroups, so beyond 256 tiles r = tiles / 256."""
import ctypes
import math

import pytest

from host_util import lib  # noqa: F401

T_VIT_B = 64 * 197          # 12 608 rows: 50 tile columns of 256 rows


def schedule(lib, T, in_f, out_f, pass_, flags):
    from transformer_explainability_amd import _lib
    out = (ctypes.c_int * 4)(-1, -1, -1, -1)
    rc = lib.te_linear_x6_schedule(T, in_f, out_f, pass_, flags, out)
    assert rc == _lib.TE_OK, rc
    return dict(geometry=out[0], schedule=out[1], grid=out[2], tiles=out[3])


def whole_by_rule(tiles, workgroups, nks, margin):
    """The cost comparison, written out from the numbers of the module docstring."""
    r = tiles / workgroups
    f = min(1.0, max(0.0, (nks - 48) / 96))
    t_lock, t_skew = 2.27 + (2.00 - 2.27) * f, 2.60 + (2.32 - 2.60) * f
    return math.ceil(r) * t_lock <= (1 + margin) * r * t_skew


def test_vit_b_launches_on_256_tiles(lib):
    """ViT-B/16 batch 64 with the 256 x 256 pin of the concurrent step: the 450-, 600- and 1200-tile launches take whole tiles
    (claimed), the 300-tile C-passes stay on stream-K."""
    from transformer_explainability_amd import ops
    Z, C, G = ops.TE_X6_PASS_Z, ops.TE_X6_PASS_C, ops.TE_X6_PASS_PRODUCT
    pin = 2
    whole = [("qkv Z-pass", 768, 2304, Z, 450), ("qkv forward product", 768, 2304, G, 450),
             ("fc1 Z-pass", 768, 3072, Z, 600), ("fc1 forward product", 768, 3072, G, 600),
             ("fc2 input gradient", 768, 3072, G, 600), ("fc2 C-pass", 3072, 768, C, 1200)]
    for name, in_f, out_f, p, tiles in whole:
        s = schedule(lib, T_VIT_B, in_f, out_f, p, pin)
        assert s["tiles"] == tiles and s["geometry"] == 2 and s["grid"] == 256, (name, s)
        assert s["schedule"] == ops.TE_X6_SCHEDULE_WHOLE_CLAIMED, (name, s)
    for name, in_f, out_f in (("qkv C-pass", 768, 2304), ("proj C-pass", 768, 768), ("fc1 C-pass", 768, 3072)):
        s = schedule(lib, T_VIT_B, in_f, out_f, C, pin)
        assert s["tiles"] == 300 and s["grid"] == 256 and s["schedule"] == ops.TE_X6_SCHEDULE_STREAM_K, (name, s)
    # 150 tiles on 152 workgroups (the launches with 768 weight rows): one round, whole tiles as before
    s = schedule(lib, T_VIT_B, 768, 768, Z, pin)
    assert s["tiles"] == 150 and s["grid"] == 152 and s["schedule"] == ops.TE_X6_SCHEDULE_WHOLE_CLAIMED, s


@pytest.mark.parametrize("pin,in_f,out_f,pass_name,cols_stream_k,cols_whole", [
    # pinned to 256 x 256 tiles (margin 20 %).  nks = 48 (K = 768), 12 tile rows: two rounds pay from
    # r >= 2 / (1.2 * 2.60 / 2.27) = 1.455, i.e. 373 tiles
    (2, 768, 3072, "Z", 31, 32),
    # ... and three rounds from r >= 3 / 1.374 = 2.183, i.e. 559 tiles
    (2, 768, 3072, "Z", 46, 47),
    # nks = 144 (the C-pass of qkv), 6 tile rows: two rounds pay from r >= 2 / (1.2 * 2.32 / 2.00) = 1.437, i.e. 368 tiles
    (2, 768, 2304, "C", 61, 62),
    # nks = 96 (in between: 2.135 and 2.46 us), 6 tile rows: from r >= 2 / 1.3827 = 1.446, i.e. 371 tiles
    (2, 1536, 1536, "Z", 61, 62),
    # not pinned (margin 5 %; the library picks 256 x 256 tiles for these itself).  nks = 48: from r >= 2 / (1.05 * 2.60 / 2.27) =
    # 1.663, i.e. 426 tiles
    (0, 768, 3072, "Z", 35, 36),
    # nks = 144: from r >= 2 / (1.05 * 1.16) = 1.642, i.e. 421 tiles
    (0, 768, 2304, "C", 70, 71),
])
def test_either_side_of_a_threshold(lib, pin, in_f, out_f, pass_name, cols_stream_k, cols_whole):
    from transformer_explainability_amd import _lib, ops
    p = {"Z": ops.TE_X6_PASS_Z, "C": ops.TE_X6_PASS_C}[pass_name]
    nks = (out_f if pass_name == "C" else in_f) // 16
    rows = (2 * in_f if pass_name == "C" else out_f) // 256
    for cols, want in ((cols_stream_k, ops.TE_X6_SCHEDULE_STREAM_K), (cols_whole, ops.TE_X6_SCHEDULE_WHOLE_CLAIMED)):
        s = schedule(lib, 256 * cols, in_f, out_f, p, pin)
        assert s["geometry"] == _lib.TE_X6_TILE_256 and s["tiles"] == rows * cols and s["grid"] == 256, s
        assert whole_by_rule(s["tiles"], s["grid"], nks, 0.20 if pin == 2 else 0.05) == (want != ops.TE_X6_SCHEDULE_STREAM_K), (s, nks)
        assert s["schedule"] == want, (cols, s)
        # one row fewer than a full tile column changes nothing: the count of tiles decides
        assert schedule(lib, 256 * cols - 255, in_f, out_f, p, pin) == s


def test_without_the_pin_a_launch_alone_keeps_its_wall_time(lib):
    """The same ViT-B launches as the library schedules them for a caller that did not pin the geometry: the 600-tile launches
    (whole tiles 12-16 % longer) stay on stream-K, as under the slack rule."""
    from transformer_explainability_amd import _lib, ops
    for p, in_f, out_f in ((ops.TE_X6_PASS_Z, 768, 3072), (ops.TE_X6_PASS_PRODUCT, 768, 3072)):
        for flags in (0, ops.TE_X6_SLACK_RULE):
            s = schedule(lib, T_VIT_B, in_f, out_f, p, flags)
            assert s["geometry"] == _lib.TE_X6_TILE_256 and s["tiles"] == 600 and s["schedule"] == ops.TE_X6_SCHEDULE_STREAM_K, s
    s = schedule(lib, T_VIT_B, 768, 2304, ops.TE_X6_PASS_Z, 0)
    assert s["tiles"] == 450 and s["schedule"] == ops.TE_X6_SCHEDULE_WHOLE_CLAIMED, s


def test_grid_is_whole_xcds_and_bounded(lib):
    from transformer_explainability_amd import _lib, ops
    max_spx = {_lib.TE_X6_TILE_256: 32, _lib.TE_X6_TILE_128: 64, _lib.TE_X6_TILE_128x128: 96}
    for T in (1, 257, 700, 1100, 5000, T_VIT_B, 32 * 577, 1 << 20):
        for in_f, out_f in ((128, 256), (256, 512), (768, 768), (768, 2304), (3072, 768), (1024, 4096), (192, 128)):
            for p in (ops.TE_X6_PASS_Z, ops.TE_X6_PASS_C, ops.TE_X6_PASS_PRODUCT):
                for pin in (0, 1, 2, 3):
                    for extra in (0, ops.TE_X6_WHOLE_TILES, ops.TE_X6_SLACK_RULE, ops.TE_X6_TEST_SMALL_GRID):
                        s = schedule(lib, T, in_f, out_f, p, pin | extra)
                        assert s["grid"] % 8 == 0 and 8 <= s["grid"] <= 8 * max_spx[s["geometry"]], (T, in_f, out_f, p, pin, s)
                        assert s["grid"] <= max(8, 8 * -(-s["tiles"] // 8)), s
                        if extra == ops.TE_X6_TEST_SMALL_GRID:
                            assert s["grid"] <= 16 and s["schedule"] == ops.TE_X6_SCHEDULE_STREAM_K, s
                        if extra == ops.TE_X6_WHOLE_TILES:
                            assert s["schedule"] == ops.TE_X6_SCHEDULE_WHOLE_CLAIMED, s


def test_forcing_flags_override_the_rule(lib):
    from transformer_explainability_amd import ops
    Z, C = ops.TE_X6_PASS_Z, ops.TE_X6_PASS_C
    K, S, W = ops.TE_X6_SCHEDULE_STREAM_K, ops.TE_X6_SCHEDULE_WHOLE_STATIC, ops.TE_X6_SCHEDULE_WHOLE_CLAIMED
    fc1_z = (T_VIT_B, 768, 3072, Z)          # 600 tiles: whole by the cost rule, stream-K by the slack rule (3 > 1.15 * 2.34)
    qkv_c = (T_VIT_B, 768, 2304, C)          # 300 tiles: stream-K by both
    fc2_c = (T_VIT_B, 3072, 768, C)          # 1200 tiles: whole by both (5 <= 1.15 * 4.69)
    for shape, flags, want in (
            (fc1_z, 0, W), (fc1_z, ops.TE_X6_SLACK_RULE, K), (fc1_z, ops.TE_X6_STATIC_TILES, S),
            (fc1_z, ops.TE_X6_SLACK_RULE | ops.TE_X6_STATIC_TILES, K), (fc1_z, ops.TE_X6_SLACK_RULE | ops.TE_X6_WHOLE_TILES, W),
            (qkv_c, 0, K), (qkv_c, ops.TE_X6_SLACK_RULE, K), (qkv_c, ops.TE_X6_STATIC_TILES, K),
            (qkv_c, ops.TE_X6_WHOLE_TILES, W), (qkv_c, ops.TE_X6_WHOLE_TILES | ops.TE_X6_STATIC_TILES, S),
            (fc2_c, 0, W), (fc2_c, ops.TE_X6_SLACK_RULE, W), (fc2_c, ops.TE_X6_SLACK_RULE | ops.TE_X6_STATIC_TILES, S),
            (fc1_z, ops.TE_X6_TEST_SMALL_GRID, K), (fc1_z, ops.TE_X6_TEST_SMALL_GRID | ops.TE_X6_WHOLE_TILES, W),
            (fc1_z, ops.TE_X6_TEST_SMALL_GRID | ops.TE_X6_WHOLE_TILES | ops.TE_X6_STATIC_TILES, S)):
        s = schedule(lib, *shape, 2 | flags)
        assert s["schedule"] == want, (shape, hex(flags), s)
        assert s["grid"] == (16 if flags & ops.TE_X6_TEST_SMALL_GRID else 256), s
    # the per-pass pins of the rule reach the pass they name
    s = schedule(lib, T_VIT_B, 768, 3072, Z, 1 | (2 << ops.TE_X6_TILE_Z_SHIFT) | (3 << ops.TE_X6_TILE_C_SHIFT))
    assert s["geometry"] == ops._lib.TE_X6_TILE_256 and s["tiles"] == 600, s
    s = schedule(lib, T_VIT_B, 768, 3072, C, 1 | (2 << ops.TE_X6_TILE_Z_SHIFT) | (3 << ops.TE_X6_TILE_C_SHIFT))
    assert s["geometry"] == ops._lib.TE_X6_TILE_128x128 and s["tiles"] == 12 * 99, s


def test_refusals(lib):
    from transformer_explainability_amd import _lib, ops
    out = (ctypes.c_int * 4)(7, 7, 7, 7)
    Z, C, G = ops.TE_X6_PASS_Z, ops.TE_X6_PASS_C, ops.TE_X6_PASS_PRODUCT
    assert (ops.TE_X6_SLACK_RULE, ops.TE_X6_STATIC_TILES) == (0x100000, 0x80000)
    for p in (Z, C, G):
        for bad in (0x100, 0x8000, 0x40000, 0x200000, 0x40, 1 << 30):          # the retired study flags and bits nobody defined
            assert lib.te_linear_x6_schedule(T_VIT_B, 768, 3072, p, bad, out) == _lib.TE_ERR_INVALID_ARG, (p, hex(bad))
    # the plain product knows neither phases nor per-pass pins nor the signed-planes bit
    for bad in (ops.TE_X6_PHASE_Z, 2 << ops.TE_X6_TILE_Z_SHIFT, ops.TE_X6_X_PLANES_SIGNED):
        assert lib.te_linear_x6_schedule(T_VIT_B, 768, 3072, G, bad, out) == _lib.TE_ERR_INVALID_ARG, hex(bad)
        assert lib.te_linear_x6_schedule(T_VIT_B, 768, 3072, Z, bad, out) == _lib.TE_OK, hex(bad)
    assert lib.te_linear_x6_schedule(T_VIT_B, 768, 3072, 3, 0, out) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_linear_x6_schedule(T_VIT_B, 768, 3072, -1, 0, out) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_linear_x6_schedule(T_VIT_B, 768, 3072, Z, 0, None) == _lib.TE_ERR_INVALID_ARG
    assert lib.te_linear_x6_schedule(T_VIT_B, 100, 3072, Z, 0, out) == _lib.TE_ERR_UNSUPPORTED
    assert lib.te_linear_x6_schedule(0, 768, 3072, Z, 0, out) == _lib.TE_ERR_UNSUPPORTED
    # the entry points themselves refuse the same bits before they touch anything (no device needed for a refusal)
    for bad in (0x100, 0x8000, 0x40000, 0x200000):
        assert lib.te_gemm_x6_f32(None, 16, 16, None, 16, 256, 128, 128, bad, None, None, 0, None) == _lib.TE_ERR_INVALID_ARG
