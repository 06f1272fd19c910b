"""C-ABI surface checks that need no GPU: the library is built, loads through ctypes, exports every
symbol include/te_relprop.h declares, and the host-side workspace queries / argument validation work; the parser that
derives the ctypes binding from that header (_cabi.py) reads every kind of declaration and refuses what it does not know."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "te_relprop.h")


from host_util import lib  # noqa: E402,F401


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(te_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    names = declared_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in te_relprop.h but not exported by libte_relprop.so"


def test_binding_covers_header():
    from transformer_explainability_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()


SYNTHETIC = """
/* te_fake.h -- int te_in_a_comment(int x); is not a declaration,
 * nor is size_t te_another_one(void); on a continuation line */
#ifndef TE_FAKE_H
#define TE_FAKE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* te_stream_t; /* hipStream_t */
typedef uint16_t te_bf16_t;
enum {
  TE_OK = 0,
  TE_ERR_BAD = -7,   /* trailing comment, with a comma */
  TE_IMPL_FLAG = 0x1F0, // hex
  TE_NEXT        /* no value: the one before, plus one */
};
enum { TE_ONE_LINE_A = 1, TE_ONE_LINE_B = -0x10 };
#define TE_LIMIT 16   /* at most, see te_in_a_comment(int) */
#define TE_BIG (1 << 20)
#define TE_NEG -3
#define TE_TILE_128x128 3
#define TE_SPANS 0x4000   /* a comment that
                             runs over two lines */
#define TE_FN_LIKE(x) ((x) + 1)
const char* te_name(void);
size_t te_bytes();
int
te_split_over_lines(const te_bf16_t* W,
                    void* ws,   /* scratch */
                    te_stream_t stream,
                    double eps, float alpha,
                    int flags, int64_t n, size_t ws_bytes);
int te_more(const int64_t* ks, unsigned* status, const float * const x, int64_t W_);
#ifdef __cplusplus
}
#endif
#endif /* TE_FAKE_H */
"""


def _cabi():
    from transformer_explainability_amd import _cabi
    return _cabi


def test_parser_every_kind_of_declaration():
    from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p
    protos, consts = _cabi().parse(SYNTHETIC)
    assert protos == {
        "te_name": (c_char_p, []),
        "te_bytes": (c_size_t, []),
        "te_split_over_lines": (c_int, [("W", c_void_p), ("ws", c_void_p), ("stream", c_void_p), ("eps", c_double),
                                        ("alpha", c_float), ("flags", c_int), ("n", c_int64), ("ws_bytes", c_size_t)]),
        "te_more": (c_int, [("ks", c_void_p), ("status", c_void_p), ("x", c_void_p), ("W_", c_int64)]),
    }
    assert consts == {"TE_OK": 0, "TE_ERR_BAD": -7, "TE_IMPL_FLAG": 0x1F0, "TE_NEXT": 0x1F1, "TE_ONE_LINE_A": 1,
                      "TE_ONE_LINE_B": -16, "TE_LIMIT": 16, "TE_BIG": 1 << 20, "TE_NEG": -3, "TE_TILE_128x128": 3,
                      "TE_SPANS": 0x4000}
    assert all(type(v) is int for v in consts.values())


@pytest.mark.parametrize("text, names", [
    ("int te_f(int a, long b);", ["te_f", "b", "long"]),                       # unknown parameter type
    ("int te_f(int64_t);", ["te_f", "int64_t"]),                               # a parameter without a name
    ("int te_f(int a[4]);", ["te_f", "a[4]"]),
    ("int te_f(int a, void (*cb)(int));", ["te_f"]),                           # nothing the grammar has
    ("long te_f(int a);", ["te_f", "long"]),                                   # unknown return type
    ("te_f(int a);", ["te_f"]),                                                # no return type
    ("int te_ok(int a);\nint te_f(int a)\nint te_g(int b);", ["te_f"]),        # no ';'
    ("int te_f(int a, int b;", ["te_f"]),                                      # no ')'
    ("int te_f(int a) { return a; }", ["te_f"]),                               # a definition
    ("int te_f(int a);\nint te_f(int a);", ["te_f", "twice"]),
    ("#define TE_A (1 + 2)\n", ["TE_A", "1 + 2"]),                             # outside the fixed grammar: never eval'ed
    ("#define TE_A __import__('os')\n", ["TE_A"]),
    ("enum { TE_A = TE_B };", ["TE_A", "TE_B"]),
])
def test_parser_refuses_what_it_does_not_understand(text, names):
    cabi = _cabi()
    with pytest.raises(cabi.HeaderError) as e:
        cabi.parse(text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_binding_pinned_facts():
    """Facts of include/te_relprop.h written out here, not read through the parser."""
    from ctypes import c_char_p, c_double, c_int, c_int64, c_size_t, c_void_p
    from transformer_explainability_amd import _lib, ops
    S = _lib.SIGNATURES
    assert S["te_status_string"] == (c_char_p, [c_int])
    assert S["te_build_id"] == (c_char_p, []) and S["te_version"] == (c_int, [])
    assert S["te_linear_relprop_workspace_bytes"] == (c_size_t, [c_int64, c_int64, c_int64, c_int])
    args = S["te_map_similarity_f32"][1]
    assert len(args) == 13 and [i for i, t in enumerate(args) if t is c_double] == [9]
    assert _lib.PARAMS["te_map_similarity_f32"][9] == "data_range"
    res, args = S["te_attention_backward_strided_f32"]
    assert res is c_int and len(args) == 43 and args[-4:] == [c_int, c_void_p, c_size_t, c_void_p]
    assert _lib.PARAMS["te_attention_backward_strided_f32"][-4:] == ("need_qk", "ws", "ws_bytes", "stream")
    assert all(len(_lib.PARAMS[n]) == len(S[n][1]) for n in S) and sorted(_lib.PARAMS) == sorted(S)
    assert _lib.TE_OK == 0 and _lib.TE_ERR_NO_DEVICE == -4 and _lib.TE_IMPL_SIMPLE == 0x100
    assert _lib.TE_X6_WHOLE_TILES == 0x10000 and ops.TE_X6_WHOLE_TILES == 0x10000
    assert (ops.TE_X6_PHASE_SPLIT, ops.TE_X6_PHASE_Z, ops.TE_X6_PHASE_C) == (4, 8, 16)
    assert (ops.TE_X6_TEST_DROP_HANDOVER, ops.TE_X6_TILE_Z_SHIFT, ops.TE_X6_TILE_C_SHIFT, ops.TE_X6_TEST_SMALL_GRID) == \
        (0x200, 10, 12, 0x4000)
    assert _lib.TE_CLASS_TARGETS_MAX_CLASSES == 1 << 20
    assert "TE_RELPROP_H" not in _lib.CONSTANTS                                # the include guard is no constant


def test_binding_follows_the_header():
    """One int64_t fewer in one prototype of the real header: that entry's argtypes change, no other entry does."""
    from ctypes import c_int64
    cabi = _cabi()
    text = open(HEADER).read()
    victim, gone = "te_attention_backward_strided_f32", "int64_t dk_sh, "
    at = text.index(gone, text.index(f"int {victim}("))
    assert at < text.index(";", text.index(f"int {victim}("))                   # inside the victim's argument list
    before, consts = cabi.parse(text)
    after, consts_after = cabi.parse(text[:at] + text[at + len(gone):])
    assert consts_after == consts and set(after) == set(before)
    assert [n for n in before if after[n] != before[n]] == [victim]
    params = before[victim][1]
    i = [p for p, _ in params].index("dk_sh")
    assert params[i][1] is c_int64 and after[victim][1] == params[:i] + params[i + 1:]


# The entry points that replaced a family of names (0.8.0): name -> (what the retired names of its family ended in instead of
# "_f32", the most general one last; the parameter names of that most general entry as they stood before the merge).  ops.py
# passes every argument by position: a transposed pair would be a wild pointer on the device.
_BHND = ("B", "H", "N", "D")
_WS = ("ws", "ws_bytes", "stream")
MERGED = {
    "te_matmul_relprop_av_f32": (("_fwd_f32", "_fwdz_f32"), (
        "R", "r_sb", "r_sh", "r_sn", "attn", "v", "v_sb", "v_sh", "v_sn", "Z", "z_sb", "z_sh", "z_sn", "cam_attn",
        "cam_v", "cv_sb", "cv_sh", "cv_sn", *_BHND, "out_scale", "variant", *_WS)),
    "te_matmul_relprop_qk_f32": (("_fwd_f32", "_fwd_scaled_f32"), (
        "R_nn", "r_scale", "r_scale_stride", "q", "q_sb", "q_sh", "q_sn", "k", "k_sb", "k_sh", "k_sn", "Z",
        "cam_q", "cq_sb", "cq_sh", "cq_sn", "cam_k", "ck_sb", "ck_sh", "ck_sn", *_BHND, "out_scale", "variant", *_WS)),
    "te_linear_zpass_fwd_f32": (("_scaled_f32",), (
        "R", "r_scale", "r_scale_stride", "rows_per_sample", "X", "W", "Y", "bias", "S", "T", "in_f", "out_f", "stream")),
    "te_linear_relprop_fwd_f32": (("_scaled_f32",), (
        "R", "r_scale", "r_scale_stride", "rows_per_sample", "X", "W", "Y", "bias", "out", "T", "in_f", "out_f", *_WS)),
    "te_attention_forward_f32": (("_planes_f32",), (
        "qkv", "z_qk", "attn", "out", "out_planes", "out_abs_planes", "planes_bytes", *_BHND, "scale", "stream")),
    "te_attention_backward_f32": (("_out_f32",), (
        "d_out", "out", "qkv", "attn", "d_attn", "d_qkv", *_BHND, "scale", "need_qk", "stream")),
    "te_attention_backward_strided_f32": (("_out_f32",), (
        "d_out", "do_sb", "do_sh", "do_sn", "out", "o_sb", "o_sh", "o_sn", "q", "q_sb", "q_sh", "q_sn",
        "k", "k_sb", "k_sh", "k_sn", "v", "v_sb", "v_sh", "v_sn", "attn", "d_attn", "d_q", "dq_sb", "dq_sh", "dq_sn",
        "d_k", "dk_sb", "dk_sh", "dk_sn", "d_v", "dv_sb", "dv_sh", "dv_sn", *_BHND, "scale", "need_qk", *_WS)),
}
RETIRED = sorted(name[:-len("_f32")] + end for name, (ends, _) in MERGED.items() for end in ends)


def test_merged_entry_points_keep_the_general_argument_lists():
    from transformer_explainability_amd import _lib
    for name, (_, params) in MERGED.items():
        assert _lib.PARAMS[name] == params, name
    assert len(MERGED["te_attention_backward_strided_f32"][1]) == 43
    # the fp32 and the bf16 form of a rule: one argument list under one base name
    assert _lib.PARAMS["te_matmul_relprop_av_f32"] == _lib.PARAMS["te_matmul_relprop_av_bf16"]
    assert _lib.PARAMS["te_matmul_relprop_qk_f32"] == _lib.PARAMS["te_matmul_relprop_qk_bf16"]


def test_retired_entry_points_are_gone(lib):
    from transformer_explainability_amd import _lib
    assert len(RETIRED) == 9 and len(set(RETIRED)) == 9
    declared = declared_symbols()
    for name in RETIRED:
        assert name not in declared and name not in _lib.SIGNATURES and name not in _lib.PARAMS, name
        assert not hasattr(lib, name), f"{name} is still exported by libte_relprop.so"


def test_loader_refuses_an_older_library(lib, monkeypatch):
    """A library older than MIN_LIB_VERSION is refused by the version check, before the build id is looked at."""
    from transformer_explainability_amd import _lib
    assert _lib.MIN_LIB_VERSION == 800 and lib.te_version() >= 800
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "MIN_LIB_VERSION", lib.te_version() + 1)
    with pytest.raises(_lib.TeError, match=f"needs >= {lib.te_version() + 1}"):
        _lib.load()
    monkeypatch.undo()
    assert _lib.load().te_version() == lib.te_version()


def test_version_and_status_strings(lib):
    assert lib.te_version() >= 501
    assert lib.te_status_string(0) == b"ok"
    assert b"workspace" in lib.te_status_string(-2)


def test_workspace_queries(lib):
    T, i, o = 12608, 768, 3072
    assert lib.te_linear_relprop_workspace_bytes(T, i, o, 0) >= T * o * 4
    assert lib.te_linear_relprop_workspace_bytes(T, i, o, 1) >= 2 * T * o * 4
    assert lib.te_matmul_relprop_av_workspace_bytes(64, 12, 197, 64) >= 64 * 12 * 197 * 64 * 4
    assert lib.te_matmul_relprop_qk_workspace_bytes(64, 12, 197, 64) >= 64 * 12 * 197 * 197 * 4
    assert lib.te_add_relprop_workspace_bytes(64, 197 * 768) > 0
    assert lib.te_add_bcast_relprop_workspace_bytes(32, 12, 512) > 0
    assert lib.te_rollout_workspace_bytes(12, 64, 197) >= 13 * 64 * 197 * 197 * 4
    assert lib.te_linear_relprop_workspace_bytes(0, 1, 1, 0) == 0
    # x6 workspaces of long-K / narrow products (ViT-B/16 batch 64: fc2's rule and forward, K = 3072 into 768 rows): planes,
    # 64 MiB of accumulator hand-over and the flag regions, exactly -- no room for a K-split region
    planes = lambda rows, k: -(-rows // 32) * 32 * k * 6      # noqa: E731
    assert lib.te_linear_relprop_x6_workspace_bytes(T, o, i) == planes(T, o) + planes(T, i) + (64 << 20) + 2 * 65536 == 357728256
    assert lib.te_gemm_x6_workspace_bytes(T, o, i) == planes(T, o) + (64 << 20) + 65536 == 299565056
    assert lib.te_linear_relprop_x6_general_workspace_bytes(T, o, i, 0) == \
        2 * planes(T, o) + 2 * planes(T, i) + (64 << 20) + 8 * 65536 == 648609792


def test_argument_validation_without_device(lib):
    # null pointers / bad sizes are rejected on the host before any HIP call
    assert lib.te_clone_relprop_f32(None, None, None, None, None, 16, None) == -1
    assert lib.te_linear_relprop_f32(None, None, None, None, 1, 4, 4, 1.0, 0, None, 0, None) == -1
    assert lib.te_rollout_f32(None, 1, 0, 1, 4, 0, None, None, 0, None) == -1
    assert lib.te_linear_zpass_fwd_f32(None, None, 0, 1, None, None, None, None, None, 1, 4, 4, None) == -1
    assert lib.te_linear_relprop_fwd_f32(None, None, 0, 1, None, None, None, None, None, 1, 4, 4, None, 0, None) == -1
    assert lib.te_matmul_relprop_av_f32(None, 64, 64, 64, None, None, 64, 64, 64, None, 0, 0, 0, None, None, 64, 64, 64,
                                        1, 1, 4, 64, 1.0, 0, None, 0, None) == -1
    assert lib.te_matmul_relprop_qk_f32(None, None, 0, None, 64, 64, 64, None, 64, 64, 64, None, None, 64, 64, 64,
                                        None, 64, 64, 64, 1, 1, 4, 64, 1.0, 0, None, 0, None) == -1


def test_attention_entry_points_reject_on_the_host(lib):
    """What every fp32 attention entry point answers before it touches a device: the status of each refusal.  P is a fake non-null,
    16-byte-aligned address that the host never dereferences; every call below returns before the first HIP call."""
    from transformer_explainability_amd._lib import PARAMS
    P, B, H, N, D = 4096, 2, 2, 100, 64
    C = H * D
    view = lambda name: {name + "_sb": N * C, name + "_sh": 64, name + "_sn": C}      # noqa: E731
    dims = dict(B=B, H=H, N=N, D=D)

    def status(fn, base, **changed):
        assert set(changed) <= set(base) and len(base) == len(PARAMS[fn]), (fn, changed)
        return getattr(lib, fn)(*{**base, **changed}.values())

    fwd_s = dict(q=P, **view("q"), k=P, **view("k"), v=P, **view("v"), mask=None, z_qk=P, x_scaled=None, attn=P, out=P, **view("o"),
                 **dims, scale=0.125, stream=None)
    f = "te_attention_forward_strided_f32"
    assert [status(f, fwd_s, q=None), status(f, fwd_s, N=0)] == [-1, -1]
    assert [status(f, fwd_s, N=641), status(f, fwd_s, D=80), status(f, fwd_s, q_sn=66)] == [-3, -3, -3]

    ws_bytes = lib.te_attention_backward_strided_workspace_bytes(B, H, N)
    bwd_s = dict(d_out=P, **view("do"), out=P, **view("o"), q=P, **view("q"), k=P, **view("k"), v=P, **view("v"), attn=P, d_attn=P, d_q=P, **view("dq"),
                 d_k=P, **view("dk"), d_v=P, **view("dv"), **dims, scale=0.125, need_qk=1, ws=P, ws_bytes=ws_bytes, stream=None)
    f = "te_attention_backward_strided_f32"
    assert [status(f, bwd_s, d_out=None), status(f, bwd_s, d_q=None)] == [-1, -1]
    assert [status(f, bwd_s, N=641), status(f, bwd_s, D=80), status(f, bwd_s, dv_sn=66)] == [-3, -3, -3]
    assert [status(f, bwd_s, ws=None), status(f, bwd_s, ws_bytes=16), status(f, bwd_s, d_q=None, need_qk=0, ws=None)] == [-2, -2, -2]
    # `out` is optional: a NULL passes the null check and the next refusal in order answers; present, its view is validated
    assert [status(f, bwd_s, out=None, ws=None), status(f, bwd_s, o_sn=66)] == [-2, -3]
    b = dict(bwd_s, out=None, o_sb=0, o_sh=0, o_sn=0)      # every refusal above without the operand: its strides are ignored
    assert [status(f, b, d_out=None), status(f, b, d_q=None), status(f, b, N=641), status(f, b, D=80), status(f, b, dv_sn=66),
            status(f, b, ws=None), status(f, b, ws_bytes=16), status(f, b, d_q=None, need_qk=0, ws=None)] == [-1, -1, -3, -3, -3, -2, -2, -2]

    planes_bytes = lib.te_linear_x6_planes_bytes(B * N, H * D)
    assert planes_bytes > 16
    fwd_p = dict(qkv=P, z_qk=P, attn=P, out=P, out_planes=P, out_abs_planes=None, planes_bytes=planes_bytes, **dims, scale=0.125, stream=None)
    fwd = dict(fwd_p, out_planes=None, planes_bytes=0)      # no planes: planes_bytes is ignored
    f = "te_attention_forward_f32"
    assert status(f, fwd, qkv=None) == -1
    assert [status(f, fwd, N=225), status(f, fwd, D=80)] == [-3, -3]
    assert status(f, fwd_p, qkv=None) == -1
    assert [status(f, fwd_p, N=225), status(f, fwd_p, D=80)] == [-3, -3]
    # `out_planes` is optional: a NULL passes the null check (the next refusal answers); |out| planes alone are refused, and the
    # planes are validated when present
    assert status(f, fwd_p, out_planes=None, N=225) == -3
    assert status(f, fwd_p, out_planes=None, out_abs_planes=P) == -1
    assert [status(f, fwd_p, planes_bytes=16), status(f, fwd_p, out_planes=P + 4)] == [-2, -2]
    assert status(f, fwd_p, out_abs_planes=P + 4) == -2
    bwd = dict(d_out=P, out=P, qkv=P, attn=P, d_attn=P, d_qkv=P, **dims, scale=0.125, need_qk=1, stream=None)
    f = "te_attention_backward_f32"
    for out in (P, None):      # `out` is optional: with a NULL the next refusal in order answers
        assert status(f, bwd, out=out, d_out=None) == -1
        assert status(f, bwd, out=out, N=225) == -3

    ws_bytes = lib.te_matmul_relprop_av_workspace_bytes(B, H, N, D)
    av = dict(R=P, **view("r"), attn=P, v=P, **view("v"), Z=P, z_sb=H * N * D, z_sh=N * D, z_sn=D, cam_attn=P, cam_v=P, **view("cv"),
              **dims, scale=1.0, variant=0, ws=P, ws_bytes=ws_bytes, stream=None)
    f = "te_matmul_relprop_av_f32"
    for Z in (P, None):      # Z is optional: the same refusals with and without it
        assert [status(f, av, Z=Z, R=None), status(f, av, Z=Z, r_sb=-1), status(f, av, Z=Z, r_sn=0), status(f, av, Z=Z, D=0)] == [-1, -1, -1, -1]
        assert [status(f, av, Z=Z, ws=None), status(f, av, Z=Z, ws_bytes=ws_bytes - 256)] == [-2, -2]
    ws_bytes = lib.te_matmul_relprop_qk_workspace_bytes(B, H, N, D)
    qk = dict(R=P, r_scale=None, r_scale_stride=0, q=P, **view("q"), k=P, **view("k"), Z=P, cam_q=P, **view("cq"), cam_k=P, **view("ck"),
              **dims, scale=1.0, variant=0, ws=P, ws_bytes=ws_bytes, stream=None)
    f = "te_matmul_relprop_qk_f32"
    for Z, r_scale in ((P, None), (None, None), (P, P), (None, P)):      # Z and r_scale are optional: the same refusals in each state
        o = dict(Z=Z, r_scale=r_scale)
        assert [status(f, qk, **o, R=None), status(f, qk, **o, q_sb=-1)] == [-1, -1]
        assert [status(f, qk, **o, ws=None), status(f, qk, **o, ws_bytes=ws_bytes - 256)] == [-2, -2]

    assert [lib.te_attention_forward_supported(n, 64) for n in (0, 1, 224, 225)] == [0, 1, 1, 0]
    assert [lib.te_attention_strided_supported(n, 64) for n in (0, 1, 640, 641)] == [0, 1, 1, 0]
    assert lib.te_attention_forward_supported(100, 80) == 0 and lib.te_attention_strided_supported(100, 80) == 0


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from transformer_explainability_amd import ops, TeError
    x = torch.zeros(2, 8)
    with pytest.raises(TeError):
        ops.clone_relprop([x, x], x)


def test_build_id_matches_tree_and_loader_refuses_other_sources(monkeypatch):
    """te_build_id() = content hash of csrc/ + include/ (+ flags) baked in by build.py; the loader
    recomputes the source half from the tree and refuses a library built from anything else."""
    import pytest
    from transformer_explainability_amd import _buildid, _lib
    bid = _lib.build_id()
    src, flags = bid.split("-")
    assert len(src) == 16 and len(flags) == 8 and src == _buildid.source_hash()
    assert all(p.endswith((".hip", ".h")) for p in _buildid.source_files()) and len(_buildid.source_files()) >= 16
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_buildid, "source_hash", lambda: "0" * 16)
    monkeypatch.delenv("TE_RELPROP_LIB", raising=False)
    monkeypatch.delenv("TE_ALLOW_STALE_LIB", raising=False)
    with pytest.raises(_lib.TeError, match="built from other sources"):
        _lib.load()
    monkeypatch.undo()
    assert _lib.load().te_build_id().decode() == bid
