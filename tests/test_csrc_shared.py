"""CPU, text only: the device primitives the HIP kernels share are defined ONCE, in a header of csrc/, and the launchers one
translation unit defines and another calls are declared ONCE, in one header (csrc/te_common.h states the house rule).

The three-plane bf16 split is the accuracy contract of every x6 kernel, `fwd6l` recomputes scores "bit for bit" and the GELU
producer's planes are "bit for bit those of a split" -- claims that hold only while every kernel runs the same definition.  Up
to round 10 each new .hip file copied the helpers it needed from the file it was modelled on (five bodies of `split3_pk`, eight
of `Strided`); this test is what keeps the next copy from appearing."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "transformer-explainability_amd", "csrc")


def _sources():
    """{file name: text without // comments} of csrc/*.hip and csrc/*.h"""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            out[os.path.basename(path)] = re.sub(r"//[^\n]*", "", f.read())
    return out


def _function(names):          # `__device__ __forceinline__ <type> name(`: how every device helper of csrc/ is defined
    return r"__forceinline__\s+[\w:]+\s+(?:%s)\s*\(" % names


def _element_load(pointee):    # `__device__ __forceinline__ double <any name>(const <pointee>* p, int64_t i)`
    return r"__forceinline__\s+double\s+\w+\s*\(\s*const\s+%s\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)" % pointee


def _typedef(name):
    return r"\btypedef\s[^;\n]*\s%s\s*(?:__attribute__[^;\n]*)?;" % name


def _macro(name):
    return r"#\s*define\s+%s\b" % name


# (primitive, definition pattern): the table of the shared primitives.  Two names of one function are one entry.
PRIMITIVES = [
    ("split3_pk", _function("split3_pk")),
    ("split3 (scalar view of split3_pk)", _function("split3")),
    ("planes_of8 / split3_x8", _function("planes_of8|split3_x8")),
    ("plane order PA / PB", r"\bint\s+PA\s*\[\s*6\s*\]"),
    ("mfma_x6", _function("mfma_x6")),
    ("sd2", _function("sd2")),
    ("swap_halves", _function("swap_halves")),
    ("div2", _function("div2")),
    ("static_for", _function("static_for")),
    ("kFrag", r"\bint\s+kFrag\b"),
    ("struct Strided", r"\bstruct\s+Strided\b\s*\{"),
    ("crow", _function("crow")),
    ("zero16 / zero", _function("zero16|zero")),
    ("load4", _function("load4")),
    ("store4", _function("store4")),
    ("f32x4_u", _typedef("f32x4_u")),
    ("f32x2", _typedef("f32x2")),
    ("bf16x8", _typedef("bf16x8")),
    ("bf16x2", _typedef("bf16x2")),
    ("u32x4", _typedef("u32x4")),
    ("u32x2", _typedef("u32x2")),
    ("Rsrc", _typedef("Rsrc")),
    ("TE_MFMA_BF16", _macro("TE_MFMA_BF16")),
    ("TE_MFMA32", _macro("TE_MFMA32")),
    ("TE_MFMA16", _macro("TE_MFMA16")),
    # ... under whatever name: each MFMA builtin the macros wrap is spelled out once
    ("the 32x32x2 fp32 MFMA", r"__builtin_amdgcn_mfma_f32_32x32x2f32"),
    ("the 16x16x4 fp32 MFMA", r"__builtin_amdgcn_mfma_f32_16x16x4f32"),
    ("the 32x32x16 bf16 MFMA", r"__builtin_amdgcn_mfma_f32_32x32x16_bf16"),
    ("make_rsrc", _function("make_rsrc")),
    ("view_bytes", _function("view_bytes")),
    ("ld128_hidden", _function("ld128_hidden")),
    ("ld32_hidden", _function("ld32_hidden")),
    ("st128_hidden", _function("st128_hidden")),
    ("st32_hidden", _function("st32_hidden")),
    ("the buffer_load_dwordx4 asm", r'"buffer_load_dwordx4 '),
    ("the buffer_store_dwordx4 asm", r'"buffer_store_dwordx4 '),
    ("TE_VM_WAIT", _macro("TE_VM_WAIT")),
    ("TE_PIN", _macro("TE_PIN")),
    # ... and what the evaluation kernels share (te_segmetrics, te_mapsim, te_curves, te_localise, te_robust, te_faithful,
    # te_perturb, te_classes): ranks, Spearman, Gini and AP are "ties in index order" because they run ONE radix sort, and
    # the fp64 sums have "the order of map_distance" because they run ONE group load and ONE block sum
    ("te_key", _function("te_key")),
    ("te_wave_sum", _function("te_wave_sum")),
    ("te_wave_sum_u32", _function("te_wave_sum_u32|wave_sum_u32")),
    ("match_digit", _function("match_digit")),
    ("block_exclusive_scan", _function("block_exclusive_scan")),
    ("te_sort_buffers", r"__forceinline__\s+uint64_t\s*\*\s*(?:te_sort_buffers|job_buffers)\s*\("),
    ("te_sort_begin", _function("te_sort_begin")),
    ("te_sort_put", _function("te_sort_put")),
    ("te_block_sort_passes", _function("te_block_sort_passes")),
    ("te_block_sum", _function("te_block_sum|block_sum")),
    ("te_block_sum3", _function("te_block_sum3")),
    ("philox4x32_10", _function("philox4x32_10")),
    ("te_pack_bf16", _function("te_pack_bf16")),
    ("bf16_bits", _function("bf16_bits")),
    ("te_bf16_up", _function("te_bf16_up")),
    # under whatever name: an fp64 element load is `double f(const float* p, int64_t i)` and its bf16 overload
    ("te_load_f64 (fp32)", _element_load("float")),
    ("te_load_f64 (bf16)", _element_load("te_bf16_t")),
    ("te_load4_f64", _function("te_load4_f64")),
    ("kTeMaxSortN = 1 << 20", r"\bconstexpr\s+int64_t\s+\w+\s*=\s*\(int64_t\)\s*1\s*<<\s*20\s*;"),
    ("kTeMaxBatch = 65535", r"\bconstexpr\s+int64_t\s+\w+\s*=\s*65535\s*;"),
    ("struct TeChannels", r"\bstruct\s+\w+\s*\{\s*float\s+mean\s*\["),
    ("te_draws_per_block", r"\?\s*n_d\s*:\s*1\s*;"),
]

# the evaluation kernel files, with the header their shared primitives live in
EVALUATION = ["te_segmetrics.hip", "te_mapsim.hip", "te_curves.hip", "te_localise.hip", "te_robust.hip", "te_faithful.hip",
              "te_perturb.hip", "te_classes.hip", "te_common.h"]
# fp32 pair -> packed bf16, however the result is named.  (The relprop kernels round their split planes with the same
# builtin; te_x6.h owns those.)
BF16_PAIR_ROUNDING = r"__builtin_convertvector\s*\([^;]*?\bbf16x2\s*\)"

# the launchers another translation unit calls live in these namespaces (and one free function)
LAUNCHER_NAMESPACES = ["te_attn_mfma", "te_attn_rules", "te_attn_kb", "te_attn_rc", "te_attn_fwd6", "te_attn_fwd6l", "te_attn_bwd6l", "te_attn_long"]


def definitions(sources, pattern):
    """[(file, count)] of the files in which `pattern` matches"""
    found = [(name, len(re.findall(pattern, text))) for name, text in sources.items()]
    return [(name, n) for name, n in found if n]


def declaration_blocks(sources, namespace):
    """files with a `namespace <namespace> { ... }` block that only declares (no brace inside: no function body, no nested
    namespace), once per such block"""
    out = []
    for name, text in sources.items():
        for m in re.finditer(r"\bnamespace\s+%s\s*\{" % namespace, text):
            depth, i = 1, m.end()
            while depth and i < len(text):
                depth += {"{": 1, "}": -1}.get(text[i], 0)
                i += 1
            if "{" not in text[m.end():i - 1]:
                out.append(name)
    return out


@pytest.mark.parametrize("what,pattern", PRIMITIVES, ids=[p[0] for p in PRIMITIVES])
def test_shared_primitive_is_defined_once_in_a_header(what, pattern):
    found = definitions(_sources(), pattern)
    assert len(found) == 1 and found[0][1] == 1, f"{what}: expected ONE definition in csrc/, found {found}"
    assert found[0][0].endswith(".h"), f"{what} is defined in {found[0][0]}, not in a header"


@pytest.mark.parametrize("namespace", LAUNCHER_NAMESPACES)
def test_cross_file_launchers_are_declared_in_one_header(namespace):
    blocks = declaration_blocks(_sources(), namespace)
    assert len(blocks) == 1, f"declaration-only `namespace {namespace} {{...}}` blocks: {blocks} (expected one, in one header)"
    assert blocks[0].endswith(".h"), f"`namespace {namespace}` is declared by hand in {blocks[0]}"


def test_zb_cpass_launcher_is_declared_in_one_header():
    sources = _sources()
    decl = definitions(sources, r"\bte_internal_zb_cpass_tiled\s*\([^)]*\)\s*;")
    assert len(decl) == 1 and decl[0][1] == 1 and decl[0][0].endswith(".h"), decl
    # (a call ends in `)` inside an expression; a definition in `) {`)
    assert [n for n, _ in definitions(sources, r"\bbool\s+te_internal_zb_cpass_tiled\s*\([^)]*\)\s*\{")] == ["te_linear.hip"]


def test_no_more_than_three_new_headers_beside_te_common():
    headers = sorted(n for n in _sources() if n.endswith(".h"))
    assert "te_common.h" in headers and len(headers) <= 6, headers      # te_common.h, te_attn_l6.h, te_internal.h + at most three


def sort_pass_loops(sources):
    """the .hip files that call match_digit or block_exclusive_scan themselves: te_block_sort_passes is their only user, so
    such a file carries a pass loop of its own"""
    return [name for name, text in sources.items()
            if name.endswith(".hip") and re.search(r"\b(?:match_digit|block_exclusive_scan)\s*\(", text)]


def test_no_kernel_file_has_a_sort_pass_loop_of_its_own():
    assert sort_pass_loops(_sources()) == []


def test_evaluation_kernels_round_bf16_pairs_in_one_place():
    sources = _sources()
    found = definitions({name: sources[name] for name in EVALUATION}, BF16_PAIR_ROUNDING)
    assert found == [("te_common.h", 1)], found


def test_the_check_sees_a_pasted_copy():
    """The check itself: a second `split3_pk`, a retyped `Strided`, a hand-typed launcher block, a second sort pass loop, a
    renamed element load and a hand-spelled bf16 rounding in a .hip file are found."""
    sources = _sources()
    planted = dict(sources)
    planted["te_new_kernel.hip"] = """
#include "te_common.h"
namespace te_attn_kb {
bool supported(int64_t B, int64_t H, int64_t N, int64_t D);
}
namespace {
struct Strided {
  int64_t sb, sh, sn;
};
__device__ __forceinline__ void split3_pk(float x0, float x1, unsigned (&p)[3]) {}
__device__ __forceinline__ double new_value(const float* p, int64_t i) { return (double)p[i]; }
__device__ __forceinline__ double new_value(const te_bf16_t* p, int64_t i) {
  return (double)__uint_as_float((uint32_t)p[i] << 16);
}
__global__ void new_rank_kernel(uint64_t* src, uint64_t* dst, uint32_t n) {
  __shared__ uint32_t cnt[2][256 * 16], wtot[16];
  for (int pass = 0; pass < 4; ++pass) {
    uint32_t off = block_exclusive_scan(cnt[pass & 1][threadIdx.x], wtot);
    const uint64_t m = match_digit((uint32_t)(src[threadIdx.x] >> (32 + 8 * pass)) & 0xffu, threadIdx.x < n);
    dst[off + __popcll(m)] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{0.0f, 1.0f}, bf16x2));
  }
}
}
"""
    by_name = dict(PRIMITIVES)
    assert len(definitions(sources, by_name["split3_pk"])) == 1
    assert len(definitions(planted, by_name["split3_pk"])) == 2
    assert len(definitions(planted, by_name["struct Strided"])) == 2
    assert "te_new_kernel.hip" in declaration_blocks(planted, "te_attn_kb")
    assert sort_pass_loops(planted) == ["te_new_kernel.hip"]
    for overload in ("te_load_f64 (fp32)", "te_load_f64 (bf16)"):
        assert len(definitions(sources, by_name[overload])) == 1
        assert len(definitions(planted, by_name[overload])) == 2
    assert ("te_new_kernel.hip", 1) in definitions(planted, BF16_PAIR_ROUNDING)
    # a namespace block that DEFINES its launchers (the owning .hip file) is not a declaration block
    assert "te_attn_kb.hip" not in declaration_blocks(sources, "te_attn_kb")
