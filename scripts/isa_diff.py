#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, one translation unit at a time.

    python scripts/isa_diff.py OLD_TREE NEW_TREE [FILE.hip ...]

A refactor of csrc/ (helpers moved between files, headers split or merged) must not change a single instruction.  For every
entry of build.SOURCES (or only the files named) both trees' file is compiled with build.CXXFLAGS plus
`--cuda-device-only -S`, and the two listings are compared after a normalisation that removes what names alone change:

  * `__hip_cuid_<hex>` (a hash of the input path and content) becomes `__hip_cuid_X`;
  * every distinct mangled symbol `_Z...` becomes `SYM<k>`, numbered in order of first appearance: moving a parameter type
    such as `Strided` out of an anonymous namespace renames the kernel and changes nothing else.

One line per file: lines, sha256 of the old and of the new normalised listing, `same` / `DIFFERENT` (`new`: a file OLD_TREE
does not have).  A differing file gets a second line that says how it differs (`classify`): whether the line counts agree, how
many lines only have the source operands of a commutative integer opcode in another order, and how many differ otherwise; and a
third line that compares the files function by function (`gained_only`): a file that only gained kernels keeps the instructions
of every function it had.  Exit status 1 on any difference (the normalised listings of a differing file are kept in --keep DIR for `diff`).  Flags and the file list are the
flags and the list of NEW_TREE's build.py.
"""
import argparse
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "transformer-explainability_amd"
MAX_JOBS = 16


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_te_build", os.path.join(tree, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def normalise(text):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    names = {}
    return re.sub(r"_Z[A-Za-z0-9_]+", lambda m: names.setdefault(m.group(0), "SYM%d" % len(names)), text)


COMMUTATIVE = ("v_add_u32", "v_add3_u32", "v_add_co_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_and_b32", "v_or_b32", "v_xor_b32",
               "s_add_u32", "s_add_i32", "s_and_b32", "s_and_b64", "s_or_b32", "s_or_b64", "s_xor_b32", "s_xor_b64")


def classify(old, new):
    """How two normalised listings differ, line by line: None if their line counts differ; else ({opcode: lines that have the
    same opcode, the same destination and the same source operands in another order (commutative integer opcodes only)},
    the number of lines that differ in any other way)."""
    a, b = old.split("\n"), new.split("\n")
    if len(a) != len(b):
        return None
    swapped, other = {}, 0
    for x, y in zip(a, b):
        if x == y:
            continue
        px, py = x.split(None, 1), y.split(None, 1)
        if len(px) == 2 and len(py) == 2 and px[0] == py[0] and px[0].split("_e32")[0].split("_e64")[0] in COMMUTATIVE:
            ox, oy = ([s.strip() for s in p[1].split(",")] for p in (px, py))
            if ox[0] == oy[0] and sorted(ox[1:]) == sorted(oy[1:]):
                swapped[px[0]] = swapped.get(px[0], 0) + 1
                continue
        other += 1
    return swapped, other


def kernels(text):
    """The instruction text of every function of a normalised listing (label .. .Lfunc_end), without comments, with the
    symbol, block and function numbers that depend on the function's position in the file removed."""
    out, cur = [], None
    for line in text.split("\n"):
        if cur is None:
            if re.match(r"^SYM\d+:", line):
                cur = []
        elif re.match(r"^\.Lfunc_end\d+:", line):
            out.append("\n".join(cur))
            cur = None
        else:
            line = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"SYM\d+", "SYM", line.split(";")[0])).strip()
            if line:
                cur.append(line)
    return out


def gained_only(old, new):
    """(functions in old, in new, functions of old whose instructions no function of new has): a file that only GAINED
    kernels has 0 in the last place."""
    ko, kn = kernels(old), kernels(new)
    left = list(kn)
    missing = 0
    for k in ko:
        if k in left:
            left.remove(k)
        else:
            missing += 1
    return len(ko), len(kn), missing


def listing(build, tree, src, out):
    csrc = os.path.join(tree, PKG, "csrc")
    cmd = [build._hipcc(), *build.CXXFLAGS, "--cuda-device-only", "-S", "-I", os.path.join(tree, "include"), "-I", csrc,
           os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s of %s:\n%s" % (src, tree, r.stdout))
    with open(out) as f:
        return normalise(f.read())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("files", nargs="*", help="entries of build.SOURCES (default: all)")
    ap.add_argument("--keep", metavar="DIR", help="write the normalised listings of differing files here")
    ap.add_argument("-j", type=int, default=min(MAX_JOBS, os.cpu_count() or 1))
    a = ap.parse_args()
    old_tree, new_tree = os.path.abspath(a.old_tree), os.path.abspath(a.new_tree)
    build = load_build(new_tree)
    sources = a.files or build.SOURCES
    unknown = [s for s in sources if s not in build.SOURCES]
    if unknown:
        sys.exit("not in build.SOURCES: " + " ".join(unknown))
    # a translation unit that only NEW_TREE has (a new kernel file) is reported as `new`: there is nothing to compare it with
    added = [s for s in sources if not os.path.exists(os.path.join(old_tree, PKG, "csrc", s))]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max(1, min(a.j, MAX_JOBS))) as pool:
        jobs = {(side, s): pool.submit(listing, build, tree, s, os.path.join(tmp, "%s_%s.s" % (side, s)))
                for s in sources for side, tree in (("old", old_tree), ("new", new_tree)) if not (side == "old" and s in added)}
        different = 0
        print("%-22s %8s  %-16s %-16s" % ("file", "lines", "sha256 old", "sha256 new"))
        for s in sources:
            if s in added:
                new = jobs["new", s].result()
                print("%-22s %8d  %-16s %-16s new" % (s, new.count("\n"), "-", hashlib.sha256(new.encode()).hexdigest()[:16]), flush=True)
                continue
            old, new = jobs["old", s].result(), jobs["new", s].result()
            h_old, h_new = (hashlib.sha256(t.encode()).hexdigest()[:16] for t in (old, new))
            same = old == new
            different += not same
            print("%-22s %8d  %-16s %-16s %s" % (s, new.count("\n"), h_old, h_new, "same" if same else "DIFFERENT"), flush=True)
            if not same:
                kind = classify(old, new)
                print("    " + ("the listings have different numbers of lines" if kind is None else
                                "same number of lines; lines with the same opcode and destination and the source operands of a "
                                "commutative integer opcode in another order: %s; lines that differ in any other way: %d"
                                % (dict(sorted(kind[0].items())) or "none", kind[1])), flush=True)
                n_old, n_new, missing = gained_only(old, new)
                print("    functions: %d before, %d after; functions of the old listing whose instructions no function of the "
                      "new listing has: %d%s" % (n_old, n_new, missing, " (the file only gained functions)"
                                                  if missing == 0 and n_new > n_old else ""), flush=True)
            if not same and a.keep:
                os.makedirs(a.keep, exist_ok=True)
                for side, t in (("old", old), ("new", new)):
                    with open(os.path.join(a.keep, "%s.%s.s" % (s, side)), "w") as f:
                        f.write(t)
    print("%d of %d translation units differ%s" % (different, len(sources) - len(added),
                                                   ", %d new" % len(added) if added else ""))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
