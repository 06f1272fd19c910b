"""What a C header declares, as ctypes needs it: the prototypes of the te_* entry points and the integer constants.

``_lib`` binds libte_relprop.so from ``parse()`` of include/te_relprop.h, so an argument list is written in the header, in
the definition the compiler checks against it, and at the call -- nowhere else.  The header is plain C: comments and
preprocessor lines are removed, and what is left of a prototype is ``<return type> te_name(<type> <name>, ...);``.
Anything this parser does not understand is an error that names the declaration, never a guess.  No torch import, no
import from the package: the build script, stand-alone scripts and tests load it as they load ``_buildid``."""
from __future__ import annotations

import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

# by value; every pointer is a c_void_p (a `const char*` result: c_char_p)
CTYPES = {"int": c_int, "int64_t": c_int64, "size_t": c_size_t, "float": c_float, "double": c_double,
          "te_stream_t": c_void_p}

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_NAME = re.compile(r"\b(te_[a-z0-9_]+)\s*\(")
_ARGS = re.compile(r"\(([^(){};]*)\)\s*;")
_PARAM = re.compile(r"(.*[\s*])(\w+)", re.S)
_ENUM = re.compile(r"\benum\b[^{;]*\{([^}]*)\}")
_DEFINE = re.compile(r"#\s*define\s+(TE_\w+)\b(?!\()(.*)")
_INT = r"-?(?:0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)"
_EXPR = re.compile(rf"({_INT})(?:\s*<<\s*({_INT}))?")


class HeaderError(ValueError):
    pass


def _ctype(ctype: str, decl: str, result: bool = False):
    words = ctype.replace("*", " * ").split()
    if "*" in words:
        return c_char_p if result and [w for w in words if w != "const"] == ["char", "*"] else c_void_p
    words = [w for w in words if w != "const"]
    if len(words) != 1 or words[0] not in CTYPES:
        raise HeaderError(f"{decl}: unknown {'return' if result else 'parameter'} type {ctype!r}")
    return CTYPES[words[0]]


def _integer(expr: str, decl: str) -> int:
    """literal | literal << literal, optionally in one pair of parentheses; literals are decimal or hex, maybe negative"""
    text = expr.strip()
    if text.startswith("(") and text.endswith(")"):
        text = text[1:-1].strip()
    m = _EXPR.fullmatch(text)
    if not m:
        raise HeaderError(f"{decl}: {expr.strip()!r} is not an integer constant this parser evaluates")
    value, shift = (int(g, 0) if g else None for g in m.groups())
    return value if shift is None else value << shift


def parse(text: str):
    """-> (prototypes, constants): name -> (restype, [(parameter name, ctypes type), ...]) and NAME -> int"""
    text = _COMMENT.sub(" ", text)
    lines = text.split("\n")
    code = "\n".join(line for line in lines if not line.lstrip().startswith("#"))

    constants = {}
    for line in lines:
        m = _DEFINE.match(line.strip())
        if m and m.group(2).strip():                         # a define without a value (the include guard) is no constant
            constants[m.group(1)] = _integer(m.group(2), f"#define {m.group(1)}")
    for body in _ENUM.findall(code):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, eq, expr = (p.strip() for p in item.partition("="))
            value = _integer(expr, f"enumerator {name}") if eq else value + 1
            constants[name] = value

    prototypes = {}
    for m in _NAME.finditer(code):
        name = m.group(1)
        start = max(code.rfind(c, 0, m.start()) for c in ";{}") + 1
        args = _ARGS.match(code, m.end() - 1)
        if not args:
            raise HeaderError(f"{name}: not a prototype of the form `type {name}(type name, ...);`")
        if name in prototypes:
            raise HeaderError(f"{name}: declared twice")
        params = []
        for p in (p.strip() for p in args.group(1).split(",")):
            if p in ("", "void") and "," not in args.group(1):
                break
            pm = _PARAM.fullmatch(p)
            if not pm:
                raise HeaderError(f"{name}: parameter {p!r} is not `type name`")
            params.append((pm.group(2), _ctype(pm.group(1), f"{name}, parameter {pm.group(2)}")))
        prototypes[name] = (_ctype(code[start:m.start()], name, result=True), params)
    return prototypes, constants


def load(path: str):
    with open(path) as f:
        return parse(f.read())
