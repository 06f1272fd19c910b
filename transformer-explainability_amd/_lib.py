"""ctypes binding of libte_relprop.so: the C ABI exactly as include/te_relprop.h declares it.

Nothing about the ABI is restated here.  ``_cabi`` reads the header this tree ships (the one ``te_build_id()`` vouches
for) and ``SIGNATURES`` (name -> (restype, [argtypes])), ``PARAMS`` (name -> parameter names) and every ``TE_*``
integer constant of this module are what it found there: a new entry point is declared in the header, defined in csrc/
and called in ops.py, and is bound without a line in this file.

The product path has NO CPU fallback: if the shared library is missing, or no gfx950 device is
visible when an op is called, this module raises -- loudly.  PyTorch is imported first so that the
library binds to the HIP runtime torch already loaded (one libamdhip64 per process).
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (must precede dlopen of libte_relprop: loads torch's libamdhip64 first)

from . import _cabi
from ._buildid import INCLUDE

_PKG = os.path.dirname(os.path.abspath(__file__))
# (TE_RELPROP_LIB: measurement builds of the same sources under another name, e.g. an A/B of two -D variants in one process tree)
LIB_PATH = os.environ.get("TE_RELPROP_LIB") or os.path.join(_PKG, "lib", "libte_relprop.so")

MIN_LIB_VERSION = 800      # te_version(): 0.8.0, argument lists changed under existing names (one entry point per rule, optional operands NULL)

_PROTOTYPES, CONSTANTS = _cabi.load(os.path.join(INCLUDE, "te_relprop.h"))
SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in _PROTOTYPES.items()}
PARAMS = {name: tuple(p for p, _ in params) for name, (_, params) in _PROTOTYPES.items()}
globals().update(CONSTANTS)      # TE_OK, TE_ERR_*, TE_VARIANT_*, TE_X6_*, ...: importable from here, valued by the header


class TeError(RuntimeError):
    pass


_lib = None


def hip_runtimes_loaded():
    """Distinct libamdhip64 images mapped into this process (must be exactly one on a GPU box)."""
    seen = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    seen.add(line.split()[-1])
    except OSError:
        pass
    return sorted(seen)


def load():
    """dlopen libte_relprop.so and attach argtypes.  Raises TeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise TeError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            f"(python transformer-explainability_amd/build.py or __graft_entry__.build()); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.te_version() < MIN_LIB_VERSION:      # a stale in-tree build: argument lists changed (x6 flags / status words)
        raise TeError(f"{LIB_PATH} is version {lib.te_version()}, this package needs >= {MIN_LIB_VERSION}: rebuild it "
                      f"(python transformer-explainability_amd/build.py --force)")
    # provenance: the library must have been built from the sources of THIS tree (the prebuilt in-tree .so is what reaches the
    # GPU box; mtimes prove nothing there).  TE_RELPROP_LIB / TE_ALLOW_STALE_LIB=1: measurement builds of other sources.
    from ._buildid import source_hash
    bid = (lib.te_build_id() or b"").decode()
    want = source_hash()
    if bid.split("-")[0] != want and not (os.environ.get("TE_RELPROP_LIB") or os.environ.get("TE_ALLOW_STALE_LIB") == "1"):
        raise TeError(f"{LIB_PATH} was built from other sources (te_build_id() = {bid!r}, this tree hashes to {want!r}): "
                      f"rebuild it (python transformer-explainability_amd/build.py)")
    _lib = lib
    return lib


def build_id() -> str:
    """te_build_id() of the loaded library: '<source hash>-<flags hash>' (see _buildid.py)."""
    return (load().te_build_id() or b"").decode()


def check(status: int, what: str):
    if status != TE_OK:  # noqa: F821  (from the header, like every TE_* of this module)
        msg = load().te_status_string(status)
        raise TeError(f"{what} failed with status {status}: {msg.decode() if msg else '?'}")


def require_device():
    """Raise unless a gfx950 device is usable through the same HIP runtime torch uses."""
    if not torch.cuda.is_available():
        raise TeError("no HIP device visible to PyTorch: the relprop hot path runs only on MI355X (gfx950); "
                      "there is no CPU fallback")
    lib = load()
    rts = hip_runtimes_loaded()
    if len(rts) > 1:
        raise TeError(f"two HIP runtimes are mapped into this process: {rts}; import torch before loading "
                      f"libte_relprop so that both share torch's libamdhip64")
    check(lib.te_device_check(), "te_device_check")
