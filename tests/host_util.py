"""Helpers shared by tests that need no device: the built library, the C ABI's host-side refusals, bit comparison.

Belongs here: what several test files would otherwise paste from one another and what runs on a host without a GPU --
the ``lib`` fixture, ``status`` / ``header_args`` for the entry-point tests, ``free_port`` for the process-group tests,
``bits`` / ``same_bits`` for bit-for-bit comparisons and ``one_hot``.  The -m gpu files take the last three from here as
well.  This module imports ``torch``, ``pytest`` and the standard library only; the package is imported inside the
functions, so that collection never loads it.

Does not belong here: tolerances, shapes, expected values and inputs (they stay in the test files and the *_inputs
modules), anything that touches a device (gpu_util.py), and the three-line lazy importers ``te()`` / ``ops()`` / ...
"""
import os
import re
import socket

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from transformer_explainability_amd import _lib
    return _lib.load()


def status(lib, fn, base, **changed):
    """The status ``fn`` returns for the arguments ``base`` with ``changed`` replaced (argument order is base's)."""
    assert set(changed) <= set(base), changed
    return getattr(lib, fn)(*{**base, **changed}.values())


def header_args(name):
    """Number of arguments the header declares for ``name``."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "te_relprop.h")).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", header)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def bits(t):
    """t on the host as the integers of its elements' bytes (1, 2, 4 or 8 bytes wide)"""
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    """Bit for bit: equal dtype, equal shape, equal bytes -- -0.0 is not +0.0, and a NaN equals itself."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.detach().cpu().reshape(-1).contiguous().view(torch.uint8), b.detach().cpu().reshape(-1).contiguous().view(torch.uint8))


def one_hot(logits, dtype=torch.float32, device=None):
    """[B,C] of ``dtype`` with a one at every row's largest logit, made on ``device`` (default: where the logits are)"""
    device = logits.device if device is None else device
    oh = torch.zeros(logits.shape, dtype=dtype, device=device)
    oh.scatter_(1, logits.detach().float().to(device).argmax(-1, keepdim=True), 1.0)
    return oh
