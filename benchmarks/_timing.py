"""The timing protocols of the benchmark scripts, defined once.

Belongs here: what every script measures alike -- the two kinds of timed window, the alternation of the versions, the
median / min / max row of a leg, and the two memory rates of the part that the bandwidth shares are taken against.

  * ``wall_window``: the WALL-WINDOW protocol.  Host clock between two device synchronisations, calls until a least
    duration has passed.  For calls that read results back or are bound by their own host work.
  * ``event_window``: the EVENT-WINDOW protocol.  HIP events around a fixed number of calls, ended by a synchronise.  For
    pure device work.
  * ``alternate``: every version warmed, then ``rounds`` rounds in which each version gets one window, in dict order.

Does not belong here: anything that differs between scripts because their protocol differs (``_pair``, ``_verdict``,
``_report``, ``_shares``), inputs, models (see _models.py) and anything that imports the package.  This module imports
``time``, ``statistics`` and ``torch`` only.
"""
from __future__ import annotations

import statistics
import time

import torch

# MI355X: the HBM peak of the data sheet, and the copy rate measured on the part itself, the practical ceiling of a streaming
# kernel (DESIGN.md quotes both beside the curve, robustness and faithfulness tables)
HBM_BYTES_PER_S = 8e12
MEASURED_COPY_BYTES_PER_S = 6.29e12


# decided once, so that a timed window on a device makes exactly the calls it always made; without a device (the host tests of
# this module) there is nothing to wait for.  The scripts refuse to run without a device before they time anything.
_synchronize = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)


def wall_window(fn, min_s):
    """seconds per call over a window of at least min_s (and at least one call)"""
    _synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= min_s:
            break
    _synchronize()
    return (time.perf_counter() - t0) / n


def event_window(fn, n):
    """seconds per call over n calls between two HIP events, ended by a synchronise"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / n


def alternate(fns, rounds, window, warmup):
    """{name: [window(fn) of each of `rounds` rounds]}: every version warmed first, then the versions taking turns.
    ``window`` is a callable fn -> seconds, e.g. ``functools.partial(wall_window, min_s=0.2)``."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    _synchronize()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(window(fn))
    return times


def summary(ts, scale=1e6, unit="us", digits=2):
    return {f"median_{unit}": round(statistics.median(ts) * scale, digits), f"min_{unit}": round(min(ts) * scale, digits),
            f"max_{unit}": round(max(ts) * scale, digits), "windows": len(ts)}
