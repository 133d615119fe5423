"""Loader for the C++ host runtime module `_oninative` (CSV parser, formatters, lda-c reference)."""
from __future__ import annotations

import importlib
import os
import sys

_LIB = None
_ERR = None


def lib():
    global _LIB, _ERR
    if _LIB is None:
        here = os.path.join(os.path.dirname(os.path.dirname(__file__)), "_lib")
        if here not in sys.path:
            sys.path.insert(0, here)
        try:
            _LIB = importlib.import_module("_oninative")
        except Exception as e:
            _ERR = e
            raise RuntimeError(
                f"oni_ml_amd native runtime (_oninative) is not built or failed to load: {e!r}. "
                "Run `python -m oni_ml_amd._build`.") from e
        apply_thread_budget()
    return _LIB


def apply_thread_budget() -> None:
    """The native pools' default thread count (a call that passes no ``threads``) = this rank's budget
    (knobs.threads: ONI_THREADS, else the CPUs bound to the rank within the cgroup quota); re-applied by
    utils/hostres.bind_rank once the rank is pinned."""
    if _LIB is None or not hasattr(_LIB, "set_default_threads"):
        return
    from .. import knobs
    n = int(knobs.threads(16))
    _LIB.set_default_threads(n, False)
    if hasattr(_LIB, "set_background_pool"):
        _LIB.set_background_pool(max(1, n - WRITER_RESERVE))   # every background writer's threads, together


# CPUs a background writer leaves to the rank's other threads (the one driving the GPU, the HIP runtime's):
# a writer that takes the whole cgroup quota throttles the GPU-driving thread with it
WRITER_RESERVE = 2


def background_thread_budget(share: int = 1) -> None:
    """Called on a background writer thread: marks it as one (its native calls then draw their worker
    threads from the process-wide background pool of budget - WRITER_RESERVE tokens, shared by every
    writer running at the time) and asks for at most (budget - WRITER_RESERVE) / ``share`` of them."""
    if _LIB is None:
        lib()
    from .. import knobs
    _LIB.set_default_threads(max(1, (int(knobs.threads(16)) - WRITER_RESERVE) // max(1, share)), True)


def engine_plan_bound(D: int, V: int, nnz: int, team8_lo: int, xcds: int = 8) -> int:
    """Upper bound of ``engine_plan``'s buffer bytes for a corpus of these sizes."""
    return int(lib().engine_plan_bound(int(D), int(V), int(nnz), int(team8_lo), int(xcds)))


def engine_plan(doc_ptr, word_idx, counts, V: int, KS: int, U: int, buf, *, edges, tiny_variant: int,
                team8_variant: int, tiny: int, heavy: int, light: int, late_share: float, suff_split: str,
                stage_cap: float, umax: int, iso_m: int, xcds: int, defer_final: bool, threads: int = 0) -> dict:
    """The fp64 engine's host plans (csrc/native/engine_plan.cpp) from the host CSR (int64 ``doc_ptr``, int32
    ``word_idx``, int64 ``counts``) into ``buf`` (uint8 numpy array, 256-byte aligned, at least
    ``engine_plan_bound`` bytes), in one call.  Every threshold is an argument, passed by the caller from the
    Python definition that owns it (ops/hip.py ``engine_plan_thresholds``).  ``edges``: (variant, lo, hi) per
    bucket, None = the tiny bound / no upper edge.  Returns the section table {name: (byte offset, elements,
    bytes per element)}, the buckets [(variant, byte offset, elements)], the host copies ``doc_len`` /
    ``word_len`` and the plan's counts and flags."""
    e = [(int(v), -1 if lo is None else int(lo), -1 if hi is None else int(hi)) for v, lo, hi in edges]
    mode = {"off": 0, "auto": 1, "force": 2}[suff_split]
    return lib().engine_plan(doc_ptr, word_idx, counts, int(V), int(KS), int(U), e, int(tiny_variant),
                             int(team8_variant), int(tiny), int(heavy), int(light), float(late_share), mode,
                             float(stage_cap), int(umax), int(iso_m), int(xcds), bool(defer_final), buf, int(threads))


ASSIGN_NAN_COST = 2.0      # what a NaN cost counts as in assign_min: above any total-variation distance


def assign_min(cost):
    """The permutation of least total cost (csrc/native/assign.h, an O(n^3) shortest-augmenting-path Hungarian
    method): ``cost`` square float64 [n, n], every entry finite or NaN; returns int64 [n], ``match[i]`` the column
    of row i.  A NaN cost counts as ``ASSIGN_NAN_COST``.  Deterministic: the scans run in column order with strict
    comparisons, so the same input bits give the same permutation.  A rectangular problem is padded to square with
    0.0-cost dummy rows / columns by the caller."""
    import numpy as np
    c = np.ascontiguousarray(cost, np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"assign_min: cost must be square [n, n], got shape {c.shape}")
    return lib().assign_min(c, ASSIGN_NAN_COST)


def available() -> bool:
    try:
        lib()
        return True
    except RuntimeError:
        return False
