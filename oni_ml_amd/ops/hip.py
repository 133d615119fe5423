"""Loader + validated launch wrappers for the gfx950 HIP kernels (`_onihip`).

Every wrapper checks dtype / device / contiguity / shape on the host before it
hands raw addresses to the kernel (a wrong shape on a hand-written kernel can
fault the whole GPU), then launches on torch's current stream so the launch is
ordered with torch work and capturable in a hipGraph.

On a machine with a GPU the extension is mandatory: :func:`lib` raises if it
cannot be imported instead of silently falling back to eager torch.
"""
from __future__ import annotations

import importlib
import os
import sys
from typing import Optional

import torch

from .. import config as _CFG      # GROUP_BLOCK, EXPLAIN_MAX_FIELDS: read at every call, one constant for kernel and twin

_LIB = None
_ERR = None


def _import():
    global _LIB, _ERR
    if _LIB is not None or _ERR is not None:
        return
    try:
        here = os.path.join(os.path.dirname(os.path.dirname(__file__)), "_lib")
        if here not in sys.path:
            sys.path.insert(0, here)
        _LIB = importlib.import_module("_onihip")
    except Exception as e:  # pragma: no cover - depends on build state
        _ERR = e


def available() -> bool:
    _import()
    return _LIB is not None and torch.cuda.is_available()


def lib():
    """Return the extension module; raise loudly if it is missing."""
    _import()
    if _LIB is None:
        raise RuntimeError(
            "oni_ml_amd HIP extension (_onihip) is not built or failed to load: "
            f"{_ERR!r}. Run `python -m oni_ml_amd._build` (needs hipcc, gfx950)."
        )
    return _LIB


def compiled_ks():
    return list(lib().compiled_ks())


def padded_topics(K: int) -> int:
    """Smallest compiled row stride >= K (multiple of 4)."""
    for ks in (8, 12, 16, 20, 24, 32, 52, 64, 100, 128):
        if ks >= K:
            return ks
    raise ValueError(f"K={K} exceeds the largest compiled topic count (128)")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, dtype, name, shape=None, device=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a GPU tensor")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)} != {tuple(shape)}")
    return t.data_ptr()


PARAM_COUNT = 8      # device parameter block (csrc/hip/kernels.h kParamCount)
PARAM_DONE = 4       # params[PARAM_DONE] != 0: the EM loop converged, kernels skip
HIST_COLS = 6        # em_control history row: likelihood, conv, alpha, VAR_MAX_ITER, alpha_ss, -


def _params_ptr(params, dev) -> int:
    return 0 if params is None else _chk(params, torch.float64, "params", (PARAM_COUNT,), dev)


def _gate_ptr(gate, dev) -> int:
    """Pointer to a float64 flag (e.g. params[PARAM_DONE:PARAM_DONE+1]) or 0."""
    return 0 if gate is None else _chk(gate, torch.float64, "gate", (1,), dev)


def argsort_desc_stable(keys):
    """np.argsort(-keys, kind="stable") for non-negative integer keys, as numpy's O(n) radix sort on
    16-bit digits (one pass below 2^16, two below 2^32): the length plans are inside the engine
    setup, which bench.py's to-convergence clock includes (4x faster on 124 k document lengths)."""
    import numpy as np
    k = np.asarray(keys, np.int64)
    if k.size == 0:
        return np.zeros(0, np.int64)
    m = int(k.max())
    if int(k.min()) < 0 or m >= 1 << 32:
        return np.argsort(-k, kind="stable")
    r = m - k
    if m < 1 << 16:
        return np.argsort(r.astype(np.uint16), kind="stable")
    o = np.argsort((r & 0xFFFF).astype(np.uint16), kind="stable")
    return o[np.argsort((r[o] >> 16).astype(np.uint16), kind="stable")]


class SuffPlan:
    """Word order for the single-launch suff-stats kernel (gs_suff64): [heavy | medium | light] (heavy first).

    ``words``: restrict the plan to these word ids (a sub-plan; several sub-plans must together
    cover the vocabulary, since every word's class_word row is written by exactly one launch)."""
    HEAVY, LIGHT = 1024, 64

    def __init__(self, word_len, device, words=None):
        import numpy as np
        wl = np.asarray(word_len)
        ids = np.arange(wl.size, dtype=np.int64) if words is None else np.asarray(words, np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= wl.size):
            raise ValueError("suff sub-plan word ids out of range")
        self.covers_all = words is None
        order = ids[argsort_desc_stable(wl[ids])].astype(np.int32)
        L = wl[order]
        self.n_heavy = int((L > self.HEAVY).sum())
        self.n_medium = int(((L > self.LIGHT) & (L <= self.HEAVY)).sum())
        self.n_light = int((L <= self.LIGHT).sum())
        self.order = torch.from_numpy(order).to(device)
        self.n_blocks = int(lib().suff_fused_blocks(self.n_heavy, self.n_medium, self.n_light))

    @classmethod
    def from_arrays(cls, order, n_heavy: int, n_medium: int, n_light: int) -> "SuffPlan":
        """A whole-vocabulary plan from an order already on the device (the native engine plan's)."""
        self = cls.__new__(cls)
        self.covers_all = True
        self.n_heavy, self.n_medium, self.n_light = int(n_heavy), int(n_medium), int(n_light)
        self.order = order
        self.n_blocks = int(lib().suff_fused_blocks(self.n_heavy, self.n_medium, self.n_light))
        return self


def _scalar_slice(scalars, D, dev):
    if scalars is None:
        return 0, 0, 0, 0
    lik, ass, lo, hi = scalars
    if not 0 <= lo <= hi <= D:
        raise ValueError(f"scalar slice [{lo}, {hi}) outside [0, {D}]")
    return (_chk(lik, torch.float64, "lik", (D,), dev), _chk(ass, torch.float64, "alpha_ss", (D,), dev),
            int(lo), int(hi))


def rows_accumulate(rows, ptr, src, own, recv, out):
    """out[rows[i]] = 0 + sum over j in [ptr[i], ptr[i+1]) of (own[rows[i]] if src[j] < 0 else recv[src[j]]),
    fp64, in j order (parallel/dist.py VocabExchange.accumulate)."""
    dev = out.device
    V, W = out.shape
    n = rows.numel()
    if n == 0:
        return
    # ptr / src are built and bounds-checked once on the host (VocabExchange.__init__)
    lib().rows_accumulate(_chk(rows, torch.int32, "rows", (n,), dev), _chk(ptr, torch.int32, "ptr", (n + 1,), dev),
                          _chk(src, torch.int32, "src", None, dev), _chk(own, torch.float64, "own", (V, W), dev),
                          _chk(recv, torch.float64, "recv", None, dev), _chk(out, torch.float64, "out", (V, W), dev),
                          int(n), int(W), _stream())


def init_random_ss(cw, K, seed):
    """cw [V, KS] float64 <- lda-c random start 1/V + u(seed, k V + w) (native ``random_ss`` bits)."""
    V, KS = cw.shape
    lib().init_random_ss(_chk(cw, torch.float64, "cw", (V, KS), cw.device), int(V), int(K), int(KS),
                         int(seed) & 0xFFFFFFFFFFFFFFFF, _stream())


def log_beta_t(cw, class_total, K: int, floor: float, out=None):
    """[K, V] float64 log(cw[:, k]) - log(class_total[k]) (``floor`` where cw == 0) of a [V, KS] class_word: the
    saved log beta in file order (csrc/hip/reduce.hip log_beta_t_kernel; bitwise torch's transpose / log / where)."""
    dev = cw.device
    V, KS = cw.shape
    if not (0 < K <= KS):
        raise ValueError(f"log_beta_t: K={K} outside 1..{KS}")
    p_cw = _chk(cw, torch.float64, "cw", (V, KS), dev)
    p_ct = _chk(class_total, torch.float64, "class_total", None, dev)
    if class_total.numel() < K:
        raise ValueError(f"log_beta_t: class_total holds {class_total.numel()} < K = {K} values")
    if out is None:
        out = torch.empty((K, V), dtype=torch.float64, device=dev)
    p_out = _chk(out, torch.float64, "out", (K, V), dev)
    lib().log_beta_t(p_cw, int(V), int(K), int(KS), p_ct, float(floor), p_out, _stream())
    return out


def colsum_partials(part, n_blocks, out, gate=None):
    """out[k] = sum_b part[b, k] for b < n_blocks (deterministic order)."""
    dev = part.device
    cols = part.shape[1]
    if n_blocks > part.shape[0]:
        raise ValueError("n_blocks exceeds partial rows")
    lib().colsum_partials(_chk(part, torch.float64, "part", None, dev), int(n_blocks), int(cols),
                          _chk(out, torch.float64, "out", (cols,), dev), _gate_ptr(gate, dev), _stream())


def alpha_newton(scalars, num_docs, K, estimate, params, alpha_out):
    """Device lda-c opt_alpha: params[0:2] <- (alpha, lgamma(K alpha) - K lgamma(alpha))."""
    dev = params.device
    lib().alpha_newton(_chk(scalars, torch.float64, "scalars", (2,), dev), float(num_docs), int(K), bool(estimate),
                       _chk(params, torch.float64, "params", (PARAM_COUNT,), dev),
                       _chk(alpha_out, torch.float64, "alpha_out", (1,), dev), _stream())


def em_control(scalars, params, ctl, hist):
    """Device EM convergence test after one iteration (csrc/hip/em_control.hip)."""
    dev = params.device
    slots = hist.numel() // HIST_COLS
    lib().em_control(_chk(scalars, torch.float64, "scalars", (2,), dev),
                     _chk(params, torch.float64, "params", (PARAM_COUNT,), dev),
                     _chk(ctl, torch.float64, "ctl", (8,), dev),
                     _chk(hist, torch.float64, "hist", (slots * HIST_COLS,), dev),
                     int(slots), _stream())


def _bad(name):
    raise ValueError(f"{name}: buffer too small")


def score_events(theta, phi, K, dflt, doc_a, word_a, doc_b, word_b, tol):
    """Returns (score_a, score_b|None, key, flag) as new device tensors."""
    n = doc_a.numel()
    dev = doc_a.device
    D = theta.shape[0]
    V = phi.shape[0]
    if theta.dim() != 2 or phi.dim() != 2 or theta.shape[1] < K or phi.shape[1] < K:
        raise ValueError("theta/phi must be [*, >=K]")
    if theta.shape[1] != phi.shape[1]:
        raise ValueError("theta and phi row strides differ")
    Kr = theta.shape[1]
    if Kr != K:
        theta = theta[:, :K].contiguous()
        phi = phi[:, :K].contiguous()
    # index bounds (host check before a gather kernel touches memory)
    for name, idx, lim in (("doc_a", doc_a, D), ("word_a", word_a, V), ("doc_b", doc_b, D), ("word_b", word_b, V)):
        if idx is None:
            continue
        if idx.numel() != n:
            raise ValueError(f"{name}: length mismatch")
        if n and (int(idx.max()) >= lim or int(idx.min()) < -1):
            raise ValueError(f"{name}: index out of range")
    sa = torch.empty(n, dtype=torch.float64, device=dev)
    sb = torch.empty(n, dtype=torch.float64, device=dev) if doc_b is not None else None
    key = torch.empty(n, dtype=torch.float64, device=dev)
    flag = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return sa, sb, key, flag
    lib().score_events(
        _chk(theta, torch.float64, "theta", (D, K), dev), _chk(phi, torch.float64, "phi", (V, K), dev),
        int(K), float(dflt),
        _chk(doc_a, torch.int32, "doc_a", (n,), dev), _chk(word_a, torch.int32, "word_a", (n,), dev),
        _chk(doc_b, torch.int32, "doc_b", (n,), dev) if doc_b is not None else 0,
        _chk(word_b, torch.int32, "word_b", (n,), dev) if word_b is not None else 0,
        int(n), float(tol), sa.data_ptr(), sb.data_ptr() if sb is not None else 0, key.data_ptr(),
        flag.data_ptr(), _stream(),
    )
    return sa, sb, key, flag


from ..config import ENSEMBLE_MAX    # noqa: E402 -- largest member count; checked against kEnsembleMax at a launch


# ------------------------------------------------------- the scoring wrappers' checks ---
# One definition of every host-side rule of the wrappers below.  None of them reads from the device but
# ``_in_range`` and ``_segments_in_range``: a wrapper calls those two last, after every other check.

def _max_blocks(max_blocks):
    if not isinstance(max_blocks, int) or isinstance(max_blocks, bool) or max_blocks < 0:
        raise ValueError(f"max_blocks must be a non-negative int, got {max_blocks!r}")
    return max_blocks


def _block(who, block, default):
    """The block size of a wrapper: ``block``, or the ``config`` value when it is None."""
    import operator
    B = operator.index(default if block is None else block)
    if not 1 <= B < 1 << 31:
        raise ValueError(f"{who}: block must be >= 1 and < 2^31, got {B}")
    return B


def _scratch_mb(who, scratch_mb, default):
    """The scratch cap of a wrapper in MiB: ``scratch_mb``, or the ``config`` value when it is None."""
    cap_mb = float(default if scratch_mb is None else scratch_mb)
    if not cap_mb > 0:
        raise ValueError(f"{who}: scratch_mb must be > 0, got {scratch_mb!r}")
    return cap_mb


def _scratch_batch(n, per_item, cap_mb, tile=1):
    """How many of ``n`` items of ``per_item`` scratch bytes run at once under a cap of ``cap_mb`` MiB: at least
    one, and whole tiles of ``tile`` items where the items need more than one batch of at least a tile."""
    batch = max(1, min(n, int(cap_mb * (1 << 20)) // per_item))
    if batch < n and batch >= tile:
        batch -= batch % tile
    return batch


def _list_scratch_doubles(cells):
    """The doubles of a top-N list scratch of ``cells`` (value, row) cells: the doubles first, then the ints,
    rounded up to whole doubles."""
    return cells + (cells + 1) // 2


def _table(name, t, what, dev=None, width=None):
    """A contiguous float64 GPU table (on ``dev``, when given) of the shape ``what`` names: 2-D, or with
    ``width`` = (R, K) the 3-D one of that row width."""
    if not isinstance(t, torch.Tensor) or t.dim() != (2 if width is None else 3):
        raise ValueError(f"{name}: expected a {what} tensor")
    if t.dtype != torch.float64:
        raise ValueError(f"{name}: expected torch.float64, got {t.dtype}")
    if width is not None and tuple(t.shape[1:]) != width:
        raise ValueError(f"{name}: row width {tuple(t.shape[1:])} != (R, K) = {width}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a GPU tensor")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name}: on {t.device}, expected {dev}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")


def _table3(name, t, R, K, dev=None):
    _table(name, t, "[rows, R, K]", dev, (R, K))


def _members(who, R, K, r_max):
    """R members x K topics: ``1 <= R <= r_max`` and ``K >= 1``, or with ``r_max`` None both >= 1 and R K < 2^31."""
    if r_max is None:
        if R < 1 or K < 1 or R * K >= 1 << 31:
            raise ValueError(f"{who}: R and K must be >= 1 and R K < 2^31, got {R} x {K}")
        return
    if not 1 <= R <= r_max:
        raise ValueError(f"{who}: R must be in [1, {r_max}], got {R}")
    if K < 1:
        raise ValueError(f"{who}: K must be >= 1, got {K}")


def _tables3(who, theta, phi=None, r_max=None):
    """``theta`` [D, R, K] and, when given, ``phi`` [V, R, K] on theta's device: ``(R, K, device)``."""
    if not isinstance(theta, torch.Tensor) or theta.dim() != 3:
        raise ValueError("theta: expected a [rows, R, K] tensor")
    R, K = int(theta.shape[1]), int(theta.shape[2])
    _members(who, R, K, r_max)
    _table3("theta", theta, R, K)
    if phi is not None:
        _table3("phi", phi, R, K, theta.device)
    return R, K, theta.device


def _vector(name, t, who=None):
    """``t.numel()`` of a 1-D tensor; with ``who`` (the wrapper) also refused at 2^31 entries or more."""
    if not isinstance(t, torch.Tensor) or t.dim() != 1:
        raise ValueError(f"{name}: expected a 1-D tensor")
    n = t.numel()
    if who is not None and n >= 1 << 31:
        raise ValueError(f"{who}: {name} holds {n} entries (< 2^31)")
    return n


def _index(name, t, dtype, shape, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise ValueError(f"{name}: expected an {str(dtype).replace('torch.', '')} tensor")
    if t.device != dev:
        raise ValueError(f"{name}: on {t.device}, expected {dev}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)} != {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t.data_ptr()


def _fields(who, grow):
    """F of ``grow`` [n, F], the groups of a side's explained fields."""
    if not isinstance(grow, torch.Tensor) or grow.dim() != 2:
        raise ValueError("grow: expected an [n, F] tensor")
    F = int(grow.shape[1])
    if not 1 <= F <= _CFG.EXPLAIN_MAX_FIELDS:
        raise ValueError(f"{who}: F must be in [1, {_CFG.EXPLAIN_MAX_FIELDS}], got {F}")
    return F


def _order_segments(order, seg_start, seg_end, dev):
    """``order`` int32 [n_ord] and ``seg_start`` / ``seg_end`` int64 [G]: ``(G, their three pointers)``."""
    p_ord = _index("order", order, torch.int32, (_vector("order", order),), dev)
    G = _vector("seg_start", seg_start)
    return (G, p_ord, _index("seg_start", seg_start, torch.int64, (G,), dev),
            _index("seg_end", seg_end, torch.int64, (G,), dev))


def _in_range(name, idx, lo, hi):
    """Two host reads: every entry of ``idx`` in ``[lo, hi)``, before a gather kernel touches memory.  Nothing to
    read for None or an empty tensor."""
    if idx is not None and idx.numel() and (int(idx.max()) >= hi or int(idx.min()) < lo):
        raise ValueError(f"{name}: index out of range")


def _segments_in_range(order, V, seg_start, seg_end):
    """Host reads: ``order`` holds rows of a table of V rows, and 0 <= start <= end <= order.numel()."""
    _in_range("order", order, 0, V)
    n_ord = order.numel()
    if seg_start.numel() and (int(seg_start.min()) < 0 or int((seg_end - seg_start).min()) < 0
                              or int(seg_end.max()) > n_ord):
        raise ValueError(f"seg_start / seg_end: segments must satisfy 0 <= start <= end <= {n_ord}")


def score_ensemble(theta, phi, R, K, dflt, doc_a, word_a, doc_b, word_b, tol, max_blocks: int = 0):
    """Ensemble scores of R members (csrc/hip/score_ensemble.hip; ``ops.reference.score_ensemble`` is the twin):
    ``(score_a, score_b|None, key, flag, votes)`` as new device tensors.

    ``theta`` [D, R, K] / ``phi`` [V, R, K] float64: the members' tables interleaved per row.  A side's score is
    ``(((0.0 + s_0) + s_1) + ...) / R`` over the members' ``score_events`` scores s_r; ``key`` the lower side,
    ``flag`` ``key < tol``, ``votes`` (uint8) the members whose own key is under ``tol``.  R = 1 is
    ``score_events`` bit for bit.  Everything is checked on the host before the launch; ``n == 0`` launches
    nothing.  ``max_blocks``: cap on the workgroups (tests: a small cap makes the grid-stride loop wrap)."""
    import operator
    R, K = operator.index(R), operator.index(K)
    _max_blocks(max_blocks)
    _members("score_ensemble", R, K, ENSEMBLE_MAX)
    _table3("theta", theta, R, K)
    dev = theta.device
    _table3("phi", phi, R, K, dev)
    if (doc_b is None) != (word_b is None):
        raise ValueError("score_ensemble: doc_b and word_b go together")
    n = _vector("doc_a", doc_a, "score_ensemble")
    two = doc_b is not None
    sides = (("doc_a", doc_a, theta.shape[0]), ("word_a", word_a, phi.shape[0]),
             ("doc_b", doc_b, theta.shape[0]), ("word_b", word_b, phi.shape[0]))
    ptr = [0 if idx is None else _index(name, idx, torch.int32, (n,), dev) for name, idx, _ in sides]
    for name, idx, rows in sides:
        _in_range(name, idx, -1, rows)
    sa = torch.empty(n, dtype=torch.float64, device=dev)
    sb = torch.empty(n, dtype=torch.float64, device=dev) if two else None
    key = torch.empty(n, dtype=torch.float64, device=dev)
    flag = torch.empty(n, dtype=torch.uint8, device=dev)
    votes = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return sa, sb, key, flag, votes
    if lib().ensemble_max() != ENSEMBLE_MAX:
        raise RuntimeError("score_ensemble: config.ENSEMBLE_MAX differs from the compiled kEnsembleMax")
    lib().score_ensemble(theta.data_ptr(), phi.data_ptr(), R, K, float(dflt), *ptr, int(n), float(tol),
                         sa.data_ptr(), sb.data_ptr() if two else 0, key.data_ptr(), flag.data_ptr(),
                         votes.data_ptr(), int(max_blocks), _stream())
    return sa, sb, key, flag, votes


SELECT_TILE = 2048   # rows of one tile of the selection kernels (csrc/hip/kernels.h kSelectTile)


def select_lowest(key, flag, limit, max_blocks: int = 0, with_count: bool = False):
    """Row indices (int64, ascending) of the ``limit`` flagged rows that a stable ascending sort of their keys
    puts first -- ``rank_flagged(key, flag)[:limit]`` as a set; all the flagged rows when there are fewer.
    Keys order as ``sortgroup.f64_order_keys``, ties at the cut go to the lowest row (csrc/hip/select_lowest.hip:
    a radix select, no sort and no compaction of the flagged rows).  One host read (the count of selected rows).
    ``max_blocks``: cap on the workgroups per launch (tests: a small cap makes the grid-stride loops wrap).
    ``with_count``: also return the number of flagged rows."""
    import operator
    limit = operator.index(limit)      # TypeError for a float
    if limit < 1:
        raise ValueError(f"limit must be >= 1, got {limit}")
    _max_blocks(max_blocks)
    n = _vector("key", key, "select_lowest")      # the kernels count in 32 bits
    dev = key.device
    p_key = _chk(key, torch.float64, "key", (n,), dev)
    p_flag = _chk(flag, torch.uint8, "flag", (n,), dev)
    if n == 0:
        out = torch.empty(0, dtype=torch.int64, device=dev)
        return (out, 0) if with_count else out
    L = lib()
    if L.select_tile() != SELECT_TILE:
        raise RuntimeError("select_lowest: SELECT_TILE differs from the compiled kSelectTile")
    cap = min(limit, n)
    work = torch.empty(int(L.select_work_words(n)), dtype=torch.int32, device=dev)
    out = torch.empty(cap, dtype=torch.int64, device=dev)
    L.select_lowest(p_key, p_flag, int(n), int(cap), work.data_ptr(), out.data_ptr(), int(cap), int(max_blocks),
                    _stream())
    r = L.select_result_word()
    flagged, m = (int(x) for x in work[r:r + 2].cpu().tolist())
    if not 0 <= m <= cap or m != min(cap, flagged):
        raise RuntimeError(f"select_lowest: inconsistent counts (selected {m}, flagged {flagged}, limit {cap})")
    return (out[:m], flagged) if with_count else out[:m]


def host_summary(doc_a, score_a, doc_b, score_b, num_docs, tol, max_blocks: int = 0, fold: bool = True,
                 stats: bool = False):
    """Per document the scored sides folded (csrc/hip/host_summary.hip; ``ops.reference.host_summary`` is the
    twin): ``(events int64 [D], flagged int64 [D], min_score float64 [D], worst int64 [D], skipped int)``.

    Event i has the side a ``(doc_a[i], score_a[i])`` and, when ``doc_b`` / ``score_b`` are given, the side b;
    side number ``2 i + side``.  ``doc``: int32 document row in ``[0, num_docs)`` or -1 (no document: the side
    is only counted in ``skipped``).  ``events``: sides of the document; ``flagged``: of those, the sides with
    score < ``tol``; ``min_score``: their lowest non-NaN score in the order of ``sortgroup.f64_order_keys``
    (-0.0 below +0.0), +inf when there is none; ``worst``: the lowest side number that attains it, -1 when
    there is none.  Host reads: the bounds of the rows before the launch, ``skipped`` after it.
    ``max_blocks``: cap on the workgroups per launch (tests: a small cap makes the grid-stride loops wrap).
    ``fold``: a wave folds the documents that repeat in it before it adds (False: one atomic per side, 10 to 127
    times slower when one document has half of the sides, profiles/host_report.md) -- the result does not depend
    on it.  ``stats``: also return, as a sixth value, the atomics issued ``(counts, min_key, worst)``
    (measurement: scripts/host_report_bench.py)."""
    import operator
    _max_blocks(max_blocks)
    D = operator.index(num_docs)
    if D < 0 or D >= 1 << 31:
        raise ValueError(f"num_docs must be in [0, 2^31), got {D}")
    if (doc_b is None) != (score_b is None):
        raise ValueError("host_summary: doc_b and score_b go together")
    n = _vector("doc_a", doc_a, "host_summary")      # side numbers are 32-bit
    dev = doc_a.device
    two = doc_b is not None
    ptr = [_chk(doc_a, torch.int32, "doc_a", (n,), dev), _chk(score_a, torch.float64, "score_a", (n,), dev),
           _chk(doc_b, torch.int32, "doc_b", (n,), dev) if two else 0,
           _chk(score_b, torch.float64, "score_b", (n,), dev) if two else 0]
    L = lib()
    _in_range("doc_a", doc_a, -1, D)
    _in_range("doc_b", doc_b, -1, D)
    sides = n * (2 if two else 1)
    if n == 0 or D == 0:      # nothing to fold: every side (D == 0: all at -1, checked above) is skipped
        out = (torch.zeros(D, dtype=torch.int64, device=dev), torch.zeros(D, dtype=torch.int64, device=dev),
               torch.full((D,), float("inf"), dtype=torch.float64, device=dev),
               torch.full((D,), -1, dtype=torch.int64, device=dev), sides)
        return out + ((0, 0, 0),) if stats else out
    events = torch.empty(D, dtype=torch.int32, device=dev)
    flagged = torch.empty(D, dtype=torch.int32, device=dev)
    min_key = torch.empty(D, dtype=torch.int64, device=dev)
    worst = torch.empty(D, dtype=torch.int32, device=dev)
    tail = torch.empty(1 + 3, dtype=torch.int64, device=dev)      # skipped (low 32 bits), the stats words
    L.host_summary(*ptr, int(n), int(D), float(tol), events.data_ptr(), flagged.data_ptr(), min_key.data_ptr(),
                   worst.data_ptr(), tail.data_ptr(), bool(fold), tail[1:].data_ptr() if stats else 0,
                   int(max_blocks), _stream())
    u32 = lambda t: t.to(torch.int64) & 0xFFFFFFFF      # noqa: E731 -- the kernels' counters are unsigned
    w = u32(worst)
    # the order key back to the double: keys with the top bit set are the non-negatives (clear it), the
    # others the negatives with every bit flipped; all-ones: no non-NaN score
    bits = torch.where(min_key < 0, min_key ^ (-1 << 63), ~min_key)
    min_score = torch.where(min_key == -1, torch.full_like(bits, 0x7FF0000000000000), bits).view(torch.float64)
    host = tail.cpu().tolist()
    out = (u32(events), u32(flagged), min_score, torch.where(w == 0xFFFFFFFF, torch.full_like(w, -1), w),
           host[0] & 0xFFFFFFFF)
    return out + (tuple(host[1:]),) if stats else out


def group_rows_sum(table, order, seg_start, seg_end, max_blocks: int = 0, block=None):
    """Sums of table rows over segments of a row order (csrc/hip/explain.hip; ``ops.reference.group_rows_sum`` is
    the twin): float64 [G, W], row g the sum of ``table[order[seg_start[g] : seg_end[g]]]``, column by column.

    ``table`` [V, W] float64 (W = K, or R K for an ensemble's interleaved rows), ``order`` int32 [V'] of table rows,
    ``seg_start`` / ``seg_end`` int64 [G] with 0 <= start <= end <= V'.  A segment is cut into blocks of
    ``config.GROUP_BLOCK`` members; a block is summed from 0.0 in member order, a segment's block sums are added
    from 0.0 in block order: plain rounded adds, no atomics, the same bits for every grid.  Everything is checked
    on the host before the launch (host reads: the bounds of ``order`` and of the segments, the block count);
    ``G == 0`` launches nothing.  ``max_blocks``: cap on the workgroups per launch (tests: a small cap makes the
    grid-stride loops wrap).  ``block``: another block size (measurement: scripts/explain_bench.py)."""
    _max_blocks(max_blocks)
    GB = _block("group_rows_sum", block, _CFG.GROUP_BLOCK)
    _table("table", table, "[V, W]")
    dev = table.device
    V, W = table.shape
    if W < 1 or V >= 1 << 31:
        raise ValueError(f"table: shape {tuple(table.shape)} (W >= 1, V < 2^31)")
    G, p_ord, p_s, p_e = _order_segments(order, seg_start, seg_end, dev)
    if G >= 1 << 31:
        raise ValueError(f"group_rows_sum: {G} segments (G < 2^31)")
    out = torch.empty((G, W), dtype=torch.float64, device=dev)
    if G == 0:
        return out
    _segments_in_range(order, V, seg_start, seg_end)
    blk_off = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    blk_off[1:] = torch.cumsum((seg_end - seg_start + (GB - 1)) // GB, 0)
    B = int(blk_off[-1])
    if B >= 1 << 31:
        raise ValueError(f"group_rows_sum: {B} blocks (B < 2^31)")
    scratch = torch.empty((max(B, 1), W), dtype=torch.float64, device=dev)
    lib().group_rows_sum(table.data_ptr(), p_ord, p_s, p_e, blk_off.data_ptr(), int(G), int(B), int(W), int(GB),
                         scratch.data_ptr(), out.data_ptr(), int(max_blocks), _stream())
    return out


def explain_sides(theta, phi, gsum, doc, word, grow, dflt, max_blocks: int = 0):
    """Per side the conditional probability of every explained field of its word (csrc/hip/explain.hip;
    ``ops.reference.explain_sides`` is the twin): ``(cond float64 [n, F], why uint8 [n])`` as new device tensors.

    ``theta`` [D, R, K] / ``phi`` [V, R, K] as ``score_ensemble`` takes them, ``gsum`` [Gtot, R, K] the sums of phi
    rows over groups (``group_rows_sum``); ``doc`` / ``word`` int32 [n] rows or -1, ``grow`` int32 [n, F] the
    ``gsum`` row of the side's group of field f or -1.  s is the side's ``score_ensemble`` score (a side without a
    document takes the default vector), m_f the same expression over the group row, ``cond[i, f] = s / m_f``, NaN
    where ``word[i] < 0`` or ``grow[i, f] < 0``; ``why[i]`` the lowest f with the lowest non-NaN cond, 255 when
    there is none.  Everything is checked on the host before the launch; ``n == 0`` launches nothing."""
    _max_blocks(max_blocks)
    R, K, dev = _tables3("explain_sides", theta, phi, ENSEMBLE_MAX)
    _table3("gsum", gsum, R, K, dev)
    n = _vector("doc", doc, "explain_sides")
    F = _fields("explain_sides", grow)
    p_doc = _index("doc", doc, torch.int32, (n,), dev)
    p_word = _index("word", word, torch.int32, (n,), dev)
    p_grow = _index("grow", grow, torch.int32, (n, F), dev)
    _in_range("doc", doc, -1, theta.shape[0])
    _in_range("word", word, -1, phi.shape[0])
    _in_range("grow", grow, -1, gsum.shape[0])
    cond = torch.empty((n, F), dtype=torch.float64, device=dev)
    why = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return cond, why
    L = lib()
    if L.ensemble_max() != ENSEMBLE_MAX or L.explain_max_fields() != _CFG.EXPLAIN_MAX_FIELDS:
        raise RuntimeError("explain_sides: config.ENSEMBLE_MAX / EXPLAIN_MAX_FIELDS differ from the compiled limits")
    # no group row at all (every grow is -1, checked above): the kernel never reads gsum
    p_gsum = gsum.data_ptr() if gsum.shape[0] else phi.data_ptr()
    L.explain_sides(theta.data_ptr(), phi.data_ptr(), p_gsum, R, K, F, float(dflt), p_doc, p_word, p_grow,
                    int(n), cond.data_ptr(), why.data_ptr(), int(max_blocks), _stream())
    return cond, why


EXPECT_FORMS = ("blocks",)      # the forms of the expect kernel that ship (profiles/expect.md)
EXPECT_PATHS = ("registers", "global")


def expect_theta_path(R: int, K: int) -> str:
    """Where the expect kernel keeps a theta row of R members x K topics (csrc/hip/expect.hip): in ``registers`` on
    the ladder of tail_common.h, or read from ``global`` memory at every member."""
    return EXPECT_PATHS[lib().expect_theta_path(int(R), int(K))]


def expect_sides(theta, phi, order, seg_start, seg_end, doc, word, grow, dflt, max_blocks: int = 0, block=None,
                 form=None):
    """Per (document, word) pair and explained field the member of the word's group that the document's model
    finds most probable (csrc/hip/expect.hip; ``ops.reference.expect_sides`` is the twin):
    ``(best int32 [n, F], pbest float64 [n, F], above int32 [n, F])`` as new device tensors.

    ``theta`` [D, R, K] / ``phi`` [V, R, K] as ``score_ensemble`` takes them; ``order`` int32 [n_ord] of phi rows,
    ``seg_start`` / ``seg_end`` int64 [G] with 0 <= start <= end <= n_ord: group g is ``order[start[g] : end[g]]``;
    ``doc`` / ``word`` int32 [n] rows or -1, ``grow`` int32 [n, F] the group of the pair's field f or -1.  p_v is
    the pair's ``score_ensemble`` score with phi row v in place of the word (a pair without a document takes the
    default vector), s = p_word.  ``best``: the member with the greatest p_v under ``>`` -- a NaN never wins, ties
    to the lowest row -- or -1; ``pbest`` its p_v (NaN without one); ``above`` the members with p_v > s.  ``word
    < 0`` or ``grow < 0``: -1, NaN, -1.  A maximum, a tie-break by row and a count: the same bits for every grid
    and block cut, no atomics.

    The items (pair, field) are sorted by group before the launch (``ops/sortgroup.py``), a group is cut into
    blocks of ``config.GROUP_BLOCK`` members, a lane per (item, block).  Everything is checked on the host before
    the launch (host reads: the bounds of every index, the block count); ``n == 0`` launches nothing.
    ``max_blocks``: cap on the workgroups per launch (tests: a small cap makes the grid-stride loops wrap).
    ``block``: another block size (measurement: scripts/expect_bench.py).  ``form``: one of ``EXPECT_FORMS`` (None:
    the default)."""
    from . import sortgroup as SG
    _max_blocks(max_blocks)
    if form is not None and form not in EXPECT_FORMS:
        raise ValueError(f"expect_sides: form must be one of {EXPECT_FORMS}, got {form!r}")
    GB = _block("expect_sides", block, _CFG.GROUP_BLOCK)
    R, K, dev = _tables3("expect_sides", theta, phi, ENSEMBLE_MAX)
    V = int(phi.shape[0])
    if V >= 1 << 31:
        raise ValueError(f"expect_sides: {V} phi rows (V < 2^31)")
    G, p_ord, _, _ = _order_segments(order, seg_start, seg_end, dev)
    n = _vector("doc", doc)
    F = _fields("expect_sides", grow)
    M = n * F
    if M >= 1 << 31:
        raise ValueError(f"expect_sides: {n} pairs x {F} fields (n F < 2^31)")
    _index("doc", doc, torch.int32, (n,), dev)
    _index("word", word, torch.int32, (n,), dev)
    _index("grow", grow, torch.int32, (n, F), dev)
    best = torch.empty((n, F), dtype=torch.int32, device=dev)
    pbest = torch.empty((n, F), dtype=torch.float64, device=dev)
    above = torch.empty((n, F), dtype=torch.int32, device=dev)
    if n == 0:
        return best, pbest, above
    _in_range("doc", doc, -1, theta.shape[0])
    _in_range("word", word, -1, V)
    _in_range("grow", grow, -1, G)
    _segments_in_range(order, V, seg_start, seg_end)
    L = lib()
    if L.ensemble_max() != ENSEMBLE_MAX or L.explain_max_fields() != _CFG.EXPLAIN_MAX_FIELDS:
        raise RuntimeError("expect_sides: config.ENSEMBLE_MAX / EXPLAIN_MAX_FIELDS differ from the compiled limits")
    # the items (pair, field), sorted by group: the lanes of a wave then walk the same member rows
    g = grow.reshape(-1).to(torch.int64)
    pair = torch.arange(M, device=dev, dtype=torch.int64) // F
    valid = (g >= 0) & (SG.gather(word, pair) >= 0)
    _, perm = SG.sort_stable(torch.where(valid, g, torch.full_like(g, G)))
    it_pair = SG.gather(pair, perm)
    ok = SG.gather(valid, perm)
    none = torch.full((M,), -1, dtype=torch.int64, device=dev)
    if G:
        gs = SG.gather(g, perm).clamp_min(0)
        it_start = torch.where(ok, SG.gather(seg_start, gs), none)
        it_end = torch.where(ok, SG.gather(seg_end, gs), none)
    else:      # no group at all: every grow is -1 (checked above)
        it_start = it_end = none
    it_doc = SG.gather(doc, it_pair).contiguous()
    it_word = SG.gather(word, it_pair).contiguous()
    nb = (it_end - it_start + (GB - 1)) // GB      # 0 without a value (-1 - -1) and for an empty group
    blk_off = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    blk_off[1:] = torch.cumsum(nb, 0)
    B = int(blk_off[-1])
    if B >= 1 << 31:
        raise ValueError(f"expect_sides: {B} blocks (B < 2^31)")
    blk_item = SG.segment_ids(nb, B).to(torch.int32)
    part_p = torch.empty(max(B, 1), dtype=torch.float64, device=dev)
    part_i = torch.empty((2, max(B, 1)), dtype=torch.int32, device=dev)
    L.expect_sides(theta.data_ptr(), phi.data_ptr() if V else 0, R, K, float(dflt), p_ord, it_doc.data_ptr(),
                   it_word.data_ptr(), it_start.data_ptr(), it_end.data_ptr(), perm.data_ptr(), blk_off.data_ptr(),
                   blk_item.data_ptr(), int(M), int(B), int(GB), part_p.data_ptr(), part_i[0].data_ptr(),
                   part_i[1].data_ptr(), best.data_ptr(), pbest.data_ptr(), above.data_ptr(), int(max_blocks),
                   _stream())
    return best, pbest, above


TAIL_PATHS = ("registers", "lds_theta", "direct")


def tail_theta_path(R: int, K: int) -> str:
    """Which form of the tail kernel a row of R members x K topics takes (csrc/hip/tail_mass.hip): the theta row in
    ``registers``, in LDS (``lds_theta``) or both rows read from global memory (``direct``)."""
    return TAIL_PATHS[lib().tail_theta_path(int(R), int(K))]


def tail_mass(theta, phi, doc, word, block=None, max_blocks: int = 0, scratch_mb=None):
    """The host model's probability mass at or below a side's word (csrc/hip/tail_mass.hip;
    ``ops.reference.tail_mass`` is the twin): ``(le float64 [n], tot float64 [n], rarer int32 [n], ties int32 [n])``
    as new device tensors.

    ``theta`` [D, R, K] / ``phi`` [V, R, K] as ``score_ensemble`` takes them, ``doc`` / ``word`` int32 [n] rows or
    -1.  For a side with both rows, p_v is its ``score_ensemble`` score with phi row v in place of the word, s = p_w;
    the V rows are cut into blocks of ``config.TAIL_BLOCK``; within a block, from 0.0 in row order,
    ``le_b += p_v if p_v <= s else 0.0`` and ``tot_b += p_v``, and the block sums are added from 0.0 in block order:
    plain rounded adds, no atomics, the same bits for every grid.  ``rarer`` / ``ties`` count ``p_v < s`` and
    ``p_v == s``.  A side without a row gets NaN, NaN, -1, -1.  The tail probability is ``le / tot``.

    The per-block partials (24 bytes per side and block) live in a scratch of at most ``scratch_mb`` MiB
    (``config.TAIL_SCRATCH_MB``): more sides than fit are processed in batches.  Everything is checked on the host
    before the launch; ``n == 0`` launches nothing.  ``max_blocks``: cap on the workgroups per launch (tests: a
    small cap makes the grid-stride loops wrap).  ``block``: another block size (measurement:
    scripts/tail_bench.py)."""
    return _tail_launch("tail_mass", False, theta, phi, doc, word, block, max_blocks, scratch_mb)


def tail_mass_docs(theta, phi, doc, word, block=None, max_blocks: int = 0, scratch_mb=None):
    """``tail_mass`` for pairs sorted by document (csrc/hip/tail_docs.hip): the same four tensors, bit for bit, with
    p(.|d) evaluated once per (document of a tile of 256 pairs, phi row) and shared by the tile's pairs of that
    document through LDS, instead of once per pair -- the shape of ranking every event of a day by its tail, where
    the distinct pairs are the corpus entries and lie many to a document.

    Arguments and refusals as ``tail_mass``, and: ``doc`` is non-decreasing, ``doc >= 0`` and ``word >= 0`` (the caller
    drops sides without a row), else ``ValueError`` before any launch; repeated pairs are allowed.  Only the row
    widths of the register ladder (``tail_theta_path(R, K) == "registers"``); any other is refused --
    ``score.scorer.tail_pairs`` sends those to ``tail_mass``.  A scratch batch may end inside a document: a tile's
    first pair starts a document slot of its own."""
    return _tail_launch("tail_mass_docs", True, theta, phi, doc, word, block, max_blocks, scratch_mb)


def _tail_launch(who, docs, theta, phi, doc, word, block, max_blocks, scratch_mb):
    """The checks, the scratch batches and the launches of ``tail_mass`` and (``docs``) ``tail_mass_docs``."""
    _max_blocks(max_blocks)
    TB = _block(who, block, _CFG.TAIL_BLOCK)
    cap_mb = _scratch_mb(who, scratch_mb, _CFG.TAIL_SCRATCH_MB)
    R, K, dev = _tables3(who, theta, phi, ENSEMBLE_MAX)
    V = int(phi.shape[0])
    if V >= 1 << 31:
        raise ValueError(f"{who}: {V} phi rows (V < 2^31)")
    n = _vector("doc", doc, who)
    _index("doc", doc, torch.int32, (n,), dev)
    _index("word", word, torch.int32, (n,), dev)
    le = torch.empty(n, dtype=torch.float64, device=dev)
    tot = torch.empty(n, dtype=torch.float64, device=dev)
    rarer = torch.empty(n, dtype=torch.int32, device=dev)
    ties = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return le, tot, rarer, ties
    _in_range("doc", doc, 0 if docs else -1, theta.shape[0])
    _in_range("word", word, 0 if docs else -1, V)
    if docs and n > 1 and bool((doc[1:] < doc[:-1]).any()):
        raise ValueError(f"{who}: doc must be non-decreasing (the pairs sorted by document)")
    L = lib()
    if docs and L.tail_theta_path(R, K) != 0:
        raise ValueError(f"{who}: a row of {R} members x {K} topics is wider than the register ladder "
                         f"(tail_theta_path: {tail_theta_path(R, K)}); tail_mass takes it")
    launch = L.tail_mass_docs if docs else L.tail_mass
    if L.ensemble_max() != ENSEMBLE_MAX:
        raise RuntimeError(f"{who}: config.ENSEMBLE_MAX differs from the compiled limit")
    nblk = -(-V // TB)
    batch = _scratch_batch(n, 24 * max(nblk, 1), cap_mb, 256)      # whole tiles of sides
    scratch = torch.empty(batch * max(nblk, 1) * 3, dtype=torch.float64, device=dev)
    for s0 in range(0, n, batch):
        m = min(batch, n - s0)
        launch(theta.data_ptr(), phi.data_ptr() if V else 0, R, K, V, doc.data_ptr() + 4 * s0,
               word.data_ptr() + 4 * s0, int(m), int(TB), int(nblk), scratch.data_ptr(), le.data_ptr() + 8 * s0,
               tot.data_ptr() + 8 * s0, rarer.data_ptr() + 4 * s0, ties.data_ptr() + 4 * s0, int(max_blocks),
               _stream())
    return le, tot, rarer, ties


PEER_PATHS = ("registers", "direct")


def peer_theta_path(R: int, K: int) -> str:
    """Which form of the peers kernel a row of R members x K topics takes (csrc/hip/peers.hip): the query's row in
    ``registers`` (R K <= 100) or both rows read from global memory (``direct``)."""
    return PEER_PATHS[lib().peer_theta_path(int(R), int(K))]


def peer_topn(theta3, query, n, block=None, max_blocks: int = 0, scratch_mb=None):
    """The ``n`` nearest rows of every query row in L1 distance (csrc/hip/peers.hip; ``ops.reference.peer_topn`` is
    the twin): ``(rows int32 [Q, n], dist float64 [Q, n], count int32 [Q])`` as new device tensors.

    ``theta3`` [D, R, K], its rows W = R K doubles; ``query`` int32 [Q] rows.  L(q, p): from 0.0, for j = 0 .. W - 1
    in order, one rounded subtraction and one rounded add of its magnitude.  Listed are the candidates p != q lowest
    in the order (L, p) ascending, a NaN L never; ``count`` of them, the slots past it -1 and +inf.  The same bits
    for every grid, ``block`` (``config.PEERS_BLOCK`` candidate rows) and batch; no atomics.

    The per-block lists (n x 12 bytes per query and block) live in a scratch of at most ``scratch_mb`` MiB
    (``config.PEERS_SCRATCH_MB``): more queries than fit are processed in batches.  Everything is checked on the
    host before the launch; ``Q == 0`` launches nothing.  ``max_blocks``: cap on the workgroups per launch (tests: a
    small cap makes the grid-stride loops wrap)."""
    import operator
    _max_blocks(max_blocks)
    PB = _block("peer_topn", block, _CFG.PEERS_BLOCK)
    cap_mb = _scratch_mb("peer_topn", scratch_mb, _CFG.PEERS_SCRATCH_MB)
    N = operator.index(n)
    if not 1 <= N <= _CFG.PEERS_MAX:
        raise ValueError(f"peer_topn: n must be in [1, {_CFG.PEERS_MAX}], got {N}")
    R, K, dev = _tables3("peer_topn", theta3)
    D = int(theta3.shape[0])
    if D >= 1 << 31:
        raise ValueError(f"peer_topn: {D} theta rows (D < 2^31)")
    Q = _vector("query", query, "peer_topn")
    _index("query", query, torch.int32, (Q,), dev)
    rows = torch.empty((Q, N), dtype=torch.int32, device=dev)
    dist = torch.empty((Q, N), dtype=torch.float64, device=dev)
    count = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q == 0:
        return rows, dist, count
    _in_range("query", query, 0, D)
    L = lib()
    if L.peers_max() != _CFG.PEERS_MAX:
        raise RuntimeError("peer_topn: config.PEERS_MAX differs from the compiled limit")
    nblk = -(-D // PB)
    batch = _scratch_batch(Q, 12 * N * nblk, cap_mb, 256)      # whole tiles of queries
    # [nblk][N][batch] doubles, then as many ints
    scratch = torch.empty(_list_scratch_doubles(batch * nblk * N), dtype=torch.float64, device=dev)
    for s0 in range(0, Q, batch):
        m = min(batch, Q - s0)
        L.peer_topn(theta3.data_ptr(), R * K, D, query.data_ptr() + 4 * s0, int(m), N, int(PB), int(nblk),
                    scratch.data_ptr(), rows.data_ptr() + 4 * N * s0, dist.data_ptr() + 8 * N * s0,
                    count.data_ptr() + 4 * s0, int(max_blocks), _stream())
    return rows, dist, count


def topic_path(n: int, W: int) -> str:
    """Which form of the column top-N kernel ``W`` columns take at ``n`` (csrc/hip/topic_report.hip):
    ``columns`` -- a lane per column -- or ``subgroups<G>`` -- the workgroup's lanes in G row sub-groups of W lanes,
    where the table is narrower than half a workgroup."""
    G = lib().topic_groups(int(n), int(W))
    return "columns" if G == 1 else f"subgroups{G}"


def column_topn(table, n, block=None, max_blocks: int = 0, scratch_mb=None, sample=None):
    """Per column of ``table`` the ``n`` rows with the greatest values (csrc/hip/topic_report.hip;
    ``ops.reference.column_topn`` is the twin): ``(rows int32 [W, n], vals float64 [W, n], count int32 [W])`` as new
    device tensors.

    ``table`` [rows, W] float64.  Listed are the rows first in the total order (value descending under IEEE ``>``,
    row ascending): equal values, -0.0 and +0.0 among them, go to the lower row, a NaN never; ``count`` of them, the
    slots past it -1 and -inf.  The same bits for every grid, ``block`` (``config.TOPIC_BLOCK`` rows) and batch; no
    atomics.

    The per-block lists (n x 12 bytes per column and block) live in a scratch of at most ``scratch_mb`` MiB
    (``config.TOPIC_SCRATCH_MB``): more columns than fit are processed in batches.  Everything is checked on the
    host before the launch; an empty table launches nothing.  ``max_blocks``: cap on the workgroups per launch
    (tests: a small cap makes the grid-stride loops wrap).

    A table of at least 2 x ``sample`` rows (``config.TOPIC_SAMPLE``) is read twice: first the same kernels list
    every (rows // sample)-th row; a column's n-th value there is a lower bound of its n-th value in the table, so
    the pass over all rows skips what lies below it -- after that almost nothing reaches a list and the pass is a
    compare per load.  A bound from a subset of the rows excludes nothing that is listed: the same bits."""
    import operator
    _max_blocks(max_blocks)
    TB = _block("column_topn", block, _CFG.TOPIC_BLOCK)
    S = operator.index(_CFG.TOPIC_SAMPLE if sample is None else sample)
    if S < 1:
        raise ValueError(f"column_topn: sample must be >= 1, got {S}")
    cap_mb = _scratch_mb("column_topn", scratch_mb, _CFG.TOPIC_SCRATCH_MB)
    N = operator.index(n)
    if not 1 <= N <= _CFG.TOPIC_REPORT_MAX:
        raise ValueError(f"column_topn: n must be in [1, {_CFG.TOPIC_REPORT_MAX}], got {N}")
    _table("table", table, "[rows, W]")
    dev = table.device
    D, W = (int(x) for x in table.shape)
    if D > (1 << 31) - 65536 or W >= 1 << 31:
        raise ValueError(f"column_topn: table {D} x {W} (rows <= 2^31 - 65536, W < 2^31)")
    rows = torch.full((W, N), -1, dtype=torch.int32, device=dev)
    vals = torch.full((W, N), float("-inf"), dtype=torch.float64, device=dev)
    count = torch.zeros(W, dtype=torch.int32, device=dev)
    if D == 0 or W == 0:
        return rows, vals, count
    L = lib()
    if L.topic_report_max() != _CFG.TOPIC_REPORT_MAX:
        raise RuntimeError("column_topn: config.TOPIC_REPORT_MAX differs from the compiled limit")
    nblk = -(-D // TB)
    # the sample: every stride-th row.  Its pass has no bound yet, so its time goes to list inserts, not to loads:
    # blocks of at most 256 rows spread the S rows over 32 workgroups or more (a 4096-row block: two)
    stride = D // S if D >= 2 * S else 0
    s_rows_n = (D - 1) // stride + 1 if stride else 0
    s_block = min(TB, 256)
    s_nblk = -(-s_rows_n // s_block)
    # whole tiles of columns
    batch = _scratch_batch(W, 12 * N * max(nblk, s_nblk), cap_mb, L.topic_threads(N))
    # [nblk][N][batch] doubles, then as many ints
    scratch = torch.empty(_list_scratch_doubles(batch * max(nblk, s_nblk) * N), dtype=torch.float64, device=dev)
    # pass 2 in two levels where the blocks are many: the lists of the groups of blocks
    cells2 = batch * max(L.topic_merge_groups(nblk), L.topic_merge_groups(s_nblk)) * N
    scratch2 = torch.empty(_list_scratch_doubles(cells2), dtype=torch.float64, device=dev) if cells2 else None
    p2 = scratch2.data_ptr() if cells2 else 0
    if stride:
        s_out = (torch.empty((W, N), dtype=torch.int32, device=dev),
                 torch.empty((W, N), dtype=torch.float64, device=dev), torch.empty(W, dtype=torch.int32, device=dev))
    for c0 in range(0, W, batch):
        wb = int(min(batch, W - c0))
        tau = 0
        if stride:
            # the sample's N-th value per column (-inf where it lists fewer): a lower bound of the table's
            L.column_topn(table.data_ptr(), s_rows_n, W, stride * W, 0, int(c0), wb, N, int(s_block), int(s_nblk),
                          scratch.data_ptr(), p2, s_out[0].data_ptr(), s_out[1].data_ptr(), s_out[2].data_ptr(),
                          int(max_blocks), _stream())
            bound = s_out[1][:, N - 1].contiguous()
            tau = bound.data_ptr()
        L.column_topn(table.data_ptr(), D, W, W, tau, int(c0), wb, N, int(TB), int(nblk), scratch.data_ptr(), p2,
                      rows.data_ptr(), vals.data_ptr(), count.data_ptr(), int(max_blocks), _stream())
    return rows, vals, count


def row_dominant(table3, max_blocks: int = 0):
    """The dominant topic of every (row, member) and the rows per (member, topic) (csrc/hip/topic_report.hip;
    ``ops.reference.row_dominant`` is the twin): ``(arg int32 [rows, R], counts int64 [R, K])`` as new device
    tensors.  ``table3`` [rows, R, K] float64; ``arg`` the first k attaining the maximum of ``table3[row, r, :]``, a
    NaN never, -1 when every entry is NaN.  The counts are integers, added with integer atomics from per-workgroup
    LDS histograms.  Everything is checked on the host before the launch; no row launches nothing."""
    _max_blocks(max_blocks)
    if not isinstance(table3, torch.Tensor) or table3.dim() != 3:
        raise ValueError("table: expected a [rows, R, K] tensor")
    n, R, K = (int(x) for x in table3.shape)
    L = lib()
    if R < 1 or K < 1 or R * K > L.topic_columns_max():
        raise ValueError(f"row_dominant: R and K must be >= 1 and R K <= {L.topic_columns_max()}, got {R} x {K}")
    _table3("table", table3, R, K)
    if n * R >= 1 << 31:
        raise ValueError(f"row_dominant: {n} rows x {R} members (rows R < 2^31)")
    dev = table3.device
    arg = torch.empty((n, R), dtype=torch.int32, device=dev)
    counts = torch.zeros((R, K), dtype=torch.int64, device=dev)
    if n:
        L.row_dominant(table3.data_ptr(), n, R, K, arg.data_ptr(), counts.data_ptr(), int(max_blocks), _stream())
    return arg, counts


def topic_sides(theta3, phi3, doc, word, max_blocks: int = 0):
    """The topic that explains every side (csrc/hip/topic_report.hip; ``ops.reference.topic_sides`` is the twin):
    ``(col int32 [n], resp float64 [n], host_share float64 [n], host_topic int32 [n])`` as new device tensors.

    ``theta3`` [D, R, K] / ``phi3`` [V, R, K] float64; ``doc`` / ``word`` int32 [n]: the side's rows or -1.  Over the
    columns j = r K + k in order ``p_j = theta[d, j] * phi[w, j]``, one rounded product; ``col`` the first j with
    the greatest p_j, a NaN never; ``resp = p* / (s * R)`` with s the side's score as ``score_ensemble`` computes
    it; ``host_share = theta[d, col]``; ``host_topic`` the first k attaining the maximum of the host's row in col's
    member.  A side without a θ row or a φ row, or with NaN products only: -1, NaN, NaN, -1.  Every index is checked
    on the host before the launch; no side launches nothing."""
    _max_blocks(max_blocks)
    R, K, dev = _tables3("topic_sides", theta3, phi3)
    n = _vector("doc", doc, "topic_sides")
    _index("doc", doc, torch.int32, (n,), dev)
    _index("word", word, torch.int32, (n,), dev)
    col = torch.empty(n, dtype=torch.int32, device=dev)
    resp = torch.empty(n, dtype=torch.float64, device=dev)
    share = torch.empty(n, dtype=torch.float64, device=dev)
    ht = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return col, resp, share, ht
    _in_range("doc", doc, -1, theta3.shape[0])
    _in_range("word", word, -1, phi3.shape[0])
    lib().topic_sides(theta3.data_ptr(), phi3.data_ptr(), R, K, doc.data_ptr(), word.data_ptr(), n, col.data_ptr(),
                      resp.data_ptr(), share.data_ptr(), ht.data_ptr(), int(max_blocks), _stream())
    return col, resp, share, ht


def column_l1_path(Wa: int, Wb: int) -> str:
    """The output tile of the column_l1 kernel at these widths (csrc/hip/column_l1.hip): ``tile<TA>x<TB>``, 32 or
    64 columns each way (2 or 4 per lane)."""
    L = lib()
    return f"tile{L.column_l1_tile(int(Wa))}x{L.column_l1_tile(int(Wb))}"


def column_l1(A, B, ia=None, ib=None, block=None, max_blocks: int = 0, scratch_mb=None):
    """The L1 distances between the columns of two tables (csrc/hip/column_l1.hip; ``ops.reference.column_l1`` is
    the twin): float64 [Wa, Wb] as a new device tensor, ``C[a, b]`` = the sum over the M pairs of
    ``|A[ia[m], a] - B[ib[m], b]|``.

    ``A`` [Va, Wa] / ``B`` [Vb, Wb] float64; ``ia`` / ``ib`` int64 [M] rows, both None: the identity
    (Va == Vb == M).  The pairs are cut into blocks of ``block`` consecutive pairs (``config.MATCH_BLOCK``); within
    a block, from 0.0 in pair order, one rounded subtraction, its magnitude, one rounded add; the block sums are
    added from 0.0 in block order -- the block size is part of the result, the grid and the batches are not.  A NaN
    difference makes the sum NaN; no atomics.

    The blocks' partials (Wa x Wb x 8 bytes each) live in a scratch of at most ``scratch_mb`` MiB
    (``config.MATCH_SCRATCH_MB``): more blocks than fit run in batches, each continuing the running sums of the one
    before -- the same sequence of adds.  Everything is checked on the host before a launch (host reads: the bounds
    of the indices); ``M == 0`` launches nothing.  ``max_blocks``: cap on the workgroups per launch (tests: a small
    cap makes the grid-stride loops wrap)."""
    _max_blocks(max_blocks)
    MB = _block("column_l1", block, _CFG.MATCH_BLOCK)
    cap_mb = _scratch_mb("column_l1", scratch_mb, _CFG.MATCH_SCRATCH_MB)
    _table("A", A, "[rows, W]")
    dev = A.device
    _table("B", B, "[rows, W]", dev)
    (Va, Wa), (Vb, Wb) = (int(x) for x in A.shape), (int(x) for x in B.shape)
    if (ia is None) != (ib is None):
        raise ValueError("column_l1: ia and ib go together (both None: the identity)")
    if ia is None:
        if Va != Vb:
            raise ValueError(f"column_l1: the identity form needs tables of equal height, got {Va} and {Vb}")
        M, p_ia, p_ib = Va, 0, 0
    else:
        M = _vector("ia", ia)
        if _vector("ib", ib) != M:
            raise ValueError(f"column_l1: ia has {M} rows, ib {ib.numel()}")
        p_ia = _index("ia", ia, torch.int64, (M,), dev)
        p_ib = _index("ib", ib, torch.int64, (M,), dev)
    L = lib()
    if max(Wa, Wb) > L.column_l1_width_max() or M >= 1 << 40:
        raise ValueError(f"column_l1: {Wa} x {Wb} columns, {M} pairs (W <= {L.column_l1_width_max()}, M < 2^40)")
    out = torch.zeros((Wa, Wb), dtype=torch.float64, device=dev)
    if M == 0 or Wa == 0 or Wb == 0:
        return out
    _in_range("ia", ia, 0, Va)
    _in_range("ib", ib, 0, Vb)
    nblk = -(-M // MB)
    batch = _scratch_batch(nblk, 8 * Wa * Wb, cap_mb)
    scratch = torch.empty(batch * Wa * Wb, dtype=torch.float64, device=dev)
    for b0 in range(0, nblk, batch):
        L.column_l1(A.data_ptr(), B.data_ptr(), Va, Vb, Wa, Wb, p_ia, p_ib, int(M), int(MB), int(b0),
                    int(min(batch, nblk - b0)), scratch.data_ptr(), out.data_ptr(), b0 == 0, int(max_blocks),
                    _stream())
    return out


def holdout_draw(doc_ptr, counts, seed, thr, max_blocks: int = 0, rules: bool = True, lane_tokens=None):
    """Held-out tokens of every CSR entry (csrc/hip/holdout.hip; ``ops.reference.holdout_draw`` is the twin): int64
    [nnz] as a new device tensor.

    ``doc_ptr`` int64 [D + 1], ``counts`` int64 [nnz] >= 0, on the GPU.  Token j of entry e has the global index
    ``g = base[e] + j`` (base: the exclusive prefix sum of the counts) and is held out iff
    ``splitmix64(key ^ g) >> 11 < thr``, ``key = reference.holdout_key(seed)``, ``0 < thr <= 2**52``
    (``reference.holdout_thr(F)``): integers only, the same split for every grid.  An entry of at most
    ``config.HOLDOUT_LANE_TOKENS`` tokens is drawn by one lane, a longer one by waves of 64 lanes x that many
    tokens.  ``rules``: then the two document rules (``reference.holdout_rules``; False: the raw draw).
    Everything is checked on the host before the launch (host reads: the ends of ``doc_ptr``, the bounds of
    ``counts``, the token total, the chunk count); an empty corpus launches nothing.  ``max_blocks``: cap on the
    workgroups per launch (tests: a small cap makes the grid-stride loops wrap).  ``lane_tokens``: another lane
    share (measurement: scripts/holdout_bench.py)."""
    import operator

    from . import reference as REF
    _max_blocks(max_blocks)
    L = operator.index(_CFG.HOLDOUT_LANE_TOKENS if lane_tokens is None else lane_tokens)
    if not 1 <= L <= 1 << 20:
        raise ValueError(f"holdout_draw: lane_tokens must be in [1, 2^20], got {L}")
    for name, x in (("doc_ptr", doc_ptr), ("counts", counts)):
        if isinstance(x, torch.Tensor) and not x.is_cuda:
            raise ValueError(f"{name}: must be a GPU tensor")
    REF.check_holdout_draw(doc_ptr, counts, seed, thr)      # dtypes, contiguity, one device, values
    dev = counts.device
    nnz = counts.numel()
    t = torch.empty(nnz, dtype=torch.int64, device=dev)
    if nnz == 0:
        return t
    base = torch.cumsum(counts, 0) - counts
    chunk_off = torch.zeros(nnz + 1, dtype=torch.int64, device=dev)
    span = 64 * L
    chunk_off[1:] = torch.cumsum(torch.where(counts > L, (counts + (span - 1)) // span, torch.zeros_like(counts)), 0)
    chunks = int(chunk_off[-1])
    if chunks >= 1 << 31:
        raise ValueError(f"holdout_draw: {chunks} wave chunks (< 2^31); raise lane_tokens")
    lib().holdout_draw(base.data_ptr(), counts.data_ptr(), chunk_off.data_ptr(), int(nnz), chunks,
                       REF.holdout_key(seed), operator.index(thr), int(L), t.data_ptr(), int(max_blocks), _stream())
    return REF.holdout_rules(doc_ptr, counts, t) if rules else t


def holdout_entries(theta, phi, doc, word, t, word_seen, max_blocks: int = 0):
    """Held-out log-likelihood of every CSR entry (csrc/hip/holdout.hip; ``ops.reference.holdout_entries`` is the
    twin): float64 [n] as a new device tensor, ``t[e] * log_rn(theta[doc[e]] . phi[word[e]])`` for an entry with
    ``t[e] > 0`` whose word has a training entry (``word_seen[word[e]] != 0``), else 0.0.

    ``theta`` [D, K] / ``phi`` [V, K] float64, ``doc`` / ``word`` int32 [n] rows (no -1 here: every entry has its
    document and its word), ``t`` int64 [n], ``word_seen`` uint8 [V].  The dot is ``score_events``'; ``log_rn`` a
    natural log of correctly rounded fp64 operations in a fixed order.  Everything is checked on the host before
    the launch; ``n == 0`` launches nothing."""
    _max_blocks(max_blocks)
    _table("theta", theta, "[rows, K]")
    dev = theta.device
    _table("phi", phi, "[rows, K]", dev)
    (D, K), V = theta.shape, phi.shape[0]
    if K < 1 or phi.shape[1] != K:
        raise ValueError(f"theta / phi: row widths {K} and {phi.shape[1]} (one K >= 1)")
    n = _vector("doc", doc, "holdout_entries")
    p_doc = _index("doc", doc, torch.int32, (n,), dev)
    p_word = _index("word", word, torch.int32, (n,), dev)
    p_t = _index("t", t, torch.int64, (n,), dev)
    p_seen = _index("word_seen", word_seen, torch.uint8, (V,), dev)
    _in_range("doc", doc, 0, D)
    _in_range("word", word, 0, V)
    ll = torch.empty(n, dtype=torch.float64, device=dev)
    if n == 0:
        return ll
    lib().holdout_entries(theta.data_ptr(), phi.data_ptr(), int(K), p_doc, p_word, p_t, p_seen, int(n), ll.data_ptr(),
                          int(max_blocks), _stream())
    return ll


def string_entropy(bytes_u8, offsets, max_blocks: int = 0):
    """float64 [n] Shannon entropy of the byte strings [offsets[i], offsets[i + 1]) of ``bytes_u8`` (uint8, on
    the GPU), bit for bit ``ops.reference.string_entropy`` (csrc/hip/string_entropy.hip).  ``offsets``: int64
    [n + 1] on the host, where they come from (Arrow) and where they are checked before the launch:
    non-decreasing, first >= 0, last <= bytes_u8.numel(); device offsets are refused instead of being copied back
    on every call.  ``max_blocks``: cap on the workgroups (tests: a small cap makes the grid-stride loop wrap).
    The kernel reads the ``entropy_table`` of the longest string of the call."""
    from .reference import entropy_table
    _max_blocks(max_blocks)
    if not isinstance(bytes_u8, torch.Tensor) or bytes_u8.dim() != 1:
        raise ValueError("bytes: expected a 1-D tensor")
    if not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError("offsets: expected a 1-D tensor of n + 1 entries")
    if offsets.dtype != torch.int64:
        raise TypeError(f"offsets: expected {torch.int64}, got {offsets.dtype}")
    if offsets.is_cuda:
        raise ValueError("offsets: expected on the host (they are checked there, then uploaded)")
    dev = bytes_u8.device
    p_bytes = _chk(bytes_u8, torch.uint8, "bytes", None, dev)
    n = offsets.numel() - 1
    off_h = offsets
    if n:
        d = off_h[1:] - off_h[:-1]
        if int(d.min()) < 0:
            raise ValueError("offsets: must be non-decreasing")
    if int(off_h[0]) < 0 or int(off_h[-1]) > bytes_u8.numel():
        raise ValueError(f"offsets: [{int(off_h[0])}, {int(off_h[-1])}] outside the {bytes_u8.numel()} bytes")
    out = torch.empty(n, dtype=torch.float64, device=dev)
    if n == 0:
        return out
    longest = int(d.max())
    if longest >= 1 << 31:
        raise ValueError(f"string_entropy: a string of {longest} bytes, the kernel counts in 32 bits")
    table = torch.from_numpy(entropy_table(longest)).to(dev)      # longest + 1 >= 2 entries
    p_tab = _chk(table, torch.float64, "table", (longest + 1 if longest >= 1 else 2,), dev)
    off_d = offsets.to(dev)
    p_off = _chk(off_d, torch.int64, "offsets", (n + 1,), dev)
    lib().string_entropy(p_bytes, p_off, int(n), p_tab, int(table.numel()), out.data_ptr(), int(max_blocks),
                         _stream())
    return out


def flow_words(hour, minute, second, port_a, port_b, ipkt, ibyt, time_cuts, ibyt_cuts, ipkt_cuts):
    n = hour.numel()
    dev = hour.device
    cols = [hour, minute, second, port_a, port_b, ipkt, ibyt]
    names = ["hour", "minute", "second", "port_a", "port_b", "ipkt", "ibyt"]
    ptrs = [_chk(c, torch.float64, nm, (n,), dev) for c, nm in zip(cols, names)]
    cuts = [time_cuts, ibyt_cuts, ipkt_cuts]
    cptr = [_chk(c, torch.float64, "cuts", None, dev) for c in cuts]
    out = dict(
        time=torch.empty(n, dtype=torch.float64, device=dev),
        time_bin=torch.empty(n, dtype=torch.int8, device=dev),
        ibyt_bin=torch.empty(n, dtype=torch.int8, device=dev),
        ipkt_bin=torch.empty(n, dtype=torch.int8, device=dev),
        word_port=torch.empty(n, dtype=torch.float64, device=dev),
        p_case=torch.empty(n, dtype=torch.int8, device=dev),
        src_prefix=torch.empty(n, dtype=torch.int8, device=dev),
        dst_prefix=torch.empty(n, dtype=torch.int8, device=dev),
    )
    if n == 0:
        return out
    lib().flow_words(
        *ptrs, cptr[0], time_cuts.numel(), cptr[1], ibyt_cuts.numel(), cptr[2], ipkt_cuts.numel(), int(n),
        out["time"].data_ptr(), out["time_bin"].data_ptr(), out["ibyt_bin"].data_ptr(),
        out["ipkt_bin"].data_ptr(), out["word_port"].data_ptr(), out["p_case"].data_ptr(),
        out["src_prefix"].data_ptr(), out["dst_prefix"].data_ptr(), _stream(),
    )
    return out


def bin_columns(values, cuts):
    """bins[i, c] = #{cut in cuts[c] : values[c][i] > cut} (int8 [n, ncols])."""
    n = values[0].numel()
    dev = values[0].device
    vp = [_chk(v, torch.float64, "values", (n,), dev) for v in values]
    cp = [_chk(c, torch.float64, "cuts", None, dev) for c in cuts]
    out = torch.empty((n, len(values)), dtype=torch.int8, device=dev)
    if n == 0:
        return out
    lib().bin_columns(vp, cp, [int(c.numel()) for c in cuts], int(n), out.data_ptr(), _stream())
    return out


# ------------------------------------------------------- fp64 block Gauss-Seidel ---
# lda-c-faithful E-step (csrc/hip/lda_gs64.hip, gs_*.hip): double everywhere, gamma refreshed after every
# chunk of ceil(n / gs_updates) words (documents of <= gs_updates words: lda-c's per-word schedule).
GS_TINY, GS_TEAM1, GS_TEAM4, GS_TEAM8, GS_SMALL, GS_CHAIN = range(6)
GS_SMALL_MAX = 64   # csrc/hip/gs_short.hip kGsSmallMax
GS_LDS_UMAX = 32    # csrc/hip/kernels.h kGsUMax: largest U with the chunk tables in LDS (rows of csum / et)


def gs_umax(KS: int = 0) -> int:
    """Largest U (gamma refreshes per sweep) of the fp64 engine: 4096 at every KS -- past 32 the chunk
    tables live in the c.phi rows (gs_team GMT, gs_chain; at KS > 32 also gs_smallw)."""
    return int(lib().gs_umax(int(KS)))


def gs_split_umax(KS: int) -> int:
    """Largest U of the split-document kernel: 4096 at KS > 32 (chunk tables past the LDS ones in a
    per-segment scratch, GSSplitPlan ``tab``), else its LDS tables' (64 at KS <= 52, else 32)."""
    return int(lib().gs_split_umax(int(KS)))


def gs_split_lds_umax(KS: int) -> int:
    """Largest U with the split kernel's chunk tables in LDS (64 at KS <= 52, else 32)."""
    return int(lib().gs_split_lds_umax(int(KS)))


def gs_tiny_max(KS: int) -> int:
    return int(lib().gs_tiny_max(int(KS)))


def _cphi_ptr(cphi, nnz, KS, dev, ent_base):
    """Device address of c.phi row 0 of the corpus: the whole [nnz, KS] buffer, or (``ent_base`` given)
    a window [rows, KS] holding corpus entries [ent_base, ent_base + rows) -- the kernels index rows by
    corpus entry, so the address is shifted back by ent_base rows.  The caller guarantees that every
    document of the launch has its entries inside the window (GSPlan(doc_range=...))."""
    if ent_base is None:
        return _chk(cphi, torch.float64, "cphi", (nnz, KS), dev)
    ptr = _chk(cphi, torch.float64, "cphi", None, dev)
    if cphi.dim() != 2 or cphi.shape[1] != KS or not (0 <= int(ent_base) and int(ent_base) + cphi.shape[0] <= nnz):
        raise ValueError(f"cphi window {tuple(cphi.shape)} at entry {ent_base} does not fit [{nnz}, {KS}]")
    return ptr - int(ent_base) * KS * 8


class GSStage:
    """Staged beta rows of one kGsTeam8 launch (KS <= 32): every document of ``order`` gets its rows
    copied in document order into one buffer, tiled [ceil(n / 64)][KS / 2][64] double2, refilled by
    ``gs_stage`` after each M-step.  The longest document's kernel then gathers 64 consecutive words
    as 16-byte-contiguous runs (one CU walks those rows U x 20 times per E-step) instead of 64
    scattered 8 KS-byte rows; the copy itself is spread over the whole GPU.  Costs n x KS x 8 bytes."""

    def __init__(self, order, doc_ptr_host, KS: int, device):
        import numpy as np
        if KS > 32 or KS % 2:
            raise ValueError("staged rows need an even KS <= 32")
        o = np.asarray(order.cpu().numpy() if torch.is_tensor(order) else order, np.int64)
        dp = np.asarray(doc_ptr_host, np.int64)
        per = (KS // 2) * 64
        off = np.zeros(o.size, np.int64)
        ents, cnts = [], []
        nt = 0
        for i, d in enumerate(o):
            if d < 0:
                continue
            s0, n = int(dp[d]), int(dp[d + 1] - dp[d])
            T = -(-n // 64)
            off[i] = nt * per
            ents.append(s0 + 64 * np.arange(T, dtype=np.int64))
            cnts.append(np.minimum(64, n - 64 * np.arange(T, dtype=np.int64)))
            nt += T
        self.KS, self.n_tiles = int(KS), nt
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64)
        self.tile_ent = torch.from_numpy(cat(ents).astype(np.int32)).to(device)
        self.tile_cnt = torch.from_numpy(cat(cnts).astype(np.int32)).to(device)
        self.stage_off = torch.from_numpy(off).to(device)
        self.buf = torch.zeros(max(nt, 1) * per * 2, dtype=torch.float64, device=device)

    @classmethod
    def from_arrays(cls, KS: int, n_tiles: int, tile_ent, tile_cnt, stage_off, device) -> "GSStage":
        """Staged rows from tables already on the device (the native engine plan's)."""
        self = cls.__new__(cls)
        self.KS, self.n_tiles = int(KS), int(n_tiles)
        self.tile_ent, self.tile_cnt, self.stage_off = tile_ent, tile_cnt, stage_off
        self.buf = torch.zeros(max(self.n_tiles, 1) * (self.KS // 2) * 64 * 2, dtype=torch.float64, device=device)
        return self

    @property
    def nbytes(self) -> int:
        return self.n_tiles * (self.KS // 2) * 64 * 16


def gs_stage(beta, word_idx, st: "GSStage", gate=None):
    """Refill the staged rows of ``st`` from ``beta`` (after every M-step, before the team8 launch);
    ``gate``: the EM loop's done flag (a converged loop's queued iterations skip the copy)."""
    V, KS = beta.shape
    dev = beta.device
    if KS != st.KS:
        raise ValueError(f"staged rows of KS {st.KS}, beta has {KS}")
    if st.n_tiles == 0:
        return
    lib().gs_stage(_chk(beta, torch.float64, "beta", (V, KS), dev), _chk(word_idx, torch.int32, "word_idx", None, dev),
                   _chk(st.tile_ent, torch.int32, "tile_ent", (st.n_tiles,), dev),
                   _chk(st.tile_cnt, torch.int32, "tile_cnt", (st.n_tiles,), dev), st.n_tiles,
                   _chk(st.buf, torch.float64, "stage", None, dev), int(KS), _gate_ptr(gate, dev), _stream())


def _need_pad_row(t):
    """The E-step kernels load a row's topic lanes at constant offsets: lanes past KS read into the next
    row, the last row's into one pad row past the table (LDAEngine allocates beta as [V + 1, KS] and the
    c.phi rows as [nnz + 1, KS], and hands the kernels the views without it)."""
    V, KS = t.shape
    if t.untyped_storage().nbytes() < (t.storage_offset() + (V + 1) * KS) * t.element_size():
        raise ValueError("the table needs a pad row past its last row ([n + 1, KS] storage, view [:n])")


def gs_chunk_sums(order, doc_ptr, counts, gs_updates: int, device):
    """[n_items, GS_LDS_UMAX] float64: row i holds the chunk count sums of document ``order[i]`` (chunks of
    W = ceil(n / U) words; zeros past its last chunk and for the placement gaps ``order[i] < 0``), from the
    corpus' host ``doc_ptr`` / ``counts`` -- sums of integer counts, exact.  The longest-document kernel
    (gs_wsteam) reads them instead of summing the counts in every E-step (``gs_estep(csum=...)``)."""
    import numpy as np
    U = int(gs_updates)
    if not 1 <= U <= GS_LDS_UMAX:
        raise ValueError(f"chunk sums: U = {U} outside 1..{GS_LDS_UMAX}")
    o = np.asarray(order.cpu().numpy() if torch.is_tensor(order) else order, np.int64)
    dp = np.asarray(doc_ptr, np.int64)
    cnt = np.asarray(counts)
    out = np.zeros((o.size, GS_LDS_UMAX), np.float64)
    item = np.flatnonzero(o >= 0)
    s0 = dp[o[item]]
    n = dp[o[item] + 1] - s0
    item, s0, n = item[n > 0], s0[n > 0], n[n > 0]
    if item.size:
        W = -(-n // U)
        nch = -(-n // W)
        # only these documents' counts, back to back (the corpus' other entries are never touched: the
        # table is built inside the engine's setup time); a chunk then ends where the next one starts
        own = np.concatenate([cnt[a:a + m] for a, m in zip(s0.tolist(), n.tolist())])
        if own.dtype != np.int64:                     # int64 counts (Corpus) are summed as they are: exact, no cast
            own = own.astype(np.float64)
        rep = np.repeat(np.arange(item.size), nch)
        j = np.arange(rep.size) - np.repeat(np.cumsum(nch) - nch, nch)
        out[item[rep], j] = np.add.reduceat(own, (np.cumsum(n) - n)[rep] + j * W[rep])
    return torch.from_numpy(out).to(device)


def gs_et_rows(csc_ent, order, doc_ptr, gs_updates: int):
    """int32 per slot of ``csc_ent`` (device; every entry lies in a document of ``order``): item slot *
    GS_LDS_UMAX + the entry's chunk (position in the document // W), the row of ``gs_estep(et=...)``'s table
    that holds the E its c.phi row is computed with.  The per-document values (a few rows) come from the
    host ``doc_ptr``; the per-slot work is device gathers."""
    import numpy as np
    dev = csc_ent.device
    o = np.asarray(order.cpu().numpy() if torch.is_tensor(order) else order, np.int64)
    dp = np.asarray(doc_ptr, np.int64)
    slot = np.flatnonzero(o >= 0)
    s0 = dp[o[slot]]
    n = dp[o[slot] + 1] - s0
    slot, s0, n = slot[n > 0], s0[n > 0], n[n > 0]     # an empty document shares its start with the next one
    if slot.size == 0:
        if csc_ent.numel():
            raise ValueError("gs_et_rows: entries but no document")
        return torch.zeros(0, dtype=torch.int32, device=dev)
    srt = np.argsort(s0, kind="stable")
    slot, s0, n = slot[srt], s0[srt], n[srt]
    W = -(-n // int(gs_updates))
    t_s0, t_W, t_base = torch.from_numpy(np.stack([s0, W, slot * GS_LDS_UMAX])).to(dev)     # one upload
    ent = csc_ent.long()
    i = (torch.searchsorted(t_s0, ent, right=True) - 1).clamp_(min=0)             # the entry's document
    # no read-back to validate (a device synchronise inside the engine's setup time): the caller's entries are
    # those of these documents by construction (csc_subset over the same documents), and the clamp keeps any
    # other entry's row inside its document's GS_LDS_UMAX rows
    chunk = ((ent - t_s0[i]) // t_W[i]).clamp_(0, GS_LDS_UMAX - 1)
    return (t_base[i] + chunk).to(torch.int32)


def gs_estep(doc_ptr, word_idx, counts, order, beta, K, gs_updates, params, gamma, cphi, lik, alpha_ss, iters, variant,
             dbg=None, ent_base=None, stage: Optional["GSStage"] = None, csum=None, et=None):
    """One launch of the fp64 block Gauss-Seidel E-step over the documents in ``order``.
    ``params``: the device parameter block {alpha, lgamma constant, VAR_MAX_ITER, VAR_CONVERGED, done}.
    ``ent_base``: ``cphi`` is a window starting at that corpus entry (_cphi_ptr).
    ``stage``: the GSStage of this (kGsTeam8) launch, filled by ``gs_stage`` from the current beta.
    ``csum`` (kGsTeam8, KS <= 32, U <= 32): the launch's chunk count sums (``gs_chunk_sums``).
    ``et`` (same launches) [n_items * 32 * KS] float64: the deferred final pass -- the kernel leaves every
    chunk's final-sweep E there and writes no c.phi rows; ``gs_suff64(recomp=...)`` recomputes them."""
    D = doc_ptr.numel() - 1
    nnz = word_idx.numel()
    V, KS = beta.shape
    if KS not in compiled_ks():
        raise ValueError(f"beta row stride {KS} has no compiled kernel")
    if not (0 < K <= KS):
        raise ValueError("K out of range")
    if not (1 <= int(gs_updates) <= gs_umax(KS)):
        raise ValueError(f"gs_updates must be in [1, {gs_umax(KS)}] at KS {KS}")
    if variant not in (GS_TINY, GS_TEAM1, GS_TEAM4, GS_TEAM8, GS_SMALL, GS_CHAIN):
        raise ValueError(f"unknown gs variant {variant}")
    dev = beta.device
    args = [
        _chk(doc_ptr, torch.int32, "doc_ptr", (D + 1,), dev),
        _chk(word_idx, torch.int32, "word_idx", (nnz,), dev),
        _chk(counts, torch.float32, "counts", (nnz,), dev),
        _chk(order, torch.int32, "order", None, dev), order.numel(),
        _chk(beta, torch.float64, "beta", (V, KS), dev), int(K), int(KS), int(gs_updates),
        _params_ptr(params, dev) or _bad("params"),
        _chk(gamma, torch.float64, "gamma", (D, KS), dev),
        _cphi_ptr(cphi, nnz, KS, dev, ent_base),
        _chk(lik, torch.float64, "lik", (D,), dev),
        _chk(alpha_ss, torch.float64, "alpha_ss", (D,), dev),
        _chk(iters, torch.int32, "iters", (D,), dev),
        int(variant), _stream(), 0 if dbg is None else _chk(dbg, torch.int64, "dbg", (16,), dev),
        0 if stage is None else _chk(stage.buf, torch.float64, "stage", None, dev),
        0 if stage is None else _chk(stage.stage_off, torch.int64, "stage_off", (order.numel(),), dev),
        0 if csum is None else _chk(csum, torch.float64, "csum", (order.numel(), GS_LDS_UMAX), dev),
        0 if et is None else _chk(et, torch.float64, "et", (order.numel() * GS_LDS_UMAX * KS,), dev),
    ]
    _need_pad_row(beta)
    if stage is not None and (variant != GS_TEAM8 or KS != stage.KS):
        raise ValueError("staged rows: kGsTeam8 launches of the stage's KS only")
    if (csum is not None or et is not None) and (variant != GS_TEAM8 or KS > 32 or int(gs_updates) > GS_LDS_UMAX):
        raise ValueError("chunk sums / deferred final pass: kGsTeam8 launches at KS <= 32, U <= 32 only")
    if order.numel() == 0:
        return
    lib().gs_estep(*args)


def gs_suff64(word_ptr, csc_ent, plan: "SuffPlan", cphi, cw, part, gate=None, scalars=None, base=None, recomp=None):
    """class_word[w] = sum of the cphi rows of w's corpus entries (CSC order, fp64, no atomics) + per-workgroup
    partial rows part[b] = {lik slice, alpha_ss slice, column sums} for ``colsum_partials``.
    ``base`` [V, KS] (optional): added to each written row first (cw[w] = base[w] + sum).
    ``recomp`` = (beta, et, et_row, counts) (KS <= 32): the rows are not read from ``cphi`` but recomputed,
    bitwise as the deferred longest-document launch (``gs_estep(et=...)``) would have written them, from the
    word's beta row, the chunk E at row ``et_row[s]`` (``gs_et_rows``) of ``et`` and the entry's count."""
    V, KS = cw.shape
    nnz = cphi.shape[0]            # csc_ent may be a subset of the corpus entries (csc_subset)
    dev = cw.device
    if plan.covers_all and plan.order.numel() != V:
        raise ValueError("suff plan does not cover the vocabulary")
    if plan.order.numel() == 0:
        return
    if csc_ent.numel() > nnz:
        raise ValueError("csc_ent longer than the corpus")
    if part.dim() != 2 or part.shape[1] != KS + 2 or part.shape[0] < max(plan.n_blocks, 1):
        raise ValueError(f"part: shape {tuple(part.shape)}, expected [>= {plan.n_blocks}, {KS + 2}]")
    if KS > 32:
        _need_pad_row(cphi)        # paired row loads read up to one row past the last entry
    if scalars is None:
        lik = ass = 0
        lo = hi = 0
    else:
        D = scalars[0].numel()
        lik, ass, lo, hi = _scalar_slice(scalars, D, dev)
    rc = (0, 0, 0, 0)
    if recomp is not None:
        r_beta, r_et, r_row, r_cnt = recomp
        if KS > 32 or r_et.numel() % (GS_LDS_UMAX * KS):
            raise ValueError("recomputed rows: KS <= 32 and et of [n_items * 32 * KS]")
        # et_row / csc_ent values are bounds-checked where they are built (gs_et_rows, csc_subset)
        rc = (_chk(r_beta, torch.float64, "beta", (V, KS), dev), _chk(r_et, torch.float64, "et", None, dev),
              _chk(r_row, torch.int32, "et_row", (csc_ent.numel(),), dev),
              _chk(r_cnt, torch.float32, "counts", (nnz,), dev))
    lib().gs_suff64(
        _chk(word_ptr, torch.int32, "word_ptr", (V + 1,), dev), _chk(csc_ent, torch.int32, "csc_ent", None, dev),
        _chk(plan.order, torch.int32, "order", (plan.order.numel(),), dev), plan.n_heavy, plan.n_medium, plan.n_light,
        _chk(cphi, torch.float64, "cphi", (nnz, KS), dev), _chk(cw, torch.float64, "cw", (V, KS), dev),
        _chk(part, torch.float64, "part", None, dev), lik, ass, lo, hi, int(KS), _gate_ptr(gate, dev), _stream(),
        0 if base is None else _chk(base, torch.float64, "base", (V, KS), dev), *rc)


def csc_subset(word_ptr, csc_ent, csc_doc, doc_mask):
    """(word_ptr, csc_ent) of the CSC slots whose document is in ``doc_mask`` (bool [D], device), slot
    order kept; plus the per-word entry counts on the host (for a SuffPlan)."""
    from . import sortgroup as SG
    keep = SG.gather(doc_mask, csc_doc)
    ce, before = SG.compact(csc_ent, keep)       # before[s]: kept slots ahead of slot s
    ptr = SG.gather(before, word_ptr)            # word w's kept slots start where its slots do
    return ptr.to(torch.int32), ce.contiguous(), (ptr[1:] - ptr[:-1]).cpu().numpy()


def csc_docs(perm, doc_ptr, nnz: int):
    """(csc_ent, csc_doc) int32 [nnz] from the int64 permutation of the stable word-id sort: the CSR entry of
    every CSC slot and that entry's document (``doc_ptr`` int32 [D + 1] on the device), one launch."""
    dev = perm.device
    D = doc_ptr.numel() - 1
    ent = torch.empty(nnz, dtype=torch.int32, device=dev)
    doc = torch.empty(nnz, dtype=torch.int32, device=dev)
    lib().csc_docs(_chk(perm, torch.int64, "perm", (nnz,), dev), _chk(doc_ptr, torch.int32, "doc_ptr", (D + 1,), dev),
                   int(D), int(nnz), ent.data_ptr(), doc.data_ptr(), _stream())
    return ent, doc


def csc_partition(csc_ent, csc_doc, word_ptr, late, n_early: int, n_late: int, et_tables=None):
    """The early / late CSC split in one partition pass (csrc/hip/corpus_plan.hip): the slots whose document has
    ``late[d] != 0`` (uint8 [D], device) against the others, slot order kept -- what two ``csc_subset`` calls
    return as (word_ptr, csc_ent), with the two sides' slot counts given by the caller (the host plan's
    histogram; they bound the lists).  ``et_tables`` = (s0, W, base) int32 [D]: also ``gs_et_rows`` of the
    late slots, et_row = base[doc] + min((entry - s0[doc]) // W[doc], GS_LDS_UMAX - 1).
    Returns dict(ceE, ceL, wpE, wpL, et_row)."""
    dev = csc_ent.device
    nnz, V, D = csc_ent.numel(), word_ptr.numel() - 1, late.numel()
    n_early, n_late = int(n_early), int(n_late)
    if n_early < 0 or n_late < 0 or n_early + n_late != nnz:
        raise ValueError(f"csc_partition: {n_early} early + {n_late} late slots, {nnz} in the CSC")
    ce = torch.empty(nnz, dtype=torch.int32, device=dev)           # [early | late]
    wp = torch.empty(2, V + 1, dtype=torch.int32, device=dev)
    n_tiles = max(1, -(-nnz // int(lib().csc_part_tile())))
    scratch = torch.empty(n_tiles + nnz + 1, dtype=torch.int32, device=dev)     # [tile sums | late slots ahead]
    et_row, tabs = None, (0, 0, 0)
    if et_tables is not None:
        et_row = torch.empty(n_late, dtype=torch.int32, device=dev)
        tabs = tuple(_chk(t, torch.int32, "et table", (D,), dev) for t in et_tables)
    ceE, ceL = ce[:n_early], ce[n_early:]
    lib().csc_partition(_chk(csc_ent, torch.int32, "csc_ent", (nnz,), dev),
                        _chk(csc_doc, torch.int32, "csc_doc", (nnz,), dev),
                        _chk(word_ptr, torch.int32, "word_ptr", (V + 1,), dev), _chk(late, torch.uint8, "late", (D,), dev),
                        nnz, V, D, n_early, n_late, ceE.data_ptr(), ceL.data_ptr(), wp[0].data_ptr(), wp[1].data_ptr(),
                        scratch.data_ptr(), scratch[n_tiles:].data_ptr(), 0 if et_row is None else et_row.data_ptr(),
                        *tabs, GS_LDS_UMAX, _stream())
    return dict(ceE=ceE, ceL=ceL, wpE=wp[0], wpL=wp[1], et_row=et_row)


def engine_plan_thresholds(KS: int, U: int) -> dict:
    """The thresholds of the native engine plan (ops/native.py ``engine_plan``), each from the Python
    definition that owns it: GSPlan's edges and isolate_longest arguments, gs_tiny_max, SuffPlan's
    heavy / light bounds, GS_LDS_UMAX."""
    return dict(edges=GSPlan.EDGES_NARROW, tiny_variant=GS_TINY, team8_variant=GS_TEAM8,
                tiny=min(gs_tiny_max(KS), int(U)), heavy=SuffPlan.HEAVY, light=SuffPlan.LIGHT, umax=GS_LDS_UMAX,
                iso_m=GSPlan.ISO_M, xcds=GSPlan.XCDS)


def suff_group_plan(lens, V: int):
    """Host plan of the per-stream suff-stats (LDAEngine._build_suff_groups).  lens[g]: entries of each word
    in stream g's documents.  Per stream: ``unique`` -- words whose entries all lie in g (stream 0 also
    takes the words with no entry, written as zero rows), ``multi`` -- words shared with another stream,
    whose rows go to scratch rows off[g] + i; the combine CSC (wp, ce) lists, per shared word, its scratch
    rows in stream order.  None when no word is shared."""
    import numpy as np
    present = np.stack([np.asarray(ln) > 0 for ln in lens])
    nper = present.sum(0)
    multi = nper > 1
    unique, mlist, off = [], [], []
    rows = 0
    wcat, gcat, rcat = [], [], []
    for gi in range(len(lens)):
        u = np.flatnonzero(present[gi] & ~multi)
        if gi == 0:
            u = np.union1d(u, np.flatnonzero(nper == 0))
        mw = np.flatnonzero(present[gi] & multi)
        unique.append(u), mlist.append(mw), off.append(rows)
        if mw.size:
            wcat.append(mw), gcat.append(np.full(mw.size, gi)), rcat.append(rows + np.arange(mw.size))
            rows += int(mw.size)
    if rows == 0:
        return None
    w_all, g_all, r_all = np.concatenate(wcat), np.concatenate(gcat), np.concatenate(rcat)
    o = np.lexsort((g_all, w_all))                   # by word, then stream order
    cnt = np.bincount(w_all, minlength=V).astype(np.int64)
    wp = np.zeros(V + 1, np.int64)
    wp[1:] = np.cumsum(cnt)
    return dict(unique=unique, multi=mlist, off=off, rows=rows, wp=wp, ce=r_all[o], cnt=cnt,
                shared=np.flatnonzero(multi))


def csc_compact(word_ptr, csc_ent, words):
    """(word_ptr, csc_ent) of the CSC columns ``words`` (host ids), renumbered 0 .. len(words) - 1, slot
    order kept (a compact sub-CSC for a gs_suff64 pass into a scratch of len(words) rows)."""
    import numpy as np
    from . import sortgroup as SG
    dev = word_ptr.device
    w = torch.from_numpy(np.asarray(words, np.int64)).to(dev)
    st = SG.gather(word_ptr, w).long()
    ln = SG.gather(word_ptr, w + 1).long() - st
    ptr = torch.zeros(w.numel() + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(ln, 0)
    tot = int(ptr[-1])
    idx = SG.gather(st - ptr[:-1], SG.segment_ids(ln, tot)) + torch.arange(tot, device=dev)
    return ptr.to(torch.int32), SG.gather(csc_ent, idx).contiguous()


def gs_mstep_control(cw, class_total, beta, K, scalars, params, ctl, hist, done_count, rows=None, newton=None,
                     stages=(), word_idx=None):
    """fp64 M-step (beta = cw / class_total, exp(-100) floor) + alpha Newton + device EM control step.
    ``stages`` (at most 2 GSStage, with the corpus ``word_idx``): their staged rows refilled by trailing
    workgroups of the same launch, from cw / class_total (bit-equal to gs_stage from the new beta)."""
    V, KS = cw.shape
    dev = cw.device
    sets = []
    for st in stages:
        if st.KS != KS:
            raise ValueError(f"staged rows of KS {st.KS}, cw has {KS}")
        if st.n_tiles:
            sets.append((_chk(st.tile_ent, torch.int32, "tile_ent", (st.n_tiles,), dev),
                         _chk(st.tile_cnt, torch.int32, "tile_cnt", (st.n_tiles,), dev),
                         _chk(st.buf, torch.float64, "stage", None, dev), int(st.n_tiles)))
    if len(sets) > 2:
        raise ValueError("gs_mstep_control: at most 2 staged sets")
    wi = _chk(word_idx, torch.int32, "word_idx", None, dev) if sets else 0
    slots = hist.numel() // HIST_COLS
    n_rows = 0 if rows is None else int(rows.numel())
    rows_ptr = 0 if rows is None else _chk(rows, torch.int32, "rows", (n_rows,), dev)
    lib().gs_mstep_control(
        _chk(cw, torch.float64, "cw", (V, KS), dev), _chk(class_total, torch.float64, "class_total", (KS,), dev),
        _chk(beta, torch.float64, "beta", (V, KS), dev), int(V), int(K), int(KS),
        _chk(scalars, torch.float64, "scalars", (2,), dev), _chk(params, torch.float64, "params", (PARAM_COUNT,), dev),
        _chk(ctl, torch.float64, "ctl", (8,), dev), _chk(hist, torch.float64, "hist", (slots * HIST_COLS,), dev),
        int(slots), _chk(done_count, torch.int32, "done_count", (1,), dev), _stream(), rows_ptr, n_rows,
        0 if newton is None else 1, 0 if newton is None else int(bool(newton[0])),
        0.0 if newton is None else float(newton[1]),
        0 if newton is None else _chk(newton[2], torch.float64, "alpha_out", (1,), dev), wi, sets)


def gs_mstep(cw, class_total, beta, K, gate=None):
    V, KS = cw.shape
    dev = cw.device
    lib().gs_mstep(_chk(cw, torch.float64, "cw", (V, KS), dev),
                   _chk(class_total, torch.float64, "class_total", (KS,), dev),
                   _chk(beta, torch.float64, "beta", (V, KS), dev), int(V), int(K), int(KS), _gate_ptr(gate, dev),
                   _stream())


def split_spec(KS: int) -> dict:
    """The split-document plan of ONI_GS_SPLIT_MIN = 'N[,g=G][,batches=B][,words=W]': documents longer
    than N words split (default 2048 at KS > 32, 0 = off at KS <= 32), at most G workgroups per document
    (SPLIT_MAX_SEG), B launch batches (1), W words of a chunk per workgroup (0: the split kernel's
    prefetched rounds, split_seg_words)."""
    from .. import knobs
    spec = (knobs.get("ONI_GS_SPLIT_MIN") or "").strip()
    out = dict(min=2048 if KS > 32 else 0, g=SPLIT_MAX_SEG, batches=1, words=0)
    if spec:
        head, *rest = [x.strip() for x in spec.split(",")]
        if head:
            out["min"] = int(head)
        for kv in rest:
            k, v = kv.split("=")
            if k.strip() not in ("g", "batches", "words"):
                raise ValueError(f"ONI_GS_SPLIT_MIN: unknown field {k!r} in {spec!r}")
            out[k.strip()] = int(v)
    return out


def gs_split_launch_cap(KS: int) -> int:
    """Workgroups per gs_split launch: 3/4 of the co-resident capacity (occupancy API x CUs), so a
    launch's segments are resident together with room for the other streams' buckets;
    ONI_SPLIT_MAX_BLOCKS lowers it (tests, shared / partitioned GPUs)."""
    from .. import knobs
    cap = max(1, int(lib().gs_split_capacity(int(KS))) * 3 // 4)
    env = knobs.get("ONI_SPLIT_MAX_BLOCKS")
    if env:
        cap = max(1, min(cap, int(env)))
    return cap


SPLIT_MAX_SEG = 128        # csrc/hip/gs_split.hip kSplitMaxSeg2 (segments per document)
SPLIT_MAX_SEG_GATHER = 16  # kSplitMaxSeg: up to here one batched gather per chunk, above it the two-phase exchange


def gs_team8_words(KS: int) -> int:
    """Words of a chunk one 8-wave fp64 workgroup holds in its prefetched rounds (TeamShape<KS, 8>:
    slots x RMAX)."""
    tg = 4 if KS <= 32 else (8 if KS <= 64 else 16)
    kpl = -(-KS // tg)
    return 8 * (64 // tg) * (8 if kpl <= 5 else 4)


def split_seg_words(KS: int) -> int:
    """Words of a chunk one split segment holds in its prefetched rounds: the split kernel's 7 word waves
    (gs_splitw: TeamShape<KS, 8> slots and RMAX) -- a segment past it streams the rest one gather latency
    per round."""
    return gs_team8_words(KS) * 7 // 8


def split_seg_target(KS: int) -> int:
    """Smallest useful share of a chunk per split segment (words), the water-filling's cap on a document's
    segments (G <= ceil(W / target)): the split kernel's prefetched rounds at K = 100 (112 words); at KS <= 64
    (8-lane topic groups, 224 prefetched words) 96 -- the 1-day corpus at K = 50 per EM iteration: 3.15 ms with
    the prefetch-sized cap (its longest document on 4 segments), 2.94 / 2.58 / 2.88 / 3.6 ms with fixed
    shares of 128 / 96 / 64 / 48 words (profiles/r6z_split_k50.md)."""
    return 96 if KS <= 64 else split_seg_words(KS)


def split_chain_cycles(n: int, U: int, G: int, KS: int) -> float:
    """Modelled cycles of one chunk of an n-word document on G segments (G = 1: the 8-wave team kernel),
    for the plan's segment allocation only (profiles/r6_split.md): a word-phase term per word of the
    segment's share plus the exchange (one batched gather up to 16 segments, two round trips beyond)."""
    W = -(-n // U)
    per = -(-W // G)
    sw = split_seg_words(KS)
    # prefetched rounds cost ~issue + compute; streamed rounds a gather latency each
    word = 40.0 * min(per, sw) + (1800.0 * -(-(per - sw) // sw) if per > sw else 0.0) + 2000.0
    if G == 1:
        return word
    # the exchange's steps past 4 segments grow with the granules a segment reads: (KS + 1) columns each.
    # Fitted at K = 100; at K = 50 the unscaled steps stopped the 1-day corpus' longest document at 4 segments,
    # 3.15 ms per EM iteration against 2.58 with 8 (profiles/r6z_split_k50.md)
    step = 0.0 if G <= 4 else 2500.0 if G <= 8 else 8000.0 if G <= SPLIT_MAX_SEG_GATHER else 6000.0
    xch = 4000.0 + step * (KS + 1) / 101.0
    return word + xch + 1500.0


class GSSplitPlan:
    """Launch batches of the fp64 split-document kernel (gs_split): document d of n words (W = ceil(n / U)
    words per chunk) gets G workgroups, each taking 1/G of every chunk; a batch holds
    <= gs_split_launch_cap(KS) workgroups (co-resident, so the per-chunk exchange cannot deadlock).

    G per document is water-filled over the launch cap: every candidate starts at G = 1 (the 8-wave team
    kernel), and the document whose modelled chunk time (split_chain_cycles) is the largest gets more
    segments, until the cap is spent or that document is at its most useful G = ceil(W / seg_words) (at most
    SPLIT_MAX_SEG): the launch shortens the longest chain first; the budget left gives the other candidates
    two segments each, longest first.  Documents still at G = 1 stay with the team kernel (``leftover``),
    unless ``max_batches`` > 1 (ONI_GS_SPLIT_MIN batches=B, default 1) allows more batches of the rest
    (back to back on one stream: a later batch lengthens the critical path)."""

    def __init__(self, doc_ids, lengths, KS: int, gs_updates: int, device, seg_words: int = 0,
                 max_seg: int = 0, max_batches: int = 0):
        import heapq
        import numpy as np
        self.KS = int(KS)
        self.max_blocks = gs_split_launch_cap(KS)
        sp = split_spec(KS)
        # an explicit segment size (ONI_GS_SPLIT_MIN words=W, or the argument) fixes G = clamp(ceil(W / words),
        # 2, max_seg) per document, longest first; otherwise the modelled water-filling (_allocate)
        # KS <= 64: fixed 96-word shares by default -- measured ahead of the water-filling there (2.58 vs 2.74 ms
        # per EM iteration at K = 50, profiles/r6z_split_k50.md), where the model was fitted at K = 100
        self.fixed = bool(int(seg_words) or sp["words"]) or self.KS <= 64
        self.seg_words = int(seg_words) or sp["words"] or split_seg_target(KS)
        # KS <= 32: the single-round gather only (gs_splitw has no two-phase exchange in the narrow layout)
        max_seg = min(int(max_seg) or sp["g"], self.max_blocks,
                      SPLIT_MAX_SEG if self.KS > 32 else SPLIT_MAX_SEG_GATHER)
        max_batches = int(max_batches) or sp["batches"]
        U = int(gs_updates)
        self.U = U
        self.tab_lds = U <= gs_split_lds_umax(self.KS)
        self.segments = {}
        self.batches = []
        self.leftover = []
        todo = [int(d) for d in doc_ids]
        while todo and len(self.batches) < max_batches:
            G = self._allocate(todo, lengths, U, max_seg)
            docs = [(d, G[d]) for d in todo if G[d] >= 2]
            if not docs:
                break
            for d, g in docs:
                self.segments[d] = g
            self.batches.append(self._make(docs, lengths, device))
            done = {d for d, _ in docs}
            todo = [d for d in todo if d not in done]
        self.leftover = todo
        self.n_docs = len(self.segments)

    def _allocate(self, docs, lengths, U, max_seg):
        """Water-filling: segments to the document with the longest modelled chunk, within the cap."""
        import heapq
        G = {d: 1 for d in docs}
        if self.fixed:
            used = 0
            for d in docs:
                W = -(-int(lengths[d]) // U)
                g = min(max(2, -(-W // self.seg_words)), max_seg, W)
                if g >= 2 and used + g <= self.max_blocks:
                    G[d] = g
                    used += g
            return G
        gmax = {}
        for d in docs:
            W = -(-int(lengths[d]) // U)
            # a document with W >= 2 words per chunk can always take two segments
            gmax[d] = 1 if W < 2 else max(2, min(max_seg, W, -(-W // self.seg_words)))
        t = lambda d, g: split_chain_cycles(int(lengths[d]), U, g, self.KS)   # noqa: E731
        heap = [(-t(d, 1), d) for d in docs if gmax[d] >= 2]
        heapq.heapify(heap)
        used = 0
        while heap:
            tc, d = heapq.heappop(heap)
            g = G[d]
            # the fewest more segments that shorten it (the exchange's cost steps up at 5, 9 and 17 segments);
            # one workgroup -> G segments costs G launch slots
            gn = next((x for x in range(max(2, g + 1), gmax[d] + 1)
                       if used + x - (g if g > 1 else 0) <= self.max_blocks and t(d, x) < -tc), None)
            if gn is None:
                break     # the longest chain cannot shorten further: the rest cannot set the launch time
            used += gn - (g if g > 1 else 0)
            G[d] = gn
            heapq.heappush(heap, (-t(d, gn), d))
        # the budget left: two segments for each remaining candidate, longest first -- a co-resident split
        # launch is dispatched ahead of the short-document floods, where a 512-thread team workgroup can
        # queue behind them (K = 50: 4.5 -> 3.4 ms per EM iteration, profiles/r3_tuning_log.md)
        for d in docs:
            if G[d] == 1 and gmax[d] >= 2 and used + 2 <= self.max_blocks:
                G[d] = 2
                used += 2
        return G

    def _make(self, docs, lengths, device):
        import numpy as np
        sd, si, sc, sb, slot = [], [], [], [], []
        for j, (d, G) in enumerate(docs):
            base = len(sd)
            for q in range(G):
                sd.append(d), si.append(q), sc.append(G), sb.append(base), slot.append(j)
        t = lambda a: torch.tensor(np.asarray(a, np.int32), device=device)
        nb = len(sd)
        gmx = SPLIT_MAX_SEG if self.KS > 32 else SPLIT_MAX_SEG_GATHER
        if sc and max(sc) > gmx:
            raise ValueError(f"gs_split: {max(sc)} segments per document > {gmx} at KS {self.KS}")
        if nb > self.max_blocks:
            raise ValueError(f"gs_split: {nb} workgroups > the launch cap {self.max_blocks}")
        # U past the LDS chunk tables: per-segment tables in a scratch ([n_blocks][tab_rows][2][KS] doubles),
        # tab_rows = the batch's largest chunk count (<= U)
        tab_rows = 0 if self.tab_lds else max(-(-int(lengths[d]) // -(-int(lengths[d]) // self.U)) for d, _ in docs)
        gr = 2 * (self.KS + 1)
        return dict(seg_doc=t(sd), seg_index=t(si), seg_count=t(sc), seg_base=t(sb), doc_slot=t(slot), n_blocks=nb,
                    # tagged granules {uint32 half of a double, uint32 tag}: [2][n_blocks][2 (KS + 1)] partials,
                    # then [2][docs][2 (KS + 1)] totals (the two-phase exchange past 16 segments)
                    xchg=torch.zeros(2 * nb * gr + 2 * len(docs) * gr, dtype=torch.int64, device=device),
                    counter=torch.zeros(2 * len(docs), dtype=torch.int32, device=device),
                    error=torch.zeros(1, dtype=torch.int32, device=device), docs=len(docs), tab_rows=tab_rows,
                    tab=(torch.empty(nb * tab_rows * 2 * self.KS, dtype=torch.float64, device=device)
                         if tab_rows else None))

    def chunk_sums(self, doc_ptr, counts) -> None:
        """Each batch document's chunk count sums ([docs][max nch] doubles, exact: integer counts) from the
        corpus' host doc_ptr / counts, for the kernel's C_j initialisation (built once per plan)."""
        import numpy as np
        for b in self.batches:
            docs = b["seg_doc"].cpu().numpy()[b["seg_base"].cpu().numpy() == np.arange(b["n_blocks"])]
            rows = []
            for d in docs:
                s0, s1 = int(doc_ptr[d]), int(doc_ptr[d + 1])
                n = s1 - s0
                W = -(-n // self.U)
                c = np.asarray(counts[s0:s1], np.float64)
                nch = -(-n // W)
                rows.append(np.add.reduceat(c, np.arange(0, n, W)) if n else np.zeros(0))
                assert rows[-1].size == nch
            width = max(1, max(r.size for r in rows))
            cs = np.zeros((len(rows), width), np.float64)
            for i, r in enumerate(rows):
                cs[i, :r.size] = r
            b["csum"] = torch.from_numpy(cs).to(b["seg_doc"].device)
            b["csum_u"] = self.U

    def scratch_bytes(self) -> int:
        """Device bytes of the batches' chunk-table scratch (counted in the c.phi budget)."""
        return sum(b["tab"].numel() * 8 for b in self.batches if b.get("tab") is not None)


def gs_split(doc_ptr, word_idx, counts, beta, K, gs_updates, params, gamma, cphi, lik, alpha_ss, iters, batch,
             dbg=None, ent_base=None):
    """One launch of the fp64 split-document E-step over one GSSplitPlan batch.  dbg: optional int64[8]
    phase timer of workgroup 0 (word phase, barrier 1, publish + gather, barrier 2, refresh, barrier 3,
    sweep end, chunks)."""
    D = doc_ptr.numel() - 1
    nnz = word_idx.numel()
    V, KS = beta.shape
    dev = beta.device
    nb = batch["n_blocks"]
    if KS not in compiled_ks():
        raise ValueError(f"beta row stride {KS} has no compiled kernel")
    if not (0 < K <= KS) or not (1 <= int(gs_updates) <= gs_split_umax(KS)):
        raise ValueError("K or gs_updates out of range")
    for k in ("seg_doc", "seg_index", "seg_count", "seg_base", "doc_slot"):
        _chk(batch[k], torch.int32, k, (nb,), dev)
    _need_pad_row(beta)
    lib().gs_split(
        _chk(doc_ptr, torch.int32, "doc_ptr", (D + 1,), dev), _chk(word_idx, torch.int32, "word_idx", (nnz,), dev),
        _chk(counts, torch.float32, "counts", (nnz,), dev), _chk(beta, torch.float64, "beta", (V, KS), dev),
        int(K), int(KS), int(gs_updates), _params_ptr(params, dev) or _bad("params"),
        _chk(gamma, torch.float64, "gamma", (D, KS), dev), _cphi_ptr(cphi, nnz, KS, dev, ent_base),
        _chk(lik, torch.float64, "lik", (D,), dev), _chk(alpha_ss, torch.float64, "alpha_ss", (D,), dev),
        _chk(iters, torch.int32, "iters", (D,), dev),
        batch["seg_doc"].data_ptr(), batch["seg_index"].data_ptr(), batch["seg_count"].data_ptr(),
        batch["seg_base"].data_ptr(), batch["doc_slot"].data_ptr(), int(nb),
        _chk(batch["xchg"], torch.int64, "xchg", (2 * (nb + batch["docs"]) * 2 * (KS + 1),), dev),
        _chk(batch["counter"], torch.int32, "counter", (2 * batch["docs"],), dev), int(batch["docs"]),
        _chk(batch["error"], torch.int32, "error", (1,), dev), _stream(),
        0 if dbg is None else _chk(dbg, torch.int64, "dbg", (8,), dev),
        *_split_tab(batch, nb, int(gs_updates), KS, dev, doc_ptr), *_split_csum(batch, int(gs_updates), dev))


def _split_csum(batch, U, dev):
    """(address, stride) of the batch's chunk count sums (GSSplitPlan.chunk_sums), (0, 0) if not built."""
    cs = batch.get("csum")
    if cs is None:
        return 0, 0
    if batch.get("csum_u") != U:
        raise ValueError(f"gs_split: chunk sums built for U = {batch.get('csum_u')}, launched with U = {U}")
    _chk(cs, torch.float64, "csum", (batch["docs"], cs.shape[1]), dev)
    return cs.data_ptr(), int(cs.shape[1])


def _split_tab(batch, nb, U, KS, dev, doc_ptr):
    """(scratch address, rows per workgroup) of the split batch's chunk tables (required past the LDS
    tables' U); the rows must cover every document's chunk count (the kernel also checks)."""
    tab = batch.get("tab")
    if U > gs_split_lds_umax(KS):
        rows = int(batch.get("tab_rows") or 0)
        if tab is None or rows <= 0 or tab.numel() < nb * rows * 2 * KS:
            raise ValueError(f"gs_split: U = {U} needs a chunk-table scratch of {nb} x rows x 2 x {KS} doubles")
        return _chk(tab, torch.float64, "tab", None, dev), rows
    return 0, 0


class GSPlan:
    """Length buckets of the fp64 block Gauss-Seidel E-step: (variant, int32 doc order) per launch.

    tiny (TG lanes per document, literal schedule) for n <= min(gs_tiny_max(KS), U); up to 256 words
    one wave per document at KS <= 32, 16 lanes per document at KS > 32 (gs_smallw); a 4-wave workgroup
    up to 2048; an 8-wave workgroup beyond."""
    EDGES = ((GS_TEAM8, 2048, None), (GS_TEAM4, 256, 2048), (GS_SMALL, None, 256))
    # KS <= 32: documents up to GS_SMALL_MAX words go to the 16-lanes-per-document kernel
    EDGES_NARROW = ((GS_TEAM8, 2048, None), (GS_TEAM4, 256, 2048), (GS_TEAM1, GS_SMALL_MAX, 256),
                    (GS_SMALL, None, GS_SMALL_MAX))
    ISO_M, XCDS = 1, 8   # isolate_longest(o, m, xcds) of the team8 bucket at KS <= 32

    @classmethod
    def from_arrays(cls, KS: int, plan, tiny_max: int) -> "GSPlan":
        """A plan without split documents from (variant, device order) pairs (the native engine plan's)."""
        self = cls.__new__(cls)
        self.KS, self.doc_range, self.split = int(KS), None, None
        self.plan = list(plan)
        self.tiny_max = int(tiny_max)
        return self

    def __init__(self, lengths, KS: int, gs_updates: int, device, split_min: Optional[int] = None,
                 doc_range=None):
        import numpy as np
        self.KS = int(KS)
        L = np.asarray(lengths, dtype=np.int64)
        # doc_range (d0, d1): only documents d0 <= d < d1 (one c.phi window of the engine); the stable
        # sort of the range equals the range's documents in the stable sort of all of them
        self.doc_range = None if doc_range is None else (int(doc_range[0]), int(doc_range[1]))
        if self.doc_range is None:
            order = argsort_desc_stable(L).astype(np.int32)
        else:
            d0, d1 = self.doc_range
            order = (d0 + argsort_desc_stable(L[d0:d1])).astype(np.int32)
        # documents longer than split_min words: one document over several workgroups (gs_split);
        # default on for KS > 32 (the topic-group team kernels' chunk of a long document is bound
        # by one CU's row gathers), ONI_GS_SPLIT_MIN overrides (0: off; split_spec)
        # K > 32: 2048 (the whole team8 range) -- at 4096 the 2-4 k-word documents' 512-thread
        # workgroups were dispatched behind the short-document floods in some iterations (a bimodal
        # 2.75 / 4.5 ms team8 bucket); one co-resident split launch holds them all: K = 50 4.53 / 4.73
        # -> 3.36 / 3.34 ms per EM iteration (profiles/r3_tuning_log.md)
        if split_min is None:
            split_min = split_spec(KS)["min"]
        if int(gs_updates) > gs_split_umax(KS):
            split_min = 0       # KS <= 32: the split kernel's chunk tables live in LDS (U <= 32)
        self.split = None
        if split_min > 0 and (L > split_min).any():
            m = L[order] > split_min
            sp = GSSplitPlan(order[m], L, KS, gs_updates, device)
            if sp.n_docs:
                self.split = sp
                keep = np.ones(len(order), bool)
                keep[np.flatnonzero(m)] = ~np.isin(order[m], np.asarray(sorted(sp.segments), np.int64))
                order = order[keep]
        Ls = L[order]
        tiny = min(gs_tiny_max(KS), int(gs_updates))
        self.plan = []
        # team8 at KS <= 32: the longest document first in a workgroup order that gives it an XCD of its own
        # under round-robin dispatch (isolate_longest, a speed hint)
        iso = self.ISO_M if KS <= 32 else 0
        edges = self.EDGES_NARROW if KS <= 32 else self.EDGES
        if int(gs_updates) > 32:
            edges = self.wide_u_edges(int(gs_updates)) if KS > 32 else self.narrow_wide_u_edges(int(gs_updates))
        for var, lo, hi in edges:
            lo_ = tiny if lo is None else lo
            m = (Ls > lo_) if hi is None else ((Ls > lo_) & (Ls <= hi))
            if not m.any():
                continue
            o = order[m].copy()
            if var == GS_TEAM8 and iso > 0:
                o = self.isolate_longest(o, min(iso, 8), self.XCDS)
            self.plan.append((var, torch.from_numpy(o).to(device)))
        m = Ls <= tiny
        if m.any():
            self.plan.append((GS_TINY, torch.from_numpy(order[m].copy()).to(device)))
        self.tiny_max = tiny
        # (the other buckets leaving the longest document's XCD to it measured slower twice and is gone:
        # 2.20 / 2.27 vs 2.18 / 2.18 ms, then 1.746 / 1.742 / 1.761 vs 1.734 / 1.733 / 1.739 ms per EM
        # iteration; profiles/r2_tuning_log.md, r3_tuning_log.md)

    CHAIN_MAX_W = 2   # widest chunk (words) the one-wave per-word chain kernel takes (csrc/hip/kernels.h kGsChain)

    @classmethod
    def wide_u_edges(cls, U: int):
        """Team sizes by CHUNK WIDTH at K > 32 and U > 32 (the c.phi-table team kernels): a team's waves
        split a chunk's W = ceil(n / U) words, so at lda-c's per-word schedule (U = 1024: W = 1 for every
        document up to 1,024 words) a 4- or 8-wave team idles all but one word slot and pays two
        workgroup barriers per word, where one wave per document refreshes in-wave with no barrier.
        Documents of <= 256 words keep the 16-lane kernel (gs_smallw: throughput); above, up to W = 4 words per
        chunk, a per-word chain of up to U refreshes per sweep runs on one wave per document with a topic per
        lane (gs_chain); four waves up to W = 16, eight beyond (never below the U = 32 edges).  K = 100 shard at
        U = 1024 (profiles/r4_tuning_log.md): fixed length edges 172.4 ms per EM iteration, (8, 64) 133.2,
        (4, 32) 107.3, (2, 16) 106.7 with the one-wave team as the first range; the 16-lane kernel's 7
        digamma/exp chains per lane cost more latency per refresh than one wave's 2 (r5g: 66.4 vs 43.1 ms)."""
        wc, w4 = cls.CHAIN_MAX_W, 16
        ec, e4 = max(256, wc * U), max(2048, w4 * U)
        return ((GS_TEAM8, e4, None), (GS_TEAM4, ec, e4), (GS_CHAIN, 256, ec), (GS_SMALL, None, 256))

    @classmethod
    def narrow_wide_u_edges(cls, U: int):
        """KS <= 32 at U > 32 (lda-c's per-word schedule at K = 20, an opt-in parity mode): the LDS-table
        kernels (gs_small, the one-wave and word-per-lane teams, gs_wsteam) cannot hold U chunk tables, so
        every document past the tiny kernel's range runs with its tables in the c.phi rows: the per-word chain
        kernel (one wave per document, a topic per lane) up to chunks of CHAIN_MAX_W words, then the 4- and
        8-wave topic-group teams (gs_team GMT) by chunk width as at KS > 32."""
        wc, w4 = cls.CHAIN_MAX_W, 16
        ec, e4 = wc * U, max(2048, w4 * U)
        return ((GS_TEAM8, e4, None), (GS_TEAM4, ec, e4), (GS_CHAIN, None, ec))

    @staticmethod
    def isolate_longest(o, m: int, xcds: int = 8):
        """Workgroup order of the team8 launch giving each of its m longest documents an XCD of its own:
        workgroup b runs on XCD b mod 8 under round-robin dispatch (a speed hint only), so slots b = x mod 8,
        x < m, stay empty (-1) after the first round.  The longest document's packed rows then have the XCD's
        L2 to themselves."""
        import numpy as np
        head, rest = list(o[:m]), list(o[m:])
        out = []
        b = 0
        while head or rest:
            if b % xcds < m:
                out.append(head.pop(0) if head else -1)
            else:
                out.append(rest.pop(0) if rest else -1)
            b += 1
        while out and out[-1] == -1:
            out.pop()
        return np.asarray(out, dtype=np.int32)
