"""MAXRESULTS selection against the unlimited path: ``rank_flagged(key, flag)[:N]`` (prefix sum + scatter over
all rows, sort of every flagged key) and ``rank_flagged(key, flag, N)`` (HIP radix select, sort of N keys), timed
alternately in one process on seeded keys (profiles/select_lowest.md).

    python scripts/select_bench.py [--shapes 2000000:0.25:3000,2000000:0.25:100000,100000000:0.01:3000]
                                   [--windows 7] [--window-s 0.25] [--json out.json]

Every window is bracketed by device events and runs its call often enough to last ``--window-s``; the calls end
in the host copy of their result, so a window holds whole calls.  Also times ``hip.select_lowest`` alone and
relates it to the bytes its passes read, computed from the shape: 6 histogram passes, the count and the write
pass each read the n flags and, where a row is flagged, its key -- at most 9 n bytes per pass.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oni_ml_amd.ops import hip as H  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X specification
ROW_PASSES = 8         # 6 histogram passes + count + write


def make_keys(n, frac, seed):
    """Log-uniform scores in [1e-9, 1e-2) and the flags of the TOL under which ``frac`` of them fall."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    key = torch.pow(10.0, torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 7.0 - 9.0)
    tol = 10.0 ** (7.0 * frac - 9.0)
    return key, (key < tol).to(torch.uint8), tol


def window(fn, reps):
    """Milliseconds per call of ``reps`` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def reps_for(fn, window_s):
    fn()                                   # warm-up: code objects, allocator
    t = max(window(fn, 2), 1e-3)
    return max(2, int(np.ceil(window_s * 1e3 / t)))


def stats(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000000:0.25:3000,2000000:0.25:100000,100000000:0.01:3000")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("select_bench: needs a GPU")
    H.lib()
    out = []
    for spec in a.shapes.split(","):
        n, frac, N = spec.split(":")
        n, frac, N = int(n), float(frac), int(N)
        key, flag, tol = make_keys(n, frac, a.seed)
        flagged = int(flag.sum())
        paths = dict(full_then_slice=lambda: S.rank_flagged(key, flag)[:N],
                     select_then_sort=lambda: S.rank_flagged(key, flag, N),
                     select_only=lambda: H.select_lowest(key, flag, N))
        same = bool(np.array_equal(paths["full_then_slice"](), paths["select_then_sort"]()))
        reps = {k: reps_for(f, a.window_s) for k, f in paths.items()}
        times = {k: [] for k in paths}
        for _ in range(a.windows):                 # alternate the paths window by window
            for k, f in paths.items():
                times[k].append(window(f, reps[k]))
        rec = dict(n=n, flagged=flagged, tol=tol, N=N, outputs_equal=same, windows=a.windows, reps=reps,
                   **{k: stats(v) for k, v in times.items()})
        pass_bytes = 9 * n
        floor_ms = ROW_PASSES * pass_bytes / HBM_PEAK * 1e3
        rec.update(bytes_per_pass=pass_bytes, row_passes=ROW_PASSES, hbm_floor_ms=round(floor_ms, 4),
                   select_share_of_hbm_peak=round(floor_ms / rec["select_only"]["median_ms"], 4),
                   speedup=round(rec["full_then_slice"]["median_ms"] / rec["select_then_sort"]["median_ms"], 3))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del key, flag
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if not all(r["outputs_equal"] for r in out):
        sys.exit("select_bench: the two paths returned different rows")


if __name__ == "__main__":
    main()
