"""--host-report aggregate: ``hip.host_summary`` (two atomic passes, csrc/hip/host_summary.hip) against its torch
twin ``reference.host_summary`` (two int64 radix sorts of all sides) on the same GPU tensors, timed alternately
in one process on seeded inputs (profiles/host_report.md).

    python scripts/host_report_bench.py [--shapes flow:1000000:2,dns:2000000:1,flow:100000000:2:5700000]
                                        [--windows 7] [--window-s 0.25] [--json out.json]

A shape is ``source:events:sides[:documents]``.  The documents of the sides are drawn in proportion to the
document lengths of the synthetic day of that source (``synthetic_flow_corpus`` / ``synthetic_dns_corpus`` at
``--corpus-events`` events: the pipeline's own distribution); when ``documents`` is given the length vector is
tiled to that many documents (config-5 scale: no synthetic day of 100 M events is built here).  Every shape also
runs as ``hot``: half of the sides on one document.  Scores are log-uniform in [1e-9, 1e-2) and TOL is the value
under which ``--flagged`` of them fall (default 0.025: the headline flow day flags 2.4 % of its events).

Every window is bracketed by device events and runs its call often enough to last ``--window-s``.  ``wrapper``
and ``twin_sorts`` are the two public calls, each with its host checks (the bounds of the rows: two host reads
per side array) and ending in the host copy of the skipped count, so a window holds whole calls.  ``launches``
is the launcher alone on buffers allocated once (4 memsets and the two passes; nothing read back), with the wave
fold and, as ``launches_nofold``, with one atomic per side; it is related to the bytes the passes must read:
12 B per side (int32 row + float64 score) in each of the two.  ``atomics_per_side``: the atomics issued after
the filters, counted by the kernel in a separate call.  Needs a GPU.
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
from oni_ml_amd.ops import reference as R  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X specification
SIDE_BYTES = 12        # int32 document row + float64 score, read once per pass
PASSES = 2


def doc_lengths(source, events):
    """Distinct words per document of the synthetic day, float64 on the GPU."""
    if source == "flow":
        from oni_ml_amd.pipeline.flow import synthetic_flow_corpus
        corpus, _ = synthetic_flow_corpus(events=events, seed=0, device="cuda", strict=False)
    else:
        from oni_ml_amd.pipeline.dns import synthetic_dns_corpus
        corpus, _ = synthetic_dns_corpus(events=events, seed=0, device="cuda", strict=False)
    ptr = np.asarray(corpus.doc_ptr, np.int64)
    return torch.from_numpy(np.diff(ptr).astype(np.float64)).cuda()


def draw_docs(lengths, D, n, g, hot):
    """int32 [n] document rows: proportional to ``lengths`` tiled to D documents (inverse CDF, in chunks); ``hot``:
    then half of them moved to the longest document."""
    w = lengths if D == lengths.numel() else lengths.repeat(-(-D // lengths.numel()))[:D]
    cdf = torch.cumsum(w, 0)
    cdf = cdf / cdf[-1]
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    step = 1 << 24
    for lo in range(0, n, step):
        u = torch.rand(min(step, n - lo), generator=g, device="cuda", dtype=torch.float64)
        out[lo:lo + u.numel()] = torch.searchsorted(cdf, u).clamp_max(D - 1).to(torch.int32)
        if hot:
            m = torch.rand(u.numel(), generator=g, device="cuda") < 0.5
            out[lo:lo + u.numel()][m] = int(torch.argmax(w))
    return out


def make_scores(n, g):
    return torch.pow(10.0, torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 7.0 - 9.0)


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


def launches(args, fold):
    """The launcher alone, on output buffers allocated once."""
    da, sa, db, sb, D, tol = args
    i32 = lambda: torch.empty(D, dtype=torch.int32, device="cuda")      # noqa: E731
    bufs = (i32(), i32(), torch.empty(D, dtype=torch.int64, device="cuda"), i32(),
            torch.empty(1, dtype=torch.int64, device="cuda"))
    L, st = H.lib(), torch.cuda.current_stream().cuda_stream
    ptr = [da.data_ptr(), sa.data_ptr(), db.data_ptr() if db is not None else 0, sb.data_ptr() if sb is not None else 0]
    return lambda: L.host_summary(*ptr, da.numel(), D, tol, *[b.data_ptr() for b in bufs], fold, 0, 0, st)


def equal(a, b):
    return all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="flow:1000000:2,dns:2000000:1,flow:100000000:2:5700000")
    ap.add_argument("--corpus-events", type=int, default=1_000_000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.25)
    ap.add_argument("--flagged", type=float, default=0.025, help="share of the sides under TOL")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("host_report_bench: needs a GPU")
    H.lib()
    tol = 10.0 ** (7.0 * a.flagged - 9.0)
    lengths = {}
    out = []
    for spec in a.shapes.split(","):
        f = spec.split(":")
        source, n, sides = f[0], int(f[1]), int(f[2])
        if source not in lengths:
            lengths[source] = doc_lengths(source, a.corpus_events if source == "flow" else 2 * a.corpus_events)
        D = int(f[3]) if len(f) > 3 else lengths[source].numel()
        for hot in (False, True):
            g = torch.Generator(device="cuda")
            g.manual_seed(a.seed)
            da, sa = draw_docs(lengths[source], D, n, g, hot), make_scores(n, g)
            db, sb = (draw_docs(lengths[source], D, n, g, hot), make_scores(n, g)) if sides == 2 else (None, None)
            args = (da, sa, db, sb, D, tol)
            paths = dict(launches=launches(args, True), launches_nofold=launches(args, False),
                         wrapper=lambda: H.host_summary(*args), twin_sorts=lambda: R.host_summary(*args))
            want = paths["twin_sorts"]()
            same = equal(H.host_summary(*args), want) and equal(H.host_summary(*args, fold=False), want)
            reps = {k: reps_for(fn, a.window_s) for k, fn in paths.items()}
            times = {k: [] for k in paths}
            for _ in range(a.windows):                 # alternate the paths window by window
                for k, fn in paths.items():
                    times[k].append(window(fn, reps[k]))
            ns = n * sides
            atom = {}
            for name, fold in (("fold", True), ("nofold", False)):
                c = H.host_summary(*args, fold=fold, stats=True)[5]
                atom[name] = dict(counts=round(c[0] / ns, 4), min_key=round(c[1] / ns, 6), worst=round(c[2] / ns, 6))
            ev = want[0]
            rec = dict(source=source, events=n, sides=ns, documents=D, hot=hot, tol=tol, longest_share=round(float(ev.max()) / ns, 4),
                       flagged_sides=int(want[1].sum()), outputs_equal=same, windows=a.windows, reps=reps,
                       **{k: stats(v) for k, v in times.items()}, atomics_per_side=atom)
            floor_ms = PASSES * SIDE_BYTES * ns / HBM_PEAK * 1e3
            rec.update(bytes_read=PASSES * SIDE_BYTES * ns, hbm_floor_ms=round(floor_ms, 4),
                       launches_share_of_hbm_peak=round(floor_ms / rec["launches"]["median_ms"], 4),
                       speedup_over_twin=round(rec["twin_sorts"]["median_ms"] / rec["wrapper"]["median_ms"], 2))
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del da, sa, db, sb, args, paths, want, ev
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if not all(r["outputs_equal"] for r in out):
        sys.exit("host_report_bench: the kernel and the twin returned different results")


if __name__ == "__main__":
    main()
