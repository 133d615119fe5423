"""--ensemble scoring: the fused kernel ``score_ensemble`` (csrc/hip/score_ensemble.hip) against the composition
the code without it allows -- R launches of ``score_events`` on R separate [rows, K] table pairs, torch adds in
member order, the divide, the min and the compare -- timed alternately in one process (profiles/ensemble_score.md).

    python scripts/ensemble_bench.py [--shapes flow:1000000:2:8,dns:2000000:1:4,flow:1000000:2:1] [--topics 20]
                                     [--samples 20] [--json out.json] [--pipeline-events 1000000 --pipeline-r 8]

A shape is ``source:events:sides:R``.  The tables have the rows of the synthetic day of that source and size
(``synthetic_flow_corpus`` / ``synthetic_dns_corpus``); document rows are drawn in proportion to the documents'
word counts and word rows in proportion to the words' counts (the pipeline's own distributions), a tenth of each
replaced by -1.  Table values are random: the kernels' time does not depend on them.

Both variants are driven through the raw launchers on the same index tensors, without the wrappers' host checks
(those read the index bounds back and would put host round trips into both).  A sample is the time between two
device events around ``--reps`` back-to-back calls; the variants alternate sample by sample; after a warm-up,
``--samples`` samples each, reported as median and min..max.  The four shared outputs of the two variants are
compared bit for bit at the timed size, and the fused kernel's votes with the sum of the members' flags; a
difference ends the script with an error.  At R = 1 the composition is ``score_events`` alone.

Bytes: ``bytes_min`` is what must move at least -- the index and output streams plus both tables once;
``bytes_gathered`` counts the R K doubles of every side's two rows instead of the tables once (what moves with no
reuse in any cache).  ``share_of_hbm_peak`` is bytes_min over the fused median over the 8 TB/s HBM peak of the
MI355X specification: a share of that peak, not a measured bandwidth.

``--pipeline-events N``: also one ``ml_ops 20160122 flow 1e-5`` on a synthetic N-event day with and without
``--ensemble R`` (fresh processes, hip backend), their stage seconds side by side.  Needs a GPU.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oni_ml_amd.ops import hip as H  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, MI355X specification


def day_weights(source, events):
    """(document weights [D], word weights [V]) of the synthetic day, float64 on the GPU."""
    if source == "flow":
        from oni_ml_amd.pipeline.flow import synthetic_flow_corpus
        corpus, _ = synthetic_flow_corpus(events=events, seed=0, device="cuda", strict=False)
    else:
        from oni_ml_amd.pipeline.dns import synthetic_dns_corpus
        corpus, _ = synthetic_dns_corpus(events=events, seed=0, device="cuda", strict=False)
    ptr = np.asarray(corpus.doc_ptr, np.int64)
    cnt = np.asarray(corpus.counts, np.float64)
    dw = np.add.reduceat(cnt, ptr[:-1]) if cnt.size else np.zeros(0)
    ww = np.bincount(np.asarray(corpus.word_idx, np.int64), weights=cnt, minlength=corpus.num_terms)
    return torch.from_numpy(dw).cuda(), torch.from_numpy(np.maximum(ww, 1e-9)).cuda()


def draw(weights, n, g):
    """int32 [n] rows in proportion to ``weights`` (inverse CDF), a tenth of them -1."""
    cdf = torch.cumsum(weights, 0)
    cdf = cdf / cdf[-1]
    u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
    out = torch.searchsorted(cdf, u).clamp_max(weights.numel() - 1).to(torch.int32)
    out[torch.rand(n, generator=g, device="cuda") < 0.1] = -1
    return out


def sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def stats(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4))


def bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != torch.float64:
        return torch.equal(a, b)
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


def run_shape(source, n, sides, R, K, weights, a):
    dw, ww = weights
    D, V = dw.numel(), ww.numel()
    g = torch.Generator(device="cuda")
    g.manual_seed(a.seed)
    th = torch.rand(D, R, K, generator=g, device="cuda", dtype=torch.float64)
    ph = torch.rand(V, R, K, generator=g, device="cuda", dtype=torch.float64) * 1e-4
    sep = [(th[:, r].contiguous(), ph[:, r].contiguous()) for r in range(R)]      # the separate layout
    da, wa = draw(dw, n, g), draw(ww, n, g)
    db, wb = (draw(dw, n, g), draw(ww, n, g)) if sides == 2 else (None, None)
    dflt = 1.0 / K
    L, st = H.lib(), torch.cuda.current_stream().cuda_stream
    f64 = lambda: torch.empty(n, dtype=torch.float64, device="cuda")      # noqa: E731
    u8 = lambda: torch.empty(n, dtype=torch.uint8, device="cuda")         # noqa: E731
    p = lambda t: 0 if t is None else t.data_ptr()                        # noqa: E731
    # TOL: the value a fortieth of the events fall under (the headline flow day flags 2.4 %)
    probe = H.score_ensemble(th, ph, R, K, dflt, da, wa, db, wb, float("inf"))
    tol = float(torch.quantile(probe[2][:: max(1, n // 200_000)], 0.025))
    del probe

    fo = (f64(), f64() if sides == 2 else None, f64(), u8(), u8())

    def fused():
        L.score_ensemble(p(th), p(ph), R, K, dflt, p(da), p(wa), p(db), p(wb), n, tol, p(fo[0]), p(fo[1]), p(fo[2]),
                         p(fo[3]), p(fo[4]), 0, st)
        return fo

    mo = [(f64(), f64() if sides == 2 else None, f64(), u8()) for _ in range(R)]

    def members():
        for (t, w), o in zip(sep, mo):
            L.score_events(p(t), p(w), K, dflt, p(da), p(wa), p(db), p(wb), n, tol, p(o[0]), p(o[1]), p(o[2]), p(o[3]),
                           st)

    def composition():
        members()
        if R == 1:
            return mo[0]
        sa = torch.zeros(n, dtype=torch.float64, device="cuda")
        for o in mo:
            sa = sa + o[0]
        sa = sa / float(R)
        if sides == 1:
            return sa, None, sa, (sa < tol).to(torch.uint8)
        sb = torch.zeros(n, dtype=torch.float64, device="cuda")
        for o in mo:
            sb = sb + o[1]
        sb = sb / float(R)
        key = torch.where(sa < sb, sa, sb)
        return sa, sb, key, (key < tol).to(torch.uint8)

    got, want = fused(), composition()
    votes = torch.zeros(n, dtype=torch.uint8, device="cuda")
    for o in mo:
        votes = votes + o[3]
    same = all(bits(x, y) for x, y in zip(got[:4], want)) and torch.equal(got[4], votes)
    paths = dict(fused=fused, composition=composition)
    for fn in paths.values():      # warm-up: code objects, allocator
        sample(fn, 3)
    times = {k: [] for k in paths}
    for _ in range(a.samples):     # alternate the variants sample by sample
        for k, fn in paths.items():
            times[k].append(sample(fn, a.reps))
    stream = n * (sides * (8 + 8) + 8 + 1 + 1)      # int32 row pairs in, the side scores, key, flag, votes out
    row = R * K * 8
    rec = dict(source=source, events=n, sides=sides, R=R, K=K, documents=D, words=V, tol=tol,
               flagged=int(got[3].sum()), outputs_equal=bool(same), samples=a.samples, reps=a.reps,
               theta_mb=round(D * row / 1e6, 1), phi_mb=round(V * row / 1e6, 1),
               **{k: stats(v) for k, v in times.items()})
    f, c = rec["fused"], rec["composition"]
    rec.update(bytes_min=stream + (D + V) * row, bytes_gathered=stream + n * sides * 2 * row,
               speedup=round(c["median_ms"] / f["median_ms"], 3),
               # a claim needs the medians further apart than either variant's own min..max spread
               beyond_spread=bool(c["median_ms"] - f["median_ms"] > max(f["max_ms"] - f["min_ms"], c["max_ms"] - c["min_ms"])))
    rec["share_of_hbm_peak"] = round(rec["bytes_min"] / (f["median_ms"] * 1e-3) / HBM_PEAK, 4)
    rec["gathered_tb_s"] = round(rec["bytes_gathered"] / (f["median_ms"] * 1e-3) / 1e12, 3)
    return rec


def pipeline_stage_seconds(events, R):
    """{"plain": stage seconds, "ensemble": stage seconds} of ml_ops on one synthetic flow day, fresh processes;
    each is run twice and the second is kept (the first warms the page cache and the code object cache)."""
    out = {}
    with tempfile.TemporaryDirectory(prefix="oni_ens_") as tmp:
        py = [sys.executable, "-m", "oni_ml_amd"]
        subprocess.run(py + ["synth", "flow", "--out", os.path.join(tmp, "in") + "/", "--events", str(events)], cwd=ROOT,
                       check=True, stdout=subprocess.DEVNULL, timeout=600)
        for name, extra in (("plain", []), ("ensemble", ["--ensemble", str(R)])):
            for _ in range(2):
                lp = os.path.join(tmp, name)
                subprocess.run(py + ["ml_ops", "20160122", "flow", "1e-5", "--conf", os.path.join(tmp, "none.conf"),
                                     "--lpath", lp, "--flow-path", os.path.join(tmp, "in"), "--backend", "hip",
                                     "--quiet"] + extra, cwd=ROOT, check=True, stdout=subprocess.DEVNULL, timeout=600)
                with open(os.path.join(lp, "run_summary.json")) as f:
                    s = json.load(f)
            out[name] = dict(stage_seconds={k: round(v, 4) for k, v in s["stage_seconds"].items()},
                             wall_seconds=round(s["wall_seconds"], 4), scored=s.get("scored"),
                             members=[dict(em_iterations=m["em_iterations"], seconds=round(m["seconds"], 4))
                                      for m in s["lda"].get("members", [])])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="flow:1000000:2:8,dns:2000000:1:4,flow:1000000:2:1")
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pipeline-events", type=int, default=0)
    ap.add_argument("--pipeline-r", type=int, default=8)
    ap.add_argument("--json")
    a = ap.parse_args()
    result = {}
    if a.pipeline_events:      # child processes first: this one has not touched the GPU yet
        result["pipeline"] = dict(events=a.pipeline_events, R=a.pipeline_r,
                                  **pipeline_stage_seconds(a.pipeline_events, a.pipeline_r))
        print(json.dumps(result["pipeline"]), flush=True)
    shapes = [s for s in a.shapes.split(",") if s]
    if shapes and not torch.cuda.is_available():
        sys.exit("ensemble_bench: needs a GPU")
    weights, out = {}, []
    for spec in shapes:
        source, n, sides, R = spec.split(":")
        n, sides, R = int(n), int(sides), int(R)
        if (source, n) not in weights:
            weights[source, n] = day_weights(source, n)
        rec = run_shape(source, n, sides, R, a.topics, weights[source, n], a)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        torch.cuda.empty_cache()
    result["shapes"] = out
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    if not all(r["outputs_equal"] for r in out):
        sys.exit("ensemble_bench: the fused kernel and the composition returned different results")


if __name__ == "__main__":
    main()
