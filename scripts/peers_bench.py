"""Measurements of --peers on an MI355X (profiles/peers.md).  Needs a GPU: there is no CPU fall-back.

  stage    the flow scoring stage's wall with and without --peers on the 1 M-event day at TOL 1e-5, unlimited and
           with MAXRESULTS 3000 (the run without the flag takes the parent commit's path), and what the columns show
           on that day: the peer_lift histogram, how many of the 1,000 lowest-score rows have peer_lift < 10 and
           > 100, peer_identical
  kernel   ops.hip.peer_topn against the torch composition a user would write -- fp64 cdist(p=1) over slabs of
           queries that fit memory, the query's own column set to +inf, topk; not bit-equal (cdist sums in an order
           of its own, topk breaks ties its own way) -- at (Q, D, K, R) = the day's two shapes, (6,000, D, 20, 4) and
           (Q, D, 100, 1); the kernel's share of the fp64 vector add rate at 2 operations per element
  block    PEERS_BLOCK 1024 / 4096 / 16384 at the day's two shapes, at N and at N = 4
  scratch  PEERS_SCRATCH_MB 64 / 256 / 1024 at the day's unlimited shape
  scores   scorer.peer_scores (N calls of the scorer) over 100,000 sides

`rows_equal` of the kernel part is the share of list entries the composition agrees on.  Where it is far from 1, look
at cdist first: on the torch build this was measured with, fp64 cdist(p=1) on the device differed from the same call
on the CPU in most rows of a [512, 124,451] result, while the kernel was bit for bit the CPU twin (profiles/peers.md).

Every kernel timing: device events around one call, warmed up, `--reps` repetitions with the variants alternating;
the record gives the median and the range.  `python scripts/peers_bench.py --out FILE [--parts stage,kernel,...]`."""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.ops import hip as H  # noqa: E402

FP64_VECTOR_ADD_RATE = 78.6e12 / 2      # MI355X fp64 vector adds per second: the FMA peak counts two per instruction


def timed(variants, reps):
    """{name: (median ms, min ms, max ms)} of the callables, alternating, after two warm-up rounds."""
    for _ in range(2):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)) for k, v in ms.items()}


def torch_peers(th, q, n, slab=1 << 27):
    """The alternative: per slab of queries the [m, D] distances by cdist, the own column masked, topk."""
    D = th.shape[0]
    flat = th.reshape(D, -1)
    rows = torch.empty((q.numel(), n), dtype=torch.int64, device=th.device)
    dist = torch.empty((q.numel(), n), dtype=torch.float64, device=th.device)
    step = max(1, slab // D)
    for b0 in range(0, q.numel(), step):
        qs = q[b0:b0 + step].long()
        d = torch.cdist(flat[qs], flat, p=1.0)
        d[torch.arange(qs.numel(), device=th.device), qs] = float("inf")
        dist[b0:b0 + step], rows[b0:b0 + step] = torch.topk(d, n, dim=1, largest=False)
    return rows, dist


def shape_case(Q, D, K, R, n, reps, blocks=(None,), scratch=(None,), with_torch=True):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(Q % 1000 + K)
    th = torch.rand(D, R, K, dtype=torch.float64, device=dev, generator=g) ** 4
    th /= th.sum(2, keepdim=True)
    q = torch.randperm(D, device=dev, generator=g)[:Q].to(torch.int32).contiguous()
    variants = {}
    for b in blocks:
        for mb in scratch:
            name = "peer_topn" + ("" if b is None else f"@{b}") + ("" if mb is None else f"/{mb}MB")
            variants[name] = (lambda b=b, mb=mb: H.peer_topn(th, q, n, block=b, scratch_mb=mb))
    if with_torch:
        variants["torch"] = lambda: torch_peers(th, q, n)
    ms = timed(variants, reps)
    out = dict(Q=int(q.numel()), D=D, K=K, R=R, n=n, path=H.peer_theta_path(R, K), ms=ms)
    if with_torch:
        a, b = H.peer_topn(th, q, n), torch_peers(th, q, n)
        out["rows_equal"] = float((a[0].long() == b[0]).double().mean())
        out["max_abs_diff_of_dist"] = float((a[1] - b[1]).abs().max())
    ops = 2.0 * q.numel() * D * K * R
    out["fp64_add_rate_share"] = {k: round(ops / (v[0] * 1e-3) / FP64_VECTOR_ADD_RATE, 4) for k, v in ms.items()
                                  if k.startswith("peer_topn")}
    out["theta_bytes_staged"] = -(-int(q.numel()) // 256) * D * R * K * 8      # every row once per tile of queries
    out["torch_matrix_bytes_if_unbatched"] = int(q.numel()) * D * 8
    return out


def scores_case(sides, D, V, K, n, reps):
    """``scorer.peer_scores`` -- n calls of the scorer over the written sides -- beside the kernel it follows."""
    from oni_ml_amd.score import scorer as S
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(sides % 1000 + K)
    th = torch.rand(D, K, dtype=torch.float64, device=dev, generator=g)
    ph = torch.rand(V, K, dtype=torch.float64, device=dev, generator=g)
    model = S.TopicModel(th, ph, K, 1.0 / K)
    rows = torch.randint(0, D, (sides, n), device=dev, generator=g, dtype=torch.int32)
    count = torch.full((sides,), n, dtype=torch.int32, device=dev)
    doc = torch.randint(0, D, (sides,), device=dev, generator=g)
    word = torch.randint(0, V, (sides,), device=dev, generator=g)
    return dict(sides=sides, n=n, K=K, ms=timed({"peer_scores": lambda: S.peer_scores(model, rows, count, doc, word)},
                                                reps))


def shows(lp):
    """What the peers columns show on the written day, from its files."""
    rows = [ln.split(",") for ln in open(os.path.join(lp, "flow_peers.csv"), encoding="utf-8").read().split("\n")[:-1]]
    key = np.asarray([float(f[0]) for f in rows])
    low = np.argsort(key, kind="stable")[:1000]
    out = dict(rows=len(rows), lowest=int(low.size), lift_below_10=0, lift_above_100=0, lift_between=0, no_lift=0)
    for i in low.tolist():
        f = rows[i]
        sides = [(float(f[1 + 7 * j + 2]), f[1 + 7 * j + 6]) for j in (0, 1)]
        lift = min(sides)[1]      # the side that made the key
        if not lift:
            out["no_lift"] += 1
        elif float(lift) < 10:
            out["lift_below_10"] += 1
        elif float(lift) > 100:
            out["lift_above_100"] += 1
        else:
            out["lift_between"] += 1
    return out


def part_stage(reps, events, work, tol, n):
    """Flow scoring stage wall (stage_seconds["flow_post"]) of whole one-process runs, alternating the flag."""
    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.synth.flow import generate_flow_day
    generate_flow_day(os.path.join(work, "in") + "/", events=events, seed=0)
    res = []
    for limit in (-1, 3000):
        secs = {False: [], True: []}
        info = {}
        for rep in range(reps + 1):      # the first round warms up
            for flag in (False, True):
                lp = os.path.join(work, f"run_{limit}_{int(flag)}")
                shutil.rmtree(lp, ignore_errors=True)
                cfg = CFG.resolve("20160122", "flow", tol=tol, conf_path=None, environ={}, lpath=lp,
                                  flow_path=os.path.join(work, "in"), backend="hip", verbose=False, compat="fixed",
                                  max_results=limit, peers=n if flag else 0)
                cfg.settings = LDASettings()
                s = run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
                if rep:
                    secs[flag].append(s["stage_seconds"]["flow_post"])
                if flag:
                    info = dict(written=s["scored"], **{k: s[k] for k in s if k.startswith("peer")})
        entry = dict(events=events, tol=tol, max_results=limit, **info,
                     flow_post_seconds={("peers" if k else "plain"): (round(float(np.median(v)), 4), round(min(v), 4),
                                                                      round(max(v), 4)) for k, v in secs.items()})
        if limit < 0:
            entry["shows"] = shows(os.path.join(work, "run_-1_1"))
        res.append(entry)
        print(json.dumps(entry), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="stage,kernel,block,scratch,scores")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--n", type=int, default=CFG.PEERS_MAX)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("peers_bench: needs a GPU")
    parts = a.parts.split(",")
    rec = dict(device=torch.cuda.get_device_name(0), peers_block=CFG.PEERS_BLOCK, peers_scratch_mb=CFG.PEERS_SCRATCH_MB,
               n=a.n, reps=a.reps, fp64_vector_add_rate=FP64_VECTOR_ADD_RATE)
    day = [(30_000, 124_451), (6_000, 124_451)]      # (Q, D) of the day's two shapes when the stage part is off
    work = tempfile.mkdtemp(prefix="peers_bench_")

    def save():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    try:
        if "stage" in parts:
            rec["stage"] = part_stage(max(2, a.reps // 3), a.events, work, a.tol, a.n)
            day = [(max(1, e["peer_hosts"]), e["peer_candidates"]) for e in rec["stage"]]
            save()
        half = max(3, a.reps // 2)
        if "kernel" in parts:
            rec["kernel"] = []
            for Q, D, K, R, reps in ((day[0][0], day[0][1], 20, 1, a.reps), (day[1][0], day[1][1], 20, 1, a.reps),
                                     (6_000, day[0][1], 20, 4, half), (day[0][0], day[0][1], 100, 1, half)):
                rec["kernel"].append(shape_case(Q, D, K, R, a.n, reps))
                print(json.dumps(rec["kernel"][-1]), flush=True)
                save()
        if "block" in parts:
            rec["block"] = [shape_case(Q, D, 20, 1, n, half, blocks=(1024, 4096, 16384), with_torch=False)
                            for Q, D in day for n in sorted({a.n, 4}, reverse=True)]
            print(json.dumps(rec["block"]), flush=True)
            save()
        if "scratch" in parts:
            rec["scratch"] = shape_case(day[0][0], day[0][1], 20, 1, a.n, half, scratch=(64, 256, 1024),
                                        with_torch=False)
            print(json.dumps(rec["scratch"]), flush=True)
        if "scores" in parts:
            rec["scores"] = scores_case(100_000, day[0][1], 63_707, 20, a.n, half)
            print(json.dumps(rec["scores"]), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()
