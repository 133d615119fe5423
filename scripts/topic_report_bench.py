"""Measurements of --topic-report on an MI355X (profiles/topic_report.md).  Needs a GPU: there is no CPU fall-back.

  stage     the flow scoring stage's wall with and without --topic-report on the 1 M-event day at TOL 1e-5, unlimited
            and with MAXRESULTS 3000, and what the files show on that day: the written sides per topic, the minor
            sides, the resp histogram
  plain     the same stage without the flag only -- this part names nothing the flag added, so the same file runs
            from a checkout of the parent commit: the cost of the flag being off is the difference of the two
  kernel    ops.hip.column_topn against torch.topk on the transposed table and against a full stable descending sort
            along the rows (neither breaks ties by row, so `rows_equal` is the share of list entries they agree on)
            at the day's two tables (phi 63,707 x 20, theta 124,451 x 20), R = 8, K = 100 and a month-scale phi
            (4.5 M x 100; topk only); the kernel's share of the HBM peak at one read of the table
  dominant  ops.hip.row_dominant against argmax + bincount, ops.hip.topic_sides against the gathers, the product, max
            and argmax a user would write
  block     TOPIC_BLOCK 256 / 1024 / 4096 / 16384 at the day's phi, at K = 100 and at the month-scale phi
  sample    TOPIC_SAMPLE 2048 / 8192 / 32768 at the same three tables at N = 32 (the kernel part also times the kernel
            without the sampled bound, `~none`)
  scratch   TOPIC_SCRATCH_MB 64 / 256 / 1024 at the month-scale phi

Every kernel timing: device events around one call, warmed up, `--reps` repetitions with the variants alternating;
the record gives the median and the range.  `python scripts/topic_report_bench.py --out FILE [--parts stage,...]`."""
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

HBM_PEAK = 8.0e12      # MI355X HBM3E bytes per second (specification)
MONTH = (4_500_000, 100, 1)


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


def table(rows, K, R):
    g = torch.Generator(device="cuda").manual_seed(rows % 1000 + K + R)
    t = torch.rand(rows, R, K, dtype=torch.float64, device="cuda", generator=g) ** 4
    t /= t.sum(2, keepdim=True)
    return t


def topn_case(rows, K, R, n, reps, blocks=(None,), scratch=(None,), samples=(None,), with_topk=True, with_sort=True):
    from oni_ml_amd.ops import hip as H
    t = table(rows, K, R).reshape(rows, R * K)
    variants = {}
    for b in blocks:
        for mb in scratch:
            for sm in samples:      # sample = rows: no sampled bound, every value is offered
                name = "column_topn" + ("" if b is None else f"@{b}") + ("" if mb is None else f"/{mb}MB") + \
                    ("" if sm is None else "~none" if sm >= rows else f"~{sm}")
                variants[name] = (lambda b=b, mb=mb, sm=sm: H.column_topn(t, n, block=b, scratch_mb=mb, sample=sm))
    if with_topk:
        variants["topk"] = lambda: torch.topk(t.t(), n, dim=1)
    if with_sort:
        variants["sort"] = lambda: torch.sort(t, dim=0, descending=True, stable=True)
    ms = timed(variants, reps)
    out = dict(rows=rows, K=K, R=R, n=n, path=H.topic_path(n, R * K), ms=ms, table_bytes=rows * R * K * 8)
    if with_topk:
        a, b = H.column_topn(t, n), torch.topk(t.t(), n, dim=1)
        out["rows_equal"] = float((a[0].long() == b[1]).double().mean())
        out["values_equal"] = bool(torch.equal(a[1], b[0]))
    out["hbm_peak_share"] = {k: round(out["table_bytes"] / (v[0] * 1e-3) / HBM_PEAK, 4) for k, v in ms.items()
                             if k.startswith("column_topn")}
    return out


def dominant_case(rows, K, R, sides, reps):
    from oni_ml_amd.ops import hip as H
    th, ph = table(rows, K, R), table(rows // 2, K, R) * 1e-3
    g = torch.Generator(device="cuda").manual_seed(sides % 1000)
    doc = torch.randint(0, rows, (sides,), device="cuda", generator=g, dtype=torch.int32)
    word = torch.randint(0, rows // 2, (sides,), device="cuda", generator=g, dtype=torch.int32)

    def torch_dominant():
        arg = th.argmax(2)
        return arg, torch.bincount((arg + torch.arange(R, device="cuda") * K).reshape(-1), minlength=R * K)

    def torch_sides():
        tr = th[doc.long()].reshape(sides, -1)
        p = tr * ph[word.long()].reshape(sides, -1)
        best, j = p.max(1)
        s = p.reshape(sides, R, K).sum(2).sum(1) / R
        own = th[doc.long(), j // K]
        return j, best / (s * R), tr.gather(1, j.unsqueeze(1)), own.argmax(1)

    ms = timed({"row_dominant": lambda: H.row_dominant(th), "torch_dominant": torch_dominant,
                "topic_sides": lambda: H.topic_sides(th, ph, doc, word), "torch_sides": torch_sides}, reps)
    a, b = H.topic_sides(th, ph, doc, word), torch_sides()
    return dict(rows=rows, K=K, R=R, sides=sides, ms=ms,
                dominant_equal=bool(torch.equal(H.row_dominant(th)[0].long(), torch_dominant()[0])),
                sides_col_equal=float((a[0].long() == b[0]).double().mean()),
                max_abs_diff_of_resp=float((a[1] - b[1]).abs().max()))


def part_stage(reps, events, work, tol, n, flags=(False, True)):
    """Flow scoring stage wall (stage_seconds["flow_post"]) of whole one-process runs, alternating the flag."""
    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.synth.flow import generate_flow_day
    generate_flow_day(os.path.join(work, "in") + "/", events=events, seed=0)
    res = []
    for limit in (-1, 3000):
        secs = {f: [] for f in flags}
        info = {}
        for rep in range(reps + 1):      # the first round warms up
            for flag in flags:
                lp = os.path.join(work, f"run_{limit}_{int(flag)}")
                shutil.rmtree(lp, ignore_errors=True)
                more = dict(topic_report=n) if flag else {}
                cfg = CFG.resolve("20160122", "flow", tol=tol, conf_path=None, environ={}, lpath=lp,
                                  flow_path=os.path.join(work, "in"), backend="hip", verbose=False, compat="fixed",
                                  max_results=limit, **more)
                cfg.settings = LDASettings()
                s = run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
                if rep:
                    secs[flag].append(s["stage_seconds"]["flow_post"])
                if flag:
                    info = dict(written=s["scored"], **{k: s[k] for k in s if k.startswith("topic")})
        entry = dict(events=events, tol=tol, max_results=limit, **info,
                     flow_post_seconds={("topic_report" if k else "plain"): (round(float(np.median(v)), 4),
                                                                             round(min(v), 4), round(max(v), 4))
                                        for k, v in secs.items()})
        res.append(entry)
        print(json.dumps(entry), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="stage,kernel,dominant,block,sample,scratch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--n", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topic_report_bench: needs a GPU")
    parts = a.parts.split(",")
    rec = dict(device=torch.cuda.get_device_name(0), n=a.n, reps=a.reps, hbm_peak=HBM_PEAK,
               topic_block=getattr(CFG, "TOPIC_BLOCK", None), topic_scratch_mb=getattr(CFG, "TOPIC_SCRATCH_MB", None),
               topic_sample=getattr(CFG, "TOPIC_SAMPLE", None))
    work = tempfile.mkdtemp(prefix="topic_report_bench_")

    def save():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)

    def put(name, entry):
        rec.setdefault(name, []).append(entry)
        print(json.dumps(entry), flush=True)
        save()
    try:
        if "stage" in parts:
            rec["stage"] = part_stage(max(5, a.reps), a.events, work, a.tol, a.n)
            save()
        if "plain" in parts:
            rec["plain"] = part_stage(max(5, a.reps), a.events, work, a.tol, a.n, flags=(False,))
            save()
        half = max(3, a.reps // 2)
        if "kernel" in parts:
            for n in sorted({a.n, CFG.TOPIC_REPORT_MAX}):
                for rows, K, R in ((63_707, 20, 1), (124_451, 20, 1), (63_707, 20, 8), (63_707, 100, 1)):
                    put("kernel", topn_case(rows, K, R, n, a.reps, samples=(None, rows)))
                put("kernel", topn_case(*MONTH, n, half, samples=(None, MONTH[0]), with_sort=False))
        if "dominant" in parts:
            for rows, K, R in ((124_451, 20, 1), (124_451, 20, 8), (124_451, 100, 1)):
                put("dominant", dominant_case(rows, K, R, 100_000, a.reps))
        if "block" in parts:
            for rows, K, R in ((63_707, 20, 1), (63_707, 100, 1), MONTH):
                for n in sorted({a.n, CFG.TOPIC_REPORT_MAX}):
                    put("block", topn_case(rows, K, R, n, half, blocks=(256, 1024, 4096, 16384), with_topk=False,
                                           with_sort=False))
        if "sample" in parts:
            for rows, K, R in ((63_707, 20, 1), (63_707, 100, 1), MONTH):
                put("sample", topn_case(rows, K, R, CFG.TOPIC_REPORT_MAX, half, samples=(2048, 8192, 32768),
                                        with_topk=False, with_sort=False))
        if "scratch" in parts:
            put("scratch", topn_case(*MONTH, CFG.TOPIC_REPORT_MAX, half, scratch=(64, 256, 1024), with_topk=False,
                                     with_sort=False))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()
