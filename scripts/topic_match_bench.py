"""Measurements of --topic-match on an MI355X (profiles/topic_match.md).  Needs a GPU: there is no CPU fall-back.

  kernel    ops.hip.column_l1 at MATCH_BLOCK 256 / 1024 / 4096 against the torch composition a user would write --
            |A[:, :, None] - B[:, None, :]|.sum(0), chunked over the rows so that a chunk's [rows, Wa, Wb] stays
            within 256 MB -- at phi 63,707 x 20 against itself, against 8 members' interleaved columns (x 160), at
            K = 100 and at a month-scale pair of tables (4.5 M x 100); the kernel's share of the fp64 vector add
            rate (2 operations per pair and output: a subtraction and an add of a magnitude)
  stage     the flow scoring stage's wall on the 1 M-event day fitted once with --ensemble R: the stage resumed
            without the flags, with --topic-match and with --topic-match-day (a second synthetic day fitted once),
            alternating; and what the files show: mutual topics per member, the spread of dist, host_drift_hist
  plain     the unflagged stage only -- this part names nothing the option added, so the same file runs from a
            checkout of the parent commit: the cost of the flags being off is the difference of the two

Kernel timings: device events around one call, warmed up, `--reps` repetitions with the variants alternating; the
record gives the median and the range.  `python scripts/topic_match_bench.py --out FILE [--parts kernel,...]`."""
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

ADD_RATE = 39.3e12      # fp64 vector operations per second: half of 78.6 Tflop/s, which counts an FMA as two
CHUNK_DOUBLES = 1 << 25


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


def table(rows, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.rand(rows, W, dtype=torch.float64, device="cuda", generator=g) ** 4
    t /= t.sum(0, keepdim=True)
    return t


def composition(A, B):
    Wa, Wb = A.shape[1], B.shape[1]
    step = max(1, CHUNK_DOUBLES // (Wa * Wb))
    out = torch.zeros(Wa, Wb, dtype=torch.float64, device=A.device)
    for r0 in range(0, A.shape[0], step):
        out += (A[r0:r0 + step, :, None] - B[r0:r0 + step, None, :]).abs().sum(0)
    return out


def kernel_case(rows, Wa, Wb, reps, blocks=(256, 1024, 4096)):
    from oni_ml_amd.ops import hip as H
    A, B = table(rows, Wa, 1), table(rows, Wb, 2)
    variants = {f"column_l1@{b}": (lambda b=b: H.column_l1(A, B, block=b)) for b in blocks}
    variants["torch"] = lambda: composition(A, B)
    ms = timed(variants, reps)
    ops = 2.0 * rows * Wa * Wb
    got, want = H.column_l1(A, B), composition(A, B)
    return dict(rows=rows, Wa=Wa, Wb=Wb, path=H.column_l1_path(Wa, Wb), ms=ms, operations=ops,
                table_bytes=rows * (Wa + Wb) * 8,
                add_rate_share={k: round(ops / (v[0] * 1e-3) / ADD_RATE, 4) for k, v in ms.items()
                                if k.startswith("column_l1")},
                max_abs_diff=float((got - want).abs().max()), largest=float(want.max()))


def part_stage(reps, events, ensemble, work, tol, plain_only=False):
    """Flow scoring stage wall (stage_seconds["flow_post"]) of the stage resumed on one fitted work directory."""
    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.synth.flow import generate_flow_day

    def go(lp, flow, **kw):
        cfg = CFG.resolve("20160122", "flow", tol=tol, conf_path=None, environ={}, lpath=lp, flow_path=flow,
                          backend="hip", verbose=False, compat="fixed", **kw)
        cfg.settings = LDASettings()
        return run(cfg.validate(), device="cuda", log=lambda *a, **k: None)

    generate_flow_day(os.path.join(work, "in") + "/", events=events, seed=0)
    lp = os.path.join(work, "today")
    go(lp, os.path.join(work, "in"), ensemble=ensemble)
    variants = {"plain": {}}
    if not plain_only:
        generate_flow_day(os.path.join(work, "in2") + "/", events=events, seed=1)
        prev = os.path.join(work, "yesterday")
        go(prev, os.path.join(work, "in2"))
        variants["topic_match"] = dict(topic_match=True)
        variants["topic_match_day"] = dict(topic_match_day=prev)
    secs, info = {k: [] for k in variants}, {}
    for rep in range(reps + 1):      # the first round warms up
        for name, kw in variants.items():
            os.unlink(os.path.join(lp, ".stages", "flow_post.done"))
            s = go(lp, os.path.join(work, "in"), ensemble=ensemble, resume=True, **kw)
            if rep:
                secs[name].append(s["stage_seconds"]["flow_post"])
            info[name] = {k: s[k] for k in s if k.startswith("topic_match") or k == "host_drift_hist"}
    entry = dict(events=events, ensemble=ensemble, tol=tol,
                 flow_post_seconds={k: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4))
                                    for k, v in secs.items()})
    if not plain_only:
        entry["summary"] = info["topic_match_day"]
        rows = [r.rstrip("\n").split(",") for r in open(os.path.join(lp, "flow_topic_match.csv"))]
        for other in sorted({r[0] for r in rows}):
            d = np.asarray([float(r[3]) for r in rows if r[0] == other and r[3]])
            entry.setdefault("dist", {})[other] = dict(
                min=float(d.min()), median=float(np.median(d)), max=float(d.max()),
                mutual=int(sum(r[6] == "1" for r in rows if r[0] == other)))
        st = [r.rstrip("\n").split(",") for r in open(os.path.join(lp, "flow_topic_stability.csv"))]
        entry["mutual_in_every_member"] = int(sum(r[2] == r[1] for r in st))
        entry["members_mutual"] = [int(r[2]) for r in st]
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="kernel,stage")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--ensemble", type=int, default=8)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--month", type=int, default=4_500_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topic_match_bench: needs a GPU")
    parts = a.parts.split(",")
    rec = dict(device=torch.cuda.get_device_name(0), reps=a.reps, add_rate=ADD_RATE,
               match_block=getattr(CFG, "MATCH_BLOCK", None), match_scratch_mb=getattr(CFG, "MATCH_SCRATCH_MB", None))
    work = tempfile.mkdtemp(prefix="topic_match_bench_")

    def save():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    try:
        if "kernel" in parts:
            for rows, Wa, Wb, reps in ((63_707, 20, 20, a.reps), (63_707, 20, 160, a.reps), (63_707, 100, 100, a.reps),
                                       (a.month, 100, 100, 3)):
                entry = kernel_case(rows, Wa, Wb, reps)
                rec.setdefault("kernel", []).append(entry)
                print(json.dumps(entry), flush=True)
                save()
        for part in ("stage", "plain"):
            if part in parts:
                rec[part] = part_stage(a.reps, a.events, a.ensemble, work, a.tol, plain_only=part == "plain")
                print(json.dumps(rec[part]), flush=True)
                save()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()
