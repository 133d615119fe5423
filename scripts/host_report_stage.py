"""Warm ``flow_post`` stage seconds of a flow day with and without --host-report (profiles/host_report.md).

    python scripts/host_report_stage.py prepare --work DIR [--events 1000000]
    python scripts/host_report_stage.py time --work DIR [--tree CHECKOUT] [--host-report -1] [--runs 3]

``prepare`` writes the synthetic day.  ``time`` runs the whole pipeline on it (TOL 1e-3, compat fixed) ``--runs``
times in this process and prints the flow_post stage's seconds of every run as one JSON line (the first run of
a process is cold: code objects, allocator).  ``--tree``: import the package from another checkout of the project (the parent commit's, built), to
time its flow_post in the same session, alternating with this one's: that tree does not know --host-report, so
the option is not passed when it is 0."""
import argparse
import json
import os
import sys


def config(work, host_report, backend):
    from oni_ml_amd import config as CFG
    kw = dict(host_report=host_report) if host_report else {}
    cfg = CFG.resolve("20160122", "flow", tol=1e-3, conf_path=None, environ={}, lpath=os.path.join(work, "run"),
                      flow_path=os.path.join(work, "in"), backend=backend, compat="fixed", verbose=False, **kw)
    return cfg.validate()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["prepare", "time"])
    ap.add_argument("--work", required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--host-report", type=int, default=0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--device", default="cuda", help="cuda (the hip backend) or cpu")
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    import torch
    from oni_ml_amd.pipeline import run
    backend = "hip" if a.device == "cuda" else "cpu"
    quiet = lambda *x, **k: None      # noqa: E731
    if a.mode == "prepare":
        from oni_ml_amd.synth.flow import generate_flow_day
        generate_flow_day(os.path.join(a.work, "in") + "/", events=a.events, seed=0)
        print(json.dumps(dict(events=a.events, flow_path=os.path.join(a.work, "in"))), flush=True)
        return
    secs, extra = [], {}
    for _ in range(a.runs):
        s = run(config(a.work, a.host_report, backend), device=a.device, log=quiet)
        if a.device == "cuda":
            torch.cuda.synchronize()
        secs.append(round(s["stage_seconds"]["flow_post"], 4))
        extra = {k: s.get(k) for k in ("corpus", "scored", "hosts", "host_sides_skipped") if k in s}
    print(json.dumps(dict(tree=a.tree, host_report=a.host_report, flow_post_s=secs, **extra)), flush=True)


if __name__ == "__main__":
    main()
