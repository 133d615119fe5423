#!/usr/bin/env python
"""Proxy day record (profiles/proxy_day.md): at N synthetic requests, the time of the string-entropy kernel
alone, of its upload, of the numpy twin on the host, the stage times of one `ml_ops ... proxy` run, and the
share of planted requests among the lowest-scoring 1 % of events.

    python scripts/proxy_bench.py --events 1000000 --out proxy_day.md

Needs a GPU (no fall-back).  The kernel time is device events around the launch alone: the arguments are
checked and uploaded once, outside the events, and the extension's launcher is called directly.  The copy time
is device events around the copy.  Both are medians of --reps runs after a warm-up.  The wrapper call, the twin
and the stages are host clocks around synchronised work.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--out", default="proxy_day.md")
    a = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "proxy_bench needs a GPU"
    from oni_ml_amd import config as CFG
    from oni_ml_amd.features import proxy as FP
    from oni_ml_amd.ops import hip as H
    from oni_ml_amd.ops.reference import entropy_table, string_entropy
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.synth.proxy import generate_proxy_day
    H.lib()
    tmp = tempfile.mkdtemp(prefix="oni_proxy_")
    try:
        t0 = time.perf_counter()
        g = generate_proxy_day(os.path.join(tmp, "in"), events=a.events, seed=a.seed, files=4)
        synth_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        tab = FP.load_proxy(g["proxy_path"])
        load_s = time.perf_counter() - t0
        data, off = FP._offsets(tab.column("fulluri"))
        buf = np.frombuffer(data, dtype=np.uint8)[int(off[0]):int(off[-1])]
        off = off - off[0]
        lens = np.diff(off)
        nbytes = int(buf.size)

        pin = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        t0 = time.perf_counter()
        pin.numpy()[:] = buf
        fill_s = time.perf_counter() - t0
        dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        up = _events_ms(lambda: dev.copy_(pin, non_blocking=True), a.reps)
        # the launch alone: what ops.hip.string_entropy does around it (offset checks on the host, the uploads of
        # the offsets and the table, the output allocation) is done once here, outside the events
        off_h = torch.from_numpy(off)
        got = H.string_entropy(dev, off_h)
        off_d = off_h.cuda()
        table = torch.from_numpy(entropy_table(int(lens.max()))).cuda()
        res = torch.empty(tab.n, dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        launch = lambda: H.lib().string_entropy(dev.data_ptr(), off_d.data_ptr(), tab.n, table.data_ptr(),  # noqa: E731
                                                table.numel(), res.data_ptr(), 0, stream)
        kern = _events_ms(launch, a.reps)
        wrap = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            H.string_entropy(dev, off_h)
            torch.cuda.synchronize()
            wrap.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = string_entropy(buf, off)
        twin_s = time.perf_counter() - t0
        same = bool(np.array_equal(res.cpu().numpy().view(np.int64), want.view(np.int64))
                    and np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)))

        limit = max(1, tab.n // 100)
        cfg = CFG.resolve("20160122", "proxy", tol=1.0, conf_path=None, environ={}, lpath=os.path.join(tmp, "ml"),
                          proxy_path=g["proxy_path"], top1m=g["top1m"], backend="hip", verbose=False,
                          topics=a.topics, max_results=limit)
        t0 = time.perf_counter()
        summary = run(cfg.validate(), device="cuda", log=lambda *x, **k: None)
        wall_s = time.perf_counter() - t0

        # the planted rows among the written (lowest-scoring 1 %) rows, by (p_time, clientip, fulluri)
        import pyarrow as pa
        import pyarrow.parquet as pq
        day = pa.concat_tables([pq.read_table(p, columns=["p_time", "clientip", "fulluri"]) for p in g["paths"]])
        rows = day.take(pa.array(g["planted"])).to_pylist()
        key_kind = {(r["p_time"], r["clientip"], r["fulluri"]): k for r, k in zip(rows, g["planted_kinds"])}
        hit = {}
        written = 0
        with open(os.path.join(tmp, "ml", "proxy_results.csv"), encoding="utf-8", newline="\n") as f:
            for ln in f:
                c = ln.rstrip("\n").split("\t")
                written += 1
                k = key_kind.get((c[1], c[2], c[18]))
                if k is not None:
                    hit[k] = hit.get(k, 0) + 1
        planted_by_kind = {k: g["planted_kinds"].count(k) for k in sorted(set(g["planted_kinds"]))}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    n_hit = sum(hit.values())
    lines = [
        "# Proxy day on the MI355X", "",
        f"`python scripts/proxy_bench.py --events {a.events} --seed {a.seed} --reps {a.reps} --topics {a.topics}` on "
        f"{torch.cuda.get_device_name(0)}; device-event medians of {a.reps} runs after a warm-up (min .. max).", "",
        f"- day: {a.events} synthetic requests, {tab.n} kept, {tab.dropped} dropped; `fulluri` column {nbytes} bytes "
        f"(mean {nbytes / max(tab.n, 1):.1f}, longest {int(lens.max())}); synthesis {synth_s:.2f} s, parquet load {load_s:.2f} s",
        f"- string_entropy kernel alone (device events around the launch only; checks and uploads outside): "
        f"{kern[0]:.3f} ms ({kern[1]:.3f} .. {kern[2]:.3f}), {nbytes / kern[0] / 1e6:.1f} GB/s of URI bytes, "
        f"{tab.n / kern[0] / 1e3:.1f} M strings/s; bitwise equal to the twin: {same}",
        f"- `ops.hip.string_entropy` call with host offsets (host clock, synchronised; host checks of the offsets + "
        f"upload of offsets and table + kernel): median {statistics.median(wrap):.3f} ms of 5 "
        f"({min(wrap):.3f} .. {max(wrap):.3f})",
        f"- upload of the bytes, pinned host to device: {up[0]:.3f} ms ({up[1]:.3f} .. {up[2]:.3f}), "
        f"{nbytes / up[0] / 1e6:.1f} GB/s; filling the pinned buffer from the Arrow column: {fill_s * 1e3:.1f} ms (host clock, once)",
        f"- numpy twin on the host: {twin_s:.3f} s (host clock, once)",
        f"- one `ml_ops 20160122 proxy 1.0 {limit}` run (K = {a.topics}, HIP backend, in process, wall {wall_s:.2f} s); stage seconds:",
    ]
    lines += [f"  - {k}: {v:.3f}" for k, v in summary["stage_seconds"].items()]
    lines += [
        f"  - corpus {json.dumps(summary['corpus'])}, EM iterations {summary['lda']['em_iterations']}",
        f"- planted requests among the {written} lowest-scoring events (1 % of the kept rows): {n_hit} of "
        f"{len(g['planted'])} planted ({100.0 * n_hit / max(len(g['planted']), 1):.1f} % of the planted; they are "
        f"{100.0 * n_hit / max(written, 1):.2f} % of the written rows against {100.0 * len(g['planted']) / a.events:.2f} % of the day)",
    ]
    lines += [f"  - {k}: {hit.get(k, 0)} of {n}" for k, n in planted_by_kind.items()]
    lines += ["", "Records for later work to start from: no threshold is set and no test asserts these figures.", ""]
    text = "\n".join(lines)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
