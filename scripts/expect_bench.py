"""Measurements of --expect on an MI355X (profiles/expect.md).  Needs a GPU: there is no CPU fall-back.

  stage    the scoring stage's wall of whole one-process runs with --explain and with --explain --expect, on the
           flow and the DNS day at TOL 1e-5, unlimited and with MAXRESULTS 3000, alternating the flag.  The unlimited
           --expect runs also hand the kernel part their real arguments (the day's groups, the written pairs)
  kernel   ops.hip.expect_sides (form "blocks": a lane per item and block of members) against a torch composition
           on the same GPU -- gather the member rows slab by slab, batched fp64 dot, segmented max / arg-max / count
           through scatter_reduce -- on the flow day's items at R = 1 and R = 8, the DNS day's, the flow day's at
           K = 100, and a skew case (1 M x 20 table, one group of 500 k members referenced by 2,000 items)
  host     the wall inside write_expect on the flow day, split by the calls it makes
  explain  only the --explain runs of the stage part (`--tree DIR` imports the package from another checkout: the
           parent commit's, to show that the path without the new flag has not moved)

Every kernel timing: device events around one whole wrapper call, two warm-up rounds, `--reps` repetitions with the
variants alternating; the record gives the median and the range.  Stage timings: `stage_seconds` of whole runs after
a warm-up run.  `python scripts/expect_bench.py --out FILE [--parts stage,kernel] [--tree DIR]`."""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch


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
    return {k: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)) for k, v in ms.items()}


def torch_expect(theta, phi, order, seg_start, seg_end, doc, word, grow, dflt, slab=1 << 23):
    """The composition to beat: per slab of at most ``slab`` member dots gather theta and phi rows, one batched fp64
    dot (a fused sum: not the scorer's bits), then segmented max, lowest-row arg-max and count by scatter_reduce."""
    V, R, K = phi.shape
    n, F = grow.shape
    dev = phi.device
    g = grow.reshape(-1).long()
    pair = torch.arange(n * F, device=dev) // F
    w = word.long()[pair]
    items = torch.nonzero((g >= 0) & (w >= 0)).reshape(-1)
    best = torch.full((n * F,), -1, dtype=torch.int32, device=dev)
    pbest = torch.full((n * F,), float("nan"), dtype=torch.float64, device=dev)
    above = torch.full((n * F,), -1, dtype=torch.int32, device=dev)
    if items.numel() == 0:
        return best.reshape(n, F), pbest.reshape(n, F), above.reshape(n, F)
    th_all = torch.cat([theta, torch.full((1, R, K), dflt, dtype=torch.float64, device=dev)])      # row -1: default
    lens = (seg_end - seg_start)[g[items]]
    ends = torch.cumsum(lens, 0)
    cuts = [0]
    ends_h = ends.cpu().numpy()
    while cuts[-1] < items.numel():
        base = int(ends_h[cuts[-1] - 1]) if cuts[-1] else 0
        cuts.append(max(cuts[-1] + 1, int(np.searchsorted(ends_h, base + slab, side="right"))))
    for i0, i1 in zip(cuts[:-1], cuts[1:]):
        it, ln = items[i0:i1], lens[i0:i1]
        of = torch.repeat_interleave(torch.arange(it.numel(), device=dev), ln)
        first = torch.cumsum(ln, 0) - ln
        v = order.long()[seg_start[g[it]][of] + torch.arange(of.numel(), device=dev) - first[of]]
        th = th_all[doc.long()[pair[it]]]                                   # [m, R, K]
        p = (th[of] * phi[v]).sum(2).sum(1) / R
        s = (th * phi[w[it]]).sum(2).sum(1) / R
        m = it.numel()
        cnt = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, of, (p > s[of]).long())
        top = torch.full((m,), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(0, of, p, "amax")
        win = p == top[of]
        row = torch.full((m,), V, dtype=torch.int64, device=dev).scatter_reduce(0, of[win], v[win], "amin")
        best[it] = torch.where(row < V, row, torch.full_like(row, -1)).int()
        pbest[it] = top
        above[it] = cnt.int()
    return best.reshape(n, F), pbest.reshape(n, F), above.reshape(n, F)


def kernel_case(name, H, args, reps, with_torch=True):
    theta, phi, order, s, e, doc, word, grow, dflt = args
    n, F = grow.shape
    ok = (grow >= 0) & (word >= 0).unsqueeze(1)
    dots = int((e - s)[grow.long().clamp_min(0)][ok].sum())
    got = H.expect_sides(*args)
    variants = {"blocks": lambda: H.expect_sides(*args, form="blocks")}
    rec = dict(case=name, pairs=n, F=F, V=int(phi.shape[0]), R=int(phi.shape[1]), K=int(phi.shape[2]),
               member_dots=dots, theta_path=H.expect_theta_path(int(phi.shape[1]), int(phi.shape[2])))
    if with_torch:
        ref = torch_expect(*args)
        rec["best_agree"] = float((got[0] == ref[0]).double().mean())      # a fused dot may move a near-tie
        rec["above_agree"] = float((got[2] == ref[2]).double().mean())
        variants["torch"] = lambda: torch_expect(*args)
    rec["ms"] = timed(variants, reps)
    med = rec["ms"]["blocks"][0]
    rec["gflops_blocks"] = round(2.0 * dots * rec["R"] * rec["K"] / (med * 1e-3) / 1e9, 1)
    return rec


def part_kernel(H, reps, captured):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    out = []
    for kind in ("flow", "dns"):
        if kind not in captured:
            continue
        a = captured[kind]
        out.append(kernel_case(f"{kind} day", H, a, reps))
        if kind == "flow":
            theta, phi, rest = a[0], a[1], a[2:]
            jitter = lambda t, r: (t.expand(-1, r, -1) *      # noqa: E731
                                   (0.5 + torch.rand(t.shape[0], r, t.shape[2], dtype=torch.float64, device=dev,
                                                     generator=g))).contiguous()
            out.append(kernel_case("flow day, R = 8", H, (jitter(theta, 8), jitter(phi, 8)) + rest, reps))
            th100 = torch.rand(theta.shape[0], 1, 100, dtype=torch.float64, device=dev, generator=g)
            ph100 = torch.rand(phi.shape[0], 1, 100, dtype=torch.float64, device=dev, generator=g) * 1e-3
            out.append(kernel_case("flow day, K = 100", H, (th100, ph100) + rest, reps))
    # skew: one group holds half of a 1 M-row table, 2,000 items refer to it, 2,000 to groups of 16
    V, K, n = 1_000_000, 20, 4000
    r = torch.arange(V, device=dev)
    gid = torch.where(r % 2 == 0, torch.zeros_like(r), 1 + r // 32)
    sk, perm = torch.sort(gid, stable=True)
    first = torch.ones(V, dtype=torch.bool, device=dev)
    first[1:] = sk[1:] != sk[:-1]
    st = torch.nonzero(first).reshape(-1)
    s, e = st, torch.cat([st[1:], torch.tensor([V], device=dev)])
    grp_of = torch.cumsum(first.long(), 0) - 1
    of_row = torch.empty(V, dtype=torch.int64, device=dev)
    of_row[perm] = grp_of
    word = torch.cat([torch.randint(0, V // 2, (n // 2,), device=dev, generator=g) * 2,
                      torch.randint(0, V // 2, (n // 2,), device=dev, generator=g) * 2 + 1]).int()
    theta = torch.rand(5000, 1, K, dtype=torch.float64, device=dev, generator=g)
    phi = torch.rand(V, 1, K, dtype=torch.float64, device=dev, generator=g) * 1e-3
    doc = torch.randint(0, 5000, (n,), device=dev, generator=g, dtype=torch.int32)
    grow = of_row[word.long()].int().reshape(-1, 1)
    out.append(kernel_case("skew: 1 M x 20, one group of 500 k, 2,000 + 2,000 items", H,
                           (theta, phi, perm.int(), s.contiguous(), e.contiguous(), doc, word, grow.contiguous(), 0.05),
                           max(3, reps // 3)))
    return out


def part_stage(CFG, reps, events, work, flags, capture):
    """Scoring stage wall (stage_seconds["<type>_post"]) of whole one-process runs, alternating the flags."""
    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.score import scorer as S
    from oni_ml_amd.synth.dns import generate_dns_day
    from oni_ml_amd.synth.flow import generate_flow_day
    generate_flow_day(os.path.join(work, "in") + "/", events=events, seed=0)
    gen = generate_dns_day(os.path.join(work, "dns_in"), events=events, seed=0, n_names=max(20_000, events // 10),
                           n_clients=max(5_000, events // 40))
    paths = dict(flow=dict(flow_path=os.path.join(work, "in")), dns=dict(dns_path=gen["dns_path"], top1m=gen["top1m"]))
    res, captured = [], {}
    for kind in ("flow", "dns"):
        for limit in (-1, 3000):
            secs = {f: [] for f in flags}
            info = {}
            for rep in range(reps + 1):      # the first round warms up
                for flag in flags:
                    lp = os.path.join(work, f"run_{kind}_{limit}_{flag}")
                    shutil.rmtree(lp, ignore_errors=True)
                    kw = dict(explain=True)
                    if flag == "expect":
                        kw["expect"] = True
                    cfg = CFG.resolve("20160122", kind, tol=1e-5, conf_path=None, environ={}, lpath=lp, backend="hip",
                                      verbose=False, compat="fixed", max_results=limit, **paths[kind], **kw)
                    cfg.settings = LDASettings() if kind == "flow" else LDASettings(em_max_iter=5)
                    keep = []
                    spying = capture and flag == "expect" and limit == -1 and kind not in captured
                    orig = getattr(S, "expect_sides", None)      # (a tree from before the option has none)
                    if spying:      # the run's own arguments of the kernel: the day's groups, the written pairs
                        def spy(model, seg, doc, word, grow, orig=orig, keep=keep):
                            keep.append((model, seg, doc, word, grow))
                            return orig(model, seg, doc, word, grow)
                        S.expect_sides = spy
                    try:
                        s = run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
                    finally:
                        if spying:
                            S.expect_sides = orig
                    if keep:
                        model, seg, doc, word, grow = keep[0]
                        th, ph = S.model_tables3(model)
                        captured[kind] = (th.contiguous(), ph.contiguous(), seg.order.int().contiguous(),
                                          seg.seg_start.contiguous(), seg.seg_end.contiguous(), doc.int().contiguous(),
                                          word.int().contiguous(), grow.int().contiguous(), float(model.default))
                    if rep:
                        secs[flag].append(s["stage_seconds"][kind + "_post"])
                    if flag == "expect":
                        info = {k: s[k] for k in ("expect_modal_hist", "expect_pairs", "expect_member_dots", "expect_path")}
                    info["written"] = s["scored"]
            res.append(dict(kind=kind, events=events, max_results=limit, **info,
                            post_seconds={f: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4))
                                          for f, v in secs.items()}))
    return res, captured


def part_host(CFG, reps, events, work):
    """Where the option's host time goes on the flow day: wall seconds inside ``write_expect`` per run, split by the
    calls it makes (each ends in a host read, so the device work it waits for is counted with it)."""
    import time

    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.ops import native
    from oni_ml_amd.ops import sortgroup as SG
    from oni_ml_amd.pipeline import common as C
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.score import scorer as S
    from oni_ml_amd.synth.flow import generate_flow_day
    generate_flow_day(os.path.join(work, "hin") + "/", events=events, seed=0)
    L = native.lib()
    acc, on = {}, [False]

    def wrap(name, fn):
        def inner(*a, **k):
            if not on[0]:
                return fn(*a, **k)
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                acc[name] = acc.get(name, 0.0) + time.perf_counter() - t0
        return inner
    saved = (C.write_expect, S.expect_sides, SG.unique, np.unique, L.java_double_array, L.write_rows)
    inner_we = wrap("write_expect (all)", C.write_expect)

    def we(*a, **k):
        on[0] = True
        try:
            return inner_we(*a, **k)
        finally:
            on[0] = False
    C.write_expect, S.expect_sides, SG.unique = we, wrap("scorer.expect_sides", S.expect_sides), wrap("SG.unique", SG.unique)
    np.unique, L.java_double_array, L.write_rows = (wrap("np.unique", np.unique),
                                                    wrap("java_double_array", L.java_double_array),
                                                    wrap("write_rows", L.write_rows))
    out = []
    try:
        for rep in range(reps + 1):
            acc.clear()
            lp = os.path.join(work, "host_run")
            shutil.rmtree(lp, ignore_errors=True)
            cfg = CFG.resolve("20160122", "flow", tol=1e-5, conf_path=None, environ={}, lpath=lp, backend="hip",
                              verbose=False, compat="fixed", flow_path=os.path.join(work, "hin"), expect=True)
            cfg.settings = LDASettings()
            run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
            if rep:
                out.append(dict(acc))
    finally:
        C.write_expect, S.expect_sides, SG.unique, np.unique, L.java_double_array, L.write_rows = saved
    return {k: (round(float(np.median([o[k] for o in out])), 4), round(min(o[k] for o in out), 4),
                round(max(o[k] for o in out), 4)) for k in out[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="stage,kernel")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from oni_ml_amd import config as CFG
    from oni_ml_amd.ops import hip as H
    if not torch.cuda.is_available():
        raise SystemExit("expect_bench: needs a GPU")
    parts = a.parts.split(",")
    rec = dict(device=torch.cuda.get_device_name(0), group_block=CFG.GROUP_BLOCK, reps=a.reps, tree=a.tree)
    work = tempfile.mkdtemp(prefix="expect_bench_")
    try:
        captured = {}
        if "explain" in parts:
            rec["explain_only"], _ = part_stage(CFG, max(3, a.reps // 3), a.events, work, ("explain",), False)
        if "stage" in parts:
            rec["stage"], captured = part_stage(CFG, max(3, a.reps // 3), a.events, work, ("explain", "expect"), True)
            json.dump(rec, open(a.out, "w"), indent=1)
        if "host" in parts:
            rec["host"] = part_host(CFG, max(3, a.reps // 3), a.events, work)
        if "kernel" in parts:
            rec["kernel"] = part_kernel(H, a.reps, captured)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
