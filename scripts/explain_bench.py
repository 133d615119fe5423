"""Measurements of --explain on an MI355X (profiles/explain.md).  Needs a GPU: there is no CPU fall-back.

  groups   ops.hip.group_rows_sum against two torch compositions -- index_add_ into zeros (atomics: the fp64 bits
           depend on the arrival order) and sort + cumsum differences -- on the 1-day flow vocabulary with every
           field's groups, a 4 M x 100 table with Zipf group sizes, and a skew case (one group holds half of a
           1 M-row table) that is also run at GROUP_BLOCK 64, 256 and 1024
  sides    ops.hip.explain_sides against F + 1 score_events launches plus torch divisions, 100 k and 2 M sides
  stage    the flow scoring stage's wall with and without --explain on the 1 M-event day at TOL 1e-5, unlimited
           and with MAXRESULTS 3000 (the run without the flag is the parent commit's behaviour)
  sizes    median and maximum group size per field on the flow and the DNS day

Every timing: device events around one call, warmed up, `--reps` repetitions with the variants alternating; the
record gives the median and the range.  `python scripts/explain_bench.py --out FILE [--parts groups,sides,...]`."""
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
from oni_ml_amd.ops import sortgroup as SG  # noqa: E402


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


def segments_of(gid):
    """(order int32, seg_start, seg_end) of the groups of a group-id vector, rows in row order inside a group."""
    sk, perm = SG.sort_stable(gid)
    grp, G = SG.run_ids(sk)
    st = SG.run_starts(grp, G)
    return perm.to(torch.int32), st[:-1].contiguous(), st[1:].contiguous(), grp, G


def group_case(name, phi, gid, reps, blocks=(None,)):
    order, s, e, grp, G = segments_of(gid)
    V, W = phi.shape
    dense = torch.empty(V, dtype=torch.int64, device=phi.device)
    dense[order.long()] = grp      # the group number of every row

    def index_add():
        return torch.zeros(G, W, dtype=torch.float64, device=phi.device).index_add_(0, dense, phi)

    def sort_cumsum():
        cs = torch.cumsum(phi.index_select(0, order.long()), 0)
        hi = cs.index_select(0, e - 1)
        lo = torch.where((s > 0).unsqueeze(1), cs.index_select(0, (s - 1).clamp_min(0)), torch.zeros_like(hi))
        return hi - lo
    variants = {"index_add_": index_add, "sort+cumsum": sort_cumsum}
    for b in blocks:
        variants["group_rows_sum" + ("" if b is None else f"@{b}")] = \
            (lambda b=b: H.group_rows_sum(phi, order, s, e, block=b))
    want = H.group_rows_sum(phi, order, s, e)
    ref = index_add()
    err = float(((want - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    sizes = (e - s).cpu().numpy()
    return dict(case=name, V=V, W=W, groups=G, median_group=int(np.median(sizes)), max_group=int(sizes.max()),
                bytes_read=V * W * 8, max_rel_diff_to_index_add=err, ms=timed(variants, reps))


def masked_group_ids(keys, fields):
    """{field name: group id of every key} for the explained fields."""
    radix = [r for _, r, _ in fields]
    stride = [1] * len(fields)
    for i in range(len(fields) - 2, -1, -1):
        stride[i] = stride[i + 1] * radix[i + 1]
    out = {}
    for i, (n, r, e) in enumerate(fields):
        if e:
            d = keys // stride[i]
            out[n] = keys - (d if i == 0 else d % r) * stride[i]
    return out


def part_groups(reps, flow_fields):
    dev = torch.device("cuda")
    out = []
    g = torch.Generator(device="cuda").manual_seed(0)
    if flow_fields is not None:
        keys, fields = flow_fields
        k = torch.from_numpy(keys).to(dev)
        phi = torch.rand(k.numel(), 20, dtype=torch.float64, device=dev, generator=g) * 1e-3
        for n, m in masked_group_ids(k, fields).items():
            out.append(group_case(f"flow vocabulary, field {n}", phi, m, reps))
    # Zipf group sizes: 4 M rows, group of a row ~ Zipf(1.2) over 200 k groups
    V = 4_000_000
    z = torch.from_numpy(np.random.default_rng(1).zipf(1.2, V) % 200_000).to(dev)
    phi = torch.rand(V, 100, dtype=torch.float64, device=dev, generator=g)
    out.append(group_case("4 M x 100, Zipf(1.2) over 200 k groups", phi, z, max(3, reps // 3)))
    del phi
    # skew: one group holds half of 1 M rows, the rest in groups of 16
    V = 1_000_000
    r = torch.arange(V, device=dev)
    gid = torch.where(r % 2 == 0, torch.zeros_like(r), 1 + r // 32)
    phi = torch.rand(V, 20, dtype=torch.float64, device=dev, generator=g)
    out.append(group_case("skew: 1 M x 20, one group of 500 k", phi, gid, reps, blocks=(64, 256, 1024)))
    return out


def part_sides(reps):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    D, V, G, K, F = 100_000, 60_000, 200_000, 20, 4
    th = torch.rand(D, 1, K, dtype=torch.float64, device=dev, generator=g)
    ph = torch.rand(V, 1, K, dtype=torch.float64, device=dev, generator=g) * 1e-3
    gs = torch.rand(G, 1, K, dtype=torch.float64, device=dev, generator=g)
    out = []
    for n in (100_000, 2_000_000):
        doc = torch.randint(0, D, (n,), device=dev, generator=g, dtype=torch.int32)
        word = torch.randint(0, V, (n,), device=dev, generator=g, dtype=torch.int32)
        grow = torch.randint(0, G, (n, F), device=dev, generator=g, dtype=torch.int32)
        cols = [grow[:, f].contiguous() for f in range(F)]
        th2, ph2, gs2 = th[:, 0].contiguous(), ph[:, 0].contiguous(), gs[:, 0].contiguous()

        def composed():
            s = H.score_events(th2, ph2, K, 0.05, doc, word, None, None, 1.0)[0]
            return torch.stack([s / H.score_events(th2, gs2, K, 0.05, doc, c, None, None, 1.0)[0] for c in cols], 1)
        fused = lambda: H.explain_sides(th, ph, gs, doc, word, grow, 0.05)      # noqa: E731
        same = bool(torch.equal(fused()[0].view(torch.int64), composed().view(torch.int64)))
        out.append(dict(sides=n, F=F, K=K, same_bits=same,
                        ms=timed({"explain_sides": fused, "F+1 score_events + divisions": composed}, reps)))
    return out


def part_stage(reps, events, work):
    """Flow scoring stage wall (stage_seconds["flow_post"]) of whole one-process runs, alternating the flag."""
    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.synth.flow import generate_flow_day
    generate_flow_day(os.path.join(work, "in") + "/", events=events, seed=0)
    res, fields = [], None
    for limit in (-1, 3000):
        secs = {False: [], True: []}
        info = {}
        for rep in range(reps + 1):      # the first round warms up
            for flag in (False, True):
                lp = os.path.join(work, f"run_{limit}_{int(flag)}")
                shutil.rmtree(lp, ignore_errors=True)
                cfg = CFG.resolve("20160122", "flow", tol=1e-5, conf_path=None, environ={}, lpath=lp,
                                  flow_path=os.path.join(work, "in"), backend="hip", verbose=False, compat="fixed",
                                  max_results=limit, explain=flag)
                cfg.settings = LDASettings()
                s = run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
                if rep:
                    secs[flag].append(s["stage_seconds"]["flow_post"])
                if flag:
                    info = dict(written=s["scored"], why=s["explain_why_hist"], max_group=s["explain_max_group"])
                    from oni_ml_amd.pipeline.common import load_word_fields
                    fields = load_word_fields(lp)
        res.append(dict(events=events, max_results=limit, **info,
                        flow_post_seconds={("explain" if k else "plain"): (round(float(np.median(v)), 4), round(min(v), 4),
                                                                          round(max(v), 4)) for k, v in secs.items()}))
    return res, fields


def part_sizes(flow_fields, events, work):
    out = {}

    def stats(keys, fields):
        r = {}
        for n, m in masked_group_ids(torch.from_numpy(keys), fields).items():
            c = torch.unique(m, return_counts=True)[1].numpy()
            r[n] = dict(groups=int(c.size), median=int(np.median(c)), max=int(c.max()))
        return r
    if flow_fields is not None:
        out["flow"] = dict(V=int(flow_fields[0].size), fields=stats(*flow_fields))
    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.pipeline.common import load_word_fields
    from oni_ml_amd.synth.dns import generate_dns_day
    gen = generate_dns_day(os.path.join(work, "dns_in"), events=events, seed=0, n_names=max(20_000, events // 10),
                           n_clients=max(5_000, events // 40))
    lp = os.path.join(work, "dns_run")
    cfg = CFG.resolve("20160122", "dns", tol=1e-5, conf_path=None, environ={}, lpath=lp, dns_path=gen["dns_path"],
                      top1m=gen["top1m"], backend="hip", verbose=False, compat="fixed", explain=True, max_results=3000)
    cfg.settings = LDASettings(em_max_iter=5)
    s = run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
    keys, fields = load_word_fields(lp)
    out["dns"] = dict(V=int(keys.size), events=events, fields=stats(keys, fields), why=s["explain_why_hist"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="stage,groups,sides,sizes")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--events", type=int, default=1_000_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("explain_bench: needs a GPU")
    parts = a.parts.split(",")
    rec = dict(device=torch.cuda.get_device_name(0), group_block=CFG.GROUP_BLOCK, reps=a.reps)
    work = tempfile.mkdtemp(prefix="explain_bench_")
    try:
        fields = None
        if "stage" in parts:
            rec["stage"], fields = part_stage(max(2, a.reps // 3), a.events, work)
            json.dump(rec, open(a.out, "w"), indent=1)
        if "groups" in parts:
            rec["groups"] = part_groups(a.reps, fields)
            json.dump(rec, open(a.out, "w"), indent=1)
        if "sides" in parts:
            rec["sides"] = part_sides(a.reps)
            json.dump(rec, open(a.out, "w"), indent=1)
        if "sizes" in parts:
            rec["sizes"] = part_sizes(fields, a.events, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
