"""Measurements of --tail on an MI355X (profiles/tail_mass.md).  Needs a GPU: there is no CPU fall-back.

  stage    the flow scoring stage's wall with and without --tail on the 1 M-event day at TOL 1e-5, unlimited and
           with MAXRESULTS 3000 (the run without the flag is the parent commit's behaviour), and what the column
           buys on that day: the overlap of the N lowest-tail written sides with the N lowest scores, the spread of
           tail among the 1,000 lowest scores, written sides per host by quartile of the host's entropy
  kernel   ops.hip.tail_mass against the torch formulation a user would write -- batched theta_sides @ phi^T in
           fp64, a compare and masked sums; not bit-equal -- at (pairs, V, K, R) = the day's two shapes,
           (1e5, 63,707, 100, 1) and (1e4, 63,707, 20, 8); the achieved share of the fp64 vector peak and the phi
           bytes the workgroups stage against V R K 8 per tile of sides
  block    TAIL_BLOCK 256 / 1024 / 4096 at the day's unlimited shape

Every kernel timing: device events around one call, warmed up, `--reps` repetitions with the variants alternating;
the record gives the median and the range.  `python scripts/tail_bench.py --out FILE [--parts stage,kernel,block]`."""
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

FP64_VECTOR_PEAK = 78.6e12      # MI355X fp64 vector, flop/s (half the fp32 vector rate; an FMA counts two)
TILE = {"registers": 256, "lds_theta": 64, "direct": 256}      # sides per workgroup of each form


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


def torch_tail(th, ph, doc, word, slab=1 << 27):
    """The alternative: per batch of sides P = mean over members of theta @ phi^T, then compares and sums."""
    V, R, K = ph.shape
    n = doc.numel()
    le = torch.empty(n, dtype=torch.float64, device=ph.device)
    tot, rarer = torch.empty_like(le), torch.empty(n, dtype=torch.int64, device=ph.device)
    ties = torch.empty_like(rarer)
    step = max(1, slab // V)
    pt = ph.permute(1, 2, 0).contiguous()      # [R, K, V]
    for b0 in range(0, n, step):
        d, w = doc[b0:b0 + step].long(), word[b0:b0 + step].long()
        p = torch.bmm(th[d].permute(1, 0, 2), pt).sum(0) / R if R > 1 else th[d, 0] @ pt[0]
        s = p.gather(1, w.unsqueeze(1))
        le[b0:b0 + step] = torch.where(p <= s, p, torch.zeros((), dtype=p.dtype, device=p.device)).sum(1)
        tot[b0:b0 + step] = p.sum(1)
        rarer[b0:b0 + step] = (p < s).sum(1)
        ties[b0:b0 + step] = (p == s).sum(1)
    return le, tot, rarer, ties


def shape_case(pairs, V, K, R, reps, blocks=(None,), with_torch=True):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(pairs % 1000 + K)
    D = 20_000
    th = torch.rand(D, R, K, dtype=torch.float64, device=dev, generator=g)
    th /= th.sum(2, keepdim=True)
    ph = torch.rand(V, R, K, dtype=torch.float64, device=dev, generator=g) ** 8
    ph /= ph.sum(0, keepdim=True)
    doc = torch.randint(0, D, (pairs,), device=dev, generator=g, dtype=torch.int32)
    word = torch.randint(0, V, (pairs,), device=dev, generator=g, dtype=torch.int32)
    variants = {}
    for b in blocks:
        variants["tail_mass" + ("" if b is None else f"@{b}")] = (lambda b=b: H.tail_mass(th, ph, doc, word, block=b))
    if with_torch:
        variants["torch"] = lambda: torch_tail(th, ph, doc, word)
    ms = timed(variants, reps)
    out = dict(pairs=pairs, V=V, K=K, R=R, path=H.tail_theta_path(R, K), ms=ms)
    if with_torch:
        a, b = H.tail_mass(th, ph, doc, word), torch_tail(th, ph, doc, word)
        out["max_rel_diff_of_tail"] = float((((a[0] / a[1]) - (b[0] / b[1])).abs() / (b[0] / b[1])).max())
        out["counts_equal"] = float(((a[2].long() == b[2]) & (a[3].long() == b[3])).double().mean())
    flop = 2.0 * pairs * V * K * R
    for k, v in ms.items():
        if k.startswith("tail_mass"):
            out.setdefault("fp64_peak_share", {})[k] = round(flop / (v[0] * 1e-3) / FP64_VECTOR_PEAK, 4)
    tiles = -(-pairs // TILE[out["path"]])
    out["phi_bytes_staged"] = tiles * V * R * K * 8      # every row once per tile of sides: the ideal
    out["phi_table_bytes"] = V * R * K * 8
    out["torch_slab_bytes_if_unbatched"] = pairs * V * 8
    return out


def buys(lp, tol):
    """What the tail column shows on the written day, from its files."""
    from oni_ml_amd.export import lda_post
    rows = [ln.split(",") for ln in open(os.path.join(lp, "flow_tail.csv"), encoding="utf-8").read().split("\n")[:-1]]
    doc, score, tail = [], [], []
    for f in rows:
        for j in (0, 1):
            c = f[1 + 5 * j:6 + 5 * j]
            if c[3]:
                doc.append(c[0])
                score.append(float(c[2]))
                tail.append(float(c[3]))
    score, tail = np.asarray(score), np.asarray(tail)
    out = dict(sides_with_tail=int(score.size))
    by_s, by_t = np.argsort(score, kind="stable"), np.argsort(tail, kind="stable")
    for N in (1000, 10000):
        if score.size >= N:
            out[f"overlap_lowest_{N}"] = round(len(set(by_s[:N].tolist()) & set(by_t[:N].tolist())) / N, 4)
    low = tail[by_s[:1000]]
    out["tail_of_1000_lowest_scores"] = dict(min=float(low.min()), median=float(np.median(low)), max=float(low.max()))
    x, y = np.argsort(np.argsort(score)), np.argsort(np.argsort(tail))
    out["rank_correlation"] = round(float(np.corrcoef(x, y)[0, 1]), 4)
    # host entropy: H(p(. | d)) over the written table, for the hosts with a written side
    dn, th = lda_post.read_results(os.path.join(lp, "doc_results.csv"))
    _, ph = lda_post.read_results(os.path.join(lp, "word_results.csv"))
    di = {n: i for i, n in enumerate(dn)}
    hosts, inv = np.unique(np.asarray([di[d] for d in doc]), return_inverse=True)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    pt, ent = torch.from_numpy(ph).to(dev).T.contiguous(), []
    for h0 in range(0, hosts.size, 4096):      # [4096, V] at a time
        p = torch.from_numpy(th[hosts[h0:h0 + 4096]]).to(dev) @ pt
        p = p / p.sum(1, keepdim=True)
        ent.append((-(p * torch.log(p.clamp_min(1e-300))).sum(1)).cpu().numpy())
    ent = np.concatenate(ent)
    q = np.quantile(ent, [0.25, 0.5, 0.75])
    quart = np.searchsorted(q, ent)
    N = max(1, score.size // 10)
    in_s, in_t = np.zeros(score.size, bool), np.zeros(score.size, bool)
    in_s[by_s[:N]], in_t[by_t[:N]] = True, True
    out["hosts"] = int(hosts.size)
    out["entropy_quartile_edges"] = [round(float(v), 3) for v in q]
    out["per_entropy_quartile"] = []
    for k in range(4):
        h = quart == k
        sides = h[inv]
        out["per_entropy_quartile"].append(dict(
            hosts=int(h.sum()), written_sides_per_host=round(float(sides.sum() / max(1, h.sum())), 2),
            share_of_lowest_tenth_by_score=round(float((sides & in_s).sum() / N), 4),
            share_of_lowest_tenth_by_tail=round(float((sides & in_t).sum() / N), 4)))
    return out


def part_stage(reps, events, work, tol):
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
                                  max_results=limit, tail=flag)
                cfg.settings = LDASettings()
                s = run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
                if rep:
                    secs[flag].append(s["stage_seconds"]["flow_post"])
                if flag:
                    info = dict(written=s["scored"], **{k: s[k] for k in s if k.startswith("tail_")})
        entry = dict(events=events, tol=tol, max_results=limit, **info,
                     flow_post_seconds={("tail" if k else "plain"): (round(float(np.median(v)), 4), round(min(v), 4),
                                                                     round(max(v), 4)) for k, v in secs.items()})
        if limit < 0:
            entry["buys"] = buys(os.path.join(work, "run_-1_1"), tol)
        res.append(entry)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="stage,kernel,block")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--events", type=int, default=1_000_000)
    ap.add_argument("--tol", type=float, default=1e-5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tail_bench: needs a GPU")
    parts = a.parts.split(",")
    rec = dict(device=torch.cuda.get_device_name(0), tail_block=CFG.TAIL_BLOCK, reps=a.reps,
               fp64_vector_peak=FP64_VECTOR_PEAK)
    day = [(100_000, 63_707), (6_000, 63_707)]      # (pairs, V) of the day's two shapes when the stage part is off
    work = tempfile.mkdtemp(prefix="tail_bench_")
    try:
        if "stage" in parts:
            rec["stage"] = part_stage(max(2, a.reps // 3), a.events, work, a.tol)
            day = [(max(1, e["tail_pairs"]), e["tail_words"]) for e in rec["stage"]]
            json.dump(rec, open(a.out, "w"), indent=1)
        if "kernel" in parts:
            rec["kernel"] = [shape_case(day[0][0], day[0][1], 20, 1, a.reps),
                             shape_case(day[1][0], day[1][1], 20, 1, a.reps),
                             shape_case(100_000, 63_707, 100, 1, max(3, a.reps // 2)),
                             shape_case(10_000, 63_707, 20, 8, max(3, a.reps // 2))]
            json.dump(rec, open(a.out, "w"), indent=1)
        if "block" in parts:
            rec["block"] = shape_case(day[0][0], day[0][1], 20, 1, a.reps, blocks=(256, 1024, 4096), with_torch=False)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
