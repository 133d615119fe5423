"""Measurements of --tail-tol on an MI355X (profiles/tail_rank.md).  Needs a GPU: there is no CPU fall-back.

  kernel     ops.hip.tail_mass_docs against ops.hip.tail_mass (the parent commit's kernel) on the same sorted distinct
             pairs of every event of a day -- the 1 M-event flow day at K = 20 with one model and with R = 4 members,
             and the 2 M-query DNS day.  The pairs are what the day's own scoring stage hands ``scorer.tail_pairs``
             (captured from a run); the R = 4 tables are the day's θ / φ beside three row-rotated copies of
             themselves (the kernels' time depends on the shapes, not on the values).  The results are compared bit
             for bit before anything is timed.  Also the operations phases A and B execute and their share of the
             fp64 vector peak.
  crossover  the two kernels on synthetic pairs, 1 / 2 / 4 / 8 / 16 per document, at the flow day's V: the smallest
             share at which tail_mass_docs wins is config.TAIL_DOCS_MIN_SHARE; and plain --tail's call on its
             written pairs (about one per document) through the parent's ``scorer.tail_mass`` and through
             ``scorer.tail_pairs``
  stage      the flow and DNS scoring stage's wall of whole one-process runs: plain, --tail, --tail-tol at the P that
             flags as many events as TOL does, unlimited and with MAXRESULTS 3000
  buys       on the flow day: how many of the 1,000 events --tail-tol ranks first are among the 1,000 lowest scores,
             and the document lengths of the hosts in either list

Every kernel timing: device events around one call, two warm-up rounds, `--reps` repetitions with the variants
alternating; the record gives the median and the range.  `python scripts/tail_rank_bench.py --out FILE [--parts ...]`."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.ops import hip as H  # noqa: E402
from oni_ml_amd.ops import sortgroup as SG  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402
from tail_bench import FP64_VECTOR_PEAK, timed  # noqa: E402

QUIET = lambda *a, **k: None      # noqa: E731


class Day:
    """A synthetic day's inputs and its whole one-process runs on the HIP backend."""

    def __init__(self, kind, events, work, tol):
        self.kind, self.work, self.tol = kind, os.path.join(work, kind), tol
        if kind == "flow":
            from oni_ml_amd.synth.flow import generate_flow_day
            generate_flow_day(os.path.join(self.work, "in") + "/", events=events, seed=0)
            self.paths = dict(flow_path=os.path.join(self.work, "in"))
        else:
            from oni_ml_amd.synth.dns import generate_dns_day
            g = generate_dns_day(os.path.join(self.work, "in/"), events=events, seed=0, n_names=max(20_000, events // 10),
                                 n_clients=max(5_000, events // 40), with_edge_rows=False)
            self.paths = dict(dns_path=g["dns_path"], top1m=g["top1m"])

    def run(self, name, **kw):
        from oni_ml_amd.models.lda.settings import LDASettings
        from oni_ml_amd.pipeline import run
        lp = os.path.join(self.work, name)
        shutil.rmtree(lp, ignore_errors=True)
        cfg = CFG.resolve("20160122", self.kind, tol=self.tol, conf_path=None, environ={}, lpath=lp, backend="hip",
                          verbose=False, compat="fixed", **self.paths, **kw)
        cfg.settings = LDASettings()
        return lp, run(cfg.validate(), device="cuda", log=QUIET)


class Capture:
    """What a run's scoring stage computed: the arguments of every ``scorer.tail_pairs`` call and the result of
    ``tail_keys`` (the hooks are this script's; the pipeline is unchanged)."""

    def __enter__(self):
        self.pairs, self.rank = [], None
        self.tp, self.tk = S.tail_pairs, C.tail_keys

        def tail_pairs(model, doc, word):
            self.pairs.append((model, doc.clone(), word.clone()))
            return self.tp(model, doc, word)

        def tail_keys(*a, **k):
            self.rank = self.tk(*a, **k)
            return self.rank
        S.tail_pairs, C.tail_keys = tail_pairs, tail_keys
        return self

    def __exit__(self, *exc):
        S.tail_pairs, C.tail_keys = self.tp, self.tk


def same_bits(a, b):
    f = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t      # noqa: E731
    nan = torch.isnan(a[1])
    return all(torch.equal(f(x)[~nan], f(y)[~nan]) for x, y in zip(a, b)) and torch.equal(nan, torch.isnan(b[1]))


def pair_stats(doc):
    """Pairs, distinct documents, the longest document, and the document slots over the tiles of 256 pairs."""
    n = int(doc.numel())
    grp, docs = SG.run_ids(doc.to(torch.int64))
    st = SG.run_starts(grp, docs)
    first = torch.ones(n, dtype=torch.bool, device=doc.device)
    first[1:] = doc[1:] != doc[:-1]
    first[::256] = True
    return dict(pairs=n, docs=docs, pairs_per_doc=round(n / max(docs, 1), 2), longest=int((st[1:] - st[:-1]).max()),
                slots=int(first.sum()))


def kernel_case(name, theta, phi, doc, word, reps):
    theta, phi = theta.contiguous(), phi.contiguous()
    d, w = doc.to(torch.int32).contiguous(), word.to(torch.int32).contiguous()
    V, R, K = (int(x) for x in phi.shape)
    a, b = H.tail_mass_docs(theta, phi, d, w), H.tail_mass(theta, phi, d, w)
    if not same_bits(a, b):
        raise SystemExit(f"tail_rank_bench: {name}: tail_mass_docs and tail_mass differ")
    del a, b
    ms = timed({"tail_mass_docs": lambda: H.tail_mass_docs(theta, phi, d, w),
                "tail_mass": lambda: H.tail_mass(theta, phi, d, w)}, reps)
    st = pair_stats(d)
    flop_a, flop_b = 2.0 * st["slots"] * V * K * R, 2.0 * st["pairs"] * V      # multiply + add; the two adds of take()
    return dict(case=name, V=V, K=K, R=R, **st, ms=ms, bits_equal=True,
                ratio=round(ms["tail_mass"][0] / ms["tail_mass_docs"][0], 2),
                ranges_overlap=not ms["tail_mass_docs"][2] < ms["tail_mass"][1],
                flop_phase_a=flop_a, flop_phase_b=flop_b, flop_tail_mass=2.0 * st["pairs"] * V * K * R,
                fp64_peak_share=dict(
                    tail_mass_docs=round((flop_a + flop_b) / (ms["tail_mass_docs"][0] * 1e-3) / FP64_VECTOR_PEAK, 4),
                    tail_mass=round(2.0 * st["pairs"] * V * K * R / (ms["tail_mass"][0] * 1e-3) / FP64_VECTOR_PEAK, 4)))


def members4(t):
    """[rows, 1, K] -> [rows, 4, K]: the table beside three copies of itself rotated by 1, 2, 3 rows."""
    return torch.cat([t] + [t.roll(r, 0) for r in (1, 2, 3)], 1).contiguous()


def part_crossover(V, reps):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    n, K = 1 << 18, 20
    ph = torch.rand(V, 1, K, dtype=torch.float64, device=dev, generator=g) ** 8
    ph /= ph.sum(0, keepdim=True)
    out = []
    for share in (1, 2, 4, 8, 16):
        D = n // share
        th = torch.rand(D, 1, K, dtype=torch.float64, device=dev, generator=g)
        th /= th.sum(2, keepdim=True)
        doc = (torch.arange(n, device=dev) // share).to(torch.int32)
        word = torch.randint(0, V, (n,), device=dev, generator=g, dtype=torch.int32)
        ms = timed({"tail_mass_docs": lambda: H.tail_mass_docs(th, ph, doc, word),
                    "tail_mass": lambda: H.tail_mass(th, ph, doc, word)}, reps)
        out.append(dict(pairs_per_doc=share, pairs=n, V=V, K=K, ms=ms,
                        docs_wins=ms["tail_mass_docs"][2] < ms["tail_mass"][1]))
    return out


def host_timed(variants, reps):
    """{name: (median ms, min, max)} by the host clock around calls that end in a synchronise, alternating."""
    for _ in range(2):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)) for k, v in ms.items()}


def stage_rows(day, P, reps):
    """The scoring stage's wall of whole runs, the three variants alternating; the first round warms up."""
    post = f"{day.kind}_post"
    out = []
    for limit in (-1, 3000):
        variants = dict(plain={}, tail=dict(tail=True), tail_tol=dict(tail_tol=P))
        secs, info = {k: [] for k in variants}, {}
        for rep in range(reps + 1):
            for k, kw in variants.items():
                _, s = day.run(f"stage_{k}", max_results=limit, **kw)
                if rep:
                    secs[k].append(s["stage_seconds"][post])
                info[k] = dict(written=s["scored"], below=s["below_tol"],
                               **{x: s[x] for x in s if x.startswith("tail_") and x != "tail_hist"})
        out.append(dict(kind=day.kind, tol=day.tol, tail_tol=P, max_results=limit, info=info,
                        seconds={k: (round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4))
                                 for k, v in secs.items()}))
    return out


def buys(day, P, top=1000):
    """The `top` events either ranking puts first (MAXRESULTS) and the document lengths of their hosts."""
    by_s, _ = day.run("buys_score", tail=True, max_results=top)
    by_t, _ = day.run("buys_tail", tail_tol=P, max_results=top)
    corpus, docs, _ = C.load_corpus_files(by_s)
    length = dict(zip(docs, corpus.lengths().tolist()))

    def read(lp, col):
        res = open(os.path.join(lp, f"{day.kind}_results.csv"), encoding="utf-8").read().split("\n")[:-1]
        hosts = []
        for ln in open(os.path.join(lp, f"{day.kind}_tail.csv"), encoding="utf-8").read().split("\n")[:-1]:
            f = ln.split(",")
            sides = [f[1 + 5 * j:6 + 5 * j] for j in range((len(f) - 1) // 5)]
            sides = [s for s in sides if s[col]]
            if sides:      # the side that made the line's key
                hosts.append(min(sides, key=lambda s: float(s[col]))[0])
        return res, hosts
    (res_s, host_s), (res_t, host_t) = read(by_s, 2), read(by_t, 3)
    q = lambda hs: dict(zip(("min", "q25", "median", "q75", "max"),      # noqa: E731
                            (float(x) for x in np.quantile([length.get(h, 0) for h in hs], [0, .25, .5, .75, 1]))),
                        distinct_hosts=len(set(hs)))
    return dict(top=top, written_by_score=len(res_s), written_by_tail=len(res_t),
                in_both=len(set(res_s) & set(res_t)), host_length_by_score=q(host_s), host_length_by_tail=q(host_t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="kernel,crossover,stage,buys")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--flow-events", type=int, default=1_000_000)
    ap.add_argument("--dns-events", type=int, default=2_000_000)
    ap.add_argument("--tol", type=float, default=1e-5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tail_rank_bench: needs a GPU")
    parts = a.parts.split(",")
    rec = dict(device=torch.cuda.get_device_name(0), tail_block=CFG.TAIL_BLOCK, reps=a.reps, stage_reps=a.stage_reps,
               tail_docs_min_share=CFG.TAIL_DOCS_MIN_SHARE, fp64_vector_peak=FP64_VECTOR_PEAK)
    work = tempfile.mkdtemp(prefix="tail_rank_bench_")

    def save():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    try:
        for kind, events in (("flow", a.flow_events), ("dns", a.dns_events)):
            day = Day(kind, events, work, a.tol)
            # every event's pairs and tail key, from a run that flags nothing (P below every tail)
            with Capture() as cap:
                _, s0 = day.run("capture", tail_tol=1e-300)
            model, doc, word = cap.pairs[0]
            key = cap.rank.key
            _, sp = day.run("plain")
            rows = max(int(sp["scored"]), 1000)      # P: as many events as TOL flags (at least 1,000)
            good = SG.sort_stable(key[key == key])[0]
            P = float(good[min(rows, good.numel() - 1)])
            rec.setdefault("days", []).append(dict(kind=kind, events=events, tol=a.tol, rows_under_tol=int(sp["scored"]),
                                                   tail_tol=P, **{k: s0[k] for k in s0 if k.startswith("tail_rank")}))
            theta, phi = S.model_tables3(model)
            if "kernel" in parts:
                rec.setdefault("kernel", []).append(kernel_case(f"{kind} day, every event", theta, phi, doc, word, a.reps))
                if kind == "flow":
                    rec["kernel"].append(kernel_case("flow day, every event, R = 4", members4(theta), members4(phi),
                                                     doc, word, a.reps))
                save()
            if "crossover" in parts and kind == "flow":
                rec["crossover"] = part_crossover(int(phi.shape[0]), a.reps)
                with Capture() as cap:      # plain --tail's own call: the written sides' pairs
                    day.run("tail", tail=True)
                m, d, w = cap.pairs[0]
                rec["written_sides_call"] = dict(
                    **pair_stats(d.to(torch.int32)),
                    ms=host_timed({"parent: scorer.tail_mass": lambda: S.tail_mass(m, d, w),
                                   "scorer.tail_pairs": lambda: S.tail_pairs(m, d, w)}, a.reps),
                    path=S.tail_pairs(m, d, w)[1])
                save()
            del model, doc, word, key, cap, theta, phi
            if "stage" in parts:
                rec.setdefault("stage", []).extend(stage_rows(day, P, a.stage_reps))
                save()
            if "buys" in parts and kind == "flow":
                rec["buys"] = buys(day, P)
                save()
            shutil.rmtree(day.work, ignore_errors=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
