"""Measurements of --holdout on an MI355X (profiles/holdout.md).  Needs a GPU: there is no CPU fall-back.

  stage    whole one-process runs of the 1 M-event flow day with --holdout 0.2 --holdout-topics 10,20,30,50 at the
           seeds 0 and 1 (seed 0 twice: the first run warms up and is left out): the holdout stage's wall against
           the same run's lda stage, and the perplexity table by K
  kernels  ops.hip.holdout_draw and ops.hip.holdout_entries against their torch twins run on the device, on that
           day's corpus (theta and phi of its K = 20 training fit), and on a skew case -- the same corpus with one
           more entry that holds as many tokens as all the others together -- at HOLDOUT_LANE_TOKENS 16, 64 and 256

Every kernel timing: device events around one call, warmed up, `--reps` repetitions with the variants alternating;
the record gives the median and the range.  `python scripts/holdout_bench.py --out FILE [--parts stage,kernels]`."""
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
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.ops import sortgroup as SG  # noqa: E402

TOPICS = "10,20,30,50"


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


def part_stage(events, work):
    from oni_ml_amd.models.lda.settings import LDASettings
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.synth.flow import generate_flow_day
    generate_flow_day(os.path.join(work, "in") + "/", events=events, seed=0)
    runs = []
    for i, seed in enumerate((0, 0, 1)):
        lp = os.path.join(work, f"run_{i}")
        cfg = CFG.resolve("20160122", "flow", tol=1e-5, conf_path=None, environ={}, lpath=lp,
                          flow_path=os.path.join(work, "in"), backend="hip", verbose=False, compat="fixed",
                          max_results=3000, seed=seed, holdout=0.2, holdout_topics=TOPICS)
        cfg.settings = LDASettings()
        s = run(cfg.validate(), device="cuda", log=lambda *a, **k: None)
        if i == 0:
            continue      # the warm-up
        j = json.load(open(os.path.join(lp, "holdout", "holdout.json")))
        runs.append(dict(seed=seed, corpus=s["corpus"], holdout_stage_seconds=round(s["stage_seconds"]["holdout"], 4),
                         lda_stage_seconds=round(s["stage_seconds"]["lda"], 4), split=j["split"], selected=j["selected"],
                         records=[{k: r[k] for k in ("topics", "em_iterations", "perplexity", "unseen_tokens",
                                                     "evaluated_tokens", "seconds")} for r in j["records"]]))
    return dict(events=events, fraction=0.2, topics=TOPICS, runs=runs), os.path.join(work, "run_1")


def part_kernels(reps, lp):
    from oni_ml_amd.export import lda_post
    from oni_ml_amd.models.lda import holdout as HO
    from oni_ml_amd.models.lda.estimate import load_final
    from oni_ml_amd.pipeline.common import load_corpus_files
    dev = torch.device("cuda")
    c = load_corpus_files(lp)[0]
    ptr, counts = torch.from_numpy(c.doc_ptr).to(dev), torch.from_numpy(c.counts).to(dev)
    thr = R.holdout_thr(0.2)
    out = dict(corpus=dict(docs=c.num_docs, terms=c.num_terms, nnz=c.nnz, tokens=int(c.counts.sum()),
                           largest_entry=int(c.counts.max())))
    same = bool(torch.equal(H.holdout_draw(ptr, counts, 0, thr, rules=False), R.holdout_draw(ptr, counts, 0, thr, rules=False)))
    out["draw"] = dict(same=same, ms=timed({"holdout_draw": lambda: H.holdout_draw(ptr, counts, 0, thr, rules=False),
                                            "torch twin": lambda: R.holdout_draw(ptr, counts, 0, thr, rules=False),
                                            "document rules (torch, both)": lambda: R.holdout_rules(ptr, counts, counts // 5)},
                                           reps))
    # skew: one more entry (a document of its own) with as many tokens as all the others together
    big = torch.cat([counts, counts.sum().reshape(1)])
    ptr2 = torch.cat([ptr, torch.full((1,), c.nnz + 1, dtype=torch.int64, device=dev)])
    want = R.holdout_draw(ptr2, big, 0, thr, rules=False)
    v = {"torch twin": lambda: R.holdout_draw(ptr2, big, 0, thr, rules=False)}
    ok = {}
    for L in (16, 64, 256):
        v[f"holdout_draw@{L}"] = (lambda L=L: H.holdout_draw(ptr2, big, 0, thr, rules=False, lane_tokens=L))
        ok[L] = bool(torch.equal(v[f"holdout_draw@{L}"](), want))
    out["draw_skew"] = dict(tokens=int(big.sum()), largest_entry=int(big.max()), same=ok, ms=timed(v, reps))
    # the entries: theta and phi of the day's K = 20 training fit
    train, t = HO.split(c, 0.2, 0, dev)
    g, lb = load_final(os.path.join(lp, "holdout", "k20"))
    th = torch.from_numpy(np.ascontiguousarray(lda_post.doc_topics(g, strict=False))).to(dev)
    ph = torch.from_numpy(np.ascontiguousarray(lda_post.word_topics(lb, strict=False))).to(dev)
    doc = SG.segment_ids(ptr[1:] - ptr[:-1], total=c.nnz).to(torch.int32)
    word = torch.from_numpy(c.word_idx).to(dev)
    seen = torch.zeros(c.num_terms, dtype=torch.uint8, device=dev)
    seen[torch.from_numpy(train.word_idx).to(dev).long()] = 1
    a = (th, ph, doc, word, t, seen)
    same = bool(torch.equal(H.holdout_entries(*a).view(torch.int64), R.holdout_entries(*a).view(torch.int64)))
    order = torch.arange(c.nnz, dtype=torch.int32, device=dev)
    s0, s1 = ptr[:-1].contiguous(), ptr[1:].contiguous()
    ll = H.holdout_entries(*a).unsqueeze(1)
    out["entries"] = dict(K=int(th.shape[1]), entries=c.nnz, with_heldout=int((t > 0).sum()), same_bits=same,
                          ms=timed({"holdout_entries": lambda: H.holdout_entries(*a),
                                    "torch twin": lambda: R.holdout_entries(*a),
                                    "group_rows_sum per document": lambda: H.group_rows_sum(ll, order, s0, s1)}, reps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", default="stage,kernels")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--events", type=int, default=1_000_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("holdout_bench: needs a GPU")
    H.lib()
    rec = dict(device=torch.cuda.get_device_name(0), lane_tokens=CFG.HOLDOUT_LANE_TOKENS, reps=a.reps)
    work = tempfile.mkdtemp(prefix="holdout_bench_")
    try:
        rec["stage"], lp = part_stage(a.events, work)
        json.dump(rec, open(a.out, "w"), indent=1)
        if "kernels" in a.parts.split(","):
            rec["kernels"] = part_kernels(a.reps, lp)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
