"""Does --ensemble R make the result independent of the seed?  (profiles/ensemble_stability.md)

    python scripts/ensemble_stability.py [--events 100000] [--rs 1,2,4,8] [--pairs 5] [--backend auto]
                                         [--em-max-iter 100] [--json out.json]

One synthetic flow day is featurized once (the pipeline's own features, corpus and event -> row maps, compat
fixed).  For every R two ensembles are built from disjoint seed ranges, base .. base + R - 1 and base + 1000 ..
base + 1000 + R - 1, every event is scored by each (``scorer.score`` on an ``EnsembleModel``: the HIP kernel on a
GPU, the torch twin elsewhere) and the overlap of their N lowest-scoring events is reported, at N = 0.1 % and 1 %
of the day: |A and B| / N, the N lowest taken as MAXRESULTS takes them (``scorer.rank_flagged``, ties to the
lower row).  ``--pairs`` pairs of seed ranges per R (base = 2000 p), as mean and min..max.  The fits are shared:
an ensemble of R members is the first R of its range's 8 fits.  At R = 1 the figure is the seed-to-seed overlap
of single models.

The synthetic flow day plants no events, so no recall is reported for it.
"""
import argparse
import dataclasses
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oni_ml_amd.corpus.builder import concat, count_pairs, lda_pre  # noqa: E402
from oni_ml_amd.export import lda_post  # noqa: E402
from oni_ml_amd.features import flow as FF  # noqa: E402
from oni_ml_amd.models.lda.estimate import estimate  # noqa: E402
from oni_ml_amd.models.lda.settings import LDASettings  # noqa: E402
from oni_ml_amd.ops import sortgroup as SG  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402
from oni_ml_amd.synth.flow import generate_flow_day  # noqa: E402

FRACTIONS = (0.001, 0.01)


def flow_day(events, device, tmp):
    """(corpus, doc rows and word rows of every event's two sides on the device)."""
    generate_flow_day(os.path.join(tmp, "in") + "/", events=events, seed=0)
    ft = FF.load_flow(os.path.join(tmp, "in"), None, 1000, 8)
    feat = FF.featurize(ft, device)
    ws = FF.word_space_for(feat)
    src, dst = FF.word_keys(feat, ws)
    dwc = concat([count_pairs(feat.sip, src, feat.weight), count_pairs(feat.dip, dst, feat.weight)], merge=True)
    built = lda_pre(dwc)
    drow = torch.from_numpy(C.doc_rows_of(built.doc_keys, len(ft.ip_names))).to(device)
    wk = torch.from_numpy(np.asarray(built.word_keys, np.int64)).to(device)
    order = torch.argsort(wk)
    pos = torch.searchsorted(wk[order], torch.cat([src, dst]).to(torch.int64)).clamp_max(wk.numel() - 1)
    wrow = order[pos]
    assert bool((wk[wrow] == torch.cat([src, dst])).all()), "an event's word is not in the vocabulary"
    n = src.numel()
    return built.corpus, (SG.gather(drow, feat.sip), wrow[:n], SG.gather(drow, feat.dip), wrow[n:])


def fit(corpus, K, settings, seed, backend, device, tmp):
    """(theta, phi, EM iterations, seconds) of one model, through the export's arithmetic."""
    out = os.path.join(tmp, "fit")
    shutil.rmtree(out, ignore_errors=True)
    res = estimate(corpus, K, 2.5, settings, "random", out, backend=backend, device=device, seed=seed)
    th = lda_post.doc_topics(res.gamma, strict=False)
    ph = lda_post.word_topics(res.log_beta, strict=False)
    res.engine = None
    return th, ph, res.em_iterations, res.seconds


def lowest(members, rows, K, device, Ns):
    """The sets of the N lowest-scoring events of the ensemble ``members``, for every N."""
    model = S.EnsembleModel.build(members, 1.0 / K, device)
    _, _, key, flag = S.score(model, *rows, tol=float("inf"))
    order = S.rank_flagged(key, flag, limit=max(Ns))
    return [set(order[:N].tolist()) for N in Ns]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=100_000)
    ap.add_argument("--rs", default="1,2,4,8")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--topics", type=int, default=20)
    ap.add_argument("--backend", default="auto")
    ap.add_argument("--em-max-iter", type=int, default=None)
    ap.add_argument("--json")
    a = ap.parse_args()
    Rs = sorted(int(x) for x in a.rs.split(","))
    device = torch.device("cuda" if torch.cuda.is_available() and a.backend != "cpu" else "cpu")
    settings = LDASettings() if a.em_max_iter is None else LDASettings(em_max_iter=a.em_max_iter)
    settings = dataclasses.replace(settings, lag=0)
    tmp = tempfile.mkdtemp(prefix="oni_stab_")
    try:
        corpus, rows = flow_day(a.events, device, tmp)
        Ns = [max(1, int(round(f * a.events))) for f in FRACTIONS]
        head = dict(events=a.events, docs=corpus.num_docs, terms=corpus.num_terms, nnz=corpus.nnz, topics=a.topics,
                    device=str(device), backend=a.backend, Ns=Ns, pairs=a.pairs)
        print(json.dumps(head), flush=True)
        overlap = {R: [[] for _ in Ns] for R in Rs}
        fits = []
        for p in range(a.pairs):
            both = []
            for base in (2000 * p, 2000 * p + 1000):
                ms = []
                for r in range(max(Rs)):
                    th, ph, it, sec = fit(corpus, a.topics, settings, base + r, a.backend, device, tmp)
                    fits.append(dict(seed=base + r, em_iterations=it, seconds=round(sec, 4)))
                    ms.append((th, ph))
                both.append(ms)
            for R in Rs:
                A = lowest(both[0][:R], rows, a.topics, device, Ns)
                B = lowest(both[1][:R], rows, a.topics, device, Ns)
                for j, N in enumerate(Ns):
                    overlap[R][j].append(len(A[j] & B[j]) / N)
            print(json.dumps(dict(pair=p, overlap={R: [round(v[-1], 4) for v in overlap[R]] for R in Rs})), flush=True)
        recs = []
        for R in Rs:
            rec = dict(R=R)
            for f, N, v in zip(FRACTIONS, Ns, overlap[R]):
                rec[f"overlap_{f:g}"] = dict(N=N, mean=round(float(np.mean(v)), 4), min=round(min(v), 4),
                                             max=round(max(v), 4))
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        its = [f["em_iterations"] for f in fits]
        secs = [f["seconds"] for f in fits]
        summary = dict(fits=len(fits), em_iterations_median=float(np.median(its)), em_iterations_min=min(its),
                       em_iterations_max=max(its), fit_seconds_median=round(float(np.median(secs)), 4),
                       fit_seconds_total=round(float(np.sum(secs)), 2))
        print(json.dumps(summary), flush=True)
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(dict(head=head, results=recs, fits=summary, t=time.strftime("%Y-%m-%d")), f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
