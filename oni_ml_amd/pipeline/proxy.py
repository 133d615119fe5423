"""Proxy suspicious-connects pipeline (ml_ops YYYYMMDD proxy [TOL] [MAXRESULTS]).

Stages: load -> proxy_pre -> lda_pre -> lda -> lda_post -> proxy_post.  Output proxy_results.csv is
tab-separated (user agents and URIs contain commas): the 19 input columns, word, score.

One process only, and always the "fixed" rules whatever --compat says: the agent cuts are persisted
(proxy_cuts.json) and reused when scoring, the miss vector is 1/K, any K is allowed and word names are never
truncated (proxy words are longer than 20 bytes).  Analyst feedback (proxy_scores.csv) is not read.
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np
import torch

from ..config import PROXY_ONE_PROCESS as ONE_PROCESS
from ..corpus.builder import count_pairs, lda_pre
from ..features import proxy as FP
from ..score import scorer as S
from . import common as C
from .runner import StageRunner


def run(cfg, dist=None, device=None, log=print) -> dict:
    if (dist is not None and dist.active) or cfg.gpus > 1 or cfg.hdfs:
        raise ValueError(ONE_PROCESS)
    cfg = dataclasses.replace(cfg, compat="fixed")
    device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
    R = StageRunner(cfg.lpath, resume=cfg.resume, rank=0, log=log,
                    sync=(torch.cuda.synchronize if device.type == "cuda" else None))
    summary = {}
    tab = built = None
    doc_names = word_names = None
    top = None
    pre_host = None      # proxy_pre's cut-independent features: proxy_post reuses them
    ens = C.Ensemble(cfg, R, "proxy_post", device, log)      # --ensemble; inert with one model
    need_pre = not (R.done("lda_pre") and R.done("proxy_pre"))
    if need_pre or not R.done("proxy_post"):
        with R.stage("load") as res:
            tab = FP.load_proxy(cfg.proxy_path)
            top = FP.load_top_domains(cfg.top1m)
            if not top:
                log(f"warning: top-1m list {cfg.top1m!r} not found; every host gets top 0/2")
            res.update(rows=tab.n, raw_rows=tab.n_input, dropped=tab.dropped, top_domains=len(top),
                       **{"dropped_" + k: v for k, v in tab.drop_reasons.items()})
            summary["input"] = dict(rows=tab.n, dropped=tab.dropped)
    if need_pre:
        with R.stage("proxy_pre") as res:
            feat = FP.featurize(tab, device, top, threads=cfg.threads)
            pre_host = feat.host
            wsp = FP.ProxyWordSpace(feat)
            dwc = count_pairs(feat.ip, feat.word_key, feat.weight)
            C.save_json(os.path.join(cfg.lpath, "proxy_cuts.json"), dict(cuts={k: v.tolist() for k, v in feat.cuts.items()}))
            res["pairs"] = dwc.n
            log("cuts: " + " ".join(f"{k}={v.tolist()}" for k, v in feat.cuts.items()))
        with R.stage("lda_pre") as res:
            built = lda_pre(dwc)
            doc_names = [feat.ip_names[i] for i in built.doc_keys.tolist()]
            word_names = wsp.decode(built.word_keys)
            lp, b_, dn_, wn_, ipn = cfg.lpath, built, doc_names, word_names, feat.ip_names
            dwc_h = dwc.to_host() if cfg.write_doc_wc else None

            def write_files():
                if dwc_h is not None:
                    from ..corpus.builder import write_doc_wc
                    write_doc_wc(os.path.join(lp, "doc_wc.dat"), dwc_h, ipn, C.vocab_lookup(b_.word_keys, wn_))
                C.write_corpus_files(lp, b_, dn_, wn_)
            # as in the DNS pipeline: the text files on a thread during EM, the marker waits for them
            res["_defer"] = C.background(write_files, "oni-lda-pre-writer")
            res.update(docs=built.corpus.num_docs, terms=built.corpus.num_terms, nnz=built.corpus.nnz)
            summary["corpus"] = dict(docs=built.corpus.num_docs, terms=built.corpus.num_terms, nnz=built.corpus.nnz)
    else:
        R.skip("proxy_pre")
        R.skip("lda_pre")

    corpus = built.corpus if built is not None else None
    if not R.done("lda"):
        if corpus is None:
            corpus, doc_names, word_names = C.load_corpus_files(cfg.lpath)
        with R.stage("lda") as res:
            lres = C.run_lda(cfg, corpus, dist=None, device=device, log=log)
            res["_defer"] = lres.close_files
            res.update(getattr(lres, "timing", {}))
            res.update(em_iterations=lres.em_iterations, alpha=lres.alpha)
            m = lres.engine.metrics(lres.seconds, lres.em_iterations)
            res.update({k: v for k, v in m.items() if not isinstance(v, list)})
            summary["lda"] = dict(em_iterations=lres.em_iterations, timing=getattr(lres, "timing", {}),
                                  seconds=lres.seconds, alpha=lres.alpha,
                                  likelihood=lres.likelihoods[-1][0] if lres.likelihoods else None)
            ens.lda_ran(corpus, summary)     # the lda marker is written once every member is done
        gamma, log_beta = lres.gamma, lres.log_beta
    else:
        R.skip("lda")
        gamma = log_beta = None
        ens.lda_skipped(corpus, summary)     # member 0 is complete: the members that are not
    try:
        if not R.done("lda_post"):
            if doc_names is None:
                _, doc_names, word_names = C.load_corpus_files(cfg.lpath)
            if gamma is None:
                from ..models.lda.estimate import load_final
                gamma, log_beta = load_final(cfg.lpath)
            with R.stage("lda_post"):
                tables = C.run_export(cfg, doc_names, gamma, word_names, log_beta, read_back=True)
                ens.exported(tables, doc_names, word_names)
        else:
            R.skip("lda_post")
            tables = C.load_model_tables(cfg.lpath)
            ens.loaded(tables)

        if not R.done("proxy_post"):
            with R.stage("proxy_post") as res:
                res.update(score_proxy(cfg, tab, top, tables, device, log, host=pre_host))
                summary["scored"] = res.get("flagged")
                summary["below_tol"] = res.get("below_tol")
                if cfg.host_report:
                    summary["hosts"], summary["host_sides_skipped"] = res.get("hosts"), res.get("host_sides_skipped")
                ens.scored(res, summary)
        else:
            R.skip("proxy_post")
    except BaseException:
        R.finish_deferred(suppress=True)
        raise
    R.finish_deferred()
    summary["stage_seconds"] = dict(R.times)
    return summary


def score_proxy(cfg, tab: FP.ProxyTable, top, tables: C.ModelTables, device, log=print, host=None) -> dict:
    """Features again with the persisted cuts (``host``: proxy_pre's cut-independent part, when it ran in this
    process; a resumed run computes it again), score = theta[clientip] . phi[word] (one-sided), the rows under TOL
    ascending (the MAXRESULTS lowest when set) into proxy_results.csv."""
    from ..ops import native
    from ..ops import sortgroup as SG
    cuts = {k: np.asarray(v, np.float64) for k, v in C.load_json(os.path.join(cfg.lpath, "proxy_cuts.json"))["cuts"].items()}
    feat = FP.featurize(tab, device, top, cuts=cuts, threads=cfg.threads, host=host)
    wsp = FP.ProxyWordSpace(feat)
    uk, inv = SG.unique(feat.word_key, return_inverse=True)
    unames = wsp.decode(uk.cpu().numpy())
    di = tables.doc_index()
    m = np.fromiter((di.get(n, -1) for n in feat.ip_names), dtype=np.int64, count=len(feat.ip_names))
    th, ph, drow, wrow = tables.compact(m, tables.word_rows(unames))
    widx = SG.gather(torch.from_numpy(wrow).to(device), inv)
    didx = SG.gather(torch.from_numpy(drow).to(device), feat.ip)
    K = tables.K
    model = S.build_model(tables, th, ph, S.default_value("proxy", K, False), device)
    sc, _, key, flag, votes = S.score_votes(model, didx, widx, None, None, cfg.tol)
    limit = cfg.max_results if cfg.max_results > 0 else None      # MAXRESULTS: the `limit` lowest scores only
    if limit is None:
        order = S.rank_flagged(key, flag)
        below = int(order.size)
    else:
        order, below = S.rank_flagged_counted(key, flag, limit)
    n = int(order.size)
    out = os.path.join(cfg.lpath, "proxy_results.csv")

    def row_cols(order):
        """The 21 columns of the given requests, in that order."""
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(min(len(FP.COLUMNS), max(1, cfg.threads))) as ex:
            enc = list(ex.map(lambda c: tab.take_encoded(c, order), FP.COLUMNS))
        o_t = torch.from_numpy(order).to(sc.device)
        return [("dict", names, ids) for ids, names in enc] + [
            ("dict", unames, SG.gather(inv, o_t).cpu().numpy().astype(np.int32)),
            ("java", SG.gather(sc, o_t).cpu().numpy()),
        ]
    cols = row_cols(order)
    native.lib().write_rows(out, None, cols, sep="\t", threads=cfg.threads, n=n)
    log(f"proxy_post: {C.flagged_text(n, below, limit, 'requests', cfg.tol)} written to {out}")
    hosts = (C.write_host_report(cfg, tables, didx, sc, None, None, row_cols, sep="\t", log=log)
             if cfg.host_report else {})
    return dict(flagged=n, below_tol=below, events=int(feat.word_key.numel()), **hosts, **C.votes_hist(votes, order, cfg.ensemble))
