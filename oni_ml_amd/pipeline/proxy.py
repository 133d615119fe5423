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
from ..corpus.builder import count_pairs
from ..features import proxy as FP
from ..score import scorer as S
from . import common as C
from .driver import PipelineSpec, Pre, run_stages


def _load(cfg, res, summary, log):
    tab = FP.load_proxy(cfg.proxy_path)
    top = FP.load_top_domains(cfg.top1m)
    if not top:
        log(f"warning: top-1m list {cfg.top1m!r} not found; every host gets top 0/2")
    res.update(rows=tab.n, raw_rows=tab.n_input, dropped=tab.dropped, top_domains=len(top),
               **{"dropped_" + k: v for k, v in tab.drop_reasons.items()})
    summary["input"] = dict(rows=tab.n, dropped=tab.dropped)
    return tab, top


def _pre(cfg, inputs, device, res, log):
    tab, top = inputs
    feat = FP.featurize(tab, device, top, threads=cfg.threads)
    wsp = FP.ProxyWordSpace(feat)
    dwc = count_pairs(feat.ip, feat.word_key, feat.weight)
    C.save_json(os.path.join(cfg.lpath, "proxy_cuts.json"), dict(cuts={k: v.tolist() for k, v in feat.cuts.items()}))
    res["pairs"] = dwc.n
    log("cuts: " + " ".join(f"{k}={v.tolist()}" for k, v in feat.cuts.items()))
    # keep: the cut-independent features, reused
    return Pre(dwc, feat.ip_names, wsp.decode, keep=feat.host, fields=wsp.fields())


def _post(cfg, inputs, tables, device, log, pre):
    tab, top = inputs
    return score_proxy(cfg, tab, top, tables, device, log, host=None if pre is None else pre.keep)


SPEC = PipelineSpec("proxy", _load, _pre, _post)


def run(cfg, dist=None, device=None, log=print) -> dict:
    if (dist is not None and dist.active) or cfg.gpus > 1 or cfg.hdfs:
        raise ValueError(ONE_PROCESS)
    return run_stages(dataclasses.replace(cfg, compat="fixed"), SPEC, device, log)


def score_proxy(cfg, tab: FP.ProxyTable, top, tables: C.ModelTables, device, log=print, host=None) -> dict:
    """Features again with the persisted cuts (``host``: proxy_pre's cut-independent part, when it ran in this
    process; a resumed run computes it again), score = theta[clientip] . phi[word] (one-sided), the rows under TOL
    ascending (the MAXRESULTS lowest when set) into proxy_results.csv."""
    from ..ops import sortgroup as SG
    cuts = {k: np.asarray(v, np.float64) for k, v in C.load_json(os.path.join(cfg.lpath, "proxy_cuts.json"))["cuts"].items()}
    feat = FP.featurize(tab, device, top, cuts=cuts, threads=cfg.threads, host=host)
    wsp = FP.ProxyWordSpace(feat)
    uk, inv = SG.unique(feat.word_key, return_inverse=True)
    unames = wsp.decode(uk.cpu().numpy())
    th, ph, didx, widx = C.one_sided_index(tables, feat.ip_names, feat.ip, unames, inv, device)
    model = S.build_model(tables, th, ph, S.default_value("proxy", tables.K, False), device)
    sc, _, key, flag, votes = S.score_votes(model, didx, widx, None, None, cfg.tol)
    # --tail-tol: the events are flagged and ranked by their tail p-value; the files' score columns stay
    tr = C.tail_keys(cfg, model, (didx,), (widx,), log=log) if cfg.tail_tol is not None else None
    ranked = C.rank_results(cfg, key, flag) if tr is None else C.rank_results(cfg, tr.key, tr.flag)

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
    return C.write_results(cfg, tables, "requests", ranked, key, row_cols, int(feat.word_key.numel()),
                           (didx, sc, None, None), votes, log, sep="\t",
                           explain=C.ExplainInput(model, (widx,), ((feat.ip_names, feat.ip),), ((-2, -1),)),
                           tail_rank=tr)
