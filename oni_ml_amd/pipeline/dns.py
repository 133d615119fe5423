"""DNS suspicious-connects pipeline (ml_ops.sh YYYYMMDD dns [TOL]).

Stages: load -> dns_pre -> lda_pre -> lda -> lda_post -> dns_post
(reference: dns_pre_lda.scala, lda_pre.py, oni-lda-c, lda_post.py,
dns_post_lda.scala).  Output dns_results.csv has 16
columns: the 8 input fields, domain, subdomain, subdomain.length,
num.periods, subdomain.entropy, top_domain, word, score (dns_post_lda.scala:326-331).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from ..corpus.builder import count_pairs, lda_pre
from ..features import dns as FD
from ..score import scorer as S
from . import common as C
from . import prefetch
from .driver import PipelineSpec, Pre, run_stages


def _load(cfg, res, summary, log):
    """(table, top domains, the name features the input prefetch computed or None)."""
    got = prefetch.take(prefetch.dns_key(cfg))
    res["prefetched"] = got is not None
    if got is not None:
        tab, top, host = got
    else:
        tab = FD.load_dns(cfg.dns_path, cfg.feedback_path(), cfg.dupfactor, strict=cfg.strict)
        top, host = FD.load_top_domains(cfg.top1m), None
    if not top:
        log(f"warning: top-1m list {cfg.top1m!r} not found; every domain gets top_domain 0/2")
    res.update(rows=tab.n, raw_rows=tab.n_raw, feedback_rows=tab.n_feedback, dropped=tab.dropped,
               top_domains=len(top))
    summary["input"] = dict(rows=tab.n, feedback_rows=tab.n_feedback, dropped=tab.dropped)
    return tab, top, host


def _pre(cfg, inputs, device, res, log):
    tab, top, host = inputs
    feat = FD.featurize(tab, device, top, threads=cfg.threads, host=host)
    wsp = FD.DnsWordSpace(feat.cuts, feat.qpairs)
    dwc = count_pairs(feat.ip, feat.word_key, feat.weight)
    C.save_json(os.path.join(cfg.lpath, "dns_cuts.json"), dict(cuts={k: v.tolist() for k, v in feat.cuts.items()}))
    res["pairs"] = dwc.n
    log("cuts: " + " ".join(f"{k}={v.tolist()}" for k, v in feat.cuts.items()))
    # keep: dns_post takes its raw rows' slice
    return Pre(dwc, feat.ip_names, wsp.decode, keep=feat.host, fields=wsp.fields())


def _post(cfg, inputs, tables, device, log, pre):
    tab, top, host = inputs
    return score_dns(cfg, tab, top, tables, device, log, host=host if pre is None else pre.keep)


SPEC = PipelineSpec("dns", _load, _pre, _post)


def run(cfg, dist=None, device=None, log=print) -> dict:
    if dist is not None and dist.active:
        from .sharded import run_dns
        return run_dns(cfg, dist, device, log)
    return run_stages(cfg, SPEC, device, log)


def score_dns(cfg, tab: FD.DnsTable, top, tables: C.ModelTables, device, log=print, ctx=None, ip_map=None,
              host=None) -> dict:
    """dns_post_lda.scala:108-331.  ``ctx`` (several ranks): ``tab`` holds this rank's rows; cuts over
    every rank's raw rows; the survivors of all ranks merged into one ascending file.  ``ip_map``:
    doc row of every ip_dst id of the pre-LDA dictionary of ``tab`` (its raw rows' ids are a prefix)."""
    multi = ctx is not None and ctx.active
    cuts = None
    if not cfg.strict:
        cuts = {k: np.asarray(v, np.float64) for k, v in C.load_json(os.path.join(cfg.lpath, "dns_cuts.json"))["cuts"].items()}
    elif multi:
        from ..features import dns_dist as FDD
        cuts = FDD.global_cuts(ctx, tab, top, device, raw_only=True, threads=cfg.threads)
    feat = FD.featurize(tab, device, top, cuts=cuts, raw_only=True, threads=cfg.threads, host=host)
    wsp = FD.DnsWordSpace(feat.cuts, feat.qpairs)
    from ..ops import sortgroup as SG
    uk, inv = SG.unique(feat.word_key, return_inverse=True)
    unames = wsp.decode(uk.cpu().numpy())
    th, ph, didx, widx = C.one_sided_index(tables, feat.ip_names, feat.ip, unames, inv, device, ip_map=ip_map)
    K = tables.K
    if cfg.strict and K != 20:
        raise ValueError("compat=strict scores over exactly 20 topics (dns_post_lda.scala:316)")
    model = S.build_model(tables, th, ph, S.default_value("dns", K, cfg.strict), device)
    sc, _, key, flag, votes = S.score_votes(model, didx, widx, None, None, cfg.tol)
    # --tail-tol: the events are flagged and ranked by their tail p-value; the files' score columns stay
    tr = C.tail_keys(cfg, model, (didx,), (widx,), log=log) if cfg.tail_tol is not None else None
    ranked = C.rank_results(cfg, key, flag) if tr is None else C.rank_results(cfg, tr.key, tr.flag)
    H = feat.host

    def row_cols(order):
        """The 16 columns of the given queries, in that order: their 8 input columns, dictionary-encoded by
        Arrow on a thread each (its kernels release the GIL), then the features, the word and the score."""
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(len(FD.COLUMNS)) as ex:
            enc = list(ex.map(lambda c: tab.take_encoded(c, order), FD.COLUMNS))
        o_t = torch.from_numpy(order).to(sc.device)
        return [("dict", names, ids) for ids, names in enc] + [
            ("dict", H["domains"], H["domain_id"][order]),
            ("dict", H["subdomains"], H["subdomain_id"][order]),
            ("int", H["subdomain_length"][order].astype(np.int64)),
            ("int", H["num_periods"][order].astype(np.int64)),
            ("java", H["entropy"][order]),
            ("int", H["top_domain"][order].astype(np.int64)),
            ("dict", unames, inv[torch.from_numpy(order).to(inv.device)].cpu().numpy().astype(np.int32)),
            ("java", sc[o_t].cpu().numpy()),
        ]
    return C.write_results(cfg, tables, "queries", ranked, key, row_cols, int(feat.word_key.numel()),
                           (didx, sc, None, None), votes, log, ctx=ctx,
                           explain=C.ExplainInput(model, (widx,), ((feat.ip_names, feat.ip),), ((-2, -1),)),
                           tail_rank=tr)


def synthetic_dns_corpus(events: int = 2_000_000, seed: int = 0, device=None, strict: bool = True, threads: int = 8,
                         return_names: bool = False, n_names: int = None, n_clients: int = None):
    """Synthetic DNS day -> featurized (dns_pre_lda semantics) -> lda-c corpus: the bench / test input path.

    Name and client populations grow with the day's size (a 2M-query day: 200k names, 50k clients)."""
    import shutil
    import tempfile
    import time
    from ..synth.dns import generate_dns_day
    device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
    n_names = n_names or max(20_000, events // 10)
    n_clients = n_clients or max(5_000, events // 40)
    tmp = tempfile.mkdtemp(prefix="oni_dns_")
    try:
        t0 = time.perf_counter()
        gen = generate_dns_day(os.path.join(tmp, "in/"), events=events, seed=seed, n_names=n_names,
                               n_clients=n_clients, with_edge_rows=False)
        t1 = time.perf_counter()
        tab = FD.load_dns(gen["dns_path"], None, 1000, strict=strict)
        top = FD.load_top_domains(gen["top1m"])
        t2 = time.perf_counter()
        feat = FD.featurize(tab, device, top, threads=threads)
        wsp = FD.DnsWordSpace(feat.cuts, feat.qpairs)
        dwc = count_pairs(feat.ip, feat.word_key, feat.weight)
        built = lda_pre(dwc)
        if device.type == "cuda":
            torch.cuda.synchronize()
        t3 = time.perf_counter()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    info = dict(events=events, synth_s=round(t1 - t0, 3), ingest_s=round(t2 - t1, 3),
                featurize_corpus_s=round(t3 - t2, 3))
    if return_names:
        return built.corpus, info, wsp.decode(built.word_keys)
    return built.corpus, info
