"""The stage sequence of the one-process pipelines (flow, dns, proxy): load -> <type>_pre -> lda_pre -> [holdout] ->
lda -> lda_post -> <type>_post.  A pipeline supplies a ``PipelineSpec`` (what it reads, how it featurizes, how it
scores); ``run_stages`` owns the rest: the runner and its resume rules, the corpus files, the lda stage, the
model export, the ensemble, the scoring stage's summary and the deferred writers.  Imports no feature module."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Callable, List, Optional

import torch

from ..corpus.builder import BuiltCorpus, DocWordCounts, lda_pre
from . import common as C
from .runner import StageRunner


@dataclass
class Pre:
    """What a ``<type>_pre`` stage hands on."""
    dwc: DocWordCounts
    ip_names: List[str]                   # name of every ip dictionary id (documents are a subset)
    decode: Callable                      # word keys -> word names
    keep: object = None                   # what the scoring stage reuses when it runs in the same process
    fields: Optional[list] = None         # the word key's fields (``WordSpace.fields()``), for --explain
    built: Optional[BuiltCorpus] = None   # set by lda_pre
    exported: bool = False                # lda_post ran in this process: the tables' rows are ``built``'s


@dataclass
class PipelineSpec:
    name: str              # stage-name prefix: flow, dns, proxy
    load: Callable         # (cfg, res, summary, log) -> inputs; fills the load record and summary["input"]
    pre: Callable          # (cfg, inputs, device, res, log) -> Pre
    post: Callable         # (cfg, inputs, tables, device, log, pre or None) -> the score_* result
    # lda_post writes its files on a thread under the scoring stage from C.DEFER_POST_VALUES values (flow)
    defer_post: bool = False


def lda_stage(R, cfg, corpus, device, log, summary, dist=None, local_shard=False, doc_offset=0, then=None):
    """The lda stage of every pipeline, one process or sharded; ``then(corpus, summary)`` runs inside it."""
    with R.stage("lda") as res:
        lres = C.run_lda(cfg, corpus, dist=dist, device=device, log=log, local_shard=local_shard,
                         doc_offset=doc_offset)
        res["_defer"] = lres.close_files   # LAG / final model files: written while later stages run
        timing = getattr(lres, "timing", {})
        res.update(timing)
        res.update(em_iterations=lres.em_iterations, likelihood=lres.likelihoods[-1][0] if lres.likelihoods else 0.0,
                   alpha=lres.alpha)
        m = lres.engine.metrics(lres.seconds, lres.em_iterations)
        scalars = {k: v for k, v in m.items() if not isinstance(v, list)}
        res.update(scalars)
        R.emit(dict(stage="lda_detail", var_iter_hist=m["var_iter_hist"], **scalars))
        summary["lda"] = dict(em_iterations=lres.em_iterations, timing=timing, seconds=lres.seconds, alpha=lres.alpha,
                              likelihood=lres.likelihoods[-1][0] if lres.likelihoods else None)
        if then is not None:
            then(corpus, summary)
    return lres


def _write_lda_pre_files(lpath, built, doc_names, word_names, dwc_h, ip_names, fields=None):
    if dwc_h is not None:
        from ..corpus.builder import write_doc_wc
        write_doc_wc(os.path.join(lpath, "doc_wc.dat"), dwc_h, ip_names, C.vocab_lookup(built.word_keys, word_names))
    C.write_corpus_files(lpath, built, doc_names, word_names)
    if fields is not None:      # --explain: a resumed scoring stage reads the keys from here
        C.save_word_fields(lpath, built.word_keys, fields)


def run_stages(cfg, spec: PipelineSpec, device=None, log=print) -> dict:
    device = torch.device(device or ("cuda" if torch.cuda.is_available() else "cpu"))
    R = StageRunner(cfg.lpath, resume=cfg.resume, log=log,
                    sync=(torch.cuda.synchronize if device.type == "cuda" else None))
    pre_stage, post_stage = spec.name + "_pre", spec.name + "_post"
    summary = {}
    inputs = pre = corpus = doc_names = word_names = None
    need_pre = not (R.done("lda_pre") and R.done(pre_stage))
    if cfg.explain and not need_pre:
        # a resumed scoring stage explains from the keys lda_pre wrote: refused here, before any stage runs and
        # before a marker is touched
        from ..config import WORD_FIELDS
        path = os.path.join(cfg.lpath, WORD_FIELDS)
        if not os.path.exists(path):
            raise ValueError(f"--resume --explain: {path} is missing (lda_pre ran without --explain); "
                             "run again from scratch with --explain")
    hold = C.Holdout(cfg, R, device, log)                  # --holdout; inert without it.  Ahead of the ensemble: a
    ens = C.Ensemble(cfg, R, post_stage, device, log)      # resumed --holdout-select has set cfg.topics by now
    if need_pre or not R.done(post_stage):
        with R.stage("load") as res:
            inputs = spec.load(cfg, res, summary, log)
    if need_pre:
        with R.stage(pre_stage) as res:
            pre = spec.pre(cfg, inputs, device, res, log)
        with R.stage("lda_pre") as res:
            built = pre.built = lda_pre(pre.dwc)
            corpus = built.corpus
            doc_names = [pre.ip_names[i] for i in built.doc_keys.tolist()]
            word_names = pre.decode(built.word_keys)
            # host copies here, not on the writer thread (DocWordCounts.to_host)
            dwc_h = pre.dwc.to_host() if cfg.write_doc_wc else None
            # the text files are the stage contract, not an input of the in-memory lda stage: written on a
            # thread while the GPU runs EM; the lda_pre marker waits for them (finish_deferred)
            files = (cfg.lpath, built, doc_names, word_names, dwc_h, pre.ip_names,
                     pre.fields if cfg.explain else None)
            res["_defer"] = C.background(lambda: _write_lda_pre_files(*files), "oni-lda-pre-writer")
            size = dict(docs=corpus.num_docs, terms=corpus.num_terms, nnz=corpus.nnz)
            res.update(size)
            summary["corpus"] = size
    else:
        R.skip(pre_stage)
        R.skip("lda_pre")

    hold.stage(corpus, summary, ens)      # --holdout: between lda_pre and lda; --holdout-select sets cfg.topics
    gamma = log_beta = None
    if not R.done("lda"):
        if corpus is None:
            corpus, doc_names, word_names = C.load_corpus_files(cfg.lpath)
        # the lda marker is written once every ensemble member is done
        lres = lda_stage(R, cfg, corpus, device, log, summary, then=ens.lda_ran)
        gamma, log_beta = lres.gamma, lres.log_beta
    else:
        R.skip("lda")
        ens.lda_skipped(corpus, summary)     # member 0 is complete: the members that are not
    try:
        if not R.done("lda_post"):
            if doc_names is None:
                _, doc_names, word_names = C.load_corpus_files(cfg.lpath)
            if gamma is None:
                from ..models.lda.estimate import load_final
                gamma, log_beta = load_final(cfg.lpath)
            with R.stage("lda_post") as res:
                # deferred text: measured no e2e gain on the 1-day tables (tuning log); on from
                # DEFER_POST_VALUES (2^26) values, where formatting ~1 G values (config 5) overlaps scoring
                if spec.defer_post and (len(doc_names) + len(word_names)) * int(gamma.shape[1]) >= C.DEFER_POST_VALUES:
                    # the result files are written on a thread while the scoring stage runs (its tables are
                    # the text round trip of the same values); the lda_post marker waits for them
                    from ..export import lda_post as LP
                    th, ph, wn, res["_defer"] = LP.export_deferred(
                        doc_names, gamma, word_names, log_beta, os.path.join(cfg.lpath, "doc_results.csv"),
                        os.path.join(cfg.lpath, "word_results.csv"), strict=cfg.strict)
                    tables = C.ModelTables(list(doc_names), th, wn, ph)
                else:
                    tables = C.run_export(cfg, doc_names, gamma, word_names, log_beta, read_back=True)
                if pre is not None:
                    pre.exported = True
                ens.exported(tables, doc_names, word_names)
        else:
            R.skip("lda_post")
            tables = C.load_model_tables(cfg.lpath)
            ens.loaded(tables)

        if not R.done(post_stage):
            with R.stage(post_stage) as res:
                if cfg.explain:      # the keys of the φ rows: this process's vocabulary, or what lda_pre wrote
                    tables.word_fields = ((pre.built.word_keys, pre.fields) if pre is not None
                                          else C.load_word_fields(cfg.lpath))
                res.update(spec.post(cfg, inputs, tables, device, log, pre))
                summary["scored"] = res.get("flagged")
                summary["below_tol"] = res.get("below_tol")
                if cfg.host_report:
                    summary["hosts"], summary["host_sides_skipped"] = res.get("hosts"), res.get("host_sides_skipped")
                ens.scored(res, summary)
                if cfg.explain:
                    why = {k: res[k] for k in ("explain_fields", "explain_why_hist", "explain_max_group")}
                    summary.update(why)
                    R.emit(dict(stage=post_stage + "_detail", **why))
                if cfg.expect:
                    exp = {k: res[k] for k in ("expect_fields", "expect_modal_hist", "expect_pairs",
                                               "expect_member_dots", "expect_path")}
                    summary.update(exp)
                    R.emit(dict(stage=post_stage + "_detail", **exp))
                if cfg.tail:
                    tail = {k: res[k] for k in ("tail_words", "tail_pairs", "tail_hist", "tail_total_range")}
                    if cfg.tail_tol is not None:      # flagged and ranked by the tail: what that took
                        tail.update({k: res[k] for k in ("tail_tol", "tail_rank_pairs", "tail_rank_docs",
                                                         "tail_rank_path", "tail_sides_skipped")})
                    summary.update(tail)
                    R.emit(dict(stage=post_stage + "_detail", **tail))
                if cfg.peers:
                    peers = {k: res[k] for k in ("peers", "peer_hosts", "peer_candidates", "peer_path",
                                                 "peer_identical", "peer_lift_hist")}
                    summary.update(peers)
                    R.emit(dict(stage=post_stage + "_detail", **peers))
                if cfg.topic_report:
                    topics = {k: res[k] for k in C.TOPIC_REPORT_KEYS}
                    summary.update(topics)
                    R.emit(dict(stage=post_stage + "_detail", **topics))
                if cfg.topic_match:
                    matched = {k: res[k] for k in C.TOPIC_MATCH_KEYS}
                    summary.update(matched)
                    R.emit(dict(stage=post_stage + "_detail", **matched))
        else:
            R.skip(post_stage)
    except BaseException:
        R.finish_deferred(suppress=True)
        raise
    R.finish_deferred()
    summary["stage_seconds"] = dict(R.times)
    return summary
