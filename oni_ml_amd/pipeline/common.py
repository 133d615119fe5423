"""Shared by the flow, DNS and proxy pipelines: corpus files, LDA, model export and reload, the ensemble, the
scorers' tails (the stage sequence itself: pipeline/driver.py)."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from ..corpus.builder import BuiltCorpus, lda_pre
from ..corpus.csr import Corpus
from ..export import lda_post
from ..io import ldac
from ..models.lda.estimate import estimate


@dataclass
class ModelTables:
    """What the scorers consume: θ / φ and their row names (as written to the result files)."""
    doc_names: List[str]
    theta: np.ndarray          # [D, K]
    word_names: List[str]      # keys as written (strict: truncated to 20 bytes)
    phi: np.ndarray            # [V, K]
    # set when the tables were built in this process from its own vocabulary (compat=fixed): the word
    # key of every φ row and the key space that encodes them -- the flow scorer then maps event keys
    # to rows without decoding or hashing millions of word names
    word_keys: Optional[np.ndarray] = None
    key_space: Optional[object] = None
    # --ensemble: (θ, φ) of the members 1 .. R-1, rows as in theta / phi (one corpus, one set of names)
    members: Optional[list] = None
    # --explain: (int64 key of every φ row, the key's fields as ``WordSpace.fields()`` returns them)
    word_fields: Optional[tuple] = None

    def doc_index(self) -> dict:
        return {n: i for i, n in enumerate(self.doc_names)}      # later duplicates win (collectAsMap)

    def word_index(self) -> dict:
        return {n: i for i, n in enumerate(self.word_names)}

    @property
    def K(self) -> int:
        return int(self.theta.shape[1])

    def word_rows(self, names: List[str]) -> np.ndarray:
        """φ row of every word name (-1: not in word_results)."""
        idx = self.word_index()
        return np.fromiter((idx.get(n, -1) for n in names), dtype=np.int64, count=len(names))

    def compact(self, doc_rows: np.ndarray, word_rows: np.ndarray):
        """(θ, φ, doc rows, word rows) the score kernel indexes: the whole tables, rows unchanged."""
        return self.theta, self.phi, np.asarray(doc_rows, np.int64), np.asarray(word_rows, np.int64)


@dataclass
class ShardedTables:
    """The scorers' model in the row-sharded pipeline, nothing replicated: θ rows stay with the rank of
    their documents (global rows [doc_starts[r], doc_starts[r + 1])), φ rows with the rank of their
    vocabulary slice; the word name -> φ row map is hash-partitioned (``shardio.DistDict``, later rows
    win as in ``collectAsMap``).  A rank fetches only the θ / φ rows its own events reference
    (``shardio.fetch_rows``) -- the reference broadcasts the whole model to every executor
    (flow_post_lda.scala:112-123).  ``word_rows`` and ``compact`` are collective."""
    ctx: object
    theta: np.ndarray          # this rank's θ rows
    doc_starts: List[int]
    phi: np.ndarray            # this rank's φ rows (vocabulary slice)
    word_starts: List[int]
    words: object              # shardio.DistDict: word name as written -> global φ row

    @property
    def K(self) -> int:
        return int(self.theta.shape[1])

    def word_rows(self, names: List[str]) -> np.ndarray:
        return self.words.lookup(names)

    def compact(self, doc_rows: np.ndarray, word_rows: np.ndarray):
        """(θ rows, φ rows, local doc rows, local word rows): the distinct rows the given global rows
        reference, fetched from their owners, and the given rows renumbered into them (-1 kept)."""
        from ..parallel import shardio as SIO
        out = []
        for rows, tab, starts in ((doc_rows, self.theta, self.doc_starts), (word_rows, self.phi, self.word_starts)):
            rows = np.asarray(rows, np.int64)
            ok = rows >= 0
            u, inv = np.unique(rows[ok], return_inverse=True)
            got = SIO.fetch_rows(self.ctx, tab, starts, u)
            loc = np.full(rows.size, -1, np.int64)
            loc[ok] = inv
            out.append((got, loc))
        (th, dl), (ph, wl) = out
        return th, ph, dl, wl


def write_corpus_files(lpath: str, built: BuiltCorpus, doc_names: List[str], word_names: List[str]):
    ldac.write_words_dat(os.path.join(lpath, "words.dat"), word_names)
    ldac.write_doc_dat(os.path.join(lpath, "doc.dat"), doc_names)
    ldac.write_model_dat(os.path.join(lpath, "model.dat"), built.corpus)


def load_corpus_files(lpath: str):
    c = ldac.read_model_dat(os.path.join(lpath, "model.dat"))
    docs = ldac.read_index_file(os.path.join(lpath, "doc.dat"))
    words = ldac.read_index_file(os.path.join(lpath, "words.dat"))
    c.num_terms = max(c.num_terms, len(words))
    return c, docs, words


RANK_FILES_MAX_VALUES = 1 << 26
# lda_post writes its result files on a thread while the scoring stage runs from this many doc + word values
DEFER_POST_VALUES = 1 << 26


def run_lda(cfg, corpus: Corpus, dist=None, device=None, log=print, local_shard: bool = False, doc_offset: int = 0):
    outdir = cfg.lpath
    settings_path = os.path.join(outdir, "settings.txt")
    if dist is None or dist.rank == 0:
        ldac.write_settings(settings_path, cfg.settings)
    rank_files = cfg.rank_gamma
    if rank_files is None:
        # oni-lda-c's per-worker <rank>.beta / <rank>.gamma temporaries (README.md:121): on for multi-rank
        # runs while a worker's K x V beta text stays small (<= RANK_FILES_MAX_VALUES values; BASELINE
        # config 5's would be ~7 GB per rank); --rank-gamma forces them
        rank_files = dist is not None and dist.active and cfg.topics * corpus.num_terms <= RANK_FILES_MAX_VALUES
    return estimate(corpus, cfg.topics, cfg.alpha, cfg.settings, cfg.start, outdir, backend=cfg.backend,
                    device=device, dist=dist, seed=cfg.seed, resume=cfg.resume,
                    write_word_assignments=cfg.word_assignments,
                    write_rank_gamma=rank_files,
                    verbose=cfg.verbose, fault_at_iteration=cfg.extra.get("fault_at_iteration"),
                    defer_files=True, local_shard=local_shard, doc_offset=doc_offset)


def run_export(cfg, doc_names, gamma, word_names, log_beta, read_back: bool = False) -> ModelTables:
    """``read_back``: the tables as the scorers parse the files (what ``strict_tables`` computes, but
    from the writer's own formatting pass instead of a second one)."""
    th, ph, wn = lda_post.export(doc_names, gamma, word_names, log_beta,
                                 os.path.join(cfg.lpath, "doc_results.csv"),
                                 os.path.join(cfg.lpath, "word_results.csv"), strict=cfg.strict, read_back=read_back)
    return ModelTables(list(doc_names), th, wn, ph)


def load_model_tables(lpath: str) -> ModelTables:
    """Read doc_results.csv / word_results.csv exactly as the Scala scorers do."""
    dn, th = lda_post.read_results(os.path.join(lpath, "doc_results.csv"))
    wn, ph = lda_post.read_results(os.path.join(lpath, "word_results.csv"))
    return ModelTables(dn, th, wn, ph)


# ------------------------------------------------------------------ --ensemble
# Member 0 is the run without --ensemble, in LPATH.  Member r >= 1 is the same corpus fitted from the seed
# cfg.seed + r into <LPATH>/ensemble/m<r>/, a model directory of its own (final.*, likelihood.dat,
# final_model.npz, then doc_results.csv / word_results.csv) with the completion marker MEMBER_DONE.
MEMBER_DONE = ".done"


def member_dir(lpath: str, r: int) -> str:
    return os.path.join(lpath, "ensemble", f"m{r}")


def member_fit_key(cfg, r: int) -> dict:
    """What a member's marker must agree with for the member to be kept on a resume."""
    return dict(member=r, seed=cfg.seed + r, topics=cfg.topics, alpha_init=cfg.alpha, start=cfg.start,
                compat=cfg.compat)


def member_done(cfg, r: int) -> bool:
    """The member has its marker, and the marker is of this run's seed, topic count, alpha, start and compat mode
    (a resume with another --seed or --topics fits the member again instead of mixing two runs)."""
    path = os.path.join(member_dir(cfg.lpath, r), MEMBER_DONE)
    if not os.path.exists(path):
        return False
    try:
        m = load_json(path)
    except ValueError:
        return False
    return all(m.get(k) == v for k, v in member_fit_key(cfg, r).items())


def members_to_fit(cfg) -> List[int]:
    """The members r >= 1 this run has to fit: all of them, or on a resume those that are not ``member_done``."""
    return [r for r in range(1, cfg.ensemble) if not (cfg.resume and member_done(cfg, r))]


def run_lda_members(cfg, corpus: Corpus, fit: List[int], device=None, log=print) -> dict:
    """Fit the members ``fit`` one after the other, each from scratch (they are deterministic by seed): only the
    000 and final model files (lag 0), no word assignments.  Returns {r: (gamma, log_beta)}."""
    import dataclasses
    import shutil
    out = {}
    settings = dataclasses.replace(cfg.settings, lag=0)
    pending = []      # a member's model files are formatted on its writer threads while the next member fits
    try:
        for r in fit:
            mdir = member_dir(cfg.lpath, r)
            shutil.rmtree(mdir, ignore_errors=True)
            res = estimate(corpus, cfg.topics, cfg.alpha, settings, cfg.start, mdir, backend=cfg.backend,
                           device=device, seed=cfg.seed + r, resume=False, write_word_assignments=False,
                           verbose=False, defer_files=True)
            stats = dict(member_fit_key(cfg, r), em_iterations=res.em_iterations,
                         likelihood=res.likelihoods[-1][0] if res.likelihoods else None, alpha=res.alpha,
                         seconds=res.seconds)
            pending.append((mdir, stats, res.close_files))
            out[r] = (res.gamma, res.log_beta)
            res.engine = None
            log(f"lda: ensemble member {r} (seed {cfg.seed + r}): {stats['em_iterations']} EM iterations, "
                f"likelihood {stats['likelihood']}, {stats['seconds']:.3f}s")
    finally:
        err = None
        for mdir, stats, close in pending:      # the marker only once the member's files are complete
            try:
                close()
                save_json(os.path.join(mdir, MEMBER_DONE), stats)
            except Exception as e:  # noqa: BLE001 -- the other members' writers are still drained
                err = err or e
        if err is not None:
            raise err
    return out


def report_members(cfg, summary: dict):
    """Per member the EM iterations, final likelihood, alpha and seconds, into ``summary["lda"]["members"]`` and
    the "ensemble" entry of LPATH's lda_stats.json (member 0: this run's lda stage, or what an earlier run
    recorded there)."""
    path = os.path.join(cfg.lpath, "lda_stats.json")
    stats = load_json(path) if os.path.exists(path) else {}
    lda = summary.get("lda")
    if lda is not None:
        m0 = dict(member=0, seed=cfg.seed, em_iterations=lda.get("em_iterations"), likelihood=lda.get("likelihood"),
                  alpha=lda.get("alpha"), seconds=lda.get("seconds"))
    elif stats.get("ensemble"):
        m0 = stats["ensemble"][0]
    else:      # a plain run resumed with --ensemble: what its lda stage left in LPATH
        lik = None
        lp = os.path.join(cfg.lpath, "likelihood.dat")
        if os.path.exists(lp):
            with open(lp) as f:
                lines = f.read().split("\n")
            lines = [x for x in lines if x.strip()]
            lik = float(lines[-1].split()[0]) if lines else None
        m0 = dict(member=0, seed=cfg.seed, em_iterations=stats.get("em_iterations"), likelihood=lik,
                  alpha=stats.get("alpha"), seconds=stats.get("seconds"))
    keep = ("member", "seed", "em_iterations", "likelihood", "alpha", "seconds")
    members = [m0] + [{k: m.get(k) for k in keep}
                      for m in (load_json(os.path.join(member_dir(cfg.lpath, r), MEMBER_DONE))
                                for r in range(1, cfg.ensemble))]
    summary.setdefault("lda", {})["members"] = members
    if stats:
        stats["ensemble"] = members
        with open(path + ".tmp", "w") as f:
            json.dump(stats, f)
        os.replace(path + ".tmp", path)      # never a torn lda_stats.json


def export_members(cfg, doc_names, word_names, fitted: dict) -> list:
    """lda_post for the members 1 .. R-1: doc_results.csv / word_results.csv into each member directory, through
    the text round trip of ``run_export`` (``fitted``: what ``run_lda_members`` returned; a member fitted by an
    earlier run is read from its directory).  Returns their (θ, φ)."""
    from concurrent.futures import ThreadPoolExecutor

    from ..models.lda.estimate import load_final

    def one(r):
        mdir = member_dir(cfg.lpath, r)
        gamma, log_beta = fitted[r] if r in fitted else load_final(mdir)
        th, ph, _ = lda_post.export(doc_names, gamma, word_names, log_beta, os.path.join(mdir, "doc_results.csv"),
                                    os.path.join(mdir, "word_results.csv"), strict=cfg.strict, read_back=True)
        return th, ph
    # every member writes its own two files: a few at a time (the native formatters release the GIL)
    with ThreadPoolExecutor(max(1, min(4, cfg.ensemble - 1))) as ex:
        return list(ex.map(one, range(1, cfg.ensemble)))


def load_members(cfg) -> list:
    """(θ, φ) of the members 1 .. R-1 from their result files (a resumed run)."""
    out = []
    for r in range(1, cfg.ensemble):
        t = load_model_tables(member_dir(cfg.lpath, r))
        out.append((t.theta, t.phi))
    return out


def votes_hist(votes, order, R: int) -> dict:
    """``{"ensemble_votes_hist": h}``, h[v] the number of written rows (``order``) that v members flagged on their
    own; ``{}`` without votes (one model)."""
    if votes is None:
        return {}
    v = votes.cpu().numpy()[np.asarray(order, np.int64)]
    return dict(ensemble_votes_hist=np.bincount(v, minlength=R + 1).astype(np.int64).tolist())


class Ensemble:
    """The --ensemble part of a one-process pipeline (flow, dns, proxy alike); with ``cfg.ensemble == 1`` every
    method does nothing.  ``post``: the name of the pipeline's scoring stage."""

    def __init__(self, cfg, runner, post: str, device=None, log=print):
        import shutil
        self.cfg, self.R, self.post, self.device, self.log = cfg, runner, post, device, log
        self.on = cfg.ensemble > 1
        if not cfg.resume:      # a fresh run fits every member: nothing of an earlier, maybe larger, ensemble stays
            shutil.rmtree(os.path.join(cfg.lpath, "ensemble"), ignore_errors=True)
        self.fit = members_to_fit(cfg)      # the members 1 .. R-1 still to fit
        self.fitted = {}                    # {r: (gamma, log_beta)} of the members fitted in this process
        if self.fit and cfg.resume:         # a member fitted again: its tables and the scores are made again
            runner.invalidate("lda_post", post)

    def lda_ran(self, corpus: Corpus, summary: dict):
        """Inside the lda stage, after member 0: the other members, so the lda marker means every member."""
        if self.on:
            self.fitted = run_lda_members(self.cfg, corpus, self.fit, device=self.device, log=self.log)
            report_members(self.cfg, summary)

    def lda_skipped(self, corpus: Optional[Corpus], summary: dict):
        """The lda stage is complete (member 0 is): fit the members that are not, timed but without a marker of
        their own (each member directory has one)."""
        if self.fit:
            if corpus is None:
                corpus = load_corpus_files(self.cfg.lpath)[0]
            with self.R.stage("lda_members", mark=False):
                self.fitted = run_lda_members(self.cfg, corpus, self.fit, device=self.device, log=self.log)
        if self.on:
            report_members(self.cfg, summary)

    def exported(self, tables: ModelTables, doc_names, word_names):
        """Inside the lda_post stage: the members' result files, and their tables beside member 0's."""
        if self.on:
            tables.members = export_members(self.cfg, doc_names, word_names, self.fitted)

    def loaded(self, tables: ModelTables):
        """The lda_post stage is complete: the members' tables from their result files."""
        if self.on:
            tables.members = load_members(self.cfg)

    def scored(self, res: dict, summary: dict):
        """Inside the scoring stage: ensemble_votes_hist into the summary and the metrics."""
        if "ensemble_votes_hist" in res:
            summary["ensemble_votes_hist"] = res["ensemble_votes_hist"]
            self.R.emit(dict(stage=self.post + "_detail", ensemble_votes_hist=res["ensemble_votes_hist"]))


# ------------------------------------------------------------------- --holdout
# <LPATH>/holdout/: holdout.csv (a header and one line per evaluated K), holdout.json (the records, the split's
# tallies, the selection and the key they were made under) and k<K>/, the model directory of K's training fit.
HOLDOUT_CSV = ("topics", "em_iterations", "alpha", "train_likelihood", "heldout_tokens", "unseen_tokens",
               "evaluated_tokens", "split_documents", "loglik", "loglik_per_token", "perplexity")


def holdout_dir(lpath: str) -> str:
    from ..config import HOLDOUT_DIR
    return os.path.join(lpath, HOLDOUT_DIR)


def holdout_key(cfg, size: dict) -> dict:
    """What a holdout record was made under: a resume under another key is refused."""
    return dict(fraction=float(cfg.holdout), topics=cfg.holdout_list(), seed=cfg.seed, alpha_init=cfg.alpha,
                start=cfg.start, compat=cfg.compat, docs=size.get("docs"), terms=size.get("terms"), nnz=size.get("nnz"))


def run_holdout(cfg, corpus: Corpus, device=None, log=print) -> dict:
    """One split from ``cfg.seed``, then per K of the list, in list order: the training fit into
    ``<LPATH>/holdout/k<K>/`` (only the 000 and final model files, no word assignments) and its held-out record.
    A fit's model files are formatted on its writer threads while the next K fits.  Writes holdout.csv and
    holdout.json; returns the json's content."""
    import dataclasses
    import shutil
    import time

    from ..models.lda import holdout as HO
    hdir = holdout_dir(cfg.lpath)
    shutil.rmtree(hdir, ignore_errors=True)
    os.makedirs(hdir)
    t0 = time.perf_counter()
    train, t = HO.split(corpus, cfg.holdout, cfg.seed, device)
    tallies = HO.split_tallies(corpus, train, t)
    split_s = time.perf_counter() - t0
    settings = dataclasses.replace(cfg.settings, lag=0)
    records, pending = [], []
    try:
        for K in cfg.holdout_list():
            res = estimate(train, K, cfg.alpha, settings, cfg.start, os.path.join(hdir, f"k{K}"), backend=cfg.backend,
                           device=device, seed=cfg.seed, resume=False, write_word_assignments=False, verbose=False,
                           defer_files=True)
            pending.append(res.close_files)
            fit = dict(topics=K, em_iterations=res.em_iterations, alpha=res.alpha, seconds=res.seconds,
                       train_likelihood=res.likelihoods[-1][0] if res.likelihoods else None)
            rec = HO.evaluate(corpus, train, t, res.gamma, res.log_beta, device, fit=fit)
            res.engine = None
            records.append(rec)
            log(f"holdout: K = {K}: perplexity {rec['perplexity']} over {rec['evaluated_tokens']} held-out tokens "
                f"({rec['unseen_tokens']} more on words unseen in training), {rec['em_iterations']} EM iterations, "
                f"{rec['seconds']:.3f}s")
    finally:
        err = None
        for close in pending:
            try:
                close()
            except Exception as e:  # noqa: BLE001 -- the other fits' writers are still drained
                err = err or e
        if err is not None:
            raise err
    fmt = lambda v: "" if v is None else repr(v)      # noqa: E731 -- a float's repr reads back to the same bits
    with open(os.path.join(hdir, "holdout.csv"), "w") as f:
        f.write(",".join(HOLDOUT_CSV) + "\n")
        for r in records:
            f.write(",".join(fmt(r[k]) for k in HOLDOUT_CSV) + "\n")
    size = dict(docs=corpus.num_docs, terms=corpus.num_terms, nnz=corpus.nnz)
    out = dict(key=holdout_key(cfg, size), split=dict(tallies, seconds=split_s), records=records,
               selected=HO.select(records))
    save_json(os.path.join(hdir, "holdout.json"), out)
    return out


class Holdout:
    """The --holdout part of a one-process pipeline; with ``cfg.holdout == 0`` every method does nothing.  Made
    before any stage runs: a resume whose holdout stage is complete reads the record here -- a record made under
    another key is refused -- and under --holdout-select sets ``cfg.topics`` to its selection, so that everything
    after (the ensemble's member keys, the lda stage, the scorers) sees the selected K."""

    def __init__(self, cfg, runner, device=None, log=print):
        import shutil
        self.cfg, self.R, self.device, self.log = cfg, runner, device, log
        self.on = cfg.holdout > 0
        self.record = None
        if not cfg.resume:
            shutil.rmtree(holdout_dir(cfg.lpath), ignore_errors=True)
        if not (self.on and cfg.resume):
            return
        if runner.done("holdout") and not runner.done("lda_pre"):
            runner.invalidate("holdout")      # the corpus is made again: so is its split
        if runner.done("holdout"):
            path = os.path.join(holdout_dir(cfg.lpath), "holdout.json")
            try:
                rec = load_json(path)
            except (OSError, ValueError):
                raise ValueError(f"--resume --holdout: the holdout stage is complete but {path} cannot be read; "
                                 "run again from scratch") from None
            key = holdout_key(cfg, runner.info("lda_pre"))
            if rec.get("key") != json.loads(json.dumps(key)):
                raise ValueError(f"--resume --holdout: {path} was made under {rec.get('key')}, this run asks for "
                                 f"{key}; run again from scratch")
            self.record = rec
            self._select()
        elif cfg.holdout_select and runner.done("lda"):
            raise ValueError("--resume --holdout-select: the lda stage is complete but the holdout stage is not, so "
                             "the model in LPATH was not fitted with a selected topic count; run again from scratch")

    def _select(self):
        if self.cfg.holdout_select:
            k = self.record.get("selected")
            if k is None:
                raise ValueError("--holdout-select: no topic count was evaluated (no held-out token on a word seen in "
                                 "training)")
            self.cfg.topics = int(k)

    def stage(self, corpus: Optional[Corpus], summary: dict, ens: Optional["Ensemble"] = None):
        """Between lda_pre and lda: the holdout stage, or on a resume its record."""
        if not self.on:
            return
        if self.record is None:
            if corpus is None:
                corpus = load_corpus_files(self.cfg.lpath)[0]
            with self.R.stage("holdout") as res:
                self.record = run_holdout(self.cfg, corpus, device=self.device, log=self.log)
                res.update(selected=self.record["selected"], fits=len(self.record["records"]),
                           heldout_tokens=self.record["split"]["heldout_tokens"])
                self.R.emit(dict(stage="holdout_detail", **self.record))
            before = self.cfg.topics
            self._select()
            if ens is not None and ens.on and self.cfg.resume and self.cfg.topics != before:
                ens.fit = members_to_fit(self.cfg)      # the members' markers name their topic count
        else:
            self.R.skip("holdout")
        recs = self.record["records"]
        summary["holdout"] = dict(fraction=float(self.cfg.holdout), topics=[r["topics"] for r in recs],
                                  perplexity=[r["perplexity"] for r in recs], selected=self.record["selected"],
                                  select=bool(self.cfg.holdout_select), **{k: self.record["split"][k] for k in
                                  ("heldout_tokens", "split_documents")},
                                  unseen_tokens=[r["unseen_tokens"] for r in recs],
                                  seconds=sum(r["seconds"] for r in recs) + self.record["split"]["seconds"])


def strict_tables(mt: ModelTables, strict: bool = True) -> ModelTables:
    """θ/φ as the scorers see them after the text hand-off (Python-2 str -> toDouble).

    Applied in both compat modes: the result files are the stage contract, so an
    in-memory run and a run resumed from the files score identically."""
    from ..ops import native
    n = native.lib()
    return ModelTables(mt.doc_names, n.roundtrip_py2(np.ascontiguousarray(mt.theta)), mt.word_names,
                       n.roundtrip_py2(np.ascontiguousarray(mt.phi)))


def background(fn, name: str = "oni-writer"):
    """Run ``fn`` on a thread (the native writers release the GIL); returns the join callable a stage
    puts in ``result["_defer"]``, which re-raises the thread's exception."""
    import threading
    box = {}

    def body():
        from ..ops import native
        from ..utils.sched import background_priority
        background_priority()
        native.background_thread_budget()   # leaves the GPU-driving thread CPUs within the quota
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 -- handed to the joiner
            box["err"] = e

    t = threading.Thread(target=body, name=name, daemon=True)
    t.start()

    def join():
        t.join()
        if "err" in box:
            raise box["err"]
    return join


def vocab_lookup(word_keys, word_names):
    """keys -> (names, index) through the built vocabulary (every doc_wc key is in it): a vectorized
    search instead of decoding the unique keys again -- a writer thread then holds the GIL only
    briefly while the lda stage drives the GPU."""
    wk = np.asarray(word_keys)
    srt = np.argsort(wk, kind="stable")
    sk = wk[srt]

    def lookup(keys):
        return word_names, srt[np.searchsorted(sk, np.asarray(keys))]
    return lookup


def doc_rows_of(doc_keys, n_keys: int) -> np.ndarray:
    """Doc row of every dictionary id (-1: not a document): the in-memory equivalent of looking the
    names up in doc_results.csv, when the documents are ``doc_keys`` in row order."""
    rows = np.full(int(n_keys), -1, np.int64)
    dk = np.asarray(doc_keys, np.int64)
    rows[dk] = np.arange(dk.size, dtype=np.int64)
    return rows


def flagged_text(written: int, below_tol: int, limit, what: str, tol) -> str:
    """The scorers' log line: the rows written, and with a MAXRESULTS limit also the count under TOL."""
    if limit is None:
        return f"{written} {what} with score < {tol}"
    return f"{written} of the {below_tol} {what} with score < {tol} (MAXRESULTS {limit})"


def write_host_report(cfg, tables: ModelTables, doc_a, score_a, doc_b, score_b, row_cols, sep: str = ",",
                      log=print) -> dict:
    """--host-report: ``<type>_hosts.csv`` next to the results file, one line per host with a side under TOL,
    ascending by the host's lowest score (``scorer.rank_hosts``; ``cfg.host_report`` hosts, -1: all of them):
    host, sides, sides under TOL, lowest score, for two-sided events ``src`` / ``dst`` (the side that scored
    it), then that event's row exactly as the results file writes it -- ``row_cols(rows)`` is the scorer's
    column list for the given event rows.  Folds every scored side of the day, whatever MAXRESULTS is.
    ``doc_*`` / ``score_*``: θ row (-1: none) and score of every event's side(s), on the scoring device."""
    from ..ops import native
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    D = len(tables.doc_names)
    ev, fl, ms, worst, skipped = S.host_summary(doc_a, score_a, doc_b, score_b, D, cfg.tol)
    hosts = S.rank_hosts(ms, fl, None if cfg.host_report < 0 else cfg.host_report)
    h_t = torch.from_numpy(hosts).to(ms.device)
    take = lambda t: SG.gather(t, h_t).cpu().numpy()      # noqa: E731
    side = take(worst)
    cols = [("dict", [tables.doc_names[d] for d in hosts.tolist()], np.arange(hosts.size, dtype=np.int32)),
            ("int", take(ev).astype(np.int64)), ("int", take(fl).astype(np.int64)), ("java", take(ms))]
    if doc_b is not None:
        cols.append(("dict", ["src", "dst"], (side & 1).astype(np.int32)))
    cols += row_cols((side >> 1).astype(np.int64))
    out = os.path.join(cfg.lpath, f"{cfg.dsource}_hosts.csv")
    native.lib().write_rows(out, None, cols, sep=sep, threads=cfg.threads, n=int(hosts.size))
    log(f"{cfg.dsource}_post: {hosts.size} hosts with a score < {cfg.tol} written to {out}")
    return dict(hosts=int(hosts.size), host_sides_skipped=int(skipped))


@dataclass
class ExplainInput:
    """What a scorer hands ``write_results`` for --explain and --tail, per side of an event (flow: source, destination):
    ``words`` the φ row of every event's side (-1: none), ``ips`` the (names, id of every event) of the side's
    document, ``cols`` the positions (word, score) of the side's columns in the scorer's ``row_cols`` list."""
    model: object
    words: tuple
    ips: tuple
    cols: tuple


def save_word_fields(lpath: str, word_keys, fields):
    """<LPATH>/word_fields.npz (lda_pre under --explain): the int64 word keys in φ-row order and the key's fields,
    so that a resumed scoring stage can explain too."""
    from ..config import WORD_FIELDS
    np.savez(os.path.join(lpath, WORD_FIELDS), keys=np.asarray(word_keys, np.int64),
             radix=np.asarray([r for _, r, _ in fields], np.int64), names=np.asarray([n for n, _, _ in fields]),
             explained=np.asarray([bool(e) for _, _, e in fields]))


def load_word_fields(lpath: str):
    """(keys int64 [V], fields) of ``save_word_fields``."""
    from ..config import WORD_FIELDS
    with np.load(os.path.join(lpath, WORD_FIELDS), allow_pickle=False) as z:
        fields = [(str(n), int(r), bool(e)) for n, r, e in zip(z["names"], z["radix"], z["explained"])]
        return z["keys"].astype(np.int64), fields


def write_explain(cfg, tables, order, key, sides, ex: ExplainInput, cols, sep: str = ",", log=print,
                  keep: Optional[dict] = None) -> dict:
    """--explain: ``<type>_explain.csv`` next to the results file, line i describing its line i (``order``: the
    written events; ``cols``: their ``row_cols``): the key score, then per side the document, the word, the side's
    score, ``why`` -- the explained field of the word with the lowest conditional probability c_f, empty when
    there is none -- and c_f of every explained field (empty for NaN).  c_f = s / m_f, m_f the side's score with
    the φ row replaced by the sum of the φ rows that agree with the word on every field but f
    (``scorer.field_groups``, ``scorer.explain_sides``).  Returns the summary entries.  ``keep`` (--expect): a dict
    that receives what ``write_expect`` goes on from -- the sides' rows, the distinct words and their groups -- so
    that the groups are computed once for both files."""
    from ..ops import native
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    if getattr(tables, "word_fields", None) is None:
        raise ValueError("--explain: the vocabulary's word keys are not known to the scoring stage")
    word_keys, fields = tables.word_fields
    names = [n for n, _, e in fields if e]
    F = len(names)
    dev = key.device
    n = int(order.size)
    o_t = torch.from_numpy(order).to(dev)
    n_sides = len(ex.words)
    doc = torch.cat([SG.gather(sides[2 * j], o_t).to(torch.int64) for j in range(n_sides)]) if n else \
        torch.zeros(0, dtype=torch.int64, device=dev)
    word = torch.cat([SG.gather(w, o_t).to(torch.int64) for w in ex.words]) if n else doc
    cond = np.full((n_sides * n, F), np.nan)
    why = np.full(n_sides * n, 255, np.uint8)
    largest = [0] * F      # per explained field the members of the largest group a written side refers to
    if n:
        rows, inv = SG.unique(word, return_inverse=True)
        none = int(rows[0] < 0) if rows.numel() else 0      # the -1 of the sides without a φ row sorts first
        rows = rows[none:]
        seg = S.field_segments(int(S.model_tables3(ex.model)[1].shape[0]),
                               torch.from_numpy(np.asarray(word_keys, np.int64)), fields, rows, dev)
        gsum, grow_u, sizes = S.field_groups(ex.model, None, fields, rows, segments=seg)
        if keep is not None:
            keep.update(doc=doc, word=word, rows=rows, seg=seg)
        if rows.numel():
            largest = sizes.max(0).values.cpu().tolist()
        if rows.numel():
            grow = torch.where((word >= 0).unsqueeze(1), SG.gather(grow_u, (inv - none).clamp_min(0)),
                               torch.full((1, 1), -1, dtype=torch.int64, device=dev))
        else:
            grow = torch.full((word.numel(), F), -1, dtype=torch.int64, device=dev)
        c_t, w_t = S.explain_sides(ex.model, gsum, doc, word, grow)
        cond, why = c_t.cpu().numpy(), w_t.cpu().numpy()
    out_cols = [("java", SG.gather(key, o_t).cpu().numpy())]
    for j in range(n_sides):
        ip_names, ip_ids = ex.ips[j]
        c, w = cond[j * n:(j + 1) * n], why[j * n:(j + 1) * n]
        ok = ~np.isnan(c)
        text = native.lib().java_double_array(np.ascontiguousarray(c[ok], np.float64))
        idx = np.full(c.shape, -1, np.int32)
        idx[ok] = np.arange(len(text), dtype=np.int32)
        out_cols += [("dict", ip_names, SG.gather(ip_ids, o_t).cpu().numpy().astype(np.int32)),
                     cols[ex.cols[j][0]], cols[ex.cols[j][1]],
                     ("dict", names, np.where(w == 255, -1, w.astype(np.int32)).astype(np.int32))]
        out_cols += [("dict", text, np.ascontiguousarray(idx[:, f])) for f in range(F)]
    out = os.path.join(cfg.lpath, f"{cfg.dsource}_explain.csv")
    native.lib().write_rows(out, None, out_cols, sep=sep, threads=cfg.threads, n=n)
    hist = np.bincount(np.where(why == 255, F, why), minlength=F + 1)
    log(f"{cfg.dsource}_post: {n_sides * n} sides explained in {out}")
    return dict(explain_fields=names, explain_why_hist=dict(zip(names + ["none"], hist.astype(np.int64).tolist())),
                explain_max_group=dict(zip(names, (int(x) for x in largest))))


def write_expect(cfg, tables, order, key, sides, ex: ExplainInput, cols, kept: dict, sep: str = ",",
                 log=print) -> dict:
    """--expect: ``<type>_expect.csv`` next to the results file, line i describing its line i (``order``: the written
    events; ``cols``: their ``row_cols``): the key score, then per side the document, the word, the side's score and
    per explained field ``expected_f``, ``lift_f`` and ``above_f``.  With N_f(w) the group of the side's word w --
    the vocabulary's words that agree with w on every field but f -- and p_v the side's score with the word v in
    place of w: ``expected_f`` is the word of N_f(w) with the greatest p_v, by the name the results file gives it
    (ties to the lowest φ row), ``lift_f`` = its p_v over the side's own score, one rounded division (>= 1; 1.0:
    the event has the host's usual value there), ``above_f`` the number of words of N_f(w) with p_v above the
    side's.  Cells are empty where there is no value.  The values depend on the pair (document, word) only: the
    distinct pairs of the written sides are evaluated (``scorer.expect_sides``) and gathered.  ``kept``: what
    ``write_explain`` left (the sides' rows and the groups).  Returns the summary entries."""
    from ..ops import native
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    _, fields = tables.word_fields
    names = [n for n, _, e in fields if e]
    F = len(names)
    dev = key.device
    n = int(order.size)
    o_t = torch.from_numpy(order).to(dev)
    n_sides = len(ex.words)
    V = int(S.model_tables3(ex.model)[1].shape[0])
    best = np.full((n_sides * n, F), -1, np.int64)
    above = np.full((n_sides * n, F), -1, np.int64)
    lift = np.full((n_sides * n, F), np.nan)
    pairs, dots = 0, 0
    path = "cpu" if dev.type != "cuda" else S.expect_form()
    if n and kept.get("rows") is not None and kept["rows"].numel():
        doc, word, rows, seg = kept["doc"], kept["word"], kept["rows"], kept["seg"]
        ok = word >= 0
        # a pair: (document or none, word); a side without a document takes the default vector, so it has values
        pk, inv = SG.unique(torch.where(ok, (doc + 1) * V + word, torch.full_like(doc, -1)), return_inverse=True)
        none = int(pk[0] < 0)      # the -1 of the sides without a φ row sorts first
        pk = pk[none:]
        pairs = int(pk.numel())
        if pairs:
            pd = pk // V
            pw = pk - pd * V
            at_row = torch.searchsorted(rows, pw)      # ``rows``: the distinct words, ascending
            grow = SG.gather(seg.grow, at_row)
            dots = int(SG.gather(seg.sizes, at_row).sum())
            (b_u, p_u, a_u), path = S.expect_sides(ex.model, seg, pd - 1, pw, grow)
            at = (inv - none).clamp_min(0).cpu().numpy()
            ok_h = ok.cpu().numpy()[:, None]
            s_h = np.concatenate([SG.gather(sides[2 * j + 1], o_t).cpu().numpy() for j in range(n_sides)])
            best = np.where(ok_h, b_u.cpu().numpy().astype(np.int64)[at], -1)
            above = np.where(ok_h, a_u.cpu().numpy().astype(np.int64)[at], -1)
            with np.errstate(invalid="ignore", divide="ignore"):
                lift = np.where(ok_h, p_u.cpu().numpy()[at] / s_h[:, None], np.nan)      # one rounded division
    out_cols = [("java", SG.gather(key, o_t).cpu().numpy())]
    ub, b_inv = np.unique(best[best >= 0], return_inverse=True)      # the words named, once each
    b_idx = np.full(best.shape, -1, np.int32)
    b_idx[best >= 0] = b_inv.astype(np.int32)
    b_names = [tables.word_names[i] for i in ub.tolist()]
    ua, a_inv = np.unique(above[above >= 0], return_inverse=True)
    a_idx = np.full(above.shape, -1, np.int32)
    a_idx[above >= 0] = a_inv.astype(np.int32)
    a_text = [str(int(x)) for x in ua]
    for j in range(n_sides):
        ip_names, ip_ids = ex.ips[j]
        sl = slice(j * n, (j + 1) * n)
        out_cols += [("dict", ip_names, SG.gather(ip_ids, o_t).cpu().numpy().astype(np.int32)),
                     cols[ex.cols[j][0]], cols[ex.cols[j][1]]]
        for f in range(F):
            # a column's own lifts as its dictionary: the writer takes a dictionary in whole for every column
            col = np.ascontiguousarray(lift[sl, f], np.float64)
            have = ~np.isnan(col)
            l_idx = np.full(n, -1, np.int32)
            l_idx[have] = np.arange(int(have.sum()), dtype=np.int32)
            out_cols += [("dict", b_names, np.ascontiguousarray(b_idx[sl, f])),
                         ("dict", native.lib().java_double_array(col[have]), l_idx),
                         ("dict", a_text, np.ascontiguousarray(a_idx[sl, f]))]
    out = os.path.join(cfg.lpath, f"{cfg.dsource}_expect.csv")
    native.lib().write_rows(out, None, out_cols, sep=sep, threads=cfg.threads, n=n)
    modal = (above == 0).sum(0).astype(np.int64).tolist()
    log(f"{cfg.dsource}_post: {n_sides * n} sides' expected values in {out} ({pairs} pairs, {dots} member dots x "
        f"{ex.model.K} topics, {path})")
    return dict(expect_fields=names, expect_modal_hist=dict(zip(names, modal)), expect_pairs=pairs,
                expect_member_dots=dots, expect_path=path)


@dataclass
class TailRank:
    """What ``tail_keys`` computed for every event of the day, on the scoring device: ``key`` the event's tail
    p-value (NaN: no side has one) and ``flag`` (``key < cfg.tail_tol``), per side ``tail`` (NaN: none), ``tot``,
    ``rarer`` (int64, -1: none) and ``pair`` (the side's distinct pair, -1: none), and the summary entries."""
    key: torch.Tensor
    flag: torch.Tensor
    tail: tuple
    tot: tuple
    rarer: tuple
    pair: tuple
    stats: dict


def tail_keys(cfg, model, side_docs, side_words, log=print) -> TailRank:
    """--tail-tol: the tail p-value of every event (``side_docs`` / ``side_words``: the θ / φ row of every event's
    side(s), -1: none).  Every side becomes the pair key ``d * V + w`` (-1 without a θ or a φ row); the distinct
    keys, which ``SG.unique`` returns sorted by document, go through ``scorer.tail_pairs`` once, ``tail = le / tot``
    is one rounded division, and the values are gathered back to the sides.  An event's key is the lowest of its
    sides' tails, a NaN side ignored; with no side left the key is NaN and the event is never flagged.  ``flag`` is
    ``key < cfg.tail_tol``.  From ``ops/sortgroup.py`` primitives and ``torch.where`` only (the cold-start rule of
    docs/ARCHITECTURE.md)."""
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    theta, phi = S.model_tables3(model)
    V, R, K = (int(x) for x in phi.shape)
    dev = phi.device
    n_sides = len(side_docs)
    n = int(side_docs[0].numel())
    doc = torch.cat([d.reshape(-1).to(torch.int64) for d in side_docs])
    word = torch.cat([w.reshape(-1).to(torch.int64) for w in side_words])
    ok = (doc >= 0) & (word >= 0)
    nan = torch.full((n_sides * n,), float("nan"), dtype=torch.float64, device=dev)
    tail, tot = nan, nan
    rarer = torch.full((n_sides * n,), -1, dtype=torch.int64, device=dev)
    pair = rarer
    pairs, docs, skipped = 0, 0, 0
    path = "cpu" if dev.type != "cuda" else "pairs"
    if n:
        pk, inv = SG.unique(torch.where(ok, doc * V + word, torch.full_like(doc, -1)), return_inverse=True)
        none = int(pk[0] < 0)      # the -1 of the sides without a pair sorts first
        pk = pk[none:]
        pairs = int(pk.numel())
        skipped = int((~ok).to(torch.int64).sum())
        if pairs:
            pd = pk // V
            docs = SG.run_ids(pd)[1]
            (le, tt, rr, _), path = S.tail_pairs(model, pd, pk - pd * V)
            at = (inv - none).clamp_min(0)
            tail = torch.where(ok, SG.gather(le / tt, at), nan)      # one rounded division
            tot = torch.where(ok, SG.gather(tt, at), nan)
            rarer = torch.where(ok, SG.gather(rr.to(torch.int64), at), rarer)
            pair = torch.where(ok, at, pair)
    side = lambda t: tuple(t[j * n:(j + 1) * n] for j in range(n_sides))      # noqa: E731
    key = tail[:n]
    for t in side(tail)[1:]:      # the lowest tail; a NaN side is ignored (NaN compares false)
        key = torch.where((t == t) & ((key != key) | (t < key)), t, key)
    flag = key < float(cfg.tail_tol)
    log(f"{cfg.dsource}_post: tail of every event for --tail-tol {cfg.tail_tol}: {pairs} pairs of {docs} documents "
        f"({path}), {docs} x {V} words x {K} topics x {R} members multiply-adds + {pairs} x {V} select-adds; "
        f"{skipped} sides without a pair")
    stats = dict(tail_tol=float(cfg.tail_tol), tail_rank_pairs=pairs, tail_rank_docs=docs, tail_rank_path=path,
                 tail_sides_skipped=skipped)
    return TailRank(key, flag, side(tail), side(tot), side(rarer), side(pair), stats)


TAIL_DECADES = ("<1e-6", "<1e-5", "<1e-4", "<1e-3", "<1e-2", "<1e-1", "<=1")


def write_tail(cfg, tables, order, key, sides, ex: ExplainInput, cols, sep: str = ",", log=print,
               rank: Optional[TailRank] = None) -> dict:
    """--tail: ``<type>_tail.csv`` next to the results file, line i describing its line i (``order``: the written
    events; ``cols``: their ``row_cols``): the key score, then per side the document, the word, the side's score,
    ``tail`` and ``rarer``.  ``tail`` is the share of the document's probability mass -- over the scorer's whole φ
    table -- on the words whose score at this document is at most the side's (``scorer.tail_mass``: le / tot, one
    rounded division), ``rarer`` the number of words that score strictly lower; both empty for a side without a
    θ or a φ row.  The values depend on the pair (document, word) only: the distinct pairs of the written sides are
    evaluated (``scorer.tail_pairs``) and gathered.  ``rank`` (--tail-tol): every side's values are there already,
    the written ones are gathered from them and nothing is launched.  Returns the summary entries."""
    from ..ops import native
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    dev = key.device
    n = int(order.size)
    o_t = torch.from_numpy(order).to(dev)
    n_sides = len(ex.words)
    theta, phi = S.model_tables3(ex.model)
    V, R, K = (int(x) for x in phi.shape)
    tail = np.full(n_sides * n, np.nan)
    rarer = np.full(n_sides * n, -1, np.int64)
    pairs, tot_range = 0, None
    if n and rank is not None:
        take = lambda ts: torch.cat([SG.gather(t, o_t) for t in ts]).cpu().numpy()      # noqa: E731
        tail, rarer, tot_w, pair_w = take(rank.tail), take(rank.rarer), take(rank.tot), take(rank.pair)
        pairs = int(np.unique(pair_w[pair_w >= 0]).size)
        if pairs:
            tot_range = [float(tot_w[pair_w >= 0].min()), float(tot_w[pair_w >= 0].max())]
    elif n:
        doc = torch.cat([SG.gather(sides[2 * j], o_t).to(torch.int64) for j in range(n_sides)])
        word = torch.cat([SG.gather(w, o_t).to(torch.int64) for w in ex.words])
        ok = (doc >= 0) & (word >= 0)
        pk, inv = SG.unique(torch.where(ok, doc * V + word, torch.full_like(doc, -1)), return_inverse=True)
        none = int(pk[0] < 0)      # the -1 of the sides without a pair sorts first
        pk = pk[none:]
        pairs = int(pk.numel())
        if pairs:
            (le, tot, rr, _), _ = S.tail_pairs(ex.model, pk // V, pk % V)
            at = (inv - none).clamp_min(0)
            ok_h = ok.cpu().numpy()
            with np.errstate(invalid="ignore", divide="ignore"):
                t_u = le.cpu().numpy() / tot.cpu().numpy()      # one rounded division
            at_h = at.cpu().numpy()
            tail = np.where(ok_h, t_u[at_h], np.nan)
            rarer = np.where(ok_h, rr.cpu().numpy().astype(np.int64)[at_h], -1)
            tot_range = [float(tot.min()), float(tot.max())]
    out_cols = [("java", SG.gather(key, o_t).cpu().numpy())]
    for j in range(n_sides):
        ip_names, ip_ids = ex.ips[j]
        t, r = tail[j * n:(j + 1) * n], rarer[j * n:(j + 1) * n]
        have = ~np.isnan(t)
        text = native.lib().java_double_array(np.ascontiguousarray(t[have], np.float64))
        idx = np.full(n, -1, np.int32)
        idx[have] = np.arange(len(text), dtype=np.int32)
        ur, r_inv = np.unique(r[r >= 0], return_inverse=True)
        r_idx = np.full(n, -1, np.int32)
        r_idx[r >= 0] = r_inv.astype(np.int32)
        out_cols += [("dict", ip_names, SG.gather(ip_ids, o_t).cpu().numpy().astype(np.int32)),
                     cols[ex.cols[j][0]], cols[ex.cols[j][1]], ("dict", text, idx),
                     ("dict", [str(int(x)) for x in ur], r_idx)]
    out = os.path.join(cfg.lpath, f"{cfg.dsource}_tail.csv")
    native.lib().write_rows(out, None, out_cols, sep=sep, threads=cfg.threads, n=n)
    good = tail[~np.isnan(tail)]
    edges = np.asarray([1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1])
    hist = np.bincount(np.searchsorted(edges, good, side="right"), minlength=len(TAIL_DECADES)).astype(np.int64)
    log(f"{cfg.dsource}_post: {n_sides * n} sides placed in {out} "
        f"({pairs} pairs x {V} words x {K} topics x {R} members)")
    return dict(tail_words=V, tail_pairs=pairs, tail_total_range=tot_range,
                tail_hist=dict(zip(TAIL_DECADES + ("none",), hist.tolist() + [int(tail.size - good.size)])))


PEER_LIFT_DECADES = ("<1e-2", "<1e-1", "<1", "<1e1", "<1e2", "<1e3", ">=1e3")


def write_peers(cfg, tables, order, key, sides, ex: ExplainInput, cols, sep: str = ",", log=print) -> dict:
    """--peers N: ``<type>_peers.csv`` next to the results file, line i describing its line i (``order``: the written
    events; ``cols``: their ``row_cols``): the key score, then per side the document, the word, the side's score,
    ``peers`` (how many of the document's N nearest documents were found), ``peer_dist`` (the L1 distance of the
    farthest of them / (2 R): the total-variation distance averaged over the members), ``peer_score`` (the mean
    score of the side's word at those peers, ``scorer.peer_scores``) and ``peer_lift`` = peer_score / the side's own
    score, one rounded division.  A side without a document gets four empty cells, one without a φ row ``peers``
    and ``peer_dist`` only.  And ``<type>_peer_groups.csv``: one line per distinct document of the written sides,
    ascending by θ row: the host, its count, then N x (peer host, its distance / (2 R)), empty past the count.
    The distinct documents are found with ``ops/sortgroup.py`` primitives and go through ``scorer.peer_topn`` once.
    Returns the summary entries."""
    from ..ops import native
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    dev = key.device
    N = int(cfg.peers)
    n = int(order.size)
    o_t = torch.from_numpy(order).to(dev)
    n_sides = len(ex.words)
    theta = S.model_tables3(ex.model)[0]
    D, R, K = (int(x) for x in theta.shape)
    two_r = 2.0 * R
    cnt = np.full(n_sides * n, -1, np.int64)
    far = np.full(n_sides * n, np.nan)
    ps = np.full(n_sides * n, np.nan)
    lift = np.full(n_sides * n, np.nan)
    ud = torch.zeros(0, dtype=torch.int64, device=dev)
    if n:
        doc = torch.cat([SG.gather(sides[2 * j], o_t).to(torch.int64) for j in range(n_sides)])
        word = torch.cat([SG.gather(w, o_t).to(torch.int64) for w in ex.words])
        ud, inv = SG.unique(doc, return_inverse=True)
        none = int(ud[0] < 0)      # the -1 of the sides without a document sorts first
        ud = ud[none:]
    (rows_u, dist_u, cnt_u), path = S.peer_topn(ex.model, ud, N)
    hosts = int(ud.numel())
    if hosts:
        has = doc >= 0
        at = (inv - none).clamp_min(0)
        cnt_s = torch.where(has, SG.gather(cnt_u, at).to(torch.int64), torch.zeros_like(doc))
        dist_s = SG.gather(dist_u, at)
        last = torch.gather(dist_s, 1, (cnt_s - 1).clamp_min(0).unsqueeze(1)).reshape(-1)
        ps_t = S.peer_scores(ex.model, SG.gather(rows_u, at), cnt_s, doc, word)
        s_h = np.concatenate([SG.gather(sides[2 * j + 1], o_t).cpu().numpy() for j in range(n_sides)])
        has_h, cnt_h = has.cpu().numpy(), cnt_s.cpu().numpy()
        cnt = np.where(has_h, cnt_h, -1)
        ps = ps_t.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            far = np.where(has_h & (cnt_h > 0), last.cpu().numpy() / two_r, np.nan)      # one rounded division each
            lift = ps / s_h

    def doubles(x):      # a column's own values as its dictionary, empty cells for NaN
        x = np.ascontiguousarray(x, np.float64)
        have = ~np.isnan(x)
        idx = np.full(x.size, -1, np.int32)
        idx[have] = np.arange(int(have.sum()), dtype=np.int32)
        return ("dict", native.lib().java_double_array(x[have]), idx)

    def ints(x):         # -1: an empty cell
        ux, x_inv = np.unique(x[x >= 0], return_inverse=True)
        idx = np.full(x.size, -1, np.int32)
        idx[x >= 0] = x_inv.astype(np.int32)
        return ("dict", [str(int(v)) for v in ux], idx)

    out_cols = [("java", SG.gather(key, o_t).cpu().numpy())]
    for j in range(n_sides):
        ip_names, ip_ids = ex.ips[j]
        sl = slice(j * n, (j + 1) * n)
        out_cols += [("dict", ip_names, SG.gather(ip_ids, o_t).cpu().numpy().astype(np.int32)),
                     cols[ex.cols[j][0]], cols[ex.cols[j][1]], ints(cnt[sl]), doubles(far[sl]), doubles(ps[sl]),
                     doubles(lift[sl])]
    out = os.path.join(cfg.lpath, f"{cfg.dsource}_peers.csv")
    native.lib().write_rows(out, None, out_cols, sep=sep, threads=cfg.threads, n=n)
    # the groups: one line per distinct document
    ud_h = ud.cpu().numpy()
    rows_h = rows_u.cpu().numpy().astype(np.int64).reshape(hosts, N)
    dist_h = dist_u.cpu().numpy().reshape(hosts, N)
    cnt_uh = cnt_u.cpu().numpy().astype(np.int64)
    ur, r_inv = np.unique(rows_h[rows_h >= 0], return_inverse=True)      # the hosts named, once each
    r_idx = np.full(rows_h.shape, -1, np.int32)
    r_idx[rows_h >= 0] = r_inv.astype(np.int32)
    r_names = [tables.doc_names[i] for i in ur.tolist()]
    g_cols = [("dict", [tables.doc_names[d] for d in ud_h.tolist()], np.arange(hosts, dtype=np.int32)),
              ("int", cnt_uh)]
    for i in range(N):
        g_cols += [("dict", r_names, np.ascontiguousarray(r_idx[:, i])),
                   doubles(np.where(rows_h[:, i] >= 0, dist_h[:, i] / two_r, np.nan))]
    g_out = os.path.join(cfg.lpath, f"{cfg.dsource}_peer_groups.csv")
    native.lib().write_rows(g_out, None, g_cols, sep=sep, threads=cfg.threads, n=hosts)
    good = lift[~np.isnan(lift)]
    edges = np.asarray([1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3])
    hist = np.bincount(np.searchsorted(edges, good, side="right"), minlength=len(PEER_LIFT_DECADES)).astype(np.int64)
    identical = int(((cnt_uh > 0) & (dist_h[:, 0] == 0.0)).sum()) if hosts else 0
    log(f"{cfg.dsource}_post: {n_sides * n} sides scored at their hosts' {N} nearest hosts in {out}, the groups in "
        f"{g_out} ({hosts} hosts x {D} candidates x {R * K} subtract-adds, {path})")
    return dict(peers=N, peer_hosts=hosts, peer_candidates=D, peer_path=path, peer_identical=identical,
                peer_lift_hist=dict(zip(PEER_LIFT_DECADES + ("none",), hist.tolist() + [int(lift.size - good.size)])))


TOPIC_RESP_BUCKETS = ("<0.5", "<0.9", "<0.99", ">=0.99")
TOPIC_REPORT_KEYS = ("topic_report", "topic_rows", "topic_columns", "topic_path", "topic_sides", "topic_minor_sides",
                     "topic_resp_hist")
TOPIC_REPORT_FILES = ("topics", "topic_words", "topic_hosts", "topic")      # <type>_<name>.csv


def write_topic_report(cfg, tables, order, key, sides, ex: ExplainInput, cols, sep: str = ",", log=print) -> dict:
    """--topic-report N: four files next to the results file, every line carrying (member, topic); a column of the
    scorers' tables θ [D, R, K] / φ [V, R, K] is j = member K + topic, and topics of different members are never
    matched.

    ``<type>_topics.csv``, one line per column in (member, topic) order: member, topic, ``mass`` (the column's θ
    total, ``scorer.group_rows_sum`` with one segment over all D rows in row order), ``share`` = mass / D,
    ``hosts_dominant`` and ``words_dominant`` (the θ / φ rows whose greatest entry within the member is this topic,
    ``scorer.row_dominant``), ``top_words_mass`` (the listed φ values added from 0.0 in list order),
    ``written_sides`` (the written sides this column explains) and ``minor_sides`` (those of them whose host's own
    dominant topic is another).  ``<type>_topic_words.csv``: per column its N words with the greatest φ
    (``scorer.column_topn``; fewer when the column has fewer non-NaN rows): member, topic, rank from 1, word, φ and
    ``excl`` = φ / the word's φ total over the member's topics (from 0.0 in topic order, one division).
    ``<type>_topic_hosts.csv``: the same over θ without ``excl``.  ``<type>_topic.csv``: line i describing line i of
    the results file (``order``: the written events; ``cols``: their ``row_cols``): the key score, then per side
    the document, the word, the side's score and -- ``scorer.topic_sides`` -- ``member``, ``topic`` (the column with
    the greatest θ φ product), ``resp`` (that product's share of the score), ``host_share`` (the host's θ there) and
    ``host_topic`` (the host's own dominant topic in that member); five empty cells for a side without a θ row or a
    φ row.  Returns the summary entries."""
    from ..ops import native
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    dev = key.device
    N = int(cfg.topic_report)
    n = int(order.size)
    n_sides = len(ex.words)
    theta, phi = S.model_tables3(ex.model)
    theta, phi = theta.contiguous(), phi.contiguous()
    D, R, K = (int(x) for x in theta.shape)
    V = int(phi.shape[0])
    W = R * K
    fmt = native.lib().java_double_array

    def doubles(x):      # a column's own values as its dictionary, empty cells for NaN
        x = np.ascontiguousarray(x, np.float64)
        have = ~np.isnan(x)
        idx = np.full(x.size, -1, np.int32)
        idx[have] = np.arange(int(have.sum()), dtype=np.int32)
        return ("dict", fmt(x[have]), idx)

    def ints(x):         # -1: an empty cell
        ux, x_inv = np.unique(x[x >= 0], return_inverse=True)
        idx = np.full(x.size, -1, np.int32)
        idx[x >= 0] = x_inv.astype(np.int32)
        return ("dict", [str(int(v)) for v in ux], idx)

    def path_of(name):
        return os.path.join(cfg.lpath, f"{cfg.dsource}_{name}.csv")

    # the model's tables: the N rows that carry every column, the dominant topic of every row, the column totals
    (w_rows, w_vals, w_cnt), path = S.column_topn(phi.reshape(V, W), N)
    (h_rows, h_vals, h_cnt), _ = S.column_topn(theta.reshape(D, W), N)
    (_, hosts_dom), _ = S.row_dominant(theta)
    (_, words_dom), _ = S.row_dominant(phi)
    mass = S.group_rows_sum(theta.reshape(D, W), torch.arange(D, dtype=torch.int32, device=dev),
                            torch.zeros(1, dtype=torch.int64, device=dev),
                            torch.full((1,), D, dtype=torch.int64, device=dev)).reshape(-1)
    slot = torch.arange(N, device=dev).unsqueeze(0)
    live = slot < w_cnt.unsqueeze(1)
    top_mass = torch.zeros(W, dtype=torch.float64, device=dev)
    for s in range(N):
        top_mass = torch.where(live[:, s], top_mass + w_vals[:, s], top_mass)
    # excl: the listed word's φ over its total within the member, the total from 0.0 in topic order
    member = (torch.arange(W, device=dev, dtype=torch.int64) // K).unsqueeze(1)
    own = SG.gather(phi.reshape(V * R, K), (w_rows.to(torch.int64).clamp_min(0) * R + member).reshape(-1))
    tot = torch.zeros(W * N, dtype=torch.float64, device=dev)
    for k in range(K):
        tot = tot + own[:, k]
    excl = (w_vals.reshape(-1) / tot).reshape(W, N)

    # the written sides
    o_t = torch.from_numpy(order).to(dev)
    if n:
        doc = torch.cat([SG.gather(sides[2 * j], o_t).to(torch.int64) for j in range(n_sides)])
        word = torch.cat([SG.gather(w, o_t).to(torch.int64) for w in ex.words])
    else:
        doc = word = torch.zeros(0, dtype=torch.int64, device=dev)
    (col, resp, share, host_topic), _ = S.topic_sides(ex.model, doc, word)
    col_h = col.cpu().numpy().astype(np.int64)
    resp_h, share_h, ht_h = resp.cpu().numpy(), share.cpu().numpy(), host_topic.cpu().numpy().astype(np.int64)
    has = col_h >= 0
    written = np.bincount(col_h[has], minlength=W).astype(np.int64)
    minor_of = has & (ht_h != col_h % K)
    minor = np.bincount(col_h[minor_of], minlength=W).astype(np.int64)

    # <type>_topics.csv
    j = np.arange(W, dtype=np.int64)
    mass_h = mass.cpu().numpy()
    t_cols = [("int", j // K), ("int", j % K), ("java", mass_h), ("java", mass_h / float(D) if D else mass_h),
              ("int", hosts_dom.reshape(-1).cpu().numpy()), ("int", words_dom.reshape(-1).cpu().numpy()),
              ("java", top_mass.cpu().numpy()), ("int", written), ("int", minor)]
    native.lib().write_rows(path_of("topics"), None, t_cols, sep=sep, threads=cfg.threads, n=W)

    # <type>_topic_words.csv / <type>_topic_hosts.csv: the listed slots of every column, column by column
    def lists(name, rows_t, vals_t, cnt_t, names, extra=None):
        rows_h = rows_t.cpu().numpy().astype(np.int64)
        at = np.flatnonzero((np.arange(N)[None, :] < cnt_t.cpu().numpy()[:, None]).reshape(-1))
        jj, rank = at // N, at % N + 1
        ur, r_inv = np.unique(rows_h.reshape(-1)[at], return_inverse=True)      # the rows named, once each
        l_cols = [("int", jj // K), ("int", jj % K), ("int", rank),
                  ("dict", [names[i] for i in ur.tolist()], r_inv.astype(np.int32)),
                  ("java", vals_t.cpu().numpy().reshape(-1)[at])]
        if extra is not None:
            l_cols.append(("java", extra.cpu().numpy().reshape(-1)[at]))
        native.lib().write_rows(path_of(name), None, l_cols, sep=sep, threads=cfg.threads, n=int(at.size))
        return int(at.size)

    lists("topic_words", w_rows, w_vals, w_cnt, tables.word_names, excl)
    lists("topic_hosts", h_rows, h_vals, h_cnt, tables.doc_names)

    # <type>_topic.csv
    out_cols = [("java", SG.gather(key, o_t).cpu().numpy())]
    for s in range(n_sides):
        ip_names, ip_ids = ex.ips[s]
        sl = slice(s * n, (s + 1) * n)
        c = col_h[sl]
        out_cols += [("dict", ip_names, SG.gather(ip_ids, o_t).cpu().numpy().astype(np.int32)),
                     cols[ex.cols[s][0]], cols[ex.cols[s][1]], ints(np.where(c >= 0, c // K, -1)),
                     ints(np.where(c >= 0, c % K, -1)), doubles(resp_h[sl]), doubles(share_h[sl]), ints(ht_h[sl])]
    out = path_of("topic")
    native.lib().write_rows(out, None, out_cols, sep=sep, threads=cfg.threads, n=n)

    good = resp_h[has]
    hist = np.bincount(np.searchsorted(np.asarray([0.5, 0.9, 0.99]), good, side="right"),
                       minlength=len(TOPIC_RESP_BUCKETS)).astype(np.int64)
    log(f"{cfg.dsource}_post: {W} topics of {D} hosts and {V} words described in {path_of('topics')}, the topic of "
        f"{n_sides * n} sides in {out} ({path})")
    return dict(topic_report=N, topic_rows=[D, V], topic_columns=W, topic_path=path,
                topic_sides=dict(members=[written[r * K:(r + 1) * K].tolist() for r in range(R)],
                                 none=int(has.size - has.sum())),
                topic_minor_sides=int(minor.sum()),
                topic_resp_hist=dict(zip(TOPIC_RESP_BUCKETS + ("none",), hist.tolist() + [int(has.size - has.sum())])))


DRIFT_DECADES = ("<1e-6", "<1e-5", "<1e-4", "<1e-3", "<1e-2", "<1e-1", "<=1")
TOPIC_MATCH_KEYS = ("topic_match", "topic_match_day", "topic_match_pairs", "topic_match_shared_words",
                    "topic_match_shared_hosts", "topic_match_new_hosts", "topic_match_mutual", "topic_match_path",
                    "host_drift_hist")
TOPIC_MATCH_FILES = ("topic_match", "topic_stability", "host_drift")      # <type>_<name>.csv


def match_topics(cost: np.ndarray):
    """The alignment of one other model to today's topics from ``cost`` [K, K'] (today's topic a, the other's topic
    b; a NaN: no distance): ``(match int64 [K'], nearest int64 [K'], mutual bool [K'])``.  ``match[b]``: today's
    topic of b under the minimum-cost assignment (``native.assign_min`` over the matrix padded to square with
    0.0-cost dummy rows / columns; -1: b went to a dummy, unmatched).  ``nearest[b]``: the a of lowest cost, ties to
    the lower a, a NaN never (-1: none).  ``mutual[b]``: b is matched to a, a is its nearest, and b is the
    lowest-cost column of row a, ties to the lower b."""
    from ..ops import native
    K, Kp = cost.shape
    n = max(K, Kp)
    sq = np.zeros((n, n), np.float64)
    sq[:K, :Kp] = cost
    row_to_col = np.asarray(native.assign_min(sq), np.int64)
    match = np.full(Kp, -1, np.int64)
    a = np.arange(K)
    real = row_to_col[:K] < Kp
    match[row_to_col[:K][real]] = a[real]
    far = np.where(np.isnan(cost), np.inf, cost)
    nearest = np.where(np.isfinite(far).any(0), far.argmin(0), -1).astype(np.int64) if K else np.full(Kp, -1, np.int64)
    best_col = far.argmin(1) if Kp else np.full(K, -1, np.int64)      # of every row a: the first lowest column
    b = np.arange(Kp)
    mutual = (match >= 0) & (nearest == match) & (best_col[np.clip(match, 0, None)] == b if K else False)
    return match, nearest, mutual


def write_topic_match(cfg, tables, ex: ExplainInput, sep: str = ",", log=print) -> dict:
    """--topic-match / --topic-match-day DIR: the topics of the other models aligned to today's member 0, next to
    the results file.  The others: the --ensemble members ``m1``, ``m2``, ... and, with DIR, ``prev`` -- member 0
    of ``load_model_tables(DIR)``.

    Distances (``scorer.column_l1``: per pair of columns the sum of |x - y| over the paired rows, in blocks of
    ``config.MATCH_BLOCK``).  A member shares today's rows: ``cost[a][b] = C[a][b] * 0.5``, the total-variation
    distance of φ₀'s topic a and the member's topic b.  The previous day's words are joined by name through the
    name -> row maps of ``ModelTables`` (a name that repeats takes the row its map gives it): today's rows whose
    name the previous day knows, in row order, give the pairs; ``cost[a][b] = ((C[a][b] + ua[a]) + ub[b]) * 0.5``
    with ua / ub the column's φ total over its own rows whose name the other day lacks (``scorer.group_rows_sum``,
    one segment in row order).  No shared word: every distance is 1.0.

    ``<type>_topic_match.csv``, a line per (other, its topic b): other, topic, ``match`` (today's topic; empty:
    unmatched), ``dist``, ``nearest``, ``nearest_dist``, ``mutual`` (``match_topics``), ``shared_mass`` (the
    column's φ total over its rows whose name today knows; a member: over all rows).
    ``<type>_topic_stability.csv``, a line per topic a of today: topic, ``members`` (R - 1), ``members_mutual``,
    ``mean_dist`` and ``max_dist`` (over the members' matched distances, the adds from 0.0 in member order, one
    division; empty at R = 1), ``prev_topic``, ``prev_dist``, ``prev_mutual``, ``shared_mass`` (empty without DIR).
    ``<type>_host_drift.csv`` (with DIR), a line per host of both days, joined by name: host, ``drift``, ``topic``
    (today's dominant), ``prev_topic`` (the previous day's dominant in today's numbering; empty: unmatched);
    descending by ``drift``, ties in today's row order.  ``drift``: from 0.0 over today's topics a in order
    |θ₀[d][a] - θ'[d'][b(a)]| (an unmatched a: against 0.0), then the previous day's unmatched topics in their
    order, each one rounded subtraction, its magnitude and one rounded add; then * 0.5.  Returns the summary
    entries."""
    from ..ops import native
    from ..ops import sortgroup as SG
    from ..score import scorer as S
    theta, phi = S.model_tables3(ex.model)
    dev = phi.device
    V, R, K = (int(x) for x in phi.shape)
    D = int(theta.shape[0])
    fmt = native.lib().java_double_array
    phi0 = phi[:, 0, :].contiguous()
    theta0 = theta[:, 0, :].contiguous()

    def doubles(x):      # a column's own values as its dictionary, empty cells for NaN
        x = np.ascontiguousarray(x, np.float64)
        have = ~np.isnan(x)
        idx = np.full(x.size, -1, np.int32)
        idx[have] = np.arange(int(have.sum()), dtype=np.int32)
        return ("dict", fmt(x[have]), idx)

    def ints(x):         # -1: an empty cell
        x = np.asarray(x, np.int64)
        ux, x_inv = np.unique(x[x >= 0], return_inverse=True)
        idx = np.full(x.size, -1, np.int32)
        idx[x >= 0] = x_inv.astype(np.int32)
        return ("dict", [str(int(v)) for v in ux], idx)

    def path_of(name):
        return os.path.join(cfg.lpath, f"{cfg.dsource}_{name}.csv")

    def total(table, rows):      # [W]: the column totals over ``rows`` (ascending) in row order
        if rows.numel() == 0:
            return torch.zeros(int(table.shape[1]), dtype=torch.float64, device=dev)
        return S.group_rows_sum(table, rows.to(torch.int32), torch.zeros(1, dtype=torch.int64, device=dev),
                                torch.full((1,), rows.numel(), dtype=torch.int64, device=dev)).reshape(-1)

    def rows_t(rows):
        return torch.from_numpy(np.asarray(rows, np.int64)).to(dev)

    others, path, work = [], "cpu", []      # (label, cost [K, K'] on the host, shared_mass [K'])
    if R > 1:
        C, path = S.column_l1(phi0, phi.reshape(V, R * K))
        cost = (C * 0.5).cpu().numpy()
        mass = total(phi.reshape(V, R * K), torch.arange(V, device=dev)).cpu().numpy()
        for r in range(1, R):
            others.append((f"m{r}", cost[:, r * K:(r + 1) * K], mass[r * K:(r + 1) * K], V))
        work.append(f"{V} x {K} x {R * K}")
    prev = None
    if cfg.topic_match_day:
        pt = load_model_tables(cfg.topic_match_day)
        Kp = int(pt.phi.shape[1])
        phi_p = torch.from_numpy(np.ascontiguousarray(pt.phi, np.float64)).to(dev)
        today_w, prev_w = tables.word_index(), pt.word_index()
        names = tables.word_names
        shared = np.fromiter((nm in prev_w for nm in names), dtype=bool, count=len(names))
        ia = np.fromiter((today_w[names[r]] for r in np.flatnonzero(shared)), dtype=np.int64, count=int(shared.sum()))
        ib = np.fromiter((prev_w[names[r]] for r in np.flatnonzero(shared)), dtype=np.int64, count=int(shared.sum()))
        known = np.fromiter((nm in today_w for nm in pt.word_names), dtype=bool, count=len(pt.word_names))
        M = int(ia.size)
        mass_a = total(phi0, rows_t(np.flatnonzero(shared)))
        mass_b = total(phi_p, rows_t(np.flatnonzero(known)))
        if M:
            C, path = S.column_l1(phi0, phi_p, rows_t(ia), rows_t(ib))
            ua = total(phi0, rows_t(np.flatnonzero(~shared)))
            ub = total(phi_p, rows_t(np.flatnonzero(~known)))
            cost = (((C + ua.unsqueeze(1)) + ub.unsqueeze(0)) * 0.5).cpu().numpy()
        else:
            log(f"{cfg.dsource}_post: {cfg.topic_match_day} shares no word with this run: every distance is 1.0")
            cost = np.ones((K, Kp), np.float64)
        others.append(("prev", cost, mass_b.cpu().numpy(), M))
        work.append(f"{M} x {K} x {Kp}")
        prev = (pt, Kp, mass_a.cpu().numpy())

    # <type>_topic_match.csv
    labels, col_other, col_b, col_match, col_dist, col_near, col_ndist, col_mut, col_mass = [], [], [], [], [], [], [], [], []
    aligned = []      # per other: (match [K'], mutual [K'], cost)
    for i, (label, cost, mass, _) in enumerate(others):
        match, nearest, mutual = match_topics(cost)
        Kp = cost.shape[1]
        b = np.arange(Kp)
        labels.append(label)
        col_other.append(np.full(Kp, i, np.int32))
        col_b.append(b)
        col_match.append(match)
        col_dist.append(np.where(match >= 0, cost[np.clip(match, 0, None), b], np.nan) if K else np.full(Kp, np.nan))
        col_near.append(nearest)
        col_ndist.append(np.where(nearest >= 0, cost[np.clip(nearest, 0, None), b], np.nan) if K else np.full(Kp, np.nan))
        col_mut.append(mutual.astype(np.int64))
        col_mass.append(mass)
        aligned.append((match, mutual, cost))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)      # noqa: E731
    n_lines = int(sum(x.size for x in col_b))
    native.lib().write_rows(path_of("topic_match"), None,
                            [("dict", labels, cat(col_other, np.int32)), ("int", cat(col_b, np.int64)),
                             ints(cat(col_match, np.int64)), doubles(cat(col_dist, np.float64)),
                             ints(cat(col_near, np.int64)), doubles(cat(col_ndist, np.float64)),
                             ("int", cat(col_mut, np.int64)), ("java", cat(col_mass, np.float64))],
                            sep=sep, threads=cfg.threads, n=n_lines)

    # <type>_topic_stability.csv: today's topics
    def inverse(match, mutual, cost):      # per today's topic a: its b (-1), the distance (NaN), mutual
        b_of = np.full(K, -1, np.int64)
        has = match >= 0
        b_of[match[has]] = np.flatnonzero(has)
        ok = b_of >= 0
        dist = np.where(ok, cost[np.arange(K), np.clip(b_of, 0, None)], np.nan) if cost.shape[1] else np.full(K, np.nan)
        return b_of, dist, np.where(ok, mutual[np.clip(b_of, 0, None)], False) if cost.shape[1] else np.zeros(K, bool)

    nan_k = np.full(K, np.nan)
    m_mut, m_sum, m_max = np.zeros(K, np.int64), np.zeros(K, np.float64), np.zeros(K, np.float64)
    for match, mutual, cost in aligned[:R - 1]:
        _, dist, mut = inverse(match, mutual, cost)
        m_mut += mut
        m_sum = m_sum + dist                                             # from 0.0 in member order
        m_max = np.where((dist > m_max) | np.isnan(dist), dist, m_max)   # a NaN stays
    if R > 1:
        member_cols = [("int", np.full(K, R - 1, np.int64)), ints(m_mut), doubles(m_sum / float(R - 1)), doubles(m_max)]
    else:
        member_cols = [("int", np.zeros(K, np.int64)), ints(np.full(K, -1)), doubles(nan_k), doubles(nan_k)]
    if prev is not None:
        p_b, p_dist, p_mut = inverse(*aligned[-1])
        prev_cols = [ints(p_b), doubles(p_dist), ints(np.where(p_b >= 0, p_mut.astype(np.int64), -1)), doubles(prev[2])]
    else:
        prev_cols = [ints(np.full(K, -1)), doubles(nan_k), ints(np.full(K, -1)), doubles(nan_k)]
    native.lib().write_rows(path_of("topic_stability"), None,
                            [("int", np.arange(K, dtype=np.int64))] + member_cols + prev_cols,
                            sep=sep, threads=cfg.threads, n=K)

    # <type>_host_drift.csv
    shared_hosts = new_hosts = None
    hist = {}
    if prev is not None:
        pt, Kp, _ = prev
        today_d, prev_d = tables.doc_index(), pt.doc_index()
        dn = tables.doc_names
        d_rows = np.asarray([d for d, nm in enumerate(dn) if nm in prev_d and today_d[nm] == d], np.int64)
        p_rows = np.asarray([prev_d[dn[d]] for d in d_rows.tolist()], np.int64)
        shared_hosts = int(d_rows.size)
        new_hosts = int(sum(1 for nm in today_d if nm not in prev_d))
        match = aligned[-1][0]                                           # [K']: today's topic of b, -1
        b_of = inverse(*aligned[-1])[0]                                  # [K]: the previous topic of a, -1
        th0 = SG.gather(theta0, rows_t(d_rows))                          # [n, K]
        thp = SG.gather(torch.from_numpy(np.ascontiguousarray(pt.theta, np.float64)).to(dev), rows_t(p_rows))
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        acc = torch.zeros(shared_hosts, dtype=torch.float64, device=dev)
        for a in range(K):
            other = thp[:, int(b_of[a])] if b_of[a] >= 0 else zero       # an unmatched topic: its whole entry
            acc = acc + (th0[:, a] - other).abs()
        for b in np.flatnonzero(match < 0).tolist():
            acc = acc + (zero - thp[:, b]).abs()
        drift = acc * 0.5
        (dom, _), _ = S.row_dominant(th0.reshape(shared_hosts, 1, K))
        (dom_p, _), _ = S.row_dominant(thp.reshape(shared_hosts, 1, Kp))
        dom_p = dom_p.reshape(-1).to(torch.int64)
        to_today = torch.cat([rows_t(match), torch.full((1,), -1, dtype=torch.int64, device=dev)])
        prev_topic = SG.gather(to_today, torch.where(dom_p >= 0, dom_p, torch.full_like(dom_p, Kp)))
        _, perm = torch.sort(SG.f64_order_keys(zero - drift), stable=True)      # descending, ties in row order
        perm_h = perm.cpu().numpy()
        drift_h = drift.cpu().numpy()[perm_h]
        ur, r_inv = np.unique(d_rows[perm_h], return_inverse=True)
        native.lib().write_rows(path_of("host_drift"), None,
                                [("dict", [dn[i] for i in ur.tolist()], r_inv.astype(np.int32)), doubles(drift_h),
                                 ints(dom.reshape(-1).cpu().numpy().astype(np.int64)[perm_h]),
                                 ints(prev_topic.cpu().numpy()[perm_h])],
                                sep=sep, threads=cfg.threads, n=shared_hosts)
        good = drift_h[~np.isnan(drift_h)]
        edges = np.asarray([1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1])
        h = np.bincount(np.searchsorted(edges, good, side="right"), minlength=len(DRIFT_DECADES)).astype(np.int64)
        hist = dict(zip(DRIFT_DECADES + ("none",), h.tolist() + [int(drift_h.size - good.size)]))
    log(f"{cfg.dsource}_post: {len(others)} models matched to {K} topics in {path_of('topic_match')} "
        f"(pairs x Wa x Wb: {', '.join(work) if work else 'none'}; {path})")
    return dict(topic_match=True, topic_match_day=cfg.topic_match_day or "",
                topic_match_pairs=[int(o[3]) for o in others],
                topic_match_shared_words=others[-1][3] if prev is not None else None,
                topic_match_shared_hosts=shared_hosts, topic_match_new_hosts=new_hosts,
                topic_match_mutual=[int(m.sum()) for _, m, _ in aligned], topic_match_path=path,
                host_drift_hist=hist)


def one_sided_index(tables, ip_names, ip, unames, inv, device, ip_map=None):
    """The one-sided scorers' (dns, proxy) index set-up: (θ, φ, θ row of every event, φ row of every event).
    ``ip`` / ``inv``: every event's id into ``ip_names`` / ``unames``; ``ip_map``: the doc row of every ip id
    when the caller has it (a prefix of it is used), else looked up by name."""
    from ..ops import sortgroup as SG
    if ip_map is not None:
        m = np.asarray(ip_map, np.int64)[:len(ip_names)]
    else:
        di = tables.doc_index()
        m = np.fromiter((di.get(n, -1) for n in ip_names), dtype=np.int64, count=len(ip_names))
    # the rows these events reference: the whole tables (one process) or fetched from their ranks
    th, ph, drow, wrow = tables.compact(m, tables.word_rows(unames))
    widx = SG.gather(torch.from_numpy(wrow).to(device), inv)
    didx = SG.gather(torch.from_numpy(drow).to(device), ip)
    return th, ph, didx, widx


def rank_results(cfg, key, flag):
    """(order, below, limit): the flagged events ascending by ``key`` -- with MAXRESULTS only the ``limit``
    lowest -- their count, and the limit (None: none).  ``key`` / ``flag``: the score key and its flag under TOL,
    or under --tail-tol the tail key and flag of ``tail_keys``."""
    from ..score import scorer as S
    limit = cfg.max_results if cfg.max_results > 0 else None
    if limit is None:
        order = S.rank_flagged(key, flag)
        return order, int(order.size), None
    order, below = S.rank_flagged_counted(key, flag, limit)
    return order, below, limit


def write_results(cfg, tables, what: str, ranked, key, row_cols, events: int, sides, votes, log=print, ctx=None,
                  sep: str = ",", extra=None, explain: Optional[ExplainInput] = None,
                  tail_rank: Optional[TailRank] = None) -> dict:
    """``<type>_results.csv`` from ``ranked`` (what ``rank_results`` returned) and the scorer's ``row_cols``, the
    log line, and the scoring stage's result.  One process: the rows, then the host report (``sides``: the
    ``doc_a, score_a, doc_b, score_b`` of ``write_host_report``) and the votes histogram.  Several ranks
    (``ctx``): the ranks' rows merged into one ascending file (``shardio.merge_sorted_rows``, the sortByKey
    shuffle), the counts summed.  ``extra``: further result entries.  ``explain``: the sides' φ rows and columns
    for ``write_explain``, ``write_expect``, ``write_tail``, ``write_peers`` and ``write_topic_report`` (one process,
    under --explain / --expect / --tail / --peers / --topic-report); ``write_topic_match`` (--topic-match) takes
    the model from it.
    ``tail_rank`` (--tail-tol):
    what ``tail_keys`` returned -- ``ranked`` was made from its key and flag, ``key`` stays the score key that the
    files' columns hold."""
    from ..ops import native
    order, below, limit = ranked
    n = int(order.size)
    out = os.path.join(cfg.lpath, f"{cfg.dsource}_results.csv")
    cols = row_cols(order)
    if ctx is not None and ctx.active:
        from ..ops import sortgroup as SG
        from ..parallel import shardio as SIO
        text, ends = native.lib().format_rows(None, cols, n=n, row_ends=True, threads=cfg.threads)
        key_o = SG.gather(key, torch.from_numpy(order).to(key.device)).cpu().numpy()
        total = SIO.merge_sorted_rows(ctx, key_o.astype(np.float64), text, ends, out, limit=limit)
        below = ctx.allreduce_int(below)
        log(f"{cfg.dsource}_post: {flagged_text(total, below, limit, what, cfg.tol)} written to {out} "
            f"({n} from rank {ctx.rank})")
        return dict(flagged=total, below_tol=below, rank_flagged=n, events=ctx.allreduce_int(events), **(extra or {}))
    native.lib().write_rows(out, None, cols, sep=sep, threads=cfg.threads, n=n)
    if tail_rank is not None:
        of = "" if limit is None else f" of the {below}"
        log(f"{cfg.dsource}_post: {n}{of} {what} with tail < {cfg.tail_tol}"
            f"{'' if limit is None else f' (MAXRESULTS {limit})'} written to {out}")
    else:
        log(f"{cfg.dsource}_post: {flagged_text(n, below, limit, what, cfg.tol)} written to {out}")
    hosts = write_host_report(cfg, tables, *sides, row_cols, sep=sep, log=log) if cfg.host_report else {}
    kept = {} if cfg.expect else None      # --expect goes on from the explain file's sides and groups
    why = write_explain(cfg, tables, order, key, sides, explain, cols, sep=sep, log=log,
                        keep=kept) if cfg.explain else {}
    exp = write_expect(cfg, tables, order, key, sides, explain, cols, kept, sep=sep, log=log) if cfg.expect else {}
    tail = write_tail(cfg, tables, order, key, sides, explain, cols, sep=sep, log=log,
                      rank=tail_rank) if cfg.tail else {}
    peers = write_peers(cfg, tables, order, key, sides, explain, cols, sep=sep, log=log) if cfg.peers else {}
    topics = write_topic_report(cfg, tables, order, key, sides, explain, cols, sep=sep,
                                log=log) if cfg.topic_report else {}
    matched = write_topic_match(cfg, tables, explain, sep=sep, log=log) if cfg.topic_match else {}
    return dict(flagged=n, below_tol=below, events=events, **(extra or {}), **hosts,
                **votes_hist(votes, order, cfg.ensemble), **why, **exp, **tail, **peers, **topics, **matched,
                **(tail_rank.stats if tail_rank is not None else {}))


def save_json(path: str, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))


def load_json(path: str):
    with open(path) as f:
        return json.load(f)
