"""--holdout: document-completion held-out perplexity (the standard answer to "how many topics").

A fraction F of every document's tokens is held out by a counter-based draw (``ops.hip.holdout_draw`` on the GPU,
``ops.reference.holdout_draw`` elsewhere: the same integers), the model is fitted on the rest, and the held-out
tokens are scored by the scorers' own p(word | document) = theta_d . phi_w of that fit:

    perplexity = exp(-sum_e t_e log(theta_d(e) . phi_w(e)) / sum_e t_e)

over the entries e whose word the training corpus has (the usual out-of-vocabulary rule: a held-out token of a word
unseen in training is counted in ``unseen_tokens`` and left out; lda-c's -100 floor would swamp the measure).
Every document keeps at least one training token, so D, the document ids and ``num_terms`` do not move.  The sums
run in a fixed order (``group_rows_sum``: per document, then over the documents), the log is ``log_rn``: the GPU and
the CPU path give the same bits from the same theta and phi.
"""
from __future__ import annotations

import math
import time
from typing import Optional

import numpy as np
import torch

from ...corpus.csr import Corpus
from ...ops import sortgroup as SG

RECORD_KEYS = ("topics", "em_iterations", "alpha", "train_likelihood", "heldout_tokens", "unseen_tokens",
               "evaluated_tokens", "split_documents", "loglik", "loglik_per_token", "perplexity", "seconds")


def _ops(dev: torch.device, twin: bool = False):
    """The kernels on a GPU (a missing extension is an error there, never a fall-back), the torch twins elsewhere."""
    if dev.type == "cuda" and not twin:
        from ...ops import hip as H
        H.lib()
        return H
    from ...ops import reference as REF
    return REF


def check_fraction(F: float) -> float:
    from ...config import HOLDOUT_MAX_F
    F = float(F)
    if not 0.0 < F <= HOLDOUT_MAX_F:
        raise ValueError(f"--holdout must be in (0, {HOLDOUT_MAX_F}], got {F}")
    return F


def split(corpus: Corpus, F: float, seed: int, device=None, twin: bool = False):
    """(training ``Corpus``, t): t (int64 [nnz], on ``device``) the held-out tokens of every entry of ``corpus``
    after the two document rules; the training corpus the entries with ``c - t > 0``, compacted, with those counts:
    the same documents (none empty) and the same ``num_terms``."""
    from ...ops import reference as REF
    dev = torch.device(device or "cpu")
    thr = REF.holdout_thr(check_fraction(F))
    doc_ptr = torch.from_numpy(corpus.doc_ptr).to(dev)
    counts = torch.from_numpy(corpus.counts).to(dev)
    t = _ops(dev, twin).holdout_draw(doc_ptr, counts, int(seed), thr)
    rest = counts - t
    keep = rest > 0
    words, csum = SG.compact(torch.from_numpy(corpus.word_idx).to(dev), keep)
    left, _ = SG.compact(rest, keep)
    train = Corpus(SG.gather(csum, doc_ptr).cpu().numpy(), words.cpu().numpy(), left.cpu().numpy(), corpus.num_terms,
                   meta=dict(corpus.meta, holdout=float(F)))
    return train, t


def split_tallies(corpus: Corpus, train: Corpus, t) -> dict:
    """What the split did, for the records: tokens, held-out tokens, documents with a held-out token."""
    th = t.cpu().numpy()
    per_doc = np.add.reduceat(th, corpus.doc_ptr[:-1]) if corpus.nnz else np.zeros(corpus.num_docs, np.int64)
    per_doc = np.where(np.diff(corpus.doc_ptr) > 0, per_doc, 0)      # reduceat on an empty document reads its successor
    return dict(tokens=int(corpus.counts.sum()), heldout_tokens=int(th.sum()), train_tokens=int(train.counts.sum()),
                train_nnz=train.nnz, split_documents=int((per_doc > 0).sum()))


def evaluate(corpus: Corpus, train: Corpus, t, gamma, log_beta, device=None, fit: Optional[dict] = None,
             twin: bool = False) -> dict:
    """The held-out record of one training fit (``gamma`` [D, K], ``log_beta`` [K, V] of ``train``): ``RECORD_KEYS``.
    ``fit``: the fit's own entries (topics, em_iterations, alpha, train_likelihood, seconds).  ``twin``: the torch
    twins even on a GPU (tests: the same bits)."""
    from ...export import lda_post
    t0 = time.perf_counter()
    dev = torch.device(device or "cpu")
    ops = _ops(dev, twin)
    theta = torch.from_numpy(np.ascontiguousarray(lda_post.doc_topics(gamma, strict=False))).to(dev)
    phi = torch.from_numpy(np.ascontiguousarray(lda_post.word_topics(log_beta, strict=False))).to(dev)
    D, V, nnz = corpus.num_docs, corpus.num_terms, corpus.nnz
    if tuple(theta.shape) != (D, phi.shape[1]) or phi.shape[0] != V:
        raise ValueError(f"holdout: theta {tuple(theta.shape)} / phi {tuple(phi.shape)} are not the fit of a corpus of "
                         f"{D} documents and {V} words")
    t = t.to(dev)
    doc_ptr = torch.from_numpy(corpus.doc_ptr).to(dev)
    word = torch.from_numpy(corpus.word_idx).to(dev)
    doc_of = SG.segment_ids(doc_ptr[1:] - doc_ptr[:-1], total=nnz).to(torch.int32)
    seen = torch.zeros(V, dtype=torch.uint8, device=dev)
    if train.nnz:
        tw = torch.from_numpy(train.word_idx).to(dev).to(torch.int64)
        seen.index_put_((tw,), torch.ones(tw.numel(), dtype=torch.uint8, device=dev))
    ll = ops.holdout_entries(theta, phi, doc_of, word, t, seen)
    total = 0.0
    if nnz and D:
        # a document's entries in entry order, then the documents in document order: group_rows_sum's fixed order
        doc_ll = ops.group_rows_sum(ll.unsqueeze(1), torch.arange(nnz, dtype=torch.int32, device=dev),
                                    doc_ptr[:-1].contiguous(), doc_ptr[1:].contiguous())
        total = float(ops.group_rows_sum(doc_ll, torch.arange(D, dtype=torch.int32, device=dev),
                                         torch.zeros(1, dtype=torch.int64, device=dev),
                                         torch.full((1,), D, dtype=torch.int64, device=dev))[0, 0])
    held = int(t.sum()) if nnz else 0
    unseen = int(torch.where(SG.gather(seen, word) == 0, t, torch.zeros_like(t)).sum()) if nnz else 0
    evaluated = held - unseen
    docs = split_tallies(corpus, train, t)["split_documents"]
    per_token = total / evaluated if evaluated else None
    rec = dict(fit or {})
    rec.update(heldout_tokens=held, unseen_tokens=unseen, evaluated_tokens=evaluated, split_documents=docs,
               loglik=total, loglik_per_token=per_token,
               perplexity=math.exp(-per_token) if evaluated and -per_token < 709.0 else None)
    rec["seconds"] = float(rec.get("seconds") or 0.0) + (time.perf_counter() - t0)
    for k in RECORD_KEYS:
        rec.setdefault(k, None)
    return {k: rec[k] for k in RECORD_KEYS}


def select(records) -> Optional[int]:
    """The evaluated topic count of lowest perplexity; ties go to the smaller count.  None: nothing was evaluated."""
    ok = [r for r in records if r.get("perplexity") is not None]
    return min(ok, key=lambda r: (r["perplexity"], r["topics"]))["topics"] if ok else None
