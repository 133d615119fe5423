"""Corpora and the Python-planner twin shared by tests/test_engine_plan.py and tests/test_engine_plan_gpu.py.

The corpora are the smallest at which each rule of the native engine plan can go wrong: the bucket edges from
both sides, equal lengths (stability), 0 / 1 / 8 / 9 team8 documents (the -1 gaps of isolate_longest), words
on both sides of SuffPlan's bounds, a late bucket over 60 % of the entries, large counts in one chunk, and
empty documents at both ends.
"""
import functools

import numpy as np
import torch

from oni_ml_amd.corpus.csr import Corpus, DeviceCorpus
from oni_ml_amd.models.lda.em import LDAEngine

SETTINGS = ((20, 32), (8, 8), (32, 32))      # (KS, U)
EDGE_LENGTHS = (0, 1, 8, 9, 64, 65, 256, 257, 2048, 2049, 2112, 4097)
WORD_LENGTHS = (1025, 1024, 65, 64, 1, 0)    # entries of word ids 0 .. 5 in edge_corpus


def make_corpus(lens, V, seed, forced=()):
    """Documents of distinct words; ``forced``: (word id, documents) -- the word is one of the words of each of
    those (non-empty) documents, and of no other; the remaining words are drawn from ids past the forced ones."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    nf = len(forced)
    extra = [[] for _ in lens]
    for w, docs in forced:
        for d in docs:
            extra[d].append(w)
    words = []
    for d, n in enumerate(lens.tolist()):
        head = extra[d]
        assert len(head) <= n
        words.append(np.concatenate([np.asarray(head, np.int64), nf + rng.choice(V - nf, n - len(head), replace=False)]))
    w = np.concatenate(words).astype(np.int32) if words else np.zeros(0, np.int32)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Corpus(ptr, w, rng.integers(1, 6, w.size).astype(np.int64), V)


@functools.lru_cache(maxsize=None)
def edge_corpus():
    """Every bucket edge from both sides, pairs of equal length, empty documents at the start and the end,
    1,100 short documents carrying words of 1,025 / 1,024 / 65 / 64 / 1 / 0 entries, and counts of 2^31
    through the first chunk of the longest document."""
    short = [6 + (i % 6) for i in range(1100)]
    lens = [0, 0, 0] + list(EDGE_LENGTHS) + [9, 2049, 65] + short + [0, 0]
    s0 = 3 + len(EDGE_LENGTHS) + 3
    forced = [(w, list(range(s0, s0 + n))) for w, n in enumerate(WORD_LENGTHS)]
    c = make_corpus(lens, 5000, 1, forced)
    d = 3 + EDGE_LENGTHS.index(4097)
    c.counts[c.doc_ptr[d]:c.doc_ptr[d] + 129] = 2**31
    return c


@functools.lru_cache(maxsize=None)
def team8_corpus(n8):
    """n8 documents past the team8 edge (two of them equal) among 40 shorter ones."""
    rng = np.random.default_rng(100 + n8)
    lens = [2049 + (i // 2) for i in range(n8)] + list(rng.integers(0, 300, 40))
    return make_corpus(rng.permutation(lens), 2400, 200 + n8)


@functools.lru_cache(maxsize=None)
def late_heavy_corpus():
    """The longest-document bucket holds more than 60 % of the entries: no split unless forced."""
    rng = np.random.default_rng(7)
    return make_corpus([2100] + list(rng.integers(1, 12, 100)), 2300, 8)


@functools.lru_cache(maxsize=None)
def one_bucket_corpus():
    """Every document in one bucket (and none at all past it): nothing to overlap."""
    return make_corpus([70, 80, 90, 100, 70], 300, 9)


def empty_corpus():
    return Corpus(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), 5)


def bare_engine(c, KS, U, suff_split="auto", defer_final=True, device="cpu"):
    """An LDAEngine shell with the attributes the planners read (no kernels, no state buffers)."""
    eng = LDAEngine.__new__(LDAEngine)
    eng.device = torch.device(device)
    eng.corpus, eng.D, eng.V, eng.K, eng.KS, eng._U = c, c.num_docs, c.num_terms, KS, KS, U
    eng._cwin, eng.suff_split, eng.defer_final, eng.engine_plan = None, suff_split, defer_final, "native"
    return eng


def python_plans(c, KS, U, suff_split="auto", defer_final=True, device="cpu"):
    """The Python planners' result on ``device`` (CPU tensors: the twins of the device partition are
    csc_subset and gs_et_rows run on them): a bare engine with dc, gs_plan, _stages, _csums, suff_plan,
    _suff_split."""
    from oni_ml_amd.ops import hip as H
    eng = bare_engine(c, KS, U, suff_split, defer_final, device)
    eng.dc = DeviceCorpus.build(c, device) if eng.device.type == "cpu" else DeviceCorpus._build_device(c, eng.device)
    eng.gs_plan = H.GSPlan(eng.dc.doc_len, KS, U, eng.device)
    assert eng.gs_plan.split is None
    eng._stages = eng._build_stages(c, KS)
    eng._csums = eng._build_chunk_sums(c, KS)
    eng.suff_plan = H.SuffPlan(eng.dc.word_len, eng.device)
    eng.cw = torch.zeros(c.num_terms, KS, dtype=torch.float64, device=eng.device)
    eng._suff_part = torch.zeros(max(eng.suff_plan.n_blocks, 1), 2 + KS, dtype=torch.float64, device=eng.device)
    eng._suff_split = eng._build_suff_split() if suff_split != "off" else None
    return eng


def section(p, name, dtype):
    """Numpy view of one section of a host plan (LDAEngine.host_plan)."""
    off, n, el = p["sections"][name]
    assert off % 256 == 0 and np.dtype(dtype).itemsize == el
    return p["buf"][off:off + n * el].view(dtype)


def host_et_rows(p, csc_ent_late, csc_doc_late, umax):
    """et_row of the late slots from the plan's three per-document tables (the device kernel's formula)."""
    s0, w, base = (section(p, k, np.int32).astype(np.int64) for k in ("et_s0", "et_w", "et_base"))
    d = np.asarray(csc_doc_late, np.int64)
    assert (base[d] >= 0).all()
    return base[d] + np.minimum((np.asarray(csc_ent_late, np.int64) - s0[d]) // w[d], umax - 1)
