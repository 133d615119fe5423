"""Event scoring + threshold + rank (reference: flow_post_lda.scala:227-248, dns_post_lda.scala:312-331;
SURVEY.md C5c/C5d/C7c/C7d, hot ops H12/H13).

    score(doc, word) = sum_{k<K} θ[doc]_k * φ[word]_k      (unknown doc/word -> constant default vector)
    flow key         = min(score(sip, src_word), score(dip, dest_word))
    output           = rows with key < TOL, ascending by key (sortByKey)

The gather-dot runs in the fused HIP kernel `score_events` (strict IEEE f64,
sequential over topics, as the JVM evaluates it); the survivors are compacted
and sorted on the device; only the flagged rows travel back to the host.
Ties keep input order (stable sort; Spark's order for equal keys is unspecified).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch


@dataclass
class TopicModel:
    """θ / φ tables on the device plus the name -> row lookups the scorers use."""
    theta: torch.Tensor            # [D, K] f64
    phi: torch.Tensor              # [V, K] f64
    K: int
    default: float                 # default-vector value for misses

    @staticmethod
    def build(theta: np.ndarray, phi: np.ndarray, default: float, device, K: Optional[int] = None) -> "TopicModel":
        K = int(theta.shape[1] if K is None else K)
        th = torch.from_numpy(np.ascontiguousarray(theta[:, :K], np.float64)).to(device)
        ph = torch.from_numpy(np.ascontiguousarray(phi[:, :K], np.float64)).to(device)
        return TopicModel(th, ph, K, float(default))


@dataclass
class EnsembleModel:
    """R members fitted on one corpus from different seeds (``--ensemble R``): their θ / φ interleaved per row,
    so a side's R member rows are one contiguous run.  ``score`` gives the mean of the members' scores,
    ``score_votes`` also how many members would have flagged each event on their own."""
    theta: torch.Tensor            # [D, R, K] f64
    phi: torch.Tensor              # [V, R, K] f64
    R: int
    K: int
    default: float

    @staticmethod
    def build(members: Sequence, default: float, device, K: Optional[int] = None) -> "EnsembleModel":
        """``members``: (θ [D, K'], φ [V, K']) host arrays of every member, member 0 first."""
        K = int(members[0][0].shape[1] if K is None else K)
        th = np.ascontiguousarray(np.stack([np.asarray(t, np.float64)[:, :K] for t, _ in members], axis=1))
        ph = np.ascontiguousarray(np.stack([np.asarray(p, np.float64)[:, :K] for _, p in members], axis=1))
        return EnsembleModel(torch.from_numpy(th).to(device), torch.from_numpy(ph).to(device), len(members), K,
                             float(default))


def build_model(tables, th, ph, default: float, device):
    """The scorers' model of ``tables`` (pipeline/common.py ModelTables): a TopicModel, or with ``tables.members``
    the EnsembleModel of member 0 (``th`` / ``ph``, as ``tables.compact`` returned them) and the others."""
    members = getattr(tables, "members", None)
    if members:
        return EnsembleModel.build([(th, ph)] + list(members), default, device)
    return TopicModel.build(th, ph, default, device)


def _ops(device):
    """``(ops.hip, True)`` for a CUDA device, ``(ops.reference, False)`` otherwise: the one place that knows which
    implementation a device gets.  The twins share names and signatures; imported at first use."""
    if device.type == "cuda":
        from ..ops import hip
        return hip, True
    from ..ops import reference
    return reference, False


def _i32(t):
    return None if t is None else t.to(torch.int32).contiguous()


def _i64(t):
    return None if t is None else t.to(torch.int64).contiguous()


def default_value(source: str, K: int, strict: bool) -> float:
    """Miss vector: flow 0.05 x 20, dns 0.1 x 20 in the reference (sums 1.0 and 2.0); 1/K when fixed."""
    if strict:
        return 0.05 if source == "flow" else 0.1
    return 1.0 / K


def score_votes(model, doc_a, word_a, doc_b=None, word_b=None, tol: float = float("inf")):
    """``score`` and, as a fifth value, the votes: for an EnsembleModel uint8 [n], the members whose own key is
    under ``tol``; None for one model."""
    if isinstance(model, EnsembleModel):
        return _ops(model.theta.device)[0].score_ensemble(model.theta, model.phi, model.R, model.K, model.default,
                                                          _i32(doc_a), _i32(word_a), _i32(doc_b), _i32(word_b), tol)
    return tuple(score(model, doc_a, word_a, doc_b, word_b, tol)) + (None,)


def score(model, doc_a, word_a, doc_b=None, word_b=None, tol: float = float("inf")):
    """Returns (score_a, score_b|None, key, flag) device tensors, for either model kind."""
    if isinstance(model, EnsembleModel):
        return tuple(score_votes(model, doc_a, word_a, doc_b, word_b, tol))[:4]
    O, gpu = _ops(model.theta.device)
    if gpu:
        return O.score_events(model.theta, model.phi, model.K, model.default, _i32(doc_a), _i32(word_a), _i32(doc_b),
                              _i32(word_b), tol)
    return O.score(model.theta, model.phi, model.K, model.default, doc_a, word_a, doc_b, word_b, tol)


def key_quantiles(key: torch.Tensor, qs=(1e-4, 1e-3, 1e-2, 0.1, 0.5), sample: int = 1 << 18) -> dict:
    """Quantiles of the events' scores (a strided sample of at most ``sample``), for choosing TOL: the
    fraction q of events scoring below key_q<q> would be flagged.  Metrics only: the sample goes to the
    host (a first torch.quantile on the device cost 57 ms of a cold process's wall)."""
    n = key.numel()
    if n == 0:
        return {}
    k = key[:: max(1, -(-n // sample))].to(torch.float64).cpu().numpy()
    v = np.quantile(k, np.asarray(qs, np.float64))
    return {f"key_q{q:g}": float(x) for q, x in zip(qs, v)}


def rank_flagged(key: torch.Tensor, flag: torch.Tensor, limit: Optional[int] = None) -> torch.Tensor:
    """Indices of flagged rows in ascending key order (stable) as an int64 host array.

    ``limit`` (MAXRESULTS): only the first ``limit`` of them, element for element ``rank_flagged(key, flag)[:limit]``
    -- see ``rank_flagged_counted``."""
    if limit is not None:
        return rank_flagged_counted(key, flag, limit)[0]
    from ..ops import sortgroup as SG
    sel, _ = SG.compact(torch.arange(flag.numel(), device=flag.device), flag.reshape(-1).to(torch.bool))
    if sel.numel() == 0:
        return np.zeros(0, np.int64)
    order = SG.sort_stable(SG.gather(key, sel))[1]
    return SG.gather(sel, order).cpu().numpy().astype(np.int64)


def rank_flagged_counted(key: torch.Tensor, flag: torch.Tensor, limit: int):
    """(``rank_flagged(key, flag)[:limit]``, number of flagged rows) without ranking every flagged row: the
    ``limit`` lowest are selected first (the HIP radix select ``ops.hip.select_lowest`` on the GPU, its torch
    twin elsewhere; ties at the cut to the lowest row), then only those m <= limit keys are sorted.  The
    selection arrives in row order, so the stable sort orders ties as the full sort does.  Always selects: on an
    MI355X it was 1.8 - 3.0 x faster than ranking everything at every shape measured (2 M rows with N = 3,000 and
    100,000, 100 M rows with N = 3,000: profiles/select_lowest.md), so there is no fall-back rule."""
    from ..ops import sortgroup as SG
    flag = flag.reshape(-1)
    O, gpu = _ops(key.device)
    if gpu:
        sel, flagged = O.select_lowest(key.reshape(-1).contiguous(), flag.to(torch.uint8).contiguous(), limit,
                                       with_count=True)
    else:
        sel, flagged = O.select_lowest(key.reshape(-1), flag, limit, with_count=True)
    if sel.numel() == 0:
        return np.zeros(0, np.int64), flagged
    order = SG.sort_stable(SG.gather(key, sel))[1]
    return SG.gather(sel, order).cpu().numpy().astype(np.int64), flagged


def host_summary(doc_a, score_a, doc_b, score_b, num_docs: int, tol: float):
    """The scored sides folded per document, ``(events, flagged, min_score, worst, skipped)`` -- device tensors
    [num_docs] and an int (``ops.hip.host_summary`` on the GPU, ``ops.reference.host_summary`` elsewhere).
    ``doc_*``: the θ row of every side's IP or -1; ``worst``: side number 2 * event + side of the lowest score."""
    f64 = lambda t: None if t is None else t.contiguous()                      # noqa: E731
    return _ops(score_a.device)[0].host_summary(_i32(doc_a), f64(score_a), _i32(doc_b), f64(score_b), int(num_docs),
                                                float(tol))


def group_rows_sum(table: torch.Tensor, order: torch.Tensor, seg_start: torch.Tensor, seg_end: torch.Tensor):
    """[G, W] sums of the rows ``table[order[seg_start[g] : seg_end[g]]]`` in the fixed block order of
    ``config.GROUP_BLOCK`` (``ops.hip.group_rows_sum`` on the GPU, ``ops.reference.group_rows_sum`` elsewhere:
    the same bits)."""
    O, gpu = _ops(table.device)
    if gpu:
        return O.group_rows_sum(table.contiguous(), _i32(order), _i64(seg_start), _i64(seg_end))
    return O.group_rows_sum(table, order, seg_start, seg_end)


def model_tables3(model):
    """(theta [D, R, K], phi [V, R, K]) of either model kind (one model: R = 1, a view)."""
    if isinstance(model, EnsembleModel):
        return model.theta, model.phi
    return model.theta.unsqueeze(1), model.phi.unsqueeze(1)


@dataclass
class FieldSegments:
    """The groups of ``field_segments``: the explained fields' stable sorts back to back (``order`` int32 [F V]),
    the referenced groups' segments of it (``seg_start`` / ``seg_end`` int64 [Gtot]), and per given row the group
    of every explained field (``grow`` int64 [len(rows), F]) with its size (``sizes``)."""
    order: torch.Tensor
    seg_start: torch.Tensor
    seg_end: torch.Tensor
    grow: torch.Tensor
    sizes: torch.Tensor


def field_segments(V: int, word_keys: torch.Tensor, fields, rows: torch.Tensor, device) -> FieldSegments:
    """For the φ rows ``rows`` (int64, distinct, >= 0) and every explained field of ``fields``
    (``WordSpace.fields()``: (name, radix, explained), most significant digit first), the row's group: the φ rows
    whose key (``word_keys`` int64 [V], φ-row order) agrees with the row's on every digit but that field's, the row
    among them.  On the device, from ``ops/sortgroup.py`` primitives only: per field one stable int64 sort of the V
    masked keys (ties keep row order, so a group's members ascend by row), the runs' starts, and the segments the
    given rows reference.  What --explain sums (``field_groups``) and --expect walks (``expect_sides``)."""
    from ..ops import sortgroup as SG
    dev = device
    if word_keys.numel() != V:
        raise ValueError(f"field_groups: {word_keys.numel()} word keys for {V} phi rows")
    radix = [int(r) for _, r, _ in fields]
    stride = [1] * len(fields)
    for i in range(len(fields) - 2, -1, -1):
        stride[i] = stride[i + 1] * radix[i + 1]
    keys = word_keys.to(dev).to(torch.int64)
    orders, starts, ends, grows, sizes, base = [], [], [], [], [], 0
    for i, (_, r, explained) in enumerate(fields):
        if not explained:
            continue
        digit = keys // stride[i]
        if i > 0:      # the most significant digit is whatever remains of the key
            digit = digit % r
        sk, perm = SG.sort_stable(keys - digit * stride[i])      # by (masked key, row)
        grp, G = SG.run_ids(sk)
        st = SG.run_starts(grp, G)
        of_row = torch.empty_like(grp)
        of_row[perm] = grp                                       # the group of every φ row
        ug, inv = SG.unique(SG.gather(of_row, rows), return_inverse=True)
        s, e = SG.gather(st, ug), SG.gather(st, ug + 1)
        # the fields' sorted orders lie back to back: field number len(orders) starts at that many times V
        starts.append(s + len(orders) * V)
        ends.append(e + len(orders) * V)
        orders.append(perm.to(torch.int32))
        grows.append(inv + base)
        sizes.append(SG.gather(e - s, inv))
        base += int(ug.numel())
    if not orders:
        raise ValueError("field_groups: no explained field")
    return FieldSegments(torch.cat(orders), torch.cat(starts), torch.cat(ends), torch.stack(grows, 1),
                         torch.stack(sizes, 1))


def field_groups(model, word_keys: torch.Tensor, fields, rows: torch.Tensor, segments: Optional[FieldSegments] = None):
    """--explain: for the φ rows ``rows`` (int64, distinct, >= 0) and every explained field of ``fields``
    (``WordSpace.fields()``: (name, radix, explained), most significant digit first), the sum of φ over the row's
    group -- the φ rows whose key (``word_keys`` int64 [V], φ-row order) agrees with the row's on every digit but
    that field's.  Returns ``(gsum [Gtot, R, K], grow int64 [len(rows), F], sizes int64 [len(rows), F])``:
    ``grow[i, f]`` the ``gsum`` row of ``rows[i]``'s group of the f-th explained field, ``sizes`` its members.

    The groups are ``field_segments``' (``segments``: what it returned for these arguments, when the caller has
    it) -- at most len(rows) x F group sums are made, never V x K per field."""
    theta, phi = model_tables3(model)
    V, R, K = phi.shape
    seg = segments if segments is not None else field_segments(V, word_keys, fields, rows, phi.device)
    # one launch pair (and one set of host-side bound checks) for every field's groups
    gsum = group_rows_sum(phi.reshape(V, R * K), seg.order, seg.seg_start, seg.seg_end).reshape(-1, R, K)
    return gsum, seg.grow, seg.sizes


def explain_sides(model, gsum: torch.Tensor, doc: torch.Tensor, word: torch.Tensor, grow: torch.Tensor):
    """``(cond [n, F], why uint8 [n])`` of the sides (``ops.hip.explain_sides`` on the GPU, its torch twin
    elsewhere); ``model``: a TopicModel or an EnsembleModel."""
    theta, phi = model_tables3(model)
    return _ops(theta.device)[0].explain_sides(theta.contiguous(), phi.contiguous(), gsum.contiguous(), _i32(doc),
                                               _i32(word), _i32(grow), model.default)


def expect_sides(model, seg: FieldSegments, doc: torch.Tensor, word: torch.Tensor, grow: torch.Tensor):
    """``((best int32 [n, F], pbest float64 [n, F], above int32 [n, F]), path)`` of (document, word) pairs: per
    explained field the member of the word's group (``seg``: ``field_segments``; ``grow`` [n, F] its groups or -1)
    that the document's model finds most probable, that member's score and the number of members that beat the
    word itself.  ``path``: ``"blocks"`` (``ops.hip.expect_sides``) on the GPU, ``"cpu"`` (its torch twin: the same
    bits) elsewhere; ``model``: a TopicModel or an EnsembleModel."""
    theta, phi = model_tables3(model)
    O, gpu = _ops(theta.device)
    out = O.expect_sides(theta.contiguous(), phi.contiguous(), _i32(seg.order), _i64(seg.seg_start), _i64(seg.seg_end),
                         _i32(doc), _i32(word), _i32(grow), model.default)
    return out, O.EXPECT_FORMS[0] if gpu else "cpu"


def expect_form() -> str:
    """The form of ``ops.hip.expect_sides`` that runs on the GPU (``expect_path`` of a run without a pair)."""
    from ..ops.hip import EXPECT_FORMS
    return EXPECT_FORMS[0]


def tail_mass(model, doc: torch.Tensor, word: torch.Tensor):
    """``(le, tot float64 [n]; rarer, ties int32 [n])`` of the sides: the model's probability mass on the words
    that are as rare at the side's document as its word, or rarer, the mass of the whole table, and the counts of
    rarer and equally rare words (``ops.hip.tail_mass`` on the GPU, its torch twin elsewhere: the same bits).
    ``model``: a TopicModel (one member through a ``[rows, 1, K]`` view) or an EnsembleModel; ``doc`` / ``word``: θ /
    φ rows or -1."""
    theta, phi = model_tables3(model)
    return _ops(theta.device)[0].tail_mass(theta.contiguous(), phi.contiguous(), _i32(doc), _i32(word))


def tail_pairs(model, doc: torch.Tensor, word: torch.Tensor):
    """``((le, tot, rarer, ties), path)`` of (document, word) pairs sorted by document, every ``doc >= 0`` and
    ``word >= 0`` -- what ``SG.unique`` of the keys ``d * V + w`` gives.  The values are ``tail_mass``'s bit for bit
    whichever path computes them, so the choice shows in no file:
      ``"docs"``   ``ops.hip.tail_mass_docs`` -- on the GPU, where the register ladder holds the row width and the
                   pairs per distinct document are at least ``config.TAIL_DOCS_MIN_SHARE``;
      ``"pairs"``  ``ops.hip.tail_mass`` -- on the GPU otherwise;
      ``"cpu"``    ``ops.reference.tail_mass`` -- on the CPU, always."""
    from ..config import TAIL_DOCS_MIN_SHARE
    from ..ops import sortgroup as SG
    theta, phi = model_tables3(model)
    theta, phi = theta.contiguous(), phi.contiguous()
    d32, w32 = _i32(doc), _i32(word)
    if theta.device.type != "cuda":
        from ..ops.reference import tail_mass as ref
        return ref(theta, phi, d32, w32), "cpu"
    from ..ops import hip as H
    n = int(d32.numel())
    if n and H.tail_theta_path(int(theta.shape[1]), int(theta.shape[2])) == "registers":
        docs = SG.run_ids(d32.to(torch.int64))[1]
        if n >= TAIL_DOCS_MIN_SHARE * docs:
            return H.tail_mass_docs(theta, phi, d32, w32), "docs"
    return H.tail_mass(theta, phi, d32, w32), "pairs"


def peer_topn(model, query: torch.Tensor, n: int):
    """``((rows int32 [Q, n], dist float64 [Q, n], count int32 [Q]), path)``: the ``n`` θ rows nearest to every
    ``query`` row in L1 distance over the whole row (all members), ascending by (distance, row), the query's own
    row left out (``ops.hip.peer_topn`` on the GPU, its torch twin elsewhere: the same bits).  ``path``: the
    kernel's form (``ops.hip.peer_theta_path``) or ``"cpu"``; ``model``: a TopicModel or an EnsembleModel."""
    theta = model_tables3(model)[0].contiguous()
    O, gpu = _ops(theta.device)
    out = O.peer_topn(theta, _i32(query), n)
    return out, O.peer_theta_path(int(theta.shape[1]), int(theta.shape[2])) if gpu else "cpu"


def peer_scores(model, rows: torch.Tensor, count: torch.Tensor, doc: torch.Tensor, word: torch.Tensor) -> torch.Tensor:
    """float64 [n]: the mean score of every side's word at its document's peers.  ``rows`` [n, N] / ``count`` [n]:
    the side's document's peers (``peer_topn``, gathered to the sides); ``doc`` / ``word``: the side's θ / φ row or
    -1.  From 0.0, for i = 0 .. count - 1 in peer order, ``+ score(peer i, word)`` -- N calls of the scorers on
    (peer i, word), a slot past the count masked -- then one division by (double)count.  NaN for a side without a
    document, a φ row or a peer.  The scorers' own kernels or twins: the same bits on both devices."""
    n, N = int(rows.shape[0]), int(rows.shape[1])
    ok = (doc.reshape(-1) >= 0) & (word.reshape(-1) >= 0)
    count = count.reshape(-1).to(torch.int64)
    w = word.reshape(-1)
    acc = torch.zeros(n, dtype=torch.float64, device=rows.device)
    for i in range(N):
        live = ok & (count > i)      # (a masked slot scores the default vector, which the select drops)
        s = score(model, torch.where(live, rows[:, i].to(w.dtype), torch.full_like(w, -1)), w)[0]
        acc = torch.where(live, acc + s, acc)
    return torch.where(ok & (count > 0), acc / count.to(torch.float64), torch.full_like(acc, float("nan")))


def column_topn(table: torch.Tensor, n: int):
    """``((rows int32 [W, n], vals float64 [W, n], count int32 [W]), path)``: per column of ``table`` [rows, W] the
    ``n`` rows with the greatest values, descending, ties to the lower row, a NaN never (``ops.hip.column_topn`` on
    the GPU, its torch twin elsewhere: the same bits).  ``path``: the kernel's form (``ops.hip.topic_path``) or
    ``"cpu"``."""
    table = table.contiguous()
    O, gpu = _ops(table.device)
    return O.column_topn(table, n), O.topic_path(n, int(table.shape[1])) if gpu else "cpu"


def row_dominant(table3: torch.Tensor):
    """``((arg int32 [rows, R], counts int64 [R, K]), path)``: the first topic attaining the maximum of every
    (row, member) of ``table3`` [rows, R, K] and the rows per (member, topic) (``ops.hip.row_dominant`` on the GPU,
    its torch twin elsewhere).  ``path``: ``"lanes"`` or ``"cpu"``."""
    table3 = table3.contiguous()
    O, gpu = _ops(table3.device)
    return O.row_dominant(table3), "lanes" if gpu else "cpu"


def topic_sides(model, doc: torch.Tensor, word: torch.Tensor):
    """``((col int32 [n], resp float64 [n], host_share float64 [n], host_topic int32 [n]), path)`` of the sides: the
    column j = member K + topic with the greatest θ φ product, its share ``resp`` of the side's score, the host's θ
    there and the host's own dominant topic in that member (``ops.hip.topic_sides`` on the GPU, its torch twin
    elsewhere: the same bits).  ``model``: a TopicModel or an EnsembleModel; ``doc`` / ``word``: θ / φ rows or -1;
    ``path``: ``"lanes"`` or ``"cpu"``."""
    theta, phi = model_tables3(model)
    O, gpu = _ops(theta.device)
    return O.topic_sides(theta.contiguous(), phi.contiguous(), _i32(doc), _i32(word)), "lanes" if gpu else "cpu"


def column_l1(A: torch.Tensor, B: torch.Tensor, ia: Optional[torch.Tensor] = None,
              ib: Optional[torch.Tensor] = None):
    """``(C float64 [Wa, Wb], path)``: ``C[a, b]`` = the sum over the pairs of ``|A[ia[m], a] - B[ib[m], b]|`` in
    blocks of ``config.MATCH_BLOCK`` pairs (``ops.hip.column_l1`` on the GPU, its torch twin elsewhere: the same
    bits).  ``ia`` / ``ib``: int64 rows, both None for the identity.  ``path``: ``"hip"`` or ``"cpu"``."""
    A, B = A.contiguous(), B.contiguous()
    O, gpu = _ops(A.device)
    return O.column_l1(A, B, _i64(ia), _i64(ib)), "hip" if gpu else "cpu"


def rank_hosts(min_score: torch.Tensor, flagged: torch.Tensor, limit: Optional[int] = None) -> np.ndarray:
    """Document rows with at least one flagged side, ascending by their lowest score, ties to the lowest row
    (int64 host array); ``limit``: only the first ``limit`` of them (the MAXRESULTS radix select and its tie
    rule)."""
    return rank_flagged(min_score, flagged > 0, limit)


def lookup_sorted(keys_sorted: torch.Tensor, values_idx: torch.Tensor, query: torch.Tensor) -> torch.Tensor:
    """Map query keys through a sorted key table -> row index (or -1)."""
    if keys_sorted.numel() == 0:
        return torch.full_like(query, -1, dtype=torch.int64)
    i = torch.searchsorted(keys_sorted, query).clamp_max(keys_sorted.numel() - 1)
    hit = keys_sorted[i] == query
    return torch.where(hit, values_idx[i], torch.full_like(i, -1))


class KeyIndex:
    """word-key -> word-row lookup (device).  `valid` masks rows the reference could never match
    (strict mode: word names longer than 20 bytes are truncated in word_results.csv)."""

    def __init__(self, keys: np.ndarray, device, valid: Optional[np.ndarray] = None):
        keys = np.asarray(keys, np.int64)
        rows = np.arange(keys.size, dtype=np.int64)
        if valid is not None:
            keys, rows = keys[valid], rows[valid]
        o = np.argsort(keys, kind="stable")
        self.keys = torch.from_numpy(keys[o]).to(device)
        self.rows = torch.from_numpy(rows[o]).to(device)

    def __call__(self, q: torch.Tensor) -> torch.Tensor:
        out = lookup_sorted(self.keys, self.rows, q.to(torch.int64))
        return torch.where(q >= 0, out, torch.full_like(out, -1))
