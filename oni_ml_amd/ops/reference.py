"""Pure-PyTorch reference implementations of the LDA hot ops.

The `torch` LDA backend: a vectorised Jacobi fixed-point E-step (every word's phi from one digamma
vector per variational iteration; the closed-form likelihood and lda-c's convergence rule) across
documents with per-document convergence masks, plus the suff-stats and M-step.  It is a test rehearsal
engine only -- the one whose multi-rank statistics can fold bitwise like one process
(ONI_DIST_DETERMINISTIC=chain, tests/test_sharded_pipeline.py).  The MI355X engine is the fp64 block
Gauss-Seidel of csrc/hip/lda_gs64.hip (kernels: gs_*.hip) and the CPU engine the lda-c Gauss-Seidel of
csrc/native/lda_ref.cpp; both are checked against lda_ref.cpp, not against this module.
"""
from __future__ import annotations

import math

import torch

from ..models.lda.special import digamma


def estep_jacobi(doc_ptr, word_idx, counts, beta, K, alpha, var_max_iter, var_conv, dtype=torch.float64,
                 chunk_docs=None):
    """Vectorised Jacobi variational E-step.

    Args:
      doc_ptr [D+1] int, word_idx [nnz] int, counts [nnz] float, beta [V, >=K]
      (exp log p(w|z), word-major).
    Returns dict(gamma [D,K], e [D,K], r [nnz], lik [D] f64, alpha_ss [D] f64, iters [D] int32).
    """
    dev = beta.device
    D = doc_ptr.numel() - 1
    nnz = word_idx.numel()
    doc_ptr = doc_ptr.to(dev, torch.int64)
    lens = doc_ptr[1:] - doc_ptr[:-1]
    doc_of = torch.repeat_interleave(torch.arange(D, device=dev), lens)
    widx = word_idx.to(dev, torch.int64)
    c = counts.to(dev, dtype)
    B = beta[:, :K].to(dtype)[widx]                       # [nnz, K]
    total = torch.zeros(D, dtype=torch.float64, device=dev).index_add_(0, doc_of, counts.to(dev, torch.float64))
    a = torch.tensor(float(alpha), dtype=dtype, device=dev)
    lc = math.lgamma(K * alpha) - K * math.lgamma(alpha)

    gam = (a + (total / K).to(dtype)).unsqueeze(1).expand(D, K).clone()
    psi = digamma(gam)
    e_last = torch.zeros(D, K, dtype=dtype, device=dev)
    r_last = torch.zeros(nnz, dtype=dtype, device=dev)
    lik = torch.zeros(D, dtype=torch.float64, device=dev)
    lik_old = torch.zeros(D, dtype=torch.float64, device=dev)
    conv = torch.ones(D, dtype=torch.float64, device=dev)
    iters = torch.zeros(D, dtype=torch.int32, device=dev)
    dsum_last = digamma(gam.sum(1)).to(torch.float64)
    active = torch.ones(D, dtype=torch.bool, device=dev)
    it = 0
    while True:
        cont = active & (conv > float(var_conv))
        if var_max_iter >= 0:
            cont &= iters < var_max_iter
        if not bool(cont.any()):
            break
        active = cont
        it += 1
        m = psi.max(1, keepdim=True).values
        E = torch.exp(psi - m)                               # [D,K]
        P = (E[doc_of] * B).sum(1).clamp_min(1e-30)          # [nnz]
        r = c / P
        acc = torch.zeros(D, K, dtype=dtype, device=dev).index_add_(0, doc_of, r.unsqueeze(1) * B)
        lsum = torch.zeros(D, dtype=torch.float64, device=dev).index_add_(0, doc_of, (c * torch.log(P)).double())
        gn = a + E * acc
        S = gn.sum(1)
        dS = digamma(S)
        pn = digamma(gn)
        y = pn - dS.unsqueeze(1)
        term = ((a - 1) * y + torch.lgamma(gn) - (gn - 1) * y + (gn - a) * (pn - psi)).double().sum(1)
        L = lc - torch.lgamma(S).double() + term + (lsum + m.squeeze(1).double() * total) - total * dS.double()
        cv = (lik_old - L) / lik_old
        act = active
        act2 = act.unsqueeze(1)
        gam = torch.where(act2, gn, gam)
        psi = torch.where(act2, pn, psi)
        e_last = torch.where(act2, E, e_last)
        r_last = torch.where(act[doc_of], r, r_last)
        lik = torch.where(act, L, lik)
        conv = torch.where(act, cv, conv)
        lik_old = torch.where(act, L, lik_old)
        dsum_last = torch.where(act, dS.double(), dsum_last)
        iters = iters + act.to(torch.int32)
    ass = psi.double().sum(1) - K * dsum_last
    return dict(gamma=gam, e=e_last, r=r_last, lik=lik, alpha_ss=ass, iters=iters)


def suffstats(doc_ptr, word_idx, e, r, beta, V, K):
    """class_word [V, K] = beta * scatter(E[doc] * r) (deterministic order not guaranteed)."""
    dev = e.device
    D = doc_ptr.numel() - 1
    lens = (doc_ptr[1:] - doc_ptr[:-1]).to(dev, torch.int64)
    doc_of = torch.repeat_interleave(torch.arange(D, device=dev), lens)
    contrib = e[doc_of][:, :K] * r.unsqueeze(1)
    s = torch.zeros(V, K, dtype=e.dtype, device=dev).index_add_(0, word_idx.to(dev, torch.int64), contrib)
    return beta[:, :K].to(e.dtype) * s


def mstep(cw, class_total, K):
    """beta = cw/ct where cw > 0 else exp(-100)."""
    ct = class_total[:K].to(cw.dtype)
    out = torch.where(cw[:, :K] > 0, cw[:, :K] / ct, torch.full_like(cw[:, :K], math.exp(-100.0)))
    return out


def score(theta, phi, K, dflt, doc_a, word_a, doc_b=None, word_b=None, tol=float("inf")):
    """Reference scorer: sequential (non-fused) multiply-add over topics, float64."""
    def one(d, w):
        n = d.numel()
        s = torch.zeros(n, dtype=torch.float64, device=d.device)
        th = torch.where((d >= 0).unsqueeze(1), theta[d.clamp_min(0), :K], torch.full((n, K), dflt, dtype=torch.float64, device=d.device))
        ph = torch.where((w >= 0).unsqueeze(1), phi[w.clamp_min(0), :K], torch.full((n, K), dflt, dtype=torch.float64, device=d.device))
        for k in range(K):
            s = s + th[:, k] * ph[:, k]
        return s

    sa = one(doc_a.long(), word_a.long())
    sb = one(doc_b.long(), word_b.long()) if doc_b is not None else None
    key = torch.minimum(sa, sb) if sb is not None else sa
    return sa, sb, key, (key < tol).to(torch.uint8)


def score_ensemble(theta, phi, R, K, dflt, doc_a, word_a, doc_b=None, word_b=None, tol=float("inf")):
    """Torch twin of ``ops.hip.score_ensemble`` (csrc/hip/score_ensemble.hip) on any device, bit for bit:
    ``(score_a, score_b|None, key, flag, votes)``.  ``theta`` [D, R, K] / ``phi`` [V, R, K]: the members'
    tables interleaved per row.  Member r's side scores are ``score`` on its tables; a side's ensemble score is
    ``(((0.0 + s_0) + s_1) + ... + s_{R-1}) / R``; ``votes`` counts the members whose own key is under ``tol``."""
    if theta.dim() != 3 or phi.dim() != 3 or tuple(theta.shape[1:]) != (R, K) or tuple(phi.shape[1:]) != (R, K):
        raise ValueError("score_ensemble: theta [D, R, K] and phi [V, R, K]")
    if (doc_b is None) != (word_b is None):
        raise ValueError("score_ensemble: doc_b and word_b go together")
    n = doc_a.numel()
    dev = doc_a.device
    two = doc_b is not None
    sum_a = torch.zeros(n, dtype=torch.float64, device=dev)
    sum_b = torch.zeros(n, dtype=torch.float64, device=dev) if two else None
    votes = torch.zeros(n, dtype=torch.uint8, device=dev)
    for r in range(R):
        sa, sb, _, _ = score(theta[:, r], phi[:, r], K, dflt, doc_a, word_a, doc_b, word_b, tol)
        sum_a = sum_a + sa
        if two:
            sum_b = sum_b + sb
        mk = torch.where(sa < sb, sa, sb) if two else sa       # the member's own key, a < b ? a : b as well
        votes = votes + (mk < tol).to(torch.uint8)
    ea = sum_a / float(R)
    eb = sum_b / float(R) if two else None
    key = torch.where(ea < eb, ea, eb) if two else ea      # the kernel's a < b ? a : b
    return ea, eb, key, (key < tol).to(torch.uint8), votes


def group_rows_sum(table, order, seg_start, seg_end, block=None):
    """Torch twin of ``ops.hip.group_rows_sum`` (csrc/hip/explain.hip) on any device, bit for bit: [G, W] float64,
    row g the sum of the rows ``table[order[seg_start[g] : seg_end[g]]]`` ([V, W] float64), column by column.
    The segment is cut into blocks of ``block`` members (``config.GROUP_BLOCK``); a block is summed from 0.0 in
    member order, the block sums are added from 0.0 in block order -- plain rounded adds.  (A step that a block or
    a segment does not have adds +0.0, which changes no bit of a sum that started at +0.0.)"""
    from ..config import GROUP_BLOCK
    GB = int(GROUP_BLOCK if block is None else block)
    if GB < 1:
        raise ValueError(f"group_rows_sum: block must be >= 1, got {GB}")
    if table.dim() != 2 or table.dtype != torch.float64:
        raise ValueError("group_rows_sum: table [V, W] float64")
    V, W = table.shape
    dev = table.device
    order = order.reshape(-1).to(torch.int64)
    s, e = seg_start.reshape(-1).to(torch.int64), seg_end.reshape(-1).to(torch.int64)
    G = s.numel()
    if e.numel() != G:
        raise ValueError("group_rows_sum: seg_start and seg_end differ in length")
    out = torch.zeros((G, W), dtype=torch.float64, device=dev)
    if G == 0:
        return out
    if int((e - s).min()) < 0 or int(s.min()) < 0 or int(e.max()) > order.numel():
        raise ValueError("group_rows_sum: segments outside the order")
    if order.numel() and (int(order.min()) < 0 or int(order.max()) >= V):
        raise ValueError("group_rows_sum: order out of range")
    nb = (e - s + (GB - 1)) // GB                                   # blocks of every segment
    B = int(nb.sum())
    if B == 0:
        return out
    seg = torch.repeat_interleave(torch.arange(G, device=dev), nb)          # the segment of every block
    first = torch.cumsum(nb, 0) - nb                                        # a segment's first block
    j = torch.arange(B, device=dev) - first[seg]                            # a block's number in its segment
    b_start = s[seg] + j * GB
    b_len = torch.minimum(e[seg] - b_start, torch.full_like(b_start, GB))
    part = torch.zeros((B, W), dtype=torch.float64, device=dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for m in range(int(b_len.max())):
        have = b_len > m
        rows = order[torch.where(have, b_start + m, torch.zeros_like(b_start))]
        part = part + torch.where(have.unsqueeze(1), table[rows], zero)
    for k in range(int(nb.max())):
        have = nb > k
        out = out + torch.where(have.unsqueeze(1), part[torch.where(have, first + k, torch.zeros_like(first))], zero)
    return out


def explain_sides(theta, phi, gsum, doc, word, grow, dflt):
    """Torch twin of ``ops.hip.explain_sides`` (csrc/hip/explain.hip) on any device, bit for bit:
    ``(cond float64 [n, F], why uint8 [n])``.  ``theta`` [D, R, K], ``phi`` [V, R, K], ``gsum`` [Gtot, R, K] (sums
    of phi rows over groups); ``doc`` / ``word`` [n] rows or -1, ``grow`` [n, F] gsum rows or -1.  With s the
    side's ``score_ensemble`` score and m_f the same expression over the row ``grow[:, f]`` of ``gsum`` in place of
    the phi row, ``cond[:, f] = s / m_f`` -- NaN where the side has no phi row or no group row; ``why`` is the
    lowest f with the lowest non-NaN cond, 255 when there is none.  A side without a document takes the default
    vector for theta."""
    if theta.dim() != 3 or phi.dim() != 3 or gsum.dim() != 3 or theta.shape[1:] != phi.shape[1:] \
            or gsum.shape[1:] != phi.shape[1:]:
        raise ValueError("explain_sides: theta [D, R, K], phi [V, R, K] and gsum [G, R, K]")
    if grow.dim() != 2 or grow.shape[0] != doc.numel() or word.numel() != doc.numel():
        raise ValueError("explain_sides: doc [n], word [n] and grow [n, F]")
    R, K = int(theta.shape[1]), int(theta.shape[2])
    n, F = grow.shape
    dev = doc.device
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    cond = torch.empty((n, F), dtype=torch.float64, device=dev)
    why = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    if n == 0:
        return cond, why
    has_w = word >= 0
    s = score_ensemble(theta, phi, R, K, dflt, doc, word.clamp_min(0))[0]
    best = torch.zeros(n, dtype=torch.float64, device=dev)
    for f in range(F):
        g = grow[:, f]
        if gsum.shape[0]:
            m = score_ensemble(theta, gsum, R, K, dflt, doc, g.clamp_min(0))[0]
        else:
            m = torch.ones_like(s)
        c = torch.where(has_w & (g >= 0), s / m, nan)
        cond[:, f] = c
        take = (c == c) & ((why == 255) | (c < best))      # '<': ties go to the lowest field
        best = torch.where(take, c, best)
        why = torch.where(take, torch.full_like(why, f), why)
    return cond, why


EXPECT_SLAB = 1 << 20      # (item, member) dots the expect twin holds at a time


def expect_sides(theta, phi, order, seg_start, seg_end, doc, word, grow, dflt, slab: int = EXPECT_SLAB):
    """Torch twin of ``ops.hip.expect_sides`` (csrc/hip/expect.hip) on any device, bit for bit, and the CPU
    pipeline's path: ``(best int32 [n, F], pbest float64 [n, F], above int32 [n, F])``.  ``theta`` [D, R, K],
    ``phi`` [V, R, K]; group g is the phi rows ``order[seg_start[g] : seg_end[g]]``; ``doc`` / ``word`` [n] rows or
    -1, ``grow`` [n, F] groups or -1.  For an item (pair i, field f) with a word and a group, p_v is the pair's
    ``score_ensemble`` score with member row v in place of the word -- taken from the ``score_ensemble`` twin itself,
    so s = p_word and every p_v are the scorer's bits -- ``best`` the member with the greatest p_v under ``>`` (a
    NaN never wins, ties to the lowest row, -0.0 and +0.0 tie; -1 without one), ``pbest`` its p_v (NaN without
    one), ``above`` the members with ``p_v > s``.  An item without a word or a group gets -1, NaN, -1.  Items are
    taken in slabs of at most ``slab`` member dots (a single longer group is a slab of its own)."""
    import bisect

    from . import sortgroup as SG
    if theta.dim() != 3 or phi.dim() != 3 or theta.shape[1:] != phi.shape[1:] or theta.dtype != torch.float64 \
            or phi.dtype != torch.float64:
        raise ValueError("expect_sides: theta [D, R, K] and phi [V, R, K] float64")
    if grow.dim() != 2 or grow.shape[0] != doc.numel() or word.numel() != doc.numel():
        raise ValueError("expect_sides: doc [n], word [n] and grow [n, F]")
    V, R, K = (int(x) for x in phi.shape)
    n, F = (int(x) for x in grow.shape)
    dev = theta.device
    order = order.reshape(-1).to(torch.int64)
    s0, e0 = seg_start.reshape(-1).to(torch.int64), seg_end.reshape(-1).to(torch.int64)
    G = s0.numel()
    if e0.numel() != G:
        raise ValueError("expect_sides: seg_start and seg_end differ in length")
    doc, word, g = doc.reshape(-1).to(torch.int64), word.reshape(-1).to(torch.int64), grow.reshape(-1).to(torch.int64)
    best = torch.full((n * F,), -1, dtype=torch.int32, device=dev)
    pbest = torch.full((n * F,), float("nan"), dtype=torch.float64, device=dev)
    above = torch.full((n * F,), -1, dtype=torch.int32, device=dev)
    out = lambda: (best.reshape(n, F), pbest.reshape(n, F), above.reshape(n, F))      # noqa: E731
    if n == 0:
        return out()
    if int(doc.max()) >= theta.shape[0] or int(doc.min()) < -1 or int(word.max()) >= V or int(word.min()) < -1 \
            or int(g.max()) >= G or int(g.min()) < -1:
        raise ValueError("expect_sides: doc, word or grow out of range")
    if G and (int(s0.min()) < 0 or int((e0 - s0).min()) < 0 or int(e0.max()) > order.numel()):
        raise ValueError("expect_sides: segments outside the order")
    if order.numel() and (int(order.min()) < 0 or int(order.max()) >= V):
        raise ValueError("expect_sides: order out of range")
    pair = torch.arange(n * F, device=dev, dtype=torch.int64) // F
    items = torch.nonzero((g >= 0) & (word[pair] >= 0)).reshape(-1)
    if items.numel() == 0:
        return out()
    lens = (e0 - s0)[g[items]]
    above[items] = 0      # a group without members: -1, NaN, 0
    ends = torch.cumsum(lens, 0).tolist()
    i0, done = 0, 0
    while i0 < items.numel():      # a slab: the items i0 .. i1 - 1
        i1 = max(i0 + 1, bisect.bisect_right(ends, done + int(slab), i0))
        it, ln = items[i0:i1], lens[i0:i1]
        done, i0 = ends[i1 - 1], i1
        tot = int(ln.sum())
        if tot == 0:
            continue
        of = SG.segment_ids(ln, tot)                                    # the slab item of every member dot
        first = torch.cumsum(ln, 0) - ln
        v = order[s0[g[it]][of] + torch.arange(tot, device=dev) - first[of]]
        d_it, w_it = doc[pair[it]], word[pair[it]]
        i32 = lambda t: t.to(torch.int32)      # noqa: E731
        p = score_ensemble(theta, phi, R, K, dflt, i32(d_it[of]), i32(v))[0]
        s = score_ensemble(theta, phi, R, K, dflt, i32(d_it), i32(w_it))[0]
        m = it.numel()
        cnt = torch.zeros(m, dtype=torch.int64, device=dev).index_add_(0, of, (p > s[of]).to(torch.int64))
        num = p == p
        # the greatest p_v: -0.0 and +0.0 are one value; a slab item without a number keeps -inf and no row
        pz = torch.where(p == 0, torch.zeros_like(p), p)
        top = torch.full((m,), float("-inf"), dtype=torch.float64, device=dev)
        top = top.scatter_reduce(0, of[num], pz[num], "amax", include_self=True)
        win = num & (pz == top[of])
        row = torch.full((m,), V, dtype=torch.int64, device=dev).scatter_reduce(0, of[win], v[win], "amin",
                                                                               include_self=True)
        has = row < V
        at = win & (v == row[of])                                       # the winner (a row listed twice: one value)
        pb = torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
        pb[of[at]] = p[at]
        best[it] = torch.where(has, row, torch.full_like(row, -1)).to(torch.int32)
        pbest[it] = pb
        above[it] = cnt.to(torch.int32)
    return out()


TAIL_SLAB = 1 << 22      # doubles of the [sides, V] slab the tail twin holds at a time


def tail_mass(theta, phi, doc, word, block=None, slab: int = TAIL_SLAB):
    """Torch twin of ``ops.hip.tail_mass`` (csrc/hip/tail_mass.hip) on any device, bit for bit, and the CPU
    pipeline's path: ``(le float64 [n], tot float64 [n], rarer int32 [n], ties int32 [n])``.  ``theta`` [D, R, K],
    ``phi`` [V, R, K]; ``doc`` / ``word`` [n] rows or -1.  For a side with both rows, p_v is its ``score_ensemble``
    score with phi row v in place of the word and s = p_w; the V rows are cut into blocks of ``block``
    (``config.TAIL_BLOCK``); within a block, from 0.0 in row order, ``le_b += p_v if p_v <= s else 0.0`` and
    ``tot_b += p_v``; the block sums are added from 0.0 in block order -- plain rounded adds.  (A row that the last
    block does not have adds +0.0, which changes no bit of a sum that started at +0.0.)  ``rarer`` / ``ties`` count
    ``p_v < s`` and ``p_v == s``; a NaN p_v enters neither count, enters ``le`` as 0.0 and makes ``tot`` NaN.  A
    side without a row gets NaN, NaN, -1, -1.  Sides are taken in batches of at most ``slab`` / V: the loops run
    over topic, then block position, then block."""
    from ..config import TAIL_BLOCK
    TB = int(TAIL_BLOCK if block is None else block)
    if TB < 1:
        raise ValueError(f"tail_mass: block must be >= 1, got {TB}")
    if theta.dim() != 3 or phi.dim() != 3 or theta.shape[1:] != phi.shape[1:] or theta.dtype != torch.float64 \
            or phi.dtype != torch.float64:
        raise ValueError("tail_mass: theta [D, R, K] and phi [V, R, K] float64")
    doc, word = doc.reshape(-1).to(torch.int64), word.reshape(-1).to(torch.int64)
    if doc.numel() != word.numel():
        raise ValueError("tail_mass: doc [n] and word [n]")
    V, R, K = phi.shape
    n = doc.numel()
    dev = theta.device
    le = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    tot = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    rarer = torch.full((n,), -1, dtype=torch.int32, device=dev)
    ties = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if n == 0:
        return le, tot, rarer, ties
    if int(doc.max()) >= theta.shape[0] or int(doc.min()) < -1 or int(word.max()) >= V or int(word.min()) < -1:
        raise ValueError("tail_mass: doc or word out of range")
    have = torch.nonzero((doc >= 0) & (word >= 0)).reshape(-1)
    nblk = -(-V // TB)
    pad = nblk * TB - V
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    step = max(1, int(slab) // max(V, 1))
    for b0 in range(0, have.numel(), step):
        rows = have[b0:b0 + step]
        th = theta[doc[rows]]                                           # [m, R, K]
        m = rows.numel()
        p = torch.zeros((m, V), dtype=torch.float64, device=dev)
        for r in range(R):
            acc = torch.zeros((m, V), dtype=torch.float64, device=dev)
            for k in range(K):
                acc = acc + th[:, r, k].unsqueeze(1) * phi[:, r, k].unsqueeze(0)      # rounded product, rounded sum
            p = p + acc
        if R != 1:      # x / 1.0 is x
            p = p / float(R)
        s = torch.gather(p, 1, word[rows].unsqueeze(1))                 # [m, 1]: p_w, so w counts itself
        rarer[rows] = (p < s).sum(1).to(torch.int32)
        ties[rows] = (p == s).sum(1).to(torch.int32)
        sel = torch.where(p <= s, p, zero)
        if pad:
            fill = torch.zeros((m, pad), dtype=torch.float64, device=dev)
            p, sel = torch.cat([p, fill], 1), torch.cat([sel, fill], 1)
        p, sel = p.reshape(m, nblk, TB), sel.reshape(m, nblk, TB)
        le_b = torch.zeros((m, nblk), dtype=torch.float64, device=dev)
        tot_b = torch.zeros((m, nblk), dtype=torch.float64, device=dev)
        for j in range(min(TB, V)):      # (one block: the positions past V hold the +0.0 of the padding)
            le_b = le_b + sel[:, :, j]
            tot_b = tot_b + p[:, :, j]
        le_s = torch.zeros(m, dtype=torch.float64, device=dev)
        tot_s = torch.zeros(m, dtype=torch.float64, device=dev)
        for b in range(nblk):
            le_s = le_s + le_b[:, b]
            tot_s = tot_s + tot_b[:, b]
        le[rows] = le_s
        tot[rows] = tot_s
    return le, tot, rarer, ties


PEERS_SLAB = 1 << 22      # doubles of the [queries, D] slab the peers twin holds at a time


def peer_topn(theta3, query, n, slab: int = PEERS_SLAB):
    """Torch twin of ``ops.hip.peer_topn`` (csrc/hip/peers.hip) on any device, bit for bit, and the CPU pipeline's
    path: ``(rows int32 [Q, n], dist float64 [Q, n], count int32 [Q])``.  ``theta3`` [D, R, K], its rows W = R K
    doubles; ``query`` [Q] rows.  L(q, p) is the L1 distance of rows q and p: from 0.0, for j = 0 .. W - 1 in order,
    ``t = theta[q, j] - theta[p, j]`` and ``acc = acc + |t|``, each rounded once.  The peers of q are the ``n``
    candidates p != q lowest in the order (L, p) ascending, listed in that order; a NaN L is never a peer;
    ``count`` is the number found, the slots past it hold -1 and +inf.  Queries are taken in batches of at most
    ``slab`` / D: a loop over j, then a stable ascending sort (equal distances stay in row order, torch puts NaN
    last), the query's own row made NaN first."""
    from ..config import PEERS_MAX
    n = int(n)
    if not 1 <= n <= PEERS_MAX:
        raise ValueError(f"peer_topn: n must be in [1, {PEERS_MAX}], got {n}")
    if theta3.dim() != 3 or theta3.dtype != torch.float64:
        raise ValueError("peer_topn: theta [D, R, K] float64")
    q = query.reshape(-1).to(torch.int64)
    D = int(theta3.shape[0])
    Q = q.numel()
    dev = theta3.device
    rows = torch.full((Q, n), -1, dtype=torch.int32, device=dev)
    dist = torch.full((Q, n), float("inf"), dtype=torch.float64, device=dev)
    count = torch.zeros(Q, dtype=torch.int32, device=dev)
    if Q == 0:
        return rows, dist, count
    if int(q.max()) >= D or int(q.min()) < 0:
        raise ValueError("peer_topn: query out of range")
    th = theta3.reshape(D, -1)
    m = min(n, D)
    step = max(1, int(slab) // D)
    for b0 in range(0, Q, step):
        qs = q[b0:b0 + step]
        own = th[qs]                                                    # [m, W]
        acc = torch.zeros((qs.numel(), D), dtype=torch.float64, device=dev)
        for j in range(th.shape[1]):
            acc = acc + (own[:, j].unsqueeze(1) - th[:, j].unsqueeze(0)).abs()      # rounded difference, rounded sum
        acc[torch.arange(qs.numel(), device=dev), qs] = float("nan")    # the query itself is no candidate
        sd, order = torch.sort(acc, dim=1, stable=True)
        found = (sd == sd).sum(1).clamp_max(n)
        live = torch.arange(m, device=dev).unsqueeze(0) < found.unsqueeze(1)
        rows[b0:b0 + step, :m] = torch.where(live, order[:, :m], torch.full_like(order[:, :m], -1)).to(torch.int32)
        dist[b0:b0 + step, :m] = torch.where(live, sd[:, :m], torch.full_like(sd[:, :m], float("inf")))
        count[b0:b0 + step] = found.to(torch.int32)
    return rows, dist, count


TOPIC_SLAB = 1 << 22      # doubles the topic report's twins hold at a time


def column_topn(table, n, slab: int = TOPIC_SLAB):
    """Torch twin of ``ops.hip.column_topn`` (csrc/hip/topic_report.hip) on any device, bit for bit, and the CPU
    pipeline's path: ``(rows int32 [W, n], vals float64 [W, n], count int32 [W])``.  Per column of ``table``
    [rows, W] float64 the ``n`` rows first in the total order (value descending under IEEE ``>``, row ascending):
    equal values, -0.0 and +0.0 among them, go to the lower row; a NaN is never listed; ``count`` is the number
    listed, the slots past it hold -1 and -inf.  The rows are taken in slabs of at most ``slab`` / W: a stable
    ascending sort of ``0.0 - value`` (both zeros become +0.0, equal keys stay in row order, torch puts NaN last),
    the slab's first ``n`` merged with the list so far, whose rows are all lower, by the same sort."""
    from ..config import TOPIC_REPORT_MAX
    n = int(n)
    if not 1 <= n <= TOPIC_REPORT_MAX:
        raise ValueError(f"column_topn: n must be in [1, {TOPIC_REPORT_MAX}], got {n}")
    if table.dim() != 2 or table.dtype != torch.float64:
        raise ValueError("column_topn: table [rows, W] float64")
    rows_n, W = (int(x) for x in table.shape)
    dev = table.device
    nan = float("nan")
    vals = torch.full((W, n), nan, dtype=torch.float64, device=dev)      # NaN: an empty slot, it sorts last
    rows = torch.full((W, n), -1, dtype=torch.int64, device=dev)
    step = max(1, int(slab) // max(W, 1))
    for r0 in range(0, rows_n if W else 0, step):
        x = table[r0:r0 + step].t()                                      # [W, m], a column's rows ascending
        m = min(n, int(x.shape[1]))
        order = torch.sort(0.0 - x, dim=1, stable=True)[1][:, :m]
        cand_v = torch.cat([vals, torch.gather(x, 1, order)], 1)         # the list's rows are below the slab's
        cand_r = torch.cat([rows, order + r0], 1)
        keep = torch.sort(0.0 - cand_v, dim=1, stable=True)[1][:, :n]
        vals, rows = torch.gather(cand_v, 1, keep), torch.gather(cand_r, 1, keep)
    live = vals == vals
    return (torch.where(live, rows, torch.full_like(rows, -1)).to(torch.int32),
            torch.where(live, vals, torch.full_like(vals, float("-inf"))), live.sum(1).to(torch.int32))


def row_dominant(table3, slab: int = TOPIC_SLAB):
    """Torch twin of ``ops.hip.row_dominant`` (csrc/hip/topic_report.hip) on any device:
    ``(arg int32 [rows, R], counts int64 [R, K])``.  ``arg``: the first k attaining the maximum of
    ``table3[row, r, :]`` ([rows, R, K] float64; a NaN never wins, -1 when every entry is NaN); ``counts``: the rows
    per (r, k).  Rows in slabs of at most ``slab`` / (R K): integers, no slab shows."""
    if table3.dim() != 3 or table3.dtype != torch.float64:
        raise ValueError("row_dominant: table [rows, R, K] float64")
    n, R, K = (int(x) for x in table3.shape)
    dev = table3.device
    arg = torch.full((n, R), -1, dtype=torch.int32, device=dev)
    counts = torch.zeros(R * K, dtype=torch.int64, device=dev)
    step = max(1, int(slab) // max(R * K, 1))
    base = (torch.arange(R, device=dev, dtype=torch.int64) * K).unsqueeze(0)
    for r0 in range(0, n if R * K else 0, step):
        t = table3[r0:r0 + step]
        best = torch.full(t.shape[:2], -1, dtype=torch.int64, device=dev)
        bv = torch.zeros(t.shape[:2], dtype=torch.float64, device=dev)
        for k in range(K):
            v = t[:, :, k]
            take = (v == v) & ((best < 0) | (v > bv))
            best = torch.where(take, torch.full_like(best, k), best)
            bv = torch.where(take, v, bv)
        arg[r0:r0 + step] = best.to(torch.int32)
        hit = best >= 0
        counts.index_add_(0, (best + base)[hit], torch.ones(int(hit.sum()), dtype=torch.int64, device=dev))
    return arg, counts.reshape(R, K)


def topic_sides(theta3, phi3, doc, word, slab: int = TOPIC_SLAB):
    """Torch twin of ``ops.hip.topic_sides`` (csrc/hip/topic_report.hip) on any device, bit for bit:
    ``(col int32 [n], resp float64 [n], host_share float64 [n], host_topic int32 [n])``.  ``theta3`` [D, R, K] /
    ``phi3`` [V, R, K]; ``doc`` / ``word``: the side's rows or -1.  Over the columns j = r K + k in order
    ``p_j = theta[d, j] * phi[w, j]``, one rounded product; ``col`` the first j with the greatest p_j (a NaN never
    wins); ``resp = p* / (s * R)`` with s the side's score as ``score_ensemble`` adds it (member sums in topic order
    from 0.0, the members in member order from 0.0, one division by R) -- one rounded multiply, exact at R = 1, and
    one rounded division; ``host_share = theta[d, col]``; ``host_topic`` the first k attaining the maximum of
    ``theta[d, col // K, :]``.  A side without a θ row or a φ row, or with NaN products only: -1, NaN, NaN, -1 (the
    default vector of a miss takes no part).  Sides in slabs of at most ``slab`` / (R K)."""
    if theta3.dim() != 3 or phi3.dim() != 3 or theta3.dtype != torch.float64 or phi3.dtype != torch.float64 or \
            tuple(theta3.shape[1:]) != tuple(phi3.shape[1:]):
        raise ValueError("topic_sides: theta [D, R, K] and phi [V, R, K] float64")
    D, R, K = (int(x) for x in theta3.shape)
    V = int(phi3.shape[0])
    d_all, w_all = doc.reshape(-1).to(torch.int64), word.reshape(-1).to(torch.int64)
    n = d_all.numel()
    dev = theta3.device
    if w_all.numel() != n:
        raise ValueError("topic_sides: doc and word differ in length")
    if n and (int(d_all.max()) >= D or int(d_all.min()) < -1):
        raise ValueError("doc: index out of range")
    if n and (int(w_all.max()) >= V or int(w_all.min()) < -1):
        raise ValueError("word: index out of range")
    nan = float("nan")
    col = torch.full((n,), -1, dtype=torch.int32, device=dev)
    resp = torch.full((n,), nan, dtype=torch.float64, device=dev)
    share = torch.full((n,), nan, dtype=torch.float64, device=dev)
    ht = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if n == 0 or D == 0 or V == 0 or R * K == 0:
        return col, resp, share, ht
    step = max(1, int(slab) // (R * K))
    for s0 in range(0, n, step):
        d, w = d_all[s0:s0 + step], w_all[s0:s0 + step]
        has = (d >= 0) & (w >= 0)
        tr = theta3[d.clamp_min(0)]                                      # [m, R, K]
        pr = phi3[w.clamp_min(0)]
        m = int(d.numel())
        best = torch.full((m,), -1, dtype=torch.int64, device=dev)
        bp = torch.zeros(m, dtype=torch.float64, device=dev)
        total = torch.zeros(m, dtype=torch.float64, device=dev)
        for r in range(R):
            s = torch.zeros(m, dtype=torch.float64, device=dev)
            for k in range(K):
                p = tr[:, r, k] * pr[:, r, k]                            # rounded product, then rounded sum
                s = s + p
                take = (p == p) & ((best < 0) | (p > bp))
                best = torch.where(take, torch.full_like(best, r * K + k), best)
                bp = torch.where(take, p, bp)
            total = total + s
        ok = has & (best >= 0)
        j = best.clamp_min(0)
        den = (total / float(R)) * float(R)
        own = torch.gather(tr, 1, (j // K).reshape(m, 1, 1).expand(m, 1, K)).reshape(m, 1, K)
        col[s0:s0 + step] = torch.where(ok, best, torch.full_like(best, -1)).to(torch.int32)
        resp[s0:s0 + step] = torch.where(ok, bp / den, torch.full_like(bp, nan))
        share[s0:s0 + step] = torch.where(ok, torch.gather(tr.reshape(m, R * K), 1, j.unsqueeze(1)).reshape(-1),
                                          torch.full_like(bp, nan))
        ht[s0:s0 + step] = torch.where(ok, row_dominant(own)[0].reshape(-1).to(torch.int64),
                                       torch.full_like(best, -1)).to(torch.int32)
    return col, resp, share, ht


MATCH_SLAB = 1 << 22      # doubles of the [blocks, Wa, Wb] partials the column_l1 twin holds at a time


def column_l1(A, B, ia=None, ib=None, block=None, slab: int = MATCH_SLAB):
    """Torch twin of ``ops.hip.column_l1`` (csrc/hip/column_l1.hip) on any device, bit for bit, and the CPU
    pipeline's path: float64 [Wa, Wb], ``C[a, b]`` = the sum over the M pairs of ``|A[ia[m], a] - B[ib[m], b]|``.
    ``A`` [Va, Wa] / ``B`` [Vb, Wb] float64; ``ia`` / ``ib`` [M] rows, both None: the identity (Va == Vb == M).
    The pairs are cut into blocks of ``block`` consecutive pairs (``config.MATCH_BLOCK``); within a block, from 0.0
    in pair order, one rounded subtraction, its magnitude, one rounded add; the block sums are added from 0.0 in
    block order.  A NaN difference (inf - inf among them) makes the sum NaN; M = 0 gives zeros.  The blocks are
    taken in slabs of at most ``slab`` / (Wa Wb): a loop over the position within the block (a position that a
    block does not have adds +0.0, which moves no bit of a sum that is never -0.0), then a loop over the slab's
    blocks in order, which continues the running sum."""
    from ..config import MATCH_BLOCK
    MB = int(MATCH_BLOCK if block is None else block)
    if MB < 1:
        raise ValueError(f"column_l1: block must be >= 1, got {MB}")
    for name, t in (("A", A), ("B", B)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float64:
            raise ValueError(f"column_l1: {name} must be a [rows, W] float64 tensor")
    if A.device != B.device:
        raise ValueError(f"column_l1: A on {A.device}, B on {B.device}")
    if (ia is None) != (ib is None):
        raise ValueError("column_l1: ia and ib go together")
    dev = A.device
    (Va, Wa), (Vb, Wb) = (int(x) for x in A.shape), (int(x) for x in B.shape)
    if ia is None:
        if Va != Vb:
            raise ValueError(f"column_l1: the identity form needs tables of equal height, got {Va} and {Vb}")
        M = Va
    else:
        ia, ib = ia.reshape(-1).to(torch.int64), ib.reshape(-1).to(torch.int64)
        M = ia.numel()
        if ib.numel() != M:
            raise ValueError("column_l1: ia and ib differ in length")
        if M and (int(ia.min()) < 0 or int(ia.max()) >= Va or int(ib.min()) < 0 or int(ib.max()) >= Vb):
            raise ValueError("column_l1: index out of range")
    out = torch.zeros((Wa, Wb), dtype=torch.float64, device=dev)
    if M == 0 or Wa == 0 or Wb == 0:
        return out
    nblk = -(-M // MB)
    step = max(1, int(slab) // (Wa * Wb))
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    for s0 in range(0, nblk, step):
        nb = min(step, nblk - s0)
        start = (s0 + torch.arange(nb, device=dev)) * MB
        b_len = torch.clamp(M - start, max=MB)
        part = torch.zeros((nb, Wa, Wb), dtype=torch.float64, device=dev)
        for m in range(int(b_len.max())):
            have = b_len > m
            pos = torch.where(have, start + m, torch.zeros_like(start))
            ra = A[pos if ia is None else ia[pos]]
            rb = B[pos if ib is None else ib[pos]]
            t = ra.unsqueeze(2) - rb.unsqueeze(1)                       # rounded difference, then rounded sum
            part = part + torch.where(have.reshape(nb, 1, 1), t.abs(), zero)
        for k in range(nb):
            out = out + part[k]
    return out


def select_lowest(key, flag, limit, with_count: bool = False):
    """Torch twin of ``ops.hip.select_lowest`` (csrc/hip/select_lowest.hip) on any device: the row indices
    (int64, ascending) of the ``limit`` flagged rows that a stable ascending sort of their keys puts first, all
    the flagged rows when there are fewer.  The kernels' plan from the sortgroup helpers: the cut key T is the
    m-th smallest order key of the flagged rows (m = min(limit, flagged rows)); a row is taken when its key is
    below T, or equals T with fewer than ``need`` = m - #{below T} flagged rows equal to T ahead of it.
    ``with_count``: also return the number of flagged rows."""
    import operator

    from . import sortgroup as SG
    limit = operator.index(limit)
    if limit < 1:
        raise ValueError(f"limit must be >= 1, got {limit}")
    if key.dim() != 1 or key.dtype != torch.float64 or flag.shape != key.shape:
        raise ValueError("select_lowest: key float64 [n], flag [n]")
    n = key.numel()
    dev = key.device
    on = flag.reshape(-1).to(torch.bool)
    rows = torch.arange(n, device=dev, dtype=torch.int64)
    flagged = int(on.to(torch.int64).sum()) if n else 0
    m = min(limit, flagged)
    if m == 0:
        out = torch.empty(0, dtype=torch.int64, device=dev)
        return (out, flagged) if with_count else out
    # unflagged rows sort last: no order key is the largest int64 (f64_order_keys makes every NaN the canonical one)
    ok = torch.where(on, SG.f64_order_keys(key), torch.full((n,), SG._LOW63, dtype=torch.int64, device=dev))
    T = SG.sort_stable(ok)[0][m - 1]
    lt = on & (ok < T)
    eq = on & (ok == T)
    need = m - int(lt.to(torch.int64).sum())
    ahead = torch.cumsum(eq.to(torch.int64), 0) - eq.to(torch.int64)      # flagged rows equal to T before this row
    out = SG.compact(rows, lt | (eq & (ahead < need)))[0]
    return (out, flagged) if with_count else out


def host_summary(doc_a, score_a, doc_b, score_b, num_docs, tol, max_blocks: int = 0):
    """Torch twin of ``ops.hip.host_summary`` (csrc/hip/host_summary.hip) on any device, same results:
    ``(events int64 [D], flagged int64 [D], min_score float64 [D], worst int64 [D], skipped int)``.

    From the sortgroup primitives, without atomics: the sides (side number ``2 i + side``) that name a document
    are sorted stably by order key (every NaN last) and then stably by document, which orders them by
    (document, order key, side number); run starts and a prefix sum give the counts per document, and the first
    side of every run is the document's lowest non-NaN score and the lowest side number that attains it (a NaN
    there: the document has none).  ``max_blocks`` is accepted and ignored (the kernel's launch cap)."""
    import operator

    from . import sortgroup as SG
    D = operator.index(num_docs)
    if D < 0 or D >= 1 << 31:
        raise ValueError(f"num_docs must be in [0, 2^31), got {D}")
    if not isinstance(max_blocks, int) or isinstance(max_blocks, bool) or max_blocks < 0:
        raise ValueError(f"max_blocks must be a non-negative int, got {max_blocks!r}")
    if (doc_b is None) != (score_b is None):
        raise ValueError("host_summary: doc_b and score_b go together")
    if doc_a.dim() != 1 or doc_a.dtype != torch.int32 or score_a.dtype != torch.float64 or score_a.shape != doc_a.shape:
        raise ValueError("host_summary: doc_a int32 [n], score_a float64 [n]")
    n = doc_a.numel()
    if n >= 1 << 31:
        raise ValueError(f"host_summary: {n} events, side numbers are 32-bit (n < 2^31)")
    two = doc_b is not None
    if two and (doc_b.dtype != torch.int32 or score_b.dtype != torch.float64 or doc_b.shape != doc_a.shape
                or score_b.shape != doc_a.shape):
        raise ValueError("host_summary: doc_b int32 [n], score_b float64 [n]")
    dev = doc_a.device
    if two:      # interleaved: position 2 i + side
        doc = torch.stack([doc_a, doc_b], 1).reshape(-1).to(torch.int64)
        sc = torch.stack([score_a, score_b], 1).reshape(-1)
    else:
        doc, sc = doc_a.to(torch.int64), score_a
    if n and (int(doc.max()) >= D or int(doc.min()) < -1):
        raise ValueError("host_summary: index out of range")
    events = torch.zeros(D, dtype=torch.int64, device=dev)
    flagged = torch.zeros(D, dtype=torch.int64, device=dev)
    min_score = torch.full((D,), float("inf"), dtype=torch.float64, device=dev)
    worst = torch.full((D,), -1, dtype=torch.int64, device=dev)
    num = torch.arange(doc.numel(), device=dev, dtype=torch.int64) * (1 if two else 2)      # side numbers
    num, _ = SG.compact(num, doc >= 0)
    skipped = doc.numel() - num.numel()
    if num.numel() == 0:
        return events, flagged, min_score, worst, skipped
    pos = num if two else num >> 1
    doc, sc = SG.gather(doc, pos), SG.gather(sc, pos)
    by_key = SG.sort_stable(SG.f64_order_keys(sc))[1]      # NaN (the canonical positive one) after +inf
    perm = SG.gather(by_key, SG.sort_stable(SG.gather(doc, by_key))[1])
    sd = SG.gather(doc, perm)
    grp, G = SG.run_ids(sd)
    st = SG.run_starts(grp, G)
    rows = SG.gather(sd, st[:-1])
    first = SG.gather(perm, st[:-1])
    s0 = SG.gather(sc, first)
    has = s0 == s0
    under = torch.cumsum(SG.gather((sc < tol).to(torch.int64), perm), 0)
    events.index_put_((rows,), st[1:] - st[:-1])
    flagged.index_put_((rows,), SG.diff_prepend0(SG.gather(under, st[1:] - 1)))
    min_score.index_put_((rows,), torch.where(has, s0, torch.full_like(s0, float("inf"))))
    worst.index_put_((rows,), torch.where(has, SG.gather(num, first), torch.full_like(first, -1)))
    return events, flagged, min_score, worst, skipped


def entropy_table(max_len: int):
    """t[c] = c log2(c) for c = 0 .. max_len as float64 (t[0] = t[1] = 0): the one table both
    ``string_entropy`` here and the HIP kernel (csrc/hip/string_entropy.hip) read, so neither side's log
    enters the comparison.  At least two entries."""
    import numpy as np
    c = np.arange(max(int(max_len), 1) + 1, dtype=np.float64)
    t = np.zeros_like(c)
    t[2:] = c[2:] * np.log2(c[2:])
    return t


ENTROPY_CHUNK_ROWS = 1 << 14     # rows per count matrix of string_entropy (x 256 int64: 32 MB)
ENTROPY_CHUNK_BYTES = 1 << 26    # and at most this many bytes per chunk (a row longer than it is a chunk)


def string_entropy(data, offsets, table=None):
    """Numpy twin of ``ops.hip.string_entropy`` (csrc/hip/string_entropy.hip), bit for bit: the Shannon entropy
    H = (t[n] - sum_b t[c_b]) / n of the bytes [offsets[i], offsets[i + 1]) of ``data`` (anything with the
    buffer protocol, or a uint8 array / tensor) for every i, float64 [len(offsets) - 1]; 0 for n <= 1.
    t = ``entropy_table`` of the longest string, c_b the count of the (unsigned) byte value b.

    Summation order (the kernel's): the 256 terms t[c_b] are taken in ascending byte value in 64 groups of
    four, each group summed left to right, ((t[c_4l] + t[c_4l+1]) + t[c_4l+2]) + t[c_4l+3]; the 64 group sums
    are then added as a balanced binary tree, neighbours first (x_0 + x_1, x_2 + x_3, ..., six levels).  Absent
    bytes contribute an exact +0.0.

    Rows are processed in chunks (ENTROPY_CHUNK_ROWS rows or ENTROPY_CHUNK_BYTES bytes, whichever is fewer
    rows), so a million rows never build an n x 256 matrix at once."""
    import numpy as np
    if torch.is_tensor(data):
        data = data.cpu().numpy()
    if torch.is_tensor(offsets):
        offsets = offsets.cpu().numpy()
    buf = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data.reshape(-1).view(np.uint8)
    off = np.asarray(offsets, np.int64).reshape(-1)
    n = off.size - 1
    if n < 0:
        raise ValueError("string_entropy: offsets must have n + 1 entries")
    out = np.zeros(max(n, 0), np.float64)
    if n == 0:
        return out
    lens = np.diff(off)
    if off[0] < 0 or (lens < 0).any() or off[-1] > buf.size:
        raise ValueError("string_entropy: offsets must be non-decreasing inside the bytes buffer")
    t = entropy_table(int(lens.max())) if table is None else np.asarray(table, np.float64)
    if t.size <= int(lens.max()):
        raise ValueError("string_entropy: the table is shorter than the longest string")
    lo = 0
    while lo < n:
        hi = min(n, lo + ENTROPY_CHUNK_ROWS)
        if off[hi] - off[lo] > ENTROPY_CHUNK_BYTES:
            hi = max(lo + 1, int(np.searchsorted(off, off[lo] + ENTROPY_CHUNK_BYTES, side="right")) - 1)
        m = hi - lo
        b0, b1 = int(off[lo]), int(off[hi])
        row = np.repeat(np.arange(m, dtype=np.int64), lens[lo:hi])
        cnt = np.bincount(row * 256 + buf[b0:b1], minlength=m * 256).reshape(m, 64, 4)
        x = t[cnt]
        s = ((x[:, :, 0] + x[:, :, 1]) + x[:, :, 2]) + x[:, :, 3]
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
        ln = lens[lo:hi]
        big = ln > 1
        h = np.zeros(m, np.float64)
        h[big] = (t[ln[big]] - s[big, 0]) / ln[big].astype(np.float64)
        out[lo:hi] = h
        lo = hi
    return out


def flow_words(hour, minute, second, port_a, port_b, ipkt, ibyt, time_cuts, ibyt_cuts, ipkt_cuts):
    """Torch transcription of csrc/hip/flow_words.hip (flow_pre_lda.scala:272-358)."""
    t = (hour + minute / 60) + second / 3600
    def nb(v, c):
        return (v.unsqueeze(-1) > c.to(v.device).unsqueeze(0)).sum(-1).to(torch.int8)
    dp, sp = port_a, port_b                    # reference names: dport = col 10, sport = col 11
    mn, mx = torch.minimum(dp, sp), torch.maximum(dp, sp)
    c2 = ((dp <= 1024) | (sp <= 1024)) & ((dp > 1024) | (sp > 1024)) & (mn != 0)
    c3 = ~c2 & (dp > 1024) & (sp > 1024)
    c4a = ~c2 & ~c3 & (dp == 0) & (sp != 0)
    c4b = ~c2 & ~c3 & ~c4a & (sp == 0) & (dp != 0)
    c1 = ~(c2 | c3 | c4a | c4b)
    wp = torch.where(c2, mn, torch.where(c3, torch.full_like(mn, 333333.0), torch.where(
        c4a, sp, torch.where(c4b, dp, torch.where(mn == 0, mx, torch.full_like(mn, 111111.0))))))
    pc = torch.where(c2, 2, torch.where(c3, 3, torch.where(c4a | c4b, 4, 1))).to(torch.int8)
    # the reference's if / else-if chain for the "-1_" side
    r1 = c2 & (dp < sp)
    r2 = ~r1 & c2 & (sp < dp)
    r3 = ~r1 & ~r2 & (pc == 4) & (dp == 0)
    r4 = ~r1 & ~r2 & ~r3 & (pc == 4) & (sp == 0)
    dpre = r1 | r4
    spre = r2 | r3
    return dict(time=t, time_bin=nb(t, time_cuts), ibyt_bin=nb(ibyt, ibyt_cuts), ipkt_bin=nb(ipkt, ipkt_cuts),
                word_port=wp, p_case=pc, src_prefix=spre.to(torch.int8), dst_prefix=dpre.to(torch.int8))


# ---------------------------------------------------------------------------------------------- --holdout
_M64 = (1 << 64) - 1


def _as_i64(x: int) -> int:
    """The 64 bits of a Python int as the signed value an int64 tensor holds."""
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def splitmix64_int(x: int) -> int:
    """csrc/common/splitmix64.h on a Python int (unsigned 64-bit)."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _lsr(x, n: int):
    """Logical shift right of the 64 bits an int64 tensor holds."""
    return (x >> n) & ((1 << (64 - n)) - 1)


def splitmix64(x):
    """csrc/common/splitmix64.h on an int64 tensor, bit for bit (the adds and products wrap, the shifts are
    logical)."""
    x = x + _as_i64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _as_i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _as_i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def holdout_key(seed: int) -> int:
    """The draw's key: splitmix64(seed ^ config.HOLDOUT_SALT), unsigned."""
    from ..config import HOLDOUT_SALT
    return splitmix64_int((int(seed) ^ HOLDOUT_SALT) & _M64)


def holdout_thr(F: float) -> int:
    """int(F * 2**53): exact (a double times a power of two), the integer the draw compares with."""
    return int(float(F) * float(1 << 53))


def check_holdout_draw(doc_ptr, counts, seed, thr):
    """The value checks of ``holdout_draw`` (kernel wrapper and twin alike); host reads.  Returns the token total."""
    import operator
    operator.index(seed)
    thr = operator.index(thr)
    if not 0 < thr <= 1 << 52:
        raise ValueError(f"holdout_draw: thr must be in (0, 2^52], got {thr}")
    for name, x in (("doc_ptr", doc_ptr), ("counts", counts)):
        if not isinstance(x, torch.Tensor) or x.dim() != 1 or x.dtype != torch.int64:
            raise ValueError(f"{name}: expected a 1-D int64 tensor")
        if not x.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
    if counts.device != doc_ptr.device:
        raise ValueError(f"counts: on {counts.device}, expected {doc_ptr.device} (doc_ptr's device)")
    nnz = counts.numel()
    if nnz >= 1 << 31:
        raise ValueError(f"holdout_draw: {nnz} entries (nnz < 2^31)")
    if doc_ptr.numel() < 1 or int(doc_ptr[0]) != 0 or int(doc_ptr[-1]) != nnz:
        raise ValueError("doc_ptr: must start at 0 and end at the number of entries")
    if doc_ptr.numel() > 1 and int((doc_ptr[1:] - doc_ptr[:-1]).min()) < 0:
        raise ValueError("doc_ptr: must be non-decreasing")
    if nnz and int(counts.min()) < 0:
        raise ValueError("counts: must be >= 0")
    total = int(counts.sum()) if nnz else 0
    if total >= 1 << 62:
        raise ValueError(f"holdout_draw: {total} tokens (< 2^62)")
    return total


def holdout_rules(doc_ptr, counts, t, min_tokens=None):
    """The two document rules on a raw draw ``t`` (int64 [nnz]), on any device, from int64 prefix sums and gathers
    (``ops.sortgroup``): a document of fewer than ``config.HOLDOUT_MIN_TOKENS`` tokens is not split, and a document
    all of whose tokens were drawn gets them all back -- t = 0 on all its entries either way."""
    from ..config import HOLDOUT_MIN_TOKENS
    from . import sortgroup as SG
    mt = int(HOLDOUT_MIN_TOKENS if min_tokens is None else min_tokens)
    nnz = counts.numel()
    if nnz == 0:
        return t
    dev = counts.device

    def doc_sums(x):
        cs = torch.zeros(nnz + 1, dtype=torch.int64, device=dev)
        cs[1:] = torch.cumsum(x, 0)
        return SG.gather(cs, doc_ptr[1:]) - SG.gather(cs, doc_ptr[:-1])
    d_all, d_out = doc_sums(counts), doc_sums(t)
    split = (d_all >= mt) & (d_out < d_all)
    doc_of = SG.segment_ids(doc_ptr[1:] - doc_ptr[:-1], total=nnz)
    return torch.where(SG.gather(split, doc_of), t, torch.zeros_like(t))


def holdout_draw(doc_ptr, counts, seed, thr, rules: bool = True, chunk: int = 1 << 22):
    """Torch twin of ``ops.hip.holdout_draw`` (csrc/hip/holdout.hip) on any device, bit for bit: int64 [nnz], the
    held-out tokens of every CSR entry.  Token j of entry e has the global index g = base[e] + j (base: the
    exclusive prefix sum of ``counts``) and is held out iff ``splitmix64(key ^ g) >> 11 < thr`` with
    ``key = holdout_key(seed)`` -- integers only.  ``rules``: then ``holdout_rules`` (False: the raw draw).
    The tokens are walked ``chunk`` at a time."""
    total = check_holdout_draw(doc_ptr, counts, seed, thr)
    dev = counts.device
    t = torch.zeros(counts.numel(), dtype=torch.int64, device=dev)
    if total:
        ends = torch.cumsum(counts, 0)
        key = _as_i64(holdout_key(seed))
        for a in range(0, total, int(chunk)):
            g = torch.arange(a, min(total, a + int(chunk)), dtype=torch.int64, device=dev)
            ent = torch.searchsorted(ends, g, right=True)      # the first entry that ends past g
            hit = _lsr(splitmix64(g ^ key), 11) < int(thr)
            t.index_add_(0, ent, hit.to(torch.int64))
    return holdout_rules(doc_ptr, counts, t) if rules else t


_LOG_RN_C = [2.0 / (2 * i + 3) for i in range(11)]
_LOG_RN_LN2_HI = 6.93147180369123816490e-01
_LOG_RN_LN2_LO = 1.90821492927058770002e-10


def log_rn(y):
    """Natural log of a positive float64 tensor from correctly rounded operations in a fixed order, the torch twin
    of csrc/hip/holdout.hip ``log_rn`` bit for bit (within 2 ulp of ``numpy.log`` on [1e-300, 2]): frexp to
    m in [0.5, 1) and e; m < sqrt(1/2): m doubled, e - 1; f = (m - 1) / (m + 1), s = f f; P by Horner over
    c_i = 2 / (2 i + 3), i = 10 .. 0, a rounded product then a rounded sum per step; r = (f s) P + (f + f);
    r = e ln2_lo + r; e ln2_hi + r."""
    m, e = torch.frexp(y)
    low = m < 0.70710678118654752
    m = torch.where(low, m + m, m)
    e = torch.where(low, e - 1, e)
    f = (m - 1.0) / (m + 1.0)
    s = f * f
    P = torch.full_like(s, _LOG_RN_C[10])
    for i in range(9, -1, -1):
        P = P * s
        P = P + _LOG_RN_C[i]
    r = (f * s) * P + (f + f)
    ed = e.to(torch.float64)
    r = ed * _LOG_RN_LN2_LO + r
    return ed * _LOG_RN_LN2_HI + r


def holdout_entries(theta, phi, doc, word, t, word_seen, chunk: int = 1 << 20):
    """Torch twin of ``ops.hip.holdout_entries`` (csrc/hip/holdout.hip) on any device, bit for bit: float64 [n],
    ``t[e] * log_rn(theta[doc[e]] . phi[word[e]])`` for an entry with ``t[e] > 0`` whose word has a training entry
    (``word_seen[word[e]] != 0``), else 0.0.  The dot is ``score``'s: a rounded product and a rounded sum per topic,
    from 0.0."""
    if theta.dim() != 2 or phi.dim() != 2 or theta.shape[1] != phi.shape[1] or theta.shape[1] < 1:
        raise ValueError("holdout_entries: theta [D, K] and phi [V, K]")
    n = doc.numel()
    if word.numel() != n or t.numel() != n or word_seen.numel() != phi.shape[0]:
        raise ValueError("holdout_entries: doc [n], word [n], t [n] and word_seen [V]")
    K = int(theta.shape[1])
    out = torch.zeros(n, dtype=torch.float64, device=theta.device)
    for a in range(0, n, int(chunk)):
        b = min(n, a + int(chunk))
        d, w, tt = doc[a:b].long(), word[a:b].long(), t[a:b]
        s = score(theta, phi, K, 0.0, d, w)[0]
        use = (tt > 0) & (word_seen[w] != 0)
        out[a:b] = torch.where(use, tt.to(torch.float64) * log_rn(s), torch.zeros_like(s))
    return out
