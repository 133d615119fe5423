"""The native engine plan (csrc/native/engine_plan.cpp) against the Python planners, array for array (no GPU).

Every array and count the native planner writes equals what GSPlan, SuffPlan, GSStage, gs_chunk_sums and
LDAEngine._build_suff_split derive from the same corpus; the per-document tables behind et_row give
gs_et_rows' result on the late slots of csc_subset (the CPU twins of the device partition).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import engine_plan_cases as C  # noqa: E402

from oni_ml_amd.models.lda import em as EM  # noqa: E402
from oni_ml_amd.ops import hip as H  # noqa: E402


def _np(t):
    return t.cpu().numpy()


def assert_plan_equal(p, ref, c):
    """Host plan ``p`` (LDAEngine.host_plan) against the Python planners' bare engine ``ref``."""
    dc, KS = ref.dc, ref.KS
    for name, dtype, want in (("doc_ptr", np.int32, dc.doc_ptr), ("word_idx", np.int32, dc.word_idx),
                              ("counts", np.float32, dc.counts), ("word_ptr", np.int32, dc.word_ptr)):
        got = C.section(p, name, dtype)
        assert got.dtype == _np(want).dtype and np.array_equal(got, _np(want)), name
    assert p["doc_len"].dtype == np.int64 and np.array_equal(p["doc_len"], dc.doc_len)
    assert p["word_len"].dtype == np.int64 and np.array_equal(p["word_len"], dc.word_len)
    # buckets
    plan = ref.gs_plan.plan
    assert [v for v, _, _ in p["buckets"]] == [v for v, _ in plan]
    for i, ((_, off, n), (_, order)) in enumerate(zip(p["buckets"], plan)):
        assert off % 256 == 0
        assert np.array_equal(p["buf"][off:off + 4 * n].view(np.int32), _np(order)), f"bucket {i}"
    # suff-stats plans
    def suff(name, counts, sp):
        assert np.array_equal(C.section(p, name, np.int32), _np(sp.order)), name
        assert tuple(counts) == (sp.n_heavy, sp.n_medium, sp.n_light), name
    suff("suff_order", p["suff_counts"][0], ref.suff_plan)
    ss = ref._suff_split
    assert p["split"] == (ss is not None)
    if ss is not None:
        suff("suff_order_early", p["suff_counts"][1], ss["planE"])
        suff("suff_order_late", p["suff_counts"][2], ss["planL"])
        o = _np(plan[0][1])
        mask = np.zeros(c.num_docs, np.uint8)
        mask[o[o >= 0]] = 1
        assert np.array_equal(C.section(p, "late_mask", np.uint8), mask)
        assert (p["n_early"], p["n_late"], p["late_docs"]) == (ss["ceE"].numel(), ss["ceL"].numel(), ss["late_docs"])
        assert p["defer"] == ("et_row" in ss)
        if p["defer"]:
            keep = mask[_np(dc.csc_doc)].astype(bool)
            assert np.array_equal(_np(dc.csc_ent)[keep], _np(ss["ceL"]))            # the twin's late list
            rows = C.host_et_rows(p, _np(dc.csc_ent)[keep], _np(dc.csc_doc)[keep], H.GS_LDS_UMAX)
            assert np.array_equal(rows, _np(ss["et_row"]))
    else:
        assert not p["defer"] and "late_mask" not in p["sections"]
    # per-document tables of the team8 bucket
    o8 = [o for v, o in plan if v == H.GS_TEAM8]
    st = ref._stages.get(id(o8[0])) if o8 else None
    assert p["staged"] == (st is not None)
    if st is not None:
        assert p["n_tiles"] == st.n_tiles
        for name, dtype, want in (("stage_tile_ent", np.int32, st.tile_ent), ("stage_tile_cnt", np.int32, st.tile_cnt),
                                  ("stage_off", np.int64, st.stage_off)):
            assert np.array_equal(C.section(p, name, dtype), _np(want)), name
    assert p["csum"] == bool(o8) == bool(ref._csums)
    if o8:
        got = C.section(p, "csum", np.float64).reshape(-1, H.GS_LDS_UMAX)
        assert np.array_equal(got, _np(ref._csums[id(o8[0])]))


def _check(c, KS, U, suff_split="auto", defer_final=True):
    ref = C.python_plans(c, KS, U, suff_split, defer_final)
    p = C.bare_engine(c, KS, U, suff_split, defer_final).host_plan(c, KS)
    assert p["bytes"] <= p["buf"].size
    assert_plan_equal(p, ref, c)
    return p, ref


@pytest.mark.parametrize("KS,U", C.SETTINGS)
def test_edge_corpus(KS, U):
    """Bucket edges from both sides, equal lengths, empty documents at both ends, words on both sides of the
    heavy / light bounds, counts of 2^31 through one chunk."""
    c = C.edge_corpus()
    wl = np.bincount(c.word_idx, minlength=c.num_terms)
    assert tuple(wl[:6]) == C.WORD_LENGTHS
    p, ref = _check(c, KS, U)
    assert [v for v, _ in ref.gs_plan.plan] == [H.GS_TEAM8, H.GS_TEAM4, H.GS_TEAM1, H.GS_SMALL, H.GS_TINY]
    assert p["split"] and p["defer"] and p["staged"]
    cs = C.section(p, "csum", np.float64)
    # the 129 counts of 2^31 lie in the first chunk at either U; the sums are whole numbers, exact in fp64
    assert cs.max() >= 2.0**31 * 129 and cs.max() == cs[0] and (cs == np.floor(cs)).all()
    _check(c, KS, U, "off")
    _check(c, KS, U, "auto", defer_final=False)


@pytest.mark.parametrize("n8", [0, 1, 8, 9])
def test_team8_documents(n8):
    """0, 1, 8 and 9 team8 documents: the empty slots isolate_longest leaves (8 fill a round and leave none)."""
    p, ref = _check(C.team8_corpus(n8), 20, 32, "force")
    o8 = [o.numpy() for v, o in ref.gs_plan.plan if v == H.GS_TEAM8]
    assert len(o8) == (n8 > 0)
    if n8:
        assert (o8[0] < 0).sum() == (1 if n8 == 9 else 0) and (o8[0] >= 0).sum() == n8
    assert p["defer"] == (n8 > 0)


def test_late_share_rule():
    """A late bucket over 60 % of the entries: no split; the same corpus forced: split."""
    c = C.late_heavy_corpus()
    p, _ = _check(c, 20, 32, "auto")
    assert not p["split"]
    p, _ = _check(c, 20, 32, "force")
    assert p["split"] and p["defer"] and p["n_late"] == 2100


def test_one_bucket_and_empty():
    p, _ = _check(C.one_bucket_corpus(), 20, 32, "force")
    assert not p["split"] and len(p["buckets"]) == 1
    p, _ = _check(C.empty_corpus(), 20, 32)
    assert [v for v, _, _ in p["buckets"]] == [H.GS_TINY] and not p["split"]


def test_stage_budget_one_tile_short(monkeypatch):
    """A budget one tile below the staged rows' bytes leaves the plan unstaged; the exact bytes stage it."""
    c, KS = C.team8_corpus(1), 20
    need = -(-2049 // 64) * 64 * KS * 8
    monkeypatch.setattr(EM, "_stage_budget_gb", lambda v: (need - 64 * KS * 8) / 2**30)
    p, _ = _check(c, KS, 32)
    assert not p["staged"] and p["csum"]
    monkeypatch.setattr(EM, "_stage_budget_gb", lambda v: need / 2**30)
    p, _ = _check(c, KS, 32)
    assert p["staged"] and p["n_tiles"] == 33
    monkeypatch.setattr(EM, "_stage_budget_gb", lambda v: 0.0)
    p, _ = _check(c, KS, 32)
    assert not p["staged"]


def test_buffer_too_small_and_bad_input():
    from oni_ml_amd.ops import native
    c = C.team8_corpus(1)
    eng = C.bare_engine(c, 20, 32)
    def aligned(n):
        raw = np.zeros(n + 256, np.uint8)
        a = (-raw.ctypes.data) % 256
        return raw[a:a + n]

    with pytest.raises(Exception, match="buffer too small"):
        eng.host_plan(c, 20, take=lambda n: aligned(4096))
    with pytest.raises(Exception, match="256-byte aligned"):
        eng.host_plan(c, 20, take=lambda n: aligned(n + 1)[1:])
    th = H.engine_plan_thresholds(20, 32)
    buf = aligned(1 << 20)
    kw = dict(late_share=0.6, suff_split="auto", stage_cap=0.0, defer_final=True, **th)
    bad = c.word_idx.copy()
    bad[5] = c.num_terms
    with pytest.raises(Exception, match="word index"):
        native.engine_plan(c.doc_ptr, bad, c.counts, c.num_terms, 20, 32, buf, **kw)
    ptr = c.doc_ptr.copy()
    ptr[3] = ptr[2] - 1
    with pytest.raises(Exception, match="doc_ptr"):
        native.engine_plan(ptr, c.word_idx, c.counts, c.num_terms, 20, 32, buf, **kw)


def test_eligibility(monkeypatch):
    """KS = 52, U = 64 and a c.phi window are not eligible: the Python planners stay in place; so does
    engine_plan="python", a split-document plan and a CPU device."""
    c = C.one_bucket_corpus()

    def eligible(KS=20, U=32, cwin=None, device="cuda", mode="native"):
        eng = C.bare_engine(c, KS, U, device=device)
        eng._cwin, eng.engine_plan = cwin, mode
        return eng._plan_native(KS)

    assert eligible()
    assert eligible(8, 8) and eligible(32, 32)
    assert not eligible(KS=52)
    assert not eligible(U=64)
    assert not eligible(cwin=[dict(d0=0, d1=5, e0=0, e1=c.nnz)])
    assert not eligible(device="cpu")
    monkeypatch.setenv("ONI_GS_SPLIT_MIN", "4096")
    assert not eligible()
    monkeypatch.delenv("ONI_GS_SPLIT_MIN")
    assert eligible() and not eligible(mode="python")
    from oni_ml_amd.models.lda.em import LDAEngine
    with pytest.raises(ValueError, match="engine_plan"):
        LDAEngine(c, 20, backend="cpu", engine_plan="fast")
