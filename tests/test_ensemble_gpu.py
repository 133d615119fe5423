"""--ensemble R on the GPU (gfx950): ``ops.hip.score_ensemble`` (csrc/hip/score_ensemble.hip) bit for bit the torch
twin in all five outputs over member counts x topic counts (odd K: the scalar loop; K = 20: the unrolled double2
loop; K = 2 and 16: the double2 loop over a run-time K) x one and two sides x tolerances, misses, a NaN row and a
-0.0 row included; tables that start 8 bytes off a 16-byte boundary (the scalar loop at an even K); R = 1 against
``score_events``; the grid-stride loop wrapping; n = 0 and 1; the wrapper's refusals; and a flow, a DNS and a proxy day on the HIP
backend."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal, tree, twin_scores_of_file  # noqa: E402

from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

pytestmark = pytest.mark.gpu

N, D, V = 1031, 37, 53
DFLT = 0.05
# every instantiation of the launcher: odd K (1, 3, 33) the scalar loop, K = 20 the unrolled double2 loop, any
# other even K (2, 16) the double2 loop over a run-time K
KS = [1, 2, 3, 16, 20, 33]


def edge_batch(R_, K, two, n=N, seed=0):
    """(theta [D, R, K], phi [V, R, K], doc_a, word_a, doc_b | None, word_b | None) on the CPU, seeded: about a
    tenth of the rows of each index are -1 (so either or both of a side's), document row 5 holds a NaN in its
    last member and word row 7 a -0.0 in its first."""
    g = torch.Generator().manual_seed(1000 * R_ + 10 * K + seed)
    th = torch.rand(D, R_, K, dtype=torch.float64, generator=g)
    ph = torch.rand(V, R_, K, dtype=torch.float64, generator=g) * 1e-2
    th[5, R_ - 1, K - 1] = float("nan")
    ph[7, 0, 0] = -0.0

    def idx(rows, pin):
        x = torch.randint(0, rows, (n,), generator=g, dtype=torch.int32)
        x[torch.rand(n, generator=g) < 0.1] = -1
        x[:min(n, 4)] = torch.tensor([pin, -1, pin, -1], dtype=torch.int32)[:min(n, 4)]
        return x

    def side():
        d, w = idx(D, 5), idx(V, 7)
        if n >= 4:
            w[1], w[2] = 7, -1      # rows 0-3: both special rows, word alone, document alone, both missing
        return d, w
    return (th, ph) + side() + (side() if two else (None, None))


def tols(R_, K):
    """0 (nothing under it), a mid quantile of the one-sided keys, +inf (everything that is not NaN)."""
    th, ph, da, wa, _, _ = edge_batch(R_, K, False)
    key = R.score_ensemble(th, ph, R_, K, DFLT, da, wa)[2]
    return [0.0, float(torch.nanquantile(key, 0.4)), float("inf")]


def same5(got, want):
    assert len(got) == len(want) == 5
    assert [None if t is None else t.dtype for t in got] == [None if t is None else t.dtype for t in want]
    for name, g, w in zip(("score_a", "score_b", "key", "flag", "votes"), got, want):
        assert bits_equal(None if g is None else g.cpu(), w), name


def cuda(args):
    return [None if t is None else t.cuda() for t in args]


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("R_", [1, 2, 3, 8])
def test_kernel_equals_the_twin(hip, R_, K, two):
    args = edge_batch(R_, K, two)
    assert (args[2] < 0).sum() > N // 20 and ((args[2] < 0) & (args[3] < 0)).any()
    for tol in tols(R_, K):
        want = R.score_ensemble(args[0], args[1], R_, K, DFLT, *args[2:], tol=tol)
        got = hip.score_ensemble(*cuda(args[:2]), R_, K, DFLT, *cuda(args[2:]), tol)
        assert all(t is None or t.is_cuda for t in got)
        same5(got, want)
        assert torch.isnan(want[0]).any() and want[4].dtype == torch.uint8
        if tol == 0.0:
            assert int(want[3].sum()) == 0 and int(want[4].sum()) == 0
        elif tol == float("inf"):
            assert int(want[4].max()) == R_ and int(want[3].sum()) == int((~torch.isnan(want[2])).sum())
        else:
            assert 0 < int(want[3].sum()) < N and (R_ == 1 or len(set(want[4].tolist())) > 2)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("K", KS)
def test_one_member_is_score_events(hip, K, two):
    th, ph, da, wa, db, wb = cuda(edge_batch(1, K, two))
    tol = tols(1, K)[1]
    want = hip.score_events(th[:, 0].contiguous(), ph[:, 0].contiguous(), K, DFLT, da, wa, db, wb, tol)
    got = hip.score_ensemble(th, ph, 1, K, DFLT, da, wa, db, wb, tol)
    for g, w in zip(got[:4], want):
        assert bits_equal(None if g is None else g.cpu(), None if w is None else w.cpu())
    assert torch.equal(got[4], want[3])
    # the scorer's dispatcher: int64 rows as the pipelines hold them, votes on the model
    m = S.EnsembleModel(th, ph, 1, K, DFLT)
    out = S.score_votes(m, da.long(), wa.long(), None if db is None else db.long(), None if wb is None else wb.long(),
                        tol)
    for g, w in zip(out[:4], want):
        assert bits_equal(None if g is None else g.cpu(), None if w is None else w.cpu())
    assert torch.equal(out[4], want[3])


@pytest.mark.parametrize("K", [2, 16, 20])
@pytest.mark.parametrize("off", ["theta", "phi", "both"])
def test_tables_off_the_16_byte_boundary(hip, K, off):
    """A contiguous table whose first double sits 8 bytes past a 16-byte boundary cannot be read as double2: the
    launcher takes the scalar loop, and the result is the same bits."""
    R_ = 3
    args = edge_batch(R_, K, True)
    tol = tols(R_, K)[1]
    want = R.score_ensemble(args[0], args[1], R_, K, DFLT, *args[2:], tol=tol)
    g = cuda(args)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, dtype=torch.float64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 8
        return v
    th = shifted(g[0]) if off in ("theta", "both") else g[0]
    ph = shifted(g[1]) if off in ("phi", "both") else g[1]
    same5(hip.score_ensemble(th, ph, R_, K, DFLT, *g[2:], tol), want)


@pytest.mark.parametrize("R_,K", [(3, 20), (8, 3), (2, 16)])
def test_grid_stride_wraps(hip, R_, K):
    """2 workgroups over 3,000 events: every lane goes round six times."""
    args = edge_batch(R_, K, True, n=3000)
    tol = tols(R_, K)[1]
    want = R.score_ensemble(args[0], args[1], R_, K, DFLT, *args[2:], tol=tol)
    g = cuda(args)
    same5(hip.score_ensemble(g[0], g[1], R_, K, DFLT, *g[2:], tol, max_blocks=2), want)
    same5(hip.score_ensemble(g[0], g[1], R_, K, DFLT, *g[2:], tol), want)


@pytest.mark.parametrize("two", [False, True])
def test_no_event_and_one_event(hip, two):
    for n in (0, 1):
        args = edge_batch(3, 20, two, n=n)
        g = cuda(args)
        got = hip.score_ensemble(g[0], g[1], 3, 20, DFLT, *g[2:], 1.0)
        want = R.score_ensemble(args[0], args[1], 3, 20, DFLT, *args[2:], tol=1.0)
        same5(got, want)
        assert [None if t is None else tuple(t.shape) for t in got] == [(n,), (n,) if two else None, (n,), (n,), (n,)]
        assert got[3].dtype == torch.uint8 and got[4].dtype == torch.uint8 and got[0].is_cuda


def test_wrapper_accepts_what_the_refusals_below_vary(hip):
    """The positive control of the next test: the same arguments, unspoilt, launch and agree with the twin."""
    args = edge_batch(3, 20, True, n=65)
    g = cuda(args)
    same5(hip.score_ensemble(g[0], g[1], 3, 20, DFLT, *g[2:], 0.01, max_blocks=2),
          R.score_ensemble(args[0], args[1], 3, 20, DFLT, *args[2:], tol=0.01))


def test_wrapper_refuses_bad_arguments_before_any_launch(hip):
    """Host-side checks only: every call below raises ValueError before a launch."""
    th, ph, da, wa, db, wb = cuda(edge_batch(3, 20, True, n=65))
    call = lambda **kw: hip.score_ensemble(**{**dict(theta=th, phi=ph, R=3, K=20, dflt=DFLT, doc_a=da, word_a=wa,   # noqa: E731
                                                     doc_b=db, word_b=wb, tol=0.01), **kw})
    bad = da.clone()
    bad[9] = D
    with pytest.raises(ValueError, match="out of range"):
        call(doc_a=bad)
    bad = wb.clone()
    bad[9] = V
    with pytest.raises(ValueError, match="out of range"):
        call(word_b=bad)
    bad = wa.clone()
    bad[3] = -2
    with pytest.raises(ValueError, match="out of range"):
        call(word_a=bad)
    with pytest.raises(ValueError, match="int32"):
        call(doc_a=da.long())
    with pytest.raises(ValueError, match="float64"):
        call(theta=th.float())
    with pytest.raises(ValueError, match="float64"):
        call(phi=ph.float())
    with pytest.raises(ValueError, match="contiguous"):
        call(theta=torch.cat([th, th])[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(phi=ph.transpose(1, 2).contiguous().transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous"):
        call(word_a=torch.cat([wa, wa])[::2])
    with pytest.raises(ValueError, match="row width"):
        call(R=4)
    with pytest.raises(ValueError, match="row width"):
        call(K=19)
    with pytest.raises(ValueError, match="row width"):
        call(phi=ph[:, :2].contiguous())
    with pytest.raises(ValueError, match="GPU tensor"):
        call(theta=th.cpu())
    with pytest.raises(ValueError, match="GPU tensor"):
        call(phi=ph.cpu())
    with pytest.raises(ValueError, match="expected"):
        call(doc_a=da.cpu())
    with pytest.raises(ValueError):
        call(doc_b=db[:-1], word_b=wb[:-1])
    with pytest.raises(ValueError, match="go together"):
        call(word_b=None)
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)
    for r in (0, 65):
        t = torch.zeros(2, r, 2, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError, match=r"\[1, 64\]"):
            hip.score_ensemble(t, t, r, 2, DFLT, da, wa, None, None, 0.01)


@pytest.mark.parametrize("kind,compat,scale,topics", [("flow", "strict", 5, 20), ("dns", "strict", 4, 20),
                                                      ("proxy", "fixed", 4, 20), ("flow", "fixed", 2, 16)])
def test_day_on_the_hip_backend(kind, compat, scale, topics, tmp_path_factory):
    """K = 16 (fixed rules): the pipeline on the double2 loop over a run-time K."""
    day = Day(kind, compat, tmp_path_factory.mktemp("ens_gpu_" + kind), backend="hip", device="cuda", scale=scale)
    ens, s = day.run("ens3", ensemble=3, topics=topics)
    parsed, twin, out = twin_scores_of_file(day, ens)
    assert out[0].numel() and twin[0].numel() and len(parsed) == (2 if kind == "flow" else 1)
    assert len(parsed[0]) == s["scored"] > 20
    for p, t in zip(parsed, twin):
        assert bits_equal(p, t)
    assert s["ensemble_votes_hist"] == np.bincount(out[4].numpy(), minlength=4).tolist()
    assert [m["member"] for m in s["lda"]["members"]] == [0, 1, 2]
    plain, _ = day.run("plain", topics=topics)
    a, b = tree(plain), tree(ens)
    for f in a:
        if f != day.results:
            assert a[f] == b[f], f
    assert a[day.results] != b[day.results]
    assert len((ens / "doc_results.csv").read_text().splitlines()[0].split(",")[1].split(" ")) == topics
