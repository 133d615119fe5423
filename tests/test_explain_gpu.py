"""--explain on the GPU (gfx950): ``ops.hip.group_rows_sum`` and ``ops.hip.explain_sides`` (csrc/hip/explain.hip)
bit for bit their torch twins -- segment lengths around the block size, every row width's path (odd: scalar, even:
double2, a table 8 bytes off a 16-byte boundary), the grid-stride loops wrapping, empty input, the wrappers'
refusals -- and a flow, a DNS and a proxy day on the HIP backend."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal  # noqa: E402
from test_explain import BIG, check_day_against_oracle, twin_conditionals_of_file  # noqa: E402

from oni_ml_amd.config import GROUP_BLOCK  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

V = 5003
LENS = [1, 2, 255, 256, 257, 512, 513, 1500] + [1] * 200


def rows_case(W, seed=0):
    """(table [V, W], order int32 [V], seg_start, seg_end) on the CPU: values over 8 decades, a NaN row and a -0.0
    row, a shuffled row order, the segments of LENS plus one of everything left and an empty one, selected in a
    shuffled order."""
    g = torch.Generator().manual_seed(100 + W + seed)
    t = torch.rand(V, W, dtype=torch.float64, generator=g) * 10.0 ** torch.randint(-8, 1, (V, 1), generator=g).double()
    t[11, W - 1] = float("nan")
    t[12, 0] = -0.0
    order = torch.randperm(V, generator=g).to(torch.int32)
    lens = LENS + [V - sum(LENS), 0]
    ends = np.cumsum(lens)
    starts = ends - np.asarray(lens)
    p = torch.randperm(len(lens), generator=g).numpy()
    return t, order, torch.from_numpy(starts[p].astype(np.int64)), torch.from_numpy(ends[p].astype(np.int64))


@pytest.mark.parametrize("W", [1, 3, 20, 33, 40, 100])
def test_group_rows_sum_equals_the_twin(hip, W):
    t, order, s, e = rows_case(W)
    want = R.group_rows_sum(t, order, s, e)
    assert torch.isnan(want).any() and int((e - s).max()) > 2 * 256 and int((e - s).min()) == 0
    tc, oc, sc, ec = t.cuda(), order.cuda(), s.cuda(), e.cuda()
    assert bits_equal(hip.group_rows_sum(tc, oc, sc, ec).cpu(), want)
    assert bits_equal(hip.group_rows_sum(tc, oc, sc, ec, max_blocks=2).cpu(), want)
    # the table 8 bytes off a 16-byte boundary: the scalar path at an even W, the same bits
    buf = torch.empty(t.numel() + 1, dtype=torch.float64, device="cuda")
    sh = buf[1:].view(t.shape)
    sh.copy_(tc)
    assert sh.is_contiguous() and sh.data_ptr() % 16 == 8
    assert bits_equal(hip.group_rows_sum(sh, oc, sc, ec).cpu(), want)


def test_group_rows_sum_no_segment_launches_nothing(hip):
    t, order, s, e = rows_case(20)
    out = hip.group_rows_sum(t.cuda(), order.cuda(), s[:0].cuda(), e[:0].cuda())
    assert tuple(out.shape) == (0, 20) and out.is_cuda


def test_group_rows_sum_refusals(hip):
    t, order, s, e = (x.cuda() for x in rows_case(20))
    want = R.group_rows_sum(*rows_case(20))
    call = lambda **kw: hip.group_rows_sum(**{**dict(table=t, order=order, seg_start=s, seg_end=e), **kw})   # noqa: E731
    assert bits_equal(call().cpu(), want)      # the positive control: the same arguments, unspoilt
    with pytest.raises(ValueError, match="float64"):
        call(table=t.float())
    with pytest.raises(ValueError, match="int32"):
        call(order=order.long())
    with pytest.raises(ValueError, match="int64"):
        call(seg_start=s.int())
    with pytest.raises(ValueError, match="contiguous"):
        call(table=torch.cat([t, t])[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(order=torch.cat([order, order])[::2])
    bad = order.clone()
    bad[7] = V
    with pytest.raises(ValueError, match="out of range"):
        call(order=bad)
    bad[7] = -1
    with pytest.raises(ValueError, match="out of range"):
        call(order=bad)
    bad = e.clone()
    bad[3] = s[3] - 1
    with pytest.raises(ValueError, match="segments"):
        call(seg_end=bad)
    bad = e.clone()
    bad[3] = V + 1
    with pytest.raises(ValueError, match="segments"):
        call(seg_end=bad)
    with pytest.raises(ValueError):
        call(seg_end=e[:-1])
    with pytest.raises(ValueError, match="GPU tensor"):
        call(table=t.cpu())
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)


N, D, VW, G = 1031, 37, 53, 29


def sides_case(F, R_, K, n=N, seed=0):
    g = torch.Generator().manual_seed(1000 * F + 10 * R_ + K + seed)
    th = torch.rand(D, R_, K, dtype=torch.float64, generator=g)
    ph = torch.rand(VW, R_, K, dtype=torch.float64, generator=g) * 1e-3
    gs = ph[torch.randint(0, VW, (G,), generator=g)] + torch.rand(G, R_, K, dtype=torch.float64, generator=g) * 1e-2
    gs[3, R_ - 1, K - 1] = float("nan")

    def idx(rows, shape):
        x = torch.randint(0, rows, shape, generator=g, dtype=torch.int32)
        x[torch.rand(shape, generator=g) < 0.1] = -1
        return x
    doc, word, grow = idx(D, (n,)), idx(VW, (n,)), idx(G, (n, F))
    if n >= 4:
        grow[0] = 3            # the NaN row in every field
        grow[1] = 5            # every field tied
        word[1], word[2], grow[3] = 4, -1, -1
    return th, ph, gs, doc, word, grow


def same2(got, want):
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.uint8
    assert bits_equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


@pytest.mark.parametrize("K", [1, 2, 3, 20, 33])
@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("F", [1, 4, 7])
def test_explain_sides_equals_the_twin(hip, F, R_, K):
    a = sides_case(F, R_, K)
    want = R.explain_sides(*a, 0.05)
    assert torch.isnan(want[0]).any() and (want[1] == 255).any() and int(want[1][1]) == 0
    assert F == 1 or len(set(want[1].tolist())) > 2
    same2(hip.explain_sides(*(x.cuda() for x in a), 0.05), want)


@pytest.mark.parametrize("F,R_,K", [(4, 3, 20), (7, 1, 3)])
def test_explain_sides_grid_stride_and_small_n(hip, F, R_, K):
    a = sides_case(F, R_, K, n=3000)
    same2(hip.explain_sides(*(x.cuda() for x in a), 0.05, max_blocks=2), R.explain_sides(*a, 0.05))
    for n in (0, 1):
        a = sides_case(F, R_, K, n=n)
        got = hip.explain_sides(*(x.cuda() for x in a), 0.05)
        assert tuple(got[0].shape) == (n, F) and tuple(got[1].shape) == (n,)
        same2(got, R.explain_sides(*a, 0.05))


@pytest.mark.parametrize("K", [3, 20])
def test_a_group_of_the_row_itself_gives_exactly_one(hip, K):
    th, ph, _, doc, word, _ = sides_case(1, 1, K)
    grow = word.clone().reshape(-1, 1)
    cond, why = hip.explain_sides(th.cuda(), ph.cuda(), ph.cuda(), doc.cuda(), word.cuda(), grow.cuda(), 0.05)
    c = cond.cpu()[:, 0]
    assert torch.equal(torch.isnan(c), word < 0) and bool((c[word >= 0] == 1.0).all())
    # and s is score_events' score: cond * m == s needs no test beyond R = 1 of the twin, which calls the scorer


def test_explain_sides_refusals(hip):
    a = [x.cuda() for x in sides_case(4, 3, 20, n=65)]
    names = ("theta", "phi", "gsum", "doc", "word", "grow")
    call = lambda **kw: hip.explain_sides(**{**dict(zip(names, a)), "dflt": 0.05, **kw})   # noqa: E731
    same2(call(max_blocks=2), R.explain_sides(*sides_case(4, 3, 20, n=65), 0.05))      # the positive control
    th, ph, gs, doc, word, grow = a
    for name, t, lim in (("doc", doc, D), ("word", word, VW), ("grow", grow, G)):
        bad = t.clone()
        bad.view(-1)[9] = lim
        with pytest.raises(ValueError, match="out of range"):
            call(**{name: bad})
        bad.view(-1)[9] = -2
        with pytest.raises(ValueError, match="out of range"):
            call(**{name: bad})
    with pytest.raises(ValueError, match="int32"):
        call(doc=doc.long())
    with pytest.raises(ValueError, match="float64"):
        call(gsum=gs.float())
    with pytest.raises(ValueError, match="contiguous"):
        call(phi=torch.cat([ph, ph])[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(grow=torch.cat([grow, grow])[::2])
    with pytest.raises(ValueError, match="row width"):
        call(gsum=gs[:, :2].contiguous())
    with pytest.raises(ValueError, match="GPU tensor"):
        call(phi=ph.cpu())
    with pytest.raises(ValueError):
        call(word=word[:-1])
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        call(grow=torch.zeros(65, 9, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)


@pytest.mark.parametrize("kind,compat,scale,cuts", [("flow", "strict", 5, None), ("dns", "strict", 4, None),
                                                    ("proxy", "fixed", 4, None), ("flow", "fixed", BIG["scale"], BIG["cuts"])])
def test_day_on_the_hip_backend(kind, compat, scale, cuts, tmp_path_factory):
    """The last case is the coarsely binned flow day of the CPU test: its sides refer to a group of more than one
    block, so the pipeline runs the two-pass sum."""
    day = Day(kind, compat, tmp_path_factory.mktemp("exp_gpu_" + kind), backend="hip", device="cuda", scale=scale)
    lp, s = day.run("explain", explain=True, **(dict(cuts=cuts) if cuts else {}))
    got, want, why_got, why_want = twin_conditionals_of_file(day, lp)
    assert got.shape[0] > 20 and bits_equal(got, want) and why_got == why_want
    largest = check_day_against_oracle(day, lp, s)
    assert cuts is None or largest > GROUP_BLOCK
