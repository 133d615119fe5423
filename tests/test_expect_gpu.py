"""--expect on the GPU (gfx950): ``ops.hip.expect_sides`` (csrc/hip/expect.hip) bit for bit its torch twin --
segment lengths around the block size (the direct write, the fold), ties, a NaN row, every row width's path (the
register ladder and its edge, vector and scalar loads, a table 8 bytes off a 16-byte boundary, a width that reads
theta from global memory), the grid-stride loops wrapping, empty input, the wrapper's refusals -- and a flow, a DNS
and a proxy day on the HIP backend against the CPU scoring of the same model."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal  # noqa: E402
from test_expect import check_day  # noqa: E402
from test_explain import BIG  # noqa: E402

from oni_ml_amd.config import GROUP_BLOCK  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

V, D, N = 5003, 37, 1031
LENS = [1, 2, 255, 256, 257, 512, 513, 1500] + [1] * 200
NAMES = ("theta", "phi", "order", "seg_start", "seg_end", "doc", "word", "grow")
_CASES = {}


def case(F, R_, K, n=N):
    """(theta, phi, order, seg_start, seg_end, doc, word, grow) on the CPU and the twin's result, made once: phi
    over 8 decades with a NaN row, a row of -0.0 and rows repeated inside the long segments (ties), a shuffled row
    order, the segments of LENS plus one of everything left and an empty one, a tenth of every index -1."""
    key = (F, R_, K, n)
    if key not in _CASES:
        g = torch.Generator().manual_seed(7000 * F + 10 * R_ + K + n)
        th = torch.rand(D, R_, K, dtype=torch.float64, generator=g)
        ph = torch.rand(V, R_, K, dtype=torch.float64, generator=g) * 10.0 ** torch.randint(-8, 1, (V, 1, 1),
                                                                                          generator=g).double()
        order = torch.randperm(V, generator=g).to(torch.int32)
        lens = LENS + [V - sum(LENS), 0]
        ends = np.cumsum(lens)
        starts = ends - np.asarray(lens)
        o = order.long()
        ph[o[3]] = float("nan")                      # in the segment of 255
        ph[o[300], 0, 0] = -0.0                      # in the segment of 256
        for j in (5, 6, 7, len(LENS)):               # the segments of 512, 513, 1500 and the rest: a row repeated in
            a, b = int(starts[j]), int(ends[j])      # the first and the last block, scaled up so that it is the best
            ph[o[a + 1]] = ph[o[b - 1]] = ph[o[a:b]].nan_to_num().amax(0) * 2.0
        G = len(lens)

        def idx(rows, shape):
            x = torch.randint(0, rows, shape, generator=g, dtype=torch.int32)
            x[torch.rand(shape, generator=g) < 0.1] = -1
            return x
        doc, word, grow = idx(D, (n,)), idx(V, (n,)), idx(G, (n, F))
        for i in range(min(n, G)):                   # every segment is referenced, the special ones by a whole row
            grow[i, i % F] = i
        if n > 12:
            for i in range(10):
                grow[i], doc[i], word[i] = i, i, int(o[int(starts[i])])      # the word is its group's first member
            doc[10], word[11], grow[12] = -1, -1, -1
            word[10], grow[10] = 5, 7
        a = (th, ph, order, torch.from_numpy(starts.astype(np.int64)), torch.from_numpy(ends.astype(np.int64)), doc,
             word, grow)
        _CASES[key] = (a, R.expect_sides(*a, 0.05))
    return _CASES[key]


def same3(got, want):
    assert [x.dtype for x in got] == [torch.int32, torch.float64, torch.int32]
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[2].cpu(), want[2])
    assert bits_equal(got[1].cpu(), want[1])


@pytest.mark.parametrize("K", [1, 2, 3, 20, 33])
@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("F", [1, 4, 7])
def test_expect_sides_equals_the_twin(hip, F, R_, K):
    a, want = case(F, R_, K)
    best, pbest, above = want
    # what the case is for: a fold that finds the tie across blocks, an empty group, a NaN group member, no value
    assert best[7, 0].item() == min(int(a[2][int(a[3][7]) + 1]), int(a[2][int(a[4][7]) - 1]))
    assert (above == -1).any() and (best == -1).any() and torch.isnan(pbest).any() and (above > 0).any()
    assert int((a[4] - a[3]).max()) > 2 * GROUP_BLOCK and int((a[4] - a[3]).min()) == 0
    same3(hip.expect_sides(*(x.cuda() for x in a), 0.05), want)
    same3(hip.expect_sides(*(x.cuda() for x in a), 0.05, form="blocks"), want)      # the form that ships, forced


@pytest.mark.parametrize("F,R_,K", [(4, 1, 20), (7, 3, 3)])
def test_grid_stride_block_cuts_and_small_n(hip, F, R_, K):
    a, want = case(F, R_, K)
    dev = [x.cuda() for x in a]
    same3(hip.expect_sides(*dev, 0.05, max_blocks=2), want)
    for block in (1, 7, 100000):      # every block cut: the same result
        same3(hip.expect_sides(*dev, 0.05, block=block), want)
    for n in (0, 1):
        b, w = case(F, R_, K, n=n)
        got = hip.expect_sides(*(x.cuda() for x in b), 0.05)
        assert [tuple(x.shape) for x in got] == [(n, F)] * 3
        same3(got, w)


@pytest.mark.parametrize("R_,K", [(1, 20), (3, 20), (1, 2)])
def test_a_table_off_the_16_byte_boundary(hip, R_, K):
    a, want = case(4, R_, K)
    dev = [x.cuda() for x in a]
    buf = torch.empty(a[1].numel() + 1, dtype=torch.float64, device="cuda")
    sh = buf[1:].view(a[1].shape)
    sh.copy_(dev[1])
    assert sh.is_contiguous() and sh.data_ptr() % 16 == 8 and dev[1].data_ptr() % 16 == 0
    dev[1] = sh
    same3(hip.expect_sides(*dev, 0.05), want)      # the scalar loads at an even K: the same bits


@pytest.mark.parametrize("R_,K", [(3, 50), (1, 101), (2, 50), (1, 100)])
def test_the_edge_of_the_register_ladder(hip, R_, K):
    wide = (R_, K) in ((3, 50), (1, 101))
    assert hip.expect_theta_path(R_, K) == ("global" if wide else "registers")
    assert hip.expect_theta_path(1, 20) == "registers"
    a, want = case(2, R_, K, n=300)
    same3(hip.expect_sides(*(x.cuda() for x in a), 0.05), want)


def test_expect_sides_refusals(hip):
    a, want = case(4, 3, 20, n=65)
    dev = [x.cuda() for x in a]
    call = lambda **kw: hip.expect_sides(**{**dict(zip(NAMES, dev)), "dflt": 0.05, **kw})   # noqa: E731
    same3(call(max_blocks=2), want)      # the positive control: the same arguments, unspoilt
    th, ph, order, s, e, doc, word, grow = dev
    G = s.numel()
    for name, t, lim in (("doc", doc, D), ("word", word, V), ("grow", grow, G), ("order", order, V)):
        bad = t.clone()
        bad.view(-1)[9] = lim
        with pytest.raises(ValueError, match="out of range"):
            call(**{name: bad})
        bad.view(-1)[9] = -2
        with pytest.raises(ValueError, match="out of range"):
            call(**{name: bad})
    bad = e.clone()
    bad[3] = s[3] - 1
    with pytest.raises(ValueError, match="segments"):
        call(seg_end=bad)
    bad = e.clone()
    bad[3] = V + 1
    with pytest.raises(ValueError, match="segments"):
        call(seg_end=bad)
    bad = s.clone()
    bad[0] = -1
    with pytest.raises(ValueError, match="segments"):
        call(seg_start=bad)
    with pytest.raises(ValueError, match="int32"):
        call(doc=doc.long())
    with pytest.raises(ValueError, match="int32"):
        call(order=order.long())
    with pytest.raises(ValueError, match="int64"):
        call(seg_start=s.int())
    with pytest.raises(ValueError, match="float64"):
        call(phi=ph.float())
    with pytest.raises(ValueError, match="contiguous"):
        call(phi=torch.cat([ph, ph])[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(grow=torch.cat([grow, grow])[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(order=torch.cat([order, order])[::2])
    with pytest.raises(ValueError, match="row width"):
        call(phi=ph[:, :2].contiguous())
    for name, t in zip(NAMES, dev):
        with pytest.raises(ValueError):
            call(**{name: t.cpu()})
    with pytest.raises(ValueError, match="GPU tensor"):
        call(phi=ph.cpu())
    with pytest.raises(ValueError):
        call(word=word[:-1])
    with pytest.raises(ValueError):
        call(seg_end=e[:-1])
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        call(grow=torch.zeros(65, 9, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        call(grow=torch.zeros(65, 0, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        call(theta=torch.zeros(D, 65, 2, dtype=torch.float64, device="cuda"),
             phi=torch.zeros(V, 65, 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)
    with pytest.raises(ValueError, match="block"):
        call(block=0)
    with pytest.raises(ValueError, match="form"):
        call(form="tiles")


@pytest.mark.parametrize("kind,compat,scale,cuts", [("flow", "strict", 2, None), ("dns", "strict", 4, None),
                                                    ("proxy", "fixed", 4, None), ("flow", "fixed", BIG["scale"], BIG["cuts"])])
def test_day_on_the_hip_backend(kind, compat, scale, cuts, tmp_path_factory):
    """The last case is the coarsely binned flow day of the CPU test: its groups pass one block, so the fold runs.
    The CPU run: the scoring stage of the same directory resumed on the CPU, from the model the GPU run wrote.  (The
    strict flow day is 8,000 events: at 12,000 and 20,000 the GPU's and the CPU's scoring stage put one event into
    neighbouring ibyt bins, with or without this option -- docs/ARCHITECTURE.md, "Open: the strict flow bins on the
    GPU and on the CPU" -- and the files would describe different rows.  The results files are compared first.)"""
    from oni_ml_amd.pipeline import run
    day = Day(kind, compat, tmp_path_factory.mktemp("expect_gpu_" + kind), backend="hip", device="cuda", scale=scale)
    kw = dict(cuts=cuts) if cuts else {}
    lp, s = day.run("expect", expect=True, **kw)
    assert s["expect_path"] == "blocks"
    largest = check_day(day, lp, s)
    assert cuts is None or largest > GROUP_BLOCK
    cpu = day.root / "cpu"
    shutil.copytree(lp, cpu)
    name = f"{kind}_expect.csv"
    for p in (cpu / ".stages" / f"{kind}_post.done", cpu / name, cpu / day.results, cpu / f"{kind}_explain.csv"):
        os.unlink(p)
    sc = run(day.cfg(cpu, expect=True, resume=True, **kw).validate(), device="cpu", log=lambda *a: None)
    assert sc["expect_path"] == "cpu" and sc["expect_pairs"] == s["expect_pairs"]
    for f in (day.results, f"{kind}_explain.csv", name):
        assert (cpu / f).read_bytes() == (lp / f).read_bytes(), f
