"""--tail on the GPU (gfx950): ``ops.hip.tail_mass`` (csrc/hip/tail_mass.hip) bit for bit its torch twin -- vocabulary
sizes around the block size, every row width's form (theta in registers, theta in LDS, both rows from global
memory; odd K: scalar staging, even K: 16-byte, a table 8 bytes off a 16-byte boundary), the grid-stride loop
wrapping, several scratch batches, empty input, the wrapper's refusals -- and a flow, a DNS and a proxy day on the
HIP backend.

V in {1, block - 1, block, block + 1, 2 block + 3, 5003}, block in {4, 64, TAIL_BLOCK}, K in {1, 2, 3, 20, 33, 100,
128}, R in {1, 3} and n in {0, 1, 1031} are covered by two sweeps instead of their 756-case product, so that every
case's CPU twin stays at a second or two: every V against every block at two row shapes, and every (K, R) at
V = 2 * 64 + 3 with the widest register, LDS and even / odd shapes again at V = 5003 and ``TAIL_BLOCK``."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal  # noqa: E402
from test_tail import check_tail_file, tail_case  # noqa: E402

from oni_ml_amd.config import TAIL_BLOCK  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 1031


@functools.lru_cache(maxsize=None)
def case(V, R_, K, n, block, nan):
    """The inputs and the twin's result, computed once and shared (never written to)."""
    a = tail_case(V, R_, K, n, nan=nan)
    return a, R.tail_mass(*a, block=block)


def same4(got, want):
    assert got[0].dtype == got[1].dtype == torch.float64 and got[2].dtype == got[3].dtype == torch.int32
    assert all(g.is_cuda for g in got)
    for g, w in zip(got, want):
        assert bits_equal(g.cpu(), w)


def vs_of(block):
    return [1, block - 1, block, block + 1, 2 * block + 3, 5003]


@pytest.mark.parametrize("R_,K", [(1, 20), (3, 3)])
@pytest.mark.parametrize("block", [4, 64, TAIL_BLOCK])
def test_every_vocabulary_size_against_every_block(hip, block, R_, K):
    assert TAIL_BLOCK == 1024
    for V in vs_of(block):
        a, want = case(V, R_, K, N, block, block == 64)
        ok = (a[2] >= 0) & (a[3] >= 0)
        own = ok & ~((a[3] == 11) & (block == 64) & (V > 11))      # a side at the NaN row has a NaN score: no tie
        assert int(ok.sum()) > 700 and int((~ok).sum()) > 100 and bool((want[3][own] >= 1).all())
        assert V < 12 or block != 64 or bool(torch.isnan(want[1][ok]).all())
        same4(hip.tail_mass(*(x.cuda() for x in a), block=block), want)


PATHS = {(1, 1): "registers", (2, 1): "registers", (3, 1): "registers", (20, 1): "registers", (33, 1): "registers",
         (100, 1): "registers", (128, 1): "lds_theta", (1, 3): "registers", (2, 3): "registers", (3, 3): "registers",
         (20, 3): "registers", (33, 3): "lds_theta", (100, 3): "direct", (128, 3): "direct"}


@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 20, 33, 100, 128])
def test_every_row_width(hip, K, R_):
    """K = 100 / 128 at one model straddle the register bound (100 doubles), 33 / 100 at three members the LDS
    bound (256)."""
    assert hip.tail_theta_path(R_, K) == PATHS[(K, R_)]
    a, want = case(131, R_, K, N, 64, R_ == 3)
    assert R_ == 1 or bool(torch.isnan(want[1][(a[2] >= 0) & (a[3] >= 0)]).all())
    dev = [x.cuda() for x in a]
    same4(hip.tail_mass(*dev, block=64), want)
    # phi 8 bytes off a 16-byte boundary: the scalar staging at an even K, the same bits
    buf = torch.empty(a[1].numel() + 1, dtype=torch.float64, device="cuda")
    sh = buf[1:].view(a[1].shape)
    sh.copy_(dev[1])
    assert sh.is_contiguous() and sh.data_ptr() % 16 == 8
    same4(hip.tail_mass(dev[0], sh, dev[2], dev[3], block=64), want)


@pytest.mark.parametrize("R_,K", [(1, 20), (1, 100), (1, 128), (3, 33)])
def test_the_day_shape_blocks(hip, R_, K):
    a, want = case(5003, R_, K, N, None, False)
    dev = [x.cuda() for x in a]
    same4(hip.tail_mass(*dev), want)
    # a scratch of 400 sides' partials (5 blocks x 24 bytes each): batches of 256 sides, five launches
    same4(hip.tail_mass(*dev, scratch_mb=400 * 5 * 24 / 2 ** 20), want)


@pytest.mark.parametrize("R_,K", [(1, 20), (3, 33), (3, 100)])
def test_grid_stride_and_small_n(hip, R_, K):
    a, want = case(131, R_, K, 3000, 64, False)
    same4(hip.tail_mass(*(x.cuda() for x in a), block=64, max_blocks=2), want)
    for n in (0, 1):
        a, want = case(131, R_, K, n, 64, False)
        got = hip.tail_mass(*(x.cuda() for x in a), block=64)
        assert all(tuple(g.shape) == (n,) for g in got)
        same4(got, want)


def test_most_probable_word_and_ties_on_the_device(hip):
    th, ph, _, _ = tail_case(2051, 1, 20, 0)
    D, V = th.shape[0], ph.shape[0]
    top = (th[:, 0] @ ph[:, 0].T).argmax(1)      # (far from a tie at these random tables)
    doc = torch.arange(D, dtype=torch.int32)
    le, tot, rarer, ties = (x.cpu() for x in hip.tail_mass(th.cuda(), ph.cuda(), doc.cuda(), top.to(torch.int32).cuda()))
    assert bits_equal(le, tot) and bool((le / tot == 1.0).all()) and bool((rarer + ties == V).all())
    a, want = case(131, 1, 20, N, 64, False)
    ties = hip.tail_mass(*(x.cuda() for x in a), block=64)[3].cpu()
    ok = (a[2] >= 0) & (a[3] >= 0)
    assert bool((ties[ok] >= 1).all()) and bool((ties[~ok] == -1).all())


def test_tail_mass_refusals(hip):
    a, want = case(131, 3, 20, 65, 64, False)
    th, ph, doc, word = (x.cuda() for x in a)
    call = lambda **kw: hip.tail_mass(**{**dict(theta=th, phi=ph, doc=doc, word=word, block=64), **kw})   # noqa: E731
    same4(call(max_blocks=2), want)      # the positive control: the same arguments, unspoilt
    for name, t, lim in (("doc", doc, 37), ("word", word, 131)):
        bad = t.clone()
        bad[9] = lim
        with pytest.raises(ValueError, match="out of range"):
            call(**{name: bad})
        bad[9] = -2
        with pytest.raises(ValueError, match="out of range"):
            call(**{name: bad})
    with pytest.raises(ValueError, match="int32"):
        call(doc=doc.long())
    with pytest.raises(ValueError, match="float64"):
        call(phi=ph.float())
    with pytest.raises(ValueError, match="contiguous"):
        call(phi=torch.cat([ph, ph])[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(word=torch.cat([word, word])[::2])
    with pytest.raises(ValueError, match="row width"):
        call(phi=ph[:, :2].contiguous())
    with pytest.raises(ValueError, match="GPU tensor"):
        call(phi=ph.cpu())
    with pytest.raises(ValueError):
        call(word=word[:-1])
    with pytest.raises(ValueError, match="block"):
        call(block=0)
    with pytest.raises(ValueError, match="scratch_mb"):
        call(scratch_mb=0)
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)


@pytest.mark.parametrize("kind,compat,scale", [("flow", "strict", 5), ("flow", "fixed", 5), ("dns", "strict", 4),
                                               ("proxy", "fixed", 4)])
def test_day_on_the_hip_backend(kind, compat, scale, tmp_path_factory):
    day = Day(kind, compat, tmp_path_factory.mktemp("tail_gpu_" + kind), backend="hip", device="cuda", scale=scale)
    lp, s = day.run("tail", tail=True)
    check_tail_file(day, lp, s)      # the file's bits are the CPU twin's over the written tables
    assert (lp / day.results).read_bytes() == (day.run("plain")[0] / day.results).read_bytes()
