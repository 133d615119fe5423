"""--peers on the GPU (gfx950): ``ops.hip.peer_topn`` (csrc/hip/peers.hip) bit for bit its torch twin in all three
outputs -- table sizes around N and around the block size, every row width's form (the query's row in registers,
both rows from global memory; odd W: scalar staging, even W: 16-byte, a table 8 bytes off a 16-byte boundary), the
grid-stride loop wrapping, several scratch batches, empty input, ties, NaN rows, the wrapper's refusals -- and a
flow, a DNS and a proxy day on the HIP backend.

Every D against every block runs at two row shapes; every (K, R) at D = 131.  The twin's result is computed once per
case and shared."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal  # noqa: E402
from test_peers import NP, check_peer_files, nan_table, peer_case, tripled  # noqa: E402

from oni_ml_amd.config import PEERS_BLOCK  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

Q = 1031
N = 5


@functools.lru_cache(maxsize=None)
def case(D, R_, K, q, n):
    """The inputs and the twin's result, computed once and shared (never written to)."""
    a = peer_case(D, R_, K, q)
    return a, R.peer_topn(*a, n)


def same3(got, want):
    assert got[0].dtype == got[2].dtype == torch.int32 and got[1].dtype == torch.float64
    assert all(g.is_cuda for g in got)
    for g, w in zip(got, want):
        assert g.shape == w.shape and bits_equal(g.cpu(), w)


def ds_of(block):
    return sorted({1, 2, N, N + 1, block - 1, block, block + 1, 2 * block + 3, 5003} - {0})


@pytest.mark.parametrize("K,R_", [(20, 1), (3, 3)])
@pytest.mark.parametrize("D", sorted({d for b in (4, 64, PEERS_BLOCK) for d in ds_of(b)}))
def test_every_table_size_against_every_block(hip, D, K, R_):
    (th, q), want = case(D, R_, K, Q, N)
    assert bool((want[2] == min(N, D - 1)).all())
    dev = th.cuda(), q.cuda()
    for block in (4, 64, PEERS_BLOCK):
        if D in ds_of(block):
            same3(hip.peer_topn(*dev, N, block=block), want)


PATHS = {(1, 1): "registers", (2, 1): "registers", (3, 1): "registers", (20, 1): "registers", (33, 1): "registers",
         (100, 1): "registers", (128, 1): "direct", (1, 3): "registers", (2, 3): "registers", (3, 3): "registers",
         (20, 3): "registers", (33, 3): "registers", (100, 3): "direct", (128, 3): "direct"}


@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 20, 33, 100, 128])
def test_every_row_width(hip, K, R_):
    """The register form holds a row of up to 100 doubles, whatever its split into members: K = 100 / 128 at one
    model and 33 / 100 at three members straddle it."""
    assert hip.peer_theta_path(R_, K) == PATHS[(K, R_)]
    (th, q), _ = case(131, R_, K, Q, 16)
    dev = th.cuda(), q.cuda()
    # theta 8 bytes off a 16-byte boundary: the scalar staging at an even W, the same bits
    buf = torch.empty(th.numel() + 1, dtype=torch.float64, device="cuda")
    sh = buf[1:].view(th.shape)
    sh.copy_(dev[0])
    assert sh.is_contiguous() and sh.data_ptr() % 16 == 8
    for n in (16, 1):
        want = case(131, R_, K, Q, n)[1]
        same3(hip.peer_topn(*dev, n, block=64), want)
        same3(hip.peer_topn(sh, dev[1], n, block=64), want)


@pytest.mark.parametrize("K,R_", [(20, 1), (33, 3), (100, 3)])
def test_grid_stride_scratch_batches_and_small_q(hip, K, R_):
    (th, q), want = case(131, R_, K, 3000, N)
    dev = th.cuda(), q.cuda()
    same3(hip.peer_topn(*dev, N, block=64, max_blocks=2), want)
    # a scratch of 400 queries' lists (3 blocks x 5 x 12 bytes each): batches of 256 queries, twelve launches
    same3(hip.peer_topn(*dev, N, block=64, scratch_mb=400 * 3 * N * 12 / 2 ** 20), want)
    for nq in (0, 1):
        (th, q), want = case(131, R_, K, nq, N)
        got = hip.peer_topn(th.cuda(), q.cuda(), N, block=64)
        assert tuple(got[0].shape) == tuple(got[1].shape) == (nq, N) and tuple(got[2].shape) == (nq,)
        same3(got, want)


def test_ties_and_nan_rows_on_the_device(hip):
    th = tripled()
    q = torch.arange(th.shape[0], dtype=torch.int32)
    for n, block in ((5, 4), (1, 4), (16, PEERS_BLOCK)):
        want = R.peer_topn(th, q, n)
        assert bool((want[1][:, 0] == 0.0).all())
        same3(hip.peer_topn(th.cuda(), q.cuda(), n, block=block), want)
    th, q = nan_table()
    want = R.peer_topn(th, q, 16)
    assert int((want[2] == 0).sum()) >= 2 and not bool((want[0] == 11).any())
    for block in (4, 64, PEERS_BLOCK):
        same3(hip.peer_topn(th.cuda(), q.cuda(), 16, block=block), want)


def test_peer_topn_refusals(hip):
    (th, q), want = case(131, 3, 20, 65, N)
    th, q = th.cuda(), q.cuda()
    call = lambda **kw: hip.peer_topn(**{**dict(theta3=th, query=q, n=N, block=64), **kw})   # noqa: E731
    same3(call(max_blocks=2), want)      # the positive control: the same arguments, unspoilt
    bad = q.clone()
    bad[9] = 131
    with pytest.raises(ValueError, match="out of range"):
        call(query=bad)
    bad[9] = -1
    with pytest.raises(ValueError, match="out of range"):
        call(query=bad)
    with pytest.raises(ValueError, match="int32"):
        call(query=q.long())
    with pytest.raises(ValueError, match="float64"):
        call(theta3=th.float())
    with pytest.raises(ValueError, match="contiguous"):
        call(theta3=torch.cat([th, th])[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(query=torch.cat([q, q])[::2])
    with pytest.raises(ValueError, match="GPU tensor"):
        call(theta3=th.cpu())
    with pytest.raises(ValueError, match=r"\[rows, R, K\]"):
        call(theta3=th.reshape(131, 60))
    for n in (0, 17):
        with pytest.raises(ValueError, match="n must be"):
            call(n=n)
    with pytest.raises(ValueError, match="block"):
        call(block=0)
    with pytest.raises(ValueError, match="scratch_mb"):
        call(scratch_mb=0)
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)


@pytest.mark.parametrize("kind,compat,scale", [("flow", "strict", 5), ("flow", "fixed", 5), ("dns", "strict", 4),
                                               ("proxy", "fixed", 4)])
def test_day_on_the_hip_backend(kind, compat, scale, tmp_path_factory):
    day = Day(kind, compat, tmp_path_factory.mktemp("peers_gpu_" + kind), backend="hip", device="cuda", scale=scale)
    lp, s = day.run("peers", peers=NP)
    check_peer_files(day, lp, s)      # both files' bits are the CPU twin's over the written tables
    assert (lp / day.results).read_bytes() == (day.run("plain")[0] / day.results).read_bytes()
