"""--topic-report on the GPU (gfx950): ``ops.hip.column_topn`` / ``row_dominant`` / ``topic_sides``
(csrc/hip/topic_report.hip) bit for bit their torch twins -- table heights around N and around the block size, every
width form (a lane per column, the lanes in row sub-groups; one load path of 8 bytes per lane, so a table 8 bytes
off a 16-byte boundary must simply give the same bits), N = 1, 5 and 32
(256 and 128 lanes), the sampled lower bound, the grid-stride loops wrapping, several column batches, empty input,
ties, signed zeros, NaN, the wrappers' refusals -- and a flow, a DNS and a proxy day on the HIP backend.

The twin's result is computed once per case and shared."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal  # noqa: E402
from test_topic_report import (NT, check_topic_files, dominant_case, edge_table, sides_case, topn_case,  # noqa: E402
                               tripled)

from oni_ml_amd.config import TOPIC_BLOCK, TOPIC_SAMPLE  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 5


@functools.lru_cache(maxsize=None)
def case(rows, R_, K, n):
    """The table and the twin's result, computed once and shared (never written to)."""
    t = topn_case(rows, R_, K)
    return t, R.column_topn(t, n)


def same(got, want):
    assert len(got) == len(want) and all(g.is_cuda for g in got)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and bits_equal(g.cpu(), w)


def rows_of(block):
    return sorted({1, 2, N, N + 1, block - 1, block, block + 1, 2 * block + 3, 5003} - {0})


@pytest.mark.parametrize("K,R_", [(20, 1), (3, 3)])
@pytest.mark.parametrize("rows", sorted({r for b in (4, 64, TOPIC_BLOCK) for r in rows_of(b)}))
def test_every_table_height_against_every_block(hip, rows, K, R_):
    t, want = case(rows, R_, K, N)
    dev = t.cuda()
    for block in (4, 64, TOPIC_BLOCK):
        if rows in rows_of(block):
            same(hip.column_topn(dev, N, block=block), want)
            same(hip.column_topn(dev, N, block=block, sample=16), want)      # from 32 rows on: the sampled bound


@pytest.mark.parametrize("R_", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 20, 33, 100, 128])
def test_every_width_form(hip, K, R_):
    """W = R K from 1 to 384: up to half a workgroup the lanes form row sub-groups (fewer of them at N = 32, where a
    workgroup has 128 lanes), past it a lane owns a column, past a workgroup there are several column tiles."""
    W = R_ * K
    t = case(131, R_, K, N)[0]
    dev = t.cuda()
    # the table 8 bytes off a 16-byte boundary: the kernel has a single load path, the same bits
    buf = torch.empty(t.numel() + 1, dtype=torch.float64, device="cuda")
    sh = buf[1:].view(t.shape)
    sh.copy_(dev)
    assert sh.is_contiguous() and sh.data_ptr() % 16 == 8
    for n in (1, N, 32):
        lanes = 256 if n <= 16 else 128
        assert hip.topic_path(n, W) == (f"subgroups{lanes // W}" if W <= lanes // 2 else "columns")
        want = case(131, R_, K, n)[1]
        same(hip.column_topn(dev, n, block=64), want)
        same(hip.column_topn(sh, n, block=64), want)


@pytest.mark.parametrize("K,R_", [(20, 1), (33, 3), (128, 3)])
def test_grid_stride_and_column_batches(hip, K, R_):
    W = R_ * K
    for n in (N, 32):
        t, want = case(3000, R_, K, n)
        dev = t.cuda()
        same(hip.column_topn(dev, n, block=64, max_blocks=2), want)
        same(hip.column_topn(dev, n, block=64, max_blocks=2, sample=100), want)
        same(hip.column_topn(dev, n, block=16, max_blocks=3), want)      # 188 blocks: pass 2 in two levels
        per_col = 12 * n * 47      # 47 blocks of 64 rows
        # a scratch of 7 columns' lists: batches of 7 columns, each in row sub-groups
        same(hip.column_topn(dev, n, block=64, scratch_mb=7.5 * per_col / 2 ** 20), want)
        if W > 300:      # of 300: a batch of whole tiles (256 columns), then the rest
            same(hip.column_topn(dev, n, block=64, scratch_mb=300 * per_col / 2 ** 20, max_blocks=3), want)


@pytest.mark.parametrize("n", [N, 32])
def test_a_table_tall_enough_for_the_default_sample(hip, n):
    assert 20011 >= 2 * TOPIC_SAMPLE
    t, want = case(20011, 1, 20, n)
    same(hip.column_topn(t.cuda(), n), want)
    same(hip.column_topn(t.cuda(), n, sample=20011), want)      # ... and without it


def test_ties_signed_zeros_nans_and_empty_input(hip):
    for t in (tripled(), edge_table()):
        for n, block in ((5, 4), (1, 4), (32, 64), (5, TOPIC_BLOCK)):
            want = R.column_topn(t, n)
            same(hip.column_topn(t.cuda(), n, block=block), want)
            # a bound taken from every 2nd / 16th row: a value equal to it is still offered, a NaN-only column has none
            same(hip.column_topn(t.cuda(), n, block=block, sample=8), want)
    want = R.column_topn(edge_table(), 5)
    assert want[0][2, :2].tolist() == [9, 20] and int(want[2][4]) == 0      # what the twin's own tests establish
    for W in (1, 6, 300):
        t = torch.zeros((0, W), dtype=torch.float64)
        got = hip.column_topn(t.cuda(), N)
        same(got, R.column_topn(t, N))
        assert tuple(got[0].shape) == (W, N) and not bool(got[2].any())


@pytest.mark.parametrize("K,R_", [(1, 1), (20, 1), (33, 3), (128, 3)])
def test_row_dominant_equals_the_twin(hip, K, R_):
    for rows in (0, 1, 255, 256, 257, 3000):
        t = dominant_case(rows, R_, K)
        want = R.row_dominant(t)
        same(hip.row_dominant(t.cuda()), want)
        if rows == 3000:
            same(hip.row_dominant(t.cuda(), max_blocks=2), want)
            assert int(want[1].sum()) < rows * R_      # an all-NaN member is counted nowhere


@pytest.mark.parametrize("K,R_", [(1, 1), (20, 1), (33, 3), (20, 3)])
def test_topic_sides_equals_the_twin(hip, K, R_):
    for n in (0, 1, 255, 256, 257, 3000):
        th, ph, doc, word = sides_case(n, 37, 50, R_, K)
        want = R.topic_sides(th, ph, doc, word)
        dev = th.cuda(), ph.cuda(), doc.cuda(), word.cuda()
        same(hip.topic_sides(*dev), want)
        if n == 3000:
            same(hip.topic_sides(*dev, max_blocks=2), want)
            assert int((want[0] < 0).sum()) > 100 and int((want[0] >= 0).sum()) > 1000      # misses and NaN rows


def test_wrapper_refusals(hip):
    t, want = case(131, 3, 20, N)
    t = t.cuda()
    call = lambda **kw: hip.column_topn(**{**dict(table=t, n=N, block=64), **kw})   # noqa: E731
    same(call(max_blocks=2), want)      # the positive control: the same arguments, unspoilt
    with pytest.raises(ValueError, match="float64"):
        call(table=t.float())
    with pytest.raises(ValueError, match="contiguous"):
        call(table=torch.cat([t, t])[::2])
    with pytest.raises(ValueError, match="GPU tensor"):
        call(table=t.cpu())
    with pytest.raises(ValueError, match=r"\[rows, W\]"):
        call(table=t.reshape(131, 3, 20))
    for n in (0, 33, -1):
        with pytest.raises(ValueError, match="n must be"):
            call(n=n)
    with pytest.raises(ValueError, match="block"):
        call(block=0)
    with pytest.raises(ValueError, match="scratch_mb"):
        call(scratch_mb=0)
    with pytest.raises(ValueError, match="sample"):
        call(sample=0)
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)
    # row_dominant
    t3 = dominant_case(131, 3, 20).cuda()
    same(hip.row_dominant(t3, max_blocks=2), R.row_dominant(t3.cpu()))
    with pytest.raises(ValueError, match=r"\[rows, R, K\]"):
        hip.row_dominant(t3.reshape(131, 60))
    with pytest.raises(ValueError, match="float64"):
        hip.row_dominant(t3.float())
    with pytest.raises(ValueError, match="contiguous"):
        hip.row_dominant(torch.cat([t3, t3])[::2])
    with pytest.raises(ValueError, match="GPU tensor"):
        hip.row_dominant(t3.cpu())
    with pytest.raises(ValueError, match="R K <="):
        hip.row_dominant(torch.zeros((2, 3, 4096), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="max_blocks"):
        hip.row_dominant(t3, max_blocks=-1)
    # topic_sides
    th, ph, doc, word = (x.cuda() for x in sides_case(65, 37, 50, 3, 20))
    call = lambda **kw: hip.topic_sides(**{**dict(theta3=th, phi3=ph, doc=doc, word=word), **kw})   # noqa: E731
    same(call(max_blocks=2), R.topic_sides(th.cpu(), ph.cpu(), doc.cpu(), word.cpu()))
    for name, rows in (("doc", 37), ("word", 50)):
        bad = (doc if name == "doc" else word).clone()
        bad[9] = rows
        with pytest.raises(ValueError, match=name + ": index out of range"):
            call(**{name: bad})
        bad[9] = -2
        with pytest.raises(ValueError, match=name + ": index out of range"):
            call(**{name: bad})
        with pytest.raises(ValueError, match="int32"):
            call(**{name: bad.long()})
        with pytest.raises(ValueError, match="contiguous"):
            call(**{name: torch.cat([doc, doc])[::2]})
        with pytest.raises(ValueError, match="shape"):
            call(**{name: doc[:-1]})
    with pytest.raises(ValueError, match="float64"):
        call(theta3=th.float())
    with pytest.raises(ValueError, match="row width"):
        call(phi3=ph[:, :2].contiguous())
    with pytest.raises(ValueError, match="GPU tensor"):
        call(phi3=ph.cpu())
    with pytest.raises(ValueError, match=r"\[rows, R, K\]"):
        call(theta3=th.reshape(37, 60))
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)


@pytest.mark.parametrize("kind,compat,scale", [("flow", "strict", 5), ("flow", "fixed", 5), ("dns", "strict", 4),
                                               ("proxy", "fixed", 4)])
def test_day_on_the_hip_backend(kind, compat, scale, tmp_path_factory):
    day = Day(kind, compat, tmp_path_factory.mktemp("topics_gpu_" + kind), backend="hip", device="cuda", scale=scale)
    lp, s = day.run("topics", topic_report=NT)
    check_topic_files(day, lp, s)      # all four files' bits are the CPU twins' over the written tables
    assert (lp / day.results).read_bytes() == (day.run("plain")[0] / day.results).read_bytes()
