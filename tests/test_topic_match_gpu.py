"""--topic-match on the GPU (gfx950): ``ops.hip.column_l1`` (csrc/hip/column_l1.hip) bit for bit its torch twin --
pair counts around every block size, every pair of widths across both tile edges (32 and 64 columns), the identity
form and index arrays with repeats, a reversed order and a gap, tables 8 bytes off a 16-byte boundary, the
grid-stride loops wrapping, scratch batches, no pair, signed zeros, inf and NaN, the wrapper's refusals -- and a
flow, a DNS and a proxy day on the HIP backend against the CPU's files.

The twin's result is computed once per case and shared."""
import functools
import os
import shutil
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal  # noqa: E402
from test_topic_match import FILES, l1_case  # noqa: E402

from oni_ml_amd.config import MATCH_BLOCK  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 20, 33, 100, 128)


@functools.lru_cache(maxsize=None)
def case(M, Wa, Wb, block, special=True):
    """The inputs and the twin's result, computed once and shared (never written to)."""
    A, B, ia, ib = l1_case(M, Wa, Wb, special=special)
    return (A, B, ia, ib), R.column_l1(A, B, ia, ib, block=block)


def same(got, want):
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape and bits_equal(got.cpu(), want)


def cuda(xs):
    return tuple(x.cuda() for x in xs)


def pairs_of(block):
    return sorted({1, 2, block - 1, block, block + 1, 2 * block + 3, 5003} - {0})


@pytest.mark.parametrize("M", sorted({m for b in (4, 64, MATCH_BLOCK) for m in pairs_of(b)}))
def test_every_pair_count_against_every_block(hip, M):
    for block in (4, 64, MATCH_BLOCK):
        if M in pairs_of(block):
            xs, want = case(M, 20, 20, block)
            same(hip.column_l1(*cuda(xs), block=block), want)


@pytest.mark.parametrize("Wa", WIDTHS)
def test_every_pair_of_widths(hip, Wa):
    """Wa and Wb independently: a lane's 2 or 4 columns each way, one and two tiles each way, odd widths (8-byte
    loads) and even ones (16-byte loads)."""
    for Wb in WIDTHS:
        xs, want = case(131, Wa, Wb, 64)
        same(hip.column_l1(*cuda(xs), block=64), want)
        assert hip.column_l1_path(Wa, Wb) == f"tile{32 if Wa <= 32 else 64}x{32 if Wb <= 32 else 64}"


@pytest.mark.parametrize("Wa,Wb", [(20, 160), (160, 20), (100, 50), (50, 100), (64, 65), (32, 33)])
def test_unequal_widths_across_the_tile_edges(hip, Wa, Wb):
    """(20, 160): a member against R K interleaved columns -- one tile against three."""
    xs, want = case(131, Wa, Wb, 64)
    same(hip.column_l1(*cuda(xs), block=64), want)


def test_the_identity_form_and_index_patterns(hip):
    g = torch.Generator().manual_seed(5)
    V = 300
    A = torch.rand(V, 20, generator=g, dtype=torch.float64)
    B = torch.rand(V, 33, generator=g, dtype=torch.float64)
    same(hip.column_l1(A.cuda(), B.cuda(), block=64), R.column_l1(A, B, block=64))
    ar = torch.arange(V)
    patterns = [(ar, ar), (ar.flip(0), ar), (ar[ar % 7 != 3], ar[ar % 7 != 3].flip(0)),      # reversed, a gap
                (torch.zeros(100, dtype=torch.int64), torch.full((100,), V - 1)),          # one row repeated
                (torch.randint(0, V, (500,), generator=g), torch.randint(0, V, (500,), generator=g))]
    for ia, ib in patterns:
        same(hip.column_l1(A.cuda(), B.cuda(), ia.cuda(), ib.cuda(), block=64), R.column_l1(A, B, ia, ib, block=64))
    # the identity is the index form over arange
    assert bits_equal(hip.column_l1(A.cuda(), B.cuda(), block=64).cpu(),
                      hip.column_l1(A.cuda(), B.cuda(), ar.cuda(), ar.cuda(), block=64).cpu())


@pytest.mark.parametrize("Wa,Wb", [(20, 20), (100, 34)])
def test_tables_off_the_16_byte_boundary(hip, Wa, Wb):
    """Even widths take 16-byte loads from an aligned table and 8-byte loads from one 8 bytes off: the same bits."""
    (A, B, ia, ib), want = case(131, Wa, Wb, 64)

    def off(t):
        flat = torch.empty(t.numel() + 1, dtype=torch.float64, device="cuda")
        flat[1:] = t.reshape(-1).cuda()
        v = flat[1:].view(t.shape)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v
    for a, b in ((off(A), B.cuda()), (A.cuda(), off(B)), (off(A), off(B))):
        same(hip.column_l1(a, b, ia.cuda(), ib.cuda(), block=64), want)


def test_grid_stride_and_scratch_batches(hip):
    xs, want = case(5003, 20, 20, 64)
    dev = cuda(xs)
    for mb in (1, 2):
        same(hip.column_l1(*dev, block=64, max_blocks=mb), want)
    # 79 blocks of 3,200 bytes of partials: 20 fit, so four batches continue one another
    same(hip.column_l1(*dev, block=64, scratch_mb=20 * 3200 / (1 << 20)), want)
    same(hip.column_l1(*dev, block=64, scratch_mb=1e-9, max_blocks=1), want)      # a block per batch
    xs, want = case(131, 100, 128, 64)      # four tiles a block: the items wrap too
    same(hip.column_l1(*cuda(xs), block=64, max_blocks=2, scratch_mb=0.2), want)


def test_no_pair_signed_zeros_inf_and_nan(hip):
    A = torch.rand(4, 3, dtype=torch.float64).cuda()
    e = torch.zeros(0, dtype=torch.int64).cuda()
    got = hip.column_l1(A, A[:, :2].contiguous(), e, e)
    assert got.shape == (3, 2) and not got.any() and not torch.signbit(got).any()
    assert hip.column_l1(A[:0].contiguous(), A[:0].contiguous()).shape == (3, 3)
    # every value of one side a signed zero: |(-0.0) - (+0.0)| = +0.0 added to +0.0
    z = torch.tensor([[-0.0, 0.0], [0.0, -0.0]], dtype=torch.float64)
    got = hip.column_l1(z.cuda(), z.cuda())
    assert not got.any() and not torch.signbit(got).any() and bits_equal(got.cpu(), R.column_l1(z, z))
    x = torch.tensor([[float("inf"), 1.0, float("nan")], [2.0, -float("inf"), 0.5]], dtype=torch.float64)
    y = torch.tensor([[float("inf"), 1.0], [2.0, float("inf")]], dtype=torch.float64)
    got = hip.column_l1(x.cuda(), y.cuda()).cpu()
    assert bits_equal(got, R.column_l1(x, y))
    assert torch.isnan(got[0, 0]) and torch.isinf(got[0, 1]) and torch.isnan(got[2]).all() and torch.isinf(got[1, 1])
    # the special values of the shared case reach the sums on both sides
    xs, want = case(9, 3, 3, 4)
    assert torch.isnan(want).any()
    same(hip.column_l1(*cuda(xs), block=4), want)


def test_wrapper_refusals(hip):
    A, B, ia, ib = cuda(l1_case(5, 2, 3))
    assert hip.column_l1(A, B, ia, ib).shape == (2, 3)
    bad = [lambda: hip.column_l1(A.float(), B, ia, ib), lambda: hip.column_l1(A, B.float(), ia, ib),
           lambda: hip.column_l1(A.cpu(), B, ia, ib), lambda: hip.column_l1(A, B.cpu(), ia, ib),
           lambda: hip.column_l1(A, B, ia, None), lambda: hip.column_l1(A, B, None, ib),
           lambda: hip.column_l1(A, B, ia, ib[:3]), lambda: hip.column_l1(A, B),      # identity: heights differ
           lambda: hip.column_l1(A, B, ia.int(), ib), lambda: hip.column_l1(A, B, ia.cpu(), ib),
           lambda: hip.column_l1(A, B, ia + 100, ib), lambda: hip.column_l1(A, B, ia, ib - 100),
           lambda: hip.column_l1(A, B, torch.full_like(ia, A.shape[0]), ib),
           lambda: hip.column_l1(A.t(), B, ia, ib), lambda: hip.column_l1(A[0], B, ia, ib),
           lambda: hip.column_l1(A, B, ia, ib, block=0), lambda: hip.column_l1(A, B, ia, ib, max_blocks=-1),
           lambda: hip.column_l1(A, B, ia, ib, scratch_mb=0)]
    for fn in bad:
        with pytest.raises(ValueError):
            fn()


@pytest.mark.parametrize("kind,compat,scale", [("flow", "strict", 2), ("dns", "strict", 1), ("proxy", "fixed", 1)])
def test_day_on_the_hip_backend(kind, compat, scale, tmp_path_factory):
    """The CPU run: the scoring stage of the same directory resumed on the CPU, from the models the GPU run wrote.
    (The strict flow day is 8,000 events and the results files are compared first: docs/ARCHITECTURE.md, "Open: the
    strict flow bins on the GPU and on the CPU".)"""
    from oni_ml_amd.pipeline import run
    day = Day(kind, compat, tmp_path_factory.mktemp("match_gpu_" + kind), backend="hip", device="cuda", scale=scale)
    prev, _ = day.run("prev", seed=99)
    lp, s = day.run("match", ensemble=3, topic_match_day=str(prev))
    assert s["topic_match_path"] == "hip" and len(s["topic_match_pairs"]) == 3
    assert s["topic_match_shared_hosts"] > 0 and sum(s["host_drift_hist"].values()) == s["topic_match_shared_hosts"]
    cpu = day.root / "cpu"
    shutil.copytree(lp, cpu)
    names = [f"{kind}_{f}.csv" for f in FILES]
    for p in [cpu / ".stages" / f"{kind}_post.done", cpu / day.results] + [cpu / n for n in names]:
        os.unlink(p)
    sc = run(day.cfg(cpu, ensemble=3, topic_match_day=str(prev), resume=True).validate(), device="cpu",
             log=lambda *a: None)
    assert sc["topic_match_path"] == "cpu"
    for k in ("topic_match_pairs", "topic_match_mutual", "host_drift_hist"):
        assert sc[k] == s[k], k
    for f in [day.results] + names:
        assert (cpu / f).read_bytes() == (lp / f).read_bytes(), f
