"""--tail-tol on the GPU (gfx950): ``ops.hip.tail_mass_docs`` (csrc/hip/tail_docs.hip) bit for bit the CPU twin
``ops.reference.tail_mass`` -- the document layouts a tile of 256 pairs can meet (one document, a document per pair,
runs that straddle the tile edges, 255 / 256 / 257 documents before a long run, a repeated pair), pair counts around
a tile, vocabulary sizes around the block size, every width of the register ladder on an aligned and on a shifted
phi table, the refusals, the grid-stride wrap, several scratch batches -- ``scorer.tail_pairs``' dispatch, and a
flow, a DNS and a proxy day flagged and ranked by the tail on the HIP backend.

Every oracle is the twin on the CPU, computed once per case and shared (never written to)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day  # noqa: E402
from test_tail import tail_case  # noqa: E402
from test_tail_gpu import same4  # noqa: E402
from test_tail_rank import check_ranked_by_tail, oracle_of  # noqa: E402

from oni_ml_amd.config import TAIL_BLOCK  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

pytestmark = pytest.mark.gpu

N = 1031


def by_doc(doc, word):
    """The pairs sorted by (document, word), as ``SG.unique`` of the keys d * V + w returns them (repeats kept)."""
    o = torch.argsort(doc.to(torch.int64) * (1 << 31) + word.to(torch.int64), stable=True)
    return doc[o].contiguous(), word[o].contiguous()


@functools.lru_cache(maxsize=None)
def case(V, R_, K, n, block, nan=False, D=37):
    """``tail_case`` with the -1 sides dropped and the pairs sorted by (doc, word), and the twin's result."""
    th, ph, doc, word = tail_case(V, R_, K, n, D=D, nan=nan)
    ok = (doc >= 0) & (word >= 0)
    doc, word = by_doc(doc[ok], word[ok])
    a = (th, ph, doc, word)
    return a, R.tail_mass(*a, block=block)


def runs(lengths, n):
    """Documents 0, 1, ... of the given lengths, cycled, cut at n pairs."""
    out, d = [], 0
    while len(out) < n:
        out += [d] * lengths[d % len(lengths)]
        d += 1
    return torch.tensor(out[:n], dtype=torch.int32)


LAYOUTS = {
    "one document": lambda: torch.zeros(N, dtype=torch.int32),
    "a document per pair": lambda: torch.arange(N, dtype=torch.int32),
    "runs over the tile edges": lambda: runs([1, 2, 3, 5, 40, 300], N),
    "255 then 300": lambda: torch.cat([torch.arange(255), torch.full((300,), 255)]).to(torch.int32),
    "256 then 300": lambda: torch.cat([torch.arange(256), torch.full((300,), 256)]).to(torch.int32),
    "257 then 300": lambda: torch.cat([torch.arange(257), torch.full((300,), 257)]).to(torch.int32),
}


@functools.lru_cache(maxsize=None)
def layout(name, repeat=False):
    """V = 131, (R, K) = (1, 20), D = 1031 documents; the words of ``tail_case`` (its -1 dropped) under the
    layout's documents.  ``repeat``: one pair of every eighth document's is written twice, adjacently."""
    th, ph, _, word = tail_case(131, 1, 20, 1300, D=N)
    doc = LAYOUTS[name]()
    word = word[word >= 0][:doc.numel()]
    assert word.numel() == doc.numel()
    doc, word = by_doc(doc, word)
    if repeat:
        same = torch.nonzero((doc[1:] == doc[:-1]) & (doc[1:] % 8 == 0)).reshape(-1)
        assert same.numel() > 20
        word[same + 1] = word[same]
        doc, word = by_doc(doc, word)
        assert int(((doc[1:] == doc[:-1]) & (word[1:] == word[:-1])).sum()) > 20
    a = (th, ph, doc, word)
    return a, R.tail_mass(*a, block=64)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_document_layouts(hip, name):
    a, want = layout(name)
    edges = int((a[2][1:] != a[2][:-1]).sum()) + 1
    assert edges == {"one document": 1, "a document per pair": N, "255 then 300": 256, "256 then 300": 257,
                     "257 then 300": 258}.get(name, edges)
    same4(hip.tail_mass_docs(*(x.cuda() for x in a), block=64), want)


def test_a_repeated_pair_has_the_same_bits(hip):
    a, want = layout("runs over the tile edges", True)
    got = hip.tail_mass_docs(*(x.cuda() for x in a), block=64)
    same4(got, want)
    rep = torch.nonzero((a[2][1:] == a[2][:-1]) & (a[3][1:] == a[3][:-1])).reshape(-1).cuda()
    for g in got:
        assert torch.equal(g[rep].view(torch.int64 if g.dtype == torch.float64 else g.dtype),
                           g[rep + 1].view(torch.int64 if g.dtype == torch.float64 else g.dtype))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_pair_counts_around_a_tile(hip, n):
    (th, ph, doc, word), _ = case(131, 1, 20, N, 64)
    a = (th, ph, doc[:n].contiguous(), word[:n].contiguous())
    got = hip.tail_mass_docs(*(x.cuda() for x in a), block=64)
    assert all(tuple(g.shape) == (n,) for g in got)
    same4(got, R.tail_mass(*a, block=64))


def vs_of(block):
    return [1, block - 1, block, block + 1, 2 * block + 3, 5003]


@pytest.mark.parametrize("R_,K", [(1, 20), (3, 3)])
@pytest.mark.parametrize("block", [4, 64, TAIL_BLOCK])
def test_every_vocabulary_size_against_every_block(hip, block, R_, K):
    """The mixed layout: 37 documents of about 22 pairs each, so a tile holds a dozen documents; at block 64 a NaN
    phi row (every total NaN, the counts unchanged)."""
    assert TAIL_BLOCK == 1024
    for V in vs_of(block):
        a, want = case(V, R_, K, N, block, block == 64)
        assert a[2].numel() > 700 and int(a[2].min()) >= 0 and int(a[3].min()) >= 0
        assert V < 12 or block != 64 or bool(torch.isnan(want[1]).all())
        same4(hip.tail_mass_docs(*(x.cuda() for x in a), block=block), want)


LADDER = [(1, 1), (1, 2), (1, 3), (1, 20), (1, 33), (1, 100), (3, 1), (3, 3), (3, 20)]
OFF = [(1, 128), (3, 33), (3, 100)]


@pytest.mark.parametrize("R_,K", LADDER)
def test_every_ladder_width(hip, R_, K):
    """(1, 100) is the 240-VGPR form of the ladder; odd K stages by scalars, even K by 16 bytes -- unless the table
    lies 8 bytes off a 16-byte boundary."""
    assert hip.tail_theta_path(R_, K) == "registers"
    a, want = case(131, R_, K, N, 64, R_ == 3)
    dev = [x.cuda() for x in a]
    same4(hip.tail_mass_docs(*dev, block=64), want)
    buf = torch.empty(a[1].numel() + 1, dtype=torch.float64, device="cuda")
    sh = buf[1:].view(a[1].shape)
    sh.copy_(dev[1])
    assert sh.is_contiguous() and sh.data_ptr() % 16 == 8
    same4(hip.tail_mass_docs(dev[0], sh, dev[2], dev[3], block=64), want)


@pytest.mark.parametrize("R_,K", OFF)
def test_widths_off_the_ladder_are_refused_and_dispatched_to_tail_mass(hip, R_, K):
    assert hip.tail_theta_path(R_, K) != "registers"
    a, _ = case(131, R_, K, N, 64)
    th, ph, doc, word = (x.cuda() for x in a)
    with pytest.raises(ValueError, match="register ladder"):
        hip.tail_mass_docs(th, ph, doc, word, block=64)
    model = S.EnsembleModel(th, ph, R_, K, 0.05)
    got, path = S.tail_pairs(model, doc.long(), word.long())
    assert path == "pairs"
    same4(got, R.tail_mass(*a))      # (config.TAIL_BLOCK: what the dispatcher runs with)


def test_the_dispatch_is_invisible(hip, monkeypatch):
    """Many pairs per document: the shared-vector kernel; a pair per document: ``tail_mass``; the CPU: the twin.
    The same bits from all three."""
    from oni_ml_amd import config as CFG
    a, _ = case(131, 1, 20, N, 64)
    want = R.tail_mass(*a)
    model = S.TopicModel(a[0][:, 0].contiguous().cuda(), a[1][:, 0].contiguous().cuda(), 20, 0.05)
    monkeypatch.setattr(CFG, "TAIL_DOCS_MIN_SHARE", 2.0)      # (a measured value: the test does not depend on it)
    got, path = S.tail_pairs(model, a[2].cuda().long(), a[3].cuda().long())
    assert path == "docs"
    same4(got, want)
    b, want1 = layout("a document per pair")
    model1 = S.TopicModel(b[0][:, 0].contiguous().cuda(), b[1][:, 0].contiguous().cuda(), 20, 0.05)
    got, path = S.tail_pairs(model1, b[2].cuda().long(), b[3].cuda().long())
    assert path == "pairs"
    same4(got, R.tail_mass(*b))
    cpu, path = S.tail_pairs(S.TopicModel(a[0][:, 0].contiguous(), a[1][:, 0].contiguous(), 20, 0.05),
                             a[2].long(), a[3].long())
    assert path == "cpu"
    same4([x.cuda() for x in cpu], want)


def test_refusals(hip):
    a, want = case(131, 3, 20, 200, 64)
    th, ph, doc, word = (x.cuda() for x in a)
    n = doc.numel()
    call = lambda **kw: hip.tail_mass_docs(**{**dict(theta=th, phi=ph, doc=doc, word=word, block=64), **kw})  # noqa: E731
    same4(call(max_blocks=2), want)      # the positive control: the same arguments, unspoilt
    bad = doc.clone()
    bad[9], bad[10] = doc[n - 1], doc[0]
    assert int(doc[n - 1]) > int(doc[0])
    with pytest.raises(ValueError, match="non-decreasing"):
        call(doc=bad)
    for name, t, lim in (("doc", doc, 37), ("word", word, 131)):
        for v in (-1, -2, lim):
            bad = t.clone()
            bad[n - 1 if v == lim else 0] = v      # (the documents stay sorted: the bound alone is at fault)
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
    with pytest.raises(ValueError, match="expected"):
        call(doc=doc.cpu())
    with pytest.raises(ValueError):
        call(word=word[:-1])
    with pytest.raises(ValueError, match="block"):
        call(block=0)
    with pytest.raises(ValueError, match="scratch_mb"):
        call(scratch_mb=0)
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)


@pytest.mark.parametrize("R_,K", [(1, 20), (3, 20)])
def test_grid_stride_batches_and_tail_mass_agree(hip, R_, K):
    a, want = case(131, R_, K, 3000, 64)
    dev = [x.cuda() for x in a]
    assert a[2].numel() > 2300
    same4(hip.tail_mass_docs(*dev, block=64, max_blocks=2), want)
    # a scratch of 600 pairs' partials (3 blocks x 24 bytes each): batches of 512 pairs, cut inside a document
    # (37 documents of about 65 pairs)
    assert int(a[2][511]) == int(a[2][512])
    same4(hip.tail_mass_docs(*dev, block=64, scratch_mb=600 * 3 * 24 / 2 ** 20), want)
    same4(hip.tail_mass_docs(*dev, block=64), [x.cpu() for x in hip.tail_mass(*dev, block=64)])


@pytest.mark.parametrize("kind,compat,scale", [("flow", "strict", 5), ("flow", "fixed", 5), ("dns", "strict", 4),
                                               ("proxy", "fixed", 4)])
def test_day_on_the_hip_backend(kind, compat, scale, tmp_path_factory):
    day = Day(kind, compat, tmp_path_factory.mktemp("tail_rank_gpu_" + kind), backend="hip", device="cuda",
              scale=scale)
    keys, P = oracle_of(day)
    lp, s = day.run("tail_tol", tail_tol=P)
    check_ranked_by_tail(day, lp, s, keys, P)
    assert s["tail_rank_path"] in ("docs", "pairs")
