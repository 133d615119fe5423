"""--holdout on the GPU (gfx950): ``ops.hip.holdout_draw`` and ``ops.hip.holdout_entries`` (csrc/hip/holdout.hip)
bit for bit their torch twins -- entry counts on both sides of the lane share, an entry of a million tokens over many
waves, the grid-stride loops wrapping, empty input, the wrappers' refusals -- then the planted corpus and a flow day on
the HIP backend."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal  # noqa: E402
from test_ensemble import tree as plain_tree  # noqa: E402
from test_holdout import HOLD, planted, planted_cfg, tree  # noqa: E402

from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.models.lda import holdout as HO  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402

pytestmark = pytest.mark.gpu

NNZ = [1, 255, 256, 257, 5003]
FRACTIONS = [2.0 ** -20, 0.2, 0.5]
_TWIN = {}


def draw_case(nnz):
    """(doc_ptr, counts) on the CPU: counts 1, 63, 64, 65 on both sides of the lane share of 64, a zero, a few of
    4,097 (two wave chunks: 4,096 + 1) and, where there is room, one entry of 1,000,003 (245 chunks, atomics)."""
    rng = np.random.default_rng(nnz)
    counts = rng.choice([1, 63, 64, 65], size=nnz)
    if nnz == 1:
        counts[0] = 1_000_003
    else:
        counts[rng.choice(nnz, size=max(1, nnz // 100), replace=False)] = 4097
        counts[nnz // 2], counts[nnz // 3] = 1_000_003, 0
    docs = max(1, nnz // 7)
    cuts = np.sort(rng.integers(0, nnz + 1, size=docs - 1))
    ptr = np.concatenate([[0], cuts, [nnz]])
    return torch.from_numpy(ptr.astype(np.int64)), torch.from_numpy(counts.astype(np.int64))


def twin_draw(nnz, F):
    """The twin's raw draw, computed once per case."""
    if (nnz, F) not in _TWIN:
        ptr, counts = draw_case(nnz)
        _TWIN[nnz, F] = R.holdout_draw(ptr, counts, 11, R.holdout_thr(F), rules=False)
    return _TWIN[nnz, F]


@pytest.mark.parametrize("F", FRACTIONS)
@pytest.mark.parametrize("nnz", NNZ)
def test_holdout_draw_equals_the_twin(hip, nnz, F):
    ptr, counts = draw_case(nnz)
    thr = R.holdout_thr(F)
    want = twin_draw(nnz, F)
    assert int(counts.max()) == 1_000_003 and 0 <= int(want.min()) and bool((want <= counts).all())
    if F >= 0.2:
        assert 0 < int(want.sum()) < int(counts.sum())
    pc, cc = ptr.cuda(), counts.cuda()
    got = hip.holdout_draw(pc, cc, 11, thr, rules=False)
    assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert torch.equal(hip.holdout_draw(pc, cc, 11, thr, max_blocks=2, rules=False).cpu(), want)
    # the lane share moves entries between the two paths, never a token
    for L in (1, 16, 256, 4097):
        assert torch.equal(hip.holdout_draw(pc, cc, 11, thr, rules=False, lane_tokens=L).cpu(), want), L
    # with the document rules: the same function of the raw draw as the twin's
    assert torch.equal(hip.holdout_draw(pc, cc, 11, thr).cpu(), R.holdout_rules(ptr, counts, want))


def test_holdout_draw_empty_input_launches_nothing(hip):
    z = torch.zeros(0, dtype=torch.int64, device="cuda")
    out = hip.holdout_draw(torch.zeros(1, dtype=torch.int64, device="cuda"), z, 0, R.holdout_thr(0.2))
    assert out.numel() == 0 and out.is_cuda and out.dtype == torch.int64
    # documents, all of them empty
    out = hip.holdout_draw(torch.zeros(4, dtype=torch.int64, device="cuda"), z, 0, R.holdout_thr(0.2))
    assert out.numel() == 0
    # entries without tokens
    out = hip.holdout_draw(torch.tensor([0, 3], device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"), 0, 1)
    assert out.tolist() == [0, 0, 0]


def test_holdout_draw_refusals(hip):
    ptr, counts = (x.cuda() for x in draw_case(257))
    thr = R.holdout_thr(0.2)
    call = lambda **kw: hip.holdout_draw(**{**dict(doc_ptr=ptr, counts=counts, seed=11, thr=thr, rules=False), **kw})   # noqa: E731
    assert torch.equal(call().cpu(), twin_draw(257, 0.2))      # the positive control: the same arguments, unspoilt
    assert call(thr=2 ** 52).numel() == 257
    for bad in (0, -1, 2 ** 52 + 1):
        with pytest.raises(ValueError, match="thr"):
            call(thr=bad)
    with pytest.raises(TypeError):
        call(thr=0.2)
    with pytest.raises(ValueError, match="int64"):
        call(counts=counts.int())
    with pytest.raises(ValueError, match="int64"):
        call(doc_ptr=ptr.int())
    with pytest.raises(ValueError, match="GPU"):
        call(counts=counts.cpu())
    with pytest.raises(ValueError, match="GPU"):
        call(doc_ptr=ptr.cpu(), counts=counts.cpu())
    with pytest.raises(ValueError, match="contiguous"):
        call(counts=torch.stack([counts, counts], 1)[:, 0])
    neg = counts.clone()
    neg[5] = -3
    with pytest.raises(ValueError, match=">= 0"):
        call(counts=neg)
    with pytest.raises(ValueError, match="doc_ptr"):
        call(doc_ptr=ptr[:-1].contiguous())
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-1)
    with pytest.raises(ValueError, match="lane_tokens"):
        call(lane_tokens=0)


# ------------------------------------------------------------------------------------------ the entries
def entries_case(K, n=5003, D=301, V=211):
    g = torch.Generator().manual_seed(200 + K)
    th = torch.rand(D, K, dtype=torch.float64, generator=g)
    th = th / th.sum(1, keepdim=True)
    ph = torch.rand(V, K, dtype=torch.float64, generator=g) * 10.0 ** torch.randint(-9, 0, (V, 1), generator=g).double()
    ph[7] = math.exp(-100.0)                      # a word no topic has: lda-c's floor in every column
    lens = torch.bincount(torch.randint(0, D, (n,), generator=g), minlength=D)      # n entries over D documents
    lens[5] += lens[6]
    lens[6] = 0                                   # an empty document
    ptr = torch.zeros(D + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(lens, 0)
    doc = torch.repeat_interleave(torch.arange(D), lens).to(torch.int32)
    word = torch.randint(0, V, (n,), generator=g, dtype=torch.int32)
    word[:50] = 7
    t = torch.randint(0, 4, (n,), generator=g, dtype=torch.int64)      # a quarter of the entries at t = 0
    t[3] = 1_000_003
    seen = (torch.rand(V, generator=g) < 0.9).to(torch.uint8)          # a tenth of the words unseen in training
    seen[7] = 1
    return th, ph, ptr, doc, word, t, seen


@pytest.mark.parametrize("K", [1, 3, 20, 33, 100])
def test_holdout_entries_and_the_sums_equal_the_twin(hip, K):
    th, ph, ptr, doc, word, t, seen = entries_case(K)
    n, D = doc.numel(), th.shape[0]
    want = R.holdout_entries(th, ph, doc, word, t, seen)
    used = (t > 0) & (seen[word.long()] != 0)
    assert 0 < int(used.sum()) < n and bool((want[~used] == 0).all()) and bool((want[used] < 0).all())
    assert bool((t[:50] > 0).any()) and bool((want[:50][t[:50] > 0] < -90.0).all())      # the floor row: about -100 a token
    assert int((seen == 0).sum()) > 0 and int(((t > 0) & (seen[word.long()] == 0)).sum()) > 0
    c = [x.cuda() for x in (th, ph, doc, word, t, seen)]
    got = hip.holdout_entries(*c)
    assert bits_equal(got.cpu(), want)
    assert bits_equal(hip.holdout_entries(*c, max_blocks=2).cpu(), want)
    # per document, then the total: group_rows_sum at width 1, against the twin's
    order = torch.arange(n, dtype=torch.int32)
    doc_want = R.group_rows_sum(want.unsqueeze(1), order, ptr[:-1], ptr[1:])
    tot_want = R.group_rows_sum(doc_want, torch.arange(D, dtype=torch.int32), torch.zeros(1, dtype=torch.int64),
                                torch.full((1,), D, dtype=torch.int64))
    pc = ptr.cuda()
    doc_got = hip.group_rows_sum(got.unsqueeze(1), order.cuda(), pc[:-1].contiguous(), pc[1:].contiguous())
    tot_got = hip.group_rows_sum(doc_got, torch.arange(D, dtype=torch.int32, device="cuda"),
                                 torch.zeros(1, dtype=torch.int64, device="cuda"),
                                 torch.full((1,), D, dtype=torch.int64, device="cuda"))
    assert bits_equal(doc_got.cpu(), doc_want) and bits_equal(tot_got.cpu(), tot_want)
    assert tot_want.item() < 0 and abs(tot_want.item() - float(want.sum())) < 1e-9 * abs(tot_want.item())


def test_holdout_entries_empty_and_refusals(hip):
    th, ph, ptr, doc, word, t, seen = (x.cuda() for x in entries_case(20))
    want = R.holdout_entries(*(x.cpu() for x in (th, ph, doc, word, t, seen)))
    a = dict(theta=th, phi=ph, doc=doc, word=word, t=t, word_seen=seen)
    call = lambda **kw: hip.holdout_entries(**{**a, **kw})      # noqa: E731
    assert bits_equal(call().cpu(), want)      # the positive control
    out = call(doc=doc[:0], word=word[:0], t=t[:0])
    assert out.numel() == 0 and out.is_cuda
    with pytest.raises(ValueError, match="float64"):
        call(theta=th.float())
    with pytest.raises(ValueError, match="float64"):
        call(phi=ph.float())
    with pytest.raises(ValueError, match="row widths"):
        call(phi=ph[:, :19].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        call(theta=th.t().contiguous().t())
    with pytest.raises(ValueError, match="GPU"):
        call(theta=th.cpu())
    with pytest.raises(ValueError, match="GPU"):
        call(phi=ph.cpu())
    with pytest.raises(ValueError, match="int32"):
        call(word=word.long())
    with pytest.raises(ValueError, match="int64"):
        call(t=t.int())
    with pytest.raises(ValueError, match="uint8"):
        call(word_seen=seen.bool())
    with pytest.raises(ValueError, match="shape"):
        call(word_seen=seen[:-1].contiguous())
    with pytest.raises(ValueError, match="shape"):
        call(t=t[:-1].contiguous())
    for name, idx, lim in (("word", word, ph.shape[0]), ("doc", doc, th.shape[0])):
        for v in (lim, -1):      # no -1 here: every entry has its document and its word
            bad = idx.clone()
            bad[9] = v
            with pytest.raises(ValueError, match=f"{name}: index out of range"):
                call(**{name: bad})
    with pytest.raises(ValueError, match="max_blocks"):
        call(max_blocks=-2)


# ---------------------------------------------------------------------------- the HIP backend, end to end
def test_planted_corpus_on_the_hip_backend(hip, tmp_path):
    c = planted()
    cfg = planted_cfg(tmp_path)
    cfg.backend = "hip"
    out = C.run_holdout(cfg, c, device="cuda", log=lambda *a, **k: None)
    recs = out["records"]
    print("holdout on the planted corpus, HIP backend:", [(r["topics"], r["perplexity"], r["unseen_tokens"]) for r in recs])
    held = out["split"]["heldout_tokens"]
    assert [r["topics"] for r in recs] == [4, 8, 32] and all(r["unseen_tokens"] <= 0.01 * held for r in recs)
    assert out["selected"] == 8
    # the split is the CPU path's, and the record of every fit is the twins' bit for bit from the same gamma and beta
    from oni_ml_amd.models.lda.estimate import load_final
    train_c, t_c = HO.split(c, 0.2, 0, "cpu")
    train_g, t_g = HO.split(c, 0.2, 0, "cuda")
    assert torch.equal(t_g.cpu(), t_c) and np.array_equal(train_g.doc_ptr, train_c.doc_ptr)
    assert np.array_equal(train_g.word_idx, train_c.word_idx) and np.array_equal(train_g.counts, train_c.counts)
    for r in recs:
        g, lb = load_final(str(tmp_path / "holdout" / f"k{r['topics']}"))
        for dev, twin in (("cpu", False), ("cuda", True), ("cuda", False)):
            again = HO.evaluate(c, train_c, t_c, g, lb, dev, twin=twin)
            for k in ("heldout_tokens", "unseen_tokens", "evaluated_tokens", "split_documents", "loglik",
                      "loglik_per_token", "perplexity"):
                assert again[k] == r[k], (r["topics"], dev, twin, k)


def test_a_flow_day_on_the_hip_backend(hip, tmp_path_factory):
    day = Day("flow", "fixed", tmp_path_factory.mktemp("holdout_gpu_flow"), backend="hip", device="cuda")
    plain, _ = day.run("plain")
    hold, sh = day.run("hold", **HOLD)
    a, b = plain_tree(plain), tree(hold)
    assert len(a) >= 12 and day.results in a and "final.beta" in a
    for f in a:
        assert a[f] == b[f], f
    h = sh["holdout"]
    assert h["topics"] == [10, 20] and h["selected"] in (10, 20) and all(p > 1.0 for p in h["perplexity"])
    j = json.loads((hold / "holdout" / "holdout.json").read_text())
    assert [r["topics"] for r in j["records"]] == [10, 20] and j["key"]["fraction"] == CFG.RunConfig(holdout=0.2).holdout
