"""--holdout on the CPU path: the torch twins (``ops.reference`` splitmix64, holdout_draw, holdout_rules, log_rn,
holdout_entries), the split and its training corpus, the selection on a planted corpus with the C++ engine, and a
flow day end to end on the torch LDA backend -- the plain run's files byte for byte, the records, resume at every
stage boundary, --holdout-select against a plain ``--topics K*`` run, the refusals and the ways to set the options.

"Byte-identical" leaves out what carries wall-clock times (``test_ensemble.TIMED``, the completion markers) and, in
holdout.json, the ``seconds`` entries."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import TIMED, Day  # noqa: E402
from test_ensemble import tree as plain_tree  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.corpus.csr import Corpus  # noqa: E402
from oni_ml_amd.models.lda import holdout as HO  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402

i64 = lambda x: torch.tensor(x, dtype=torch.int64)      # noqa: E731


# ------------------------------------------------------------------------------------------------ log_rn
def log_points(seed=7):
    """1e-300 .. 2, dense near 1, exact powers of two."""
    rng = np.random.default_rng(seed)
    return np.concatenate([10.0 ** rng.uniform(-300, math.log10(2.0), 400_000),
                           1.0 + rng.uniform(-1e-3, 1e-3, 400_000), 1.0 + rng.uniform(-1e-9, 1e-9, 20_000),
                           rng.uniform(0.45, 2.0, 200_000), 2.0 ** np.arange(-996, 2), np.asarray([1e-300, 2.0, 1.0])])


def test_log_rn_is_within_3_ulp_of_numpy_log():
    y = log_points()
    got = R.log_rn(torch.from_numpy(y)).numpy()
    want = np.log(y)
    ulp = np.spacing(np.abs(want))
    err = np.abs(got - want) / np.where(want == 0.0, 5e-324, ulp)
    worst = float(err.max())
    print("log_rn: largest distance from numpy.log", worst, "ulp at", y[err.argmax()])
    assert worst <= 3.0
    assert got[y == 1.0].tolist() == [0.0] * int((y == 1.0).sum())      # log 1 is exactly +0.0


def test_log_rn_is_the_written_sequence():
    """One value by hand, in Python floats (every operation one correctly rounded double operation)."""
    for y in (0.3, 0.71, 1.5, 3.7e-44, 1.0 - 2.0 ** -53):
        m, e = math.frexp(y)
        if m < 0.70710678118654752:
            m, e = m + m, e - 1
        f = (m - 1.0) / (m + 1.0)
        s = f * f
        P = 2.0 / 23.0
        for i in range(9, -1, -1):
            P = P * s
            P = P + 2.0 / (2 * i + 3)
        r = (f * s) * P + (f + f)
        r = e * 1.90821492927058770002e-10 + r
        want = e * 6.93147180369123816490e-01 + r
        assert R.log_rn(torch.tensor([y], dtype=torch.float64)).item() == want, y


# ---------------------------------------------------------------------------------------------- the draw
def test_splitmix64_twin_is_the_python_integers():
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-2 ** 63, 2 ** 63 - 1, (2000,), generator=g, dtype=torch.int64)
    x[:4] = i64([0, -1, 2 ** 63 - 1, -2 ** 63])
    want = [R._as_i64(R.splitmix64_int(v & R._M64)) for v in x.tolist()]
    assert R.splitmix64(x).tolist() == want
    assert R.splitmix64_int(0) == 0xE220A8397B1DCDAF      # the published first output of splitmix64 from state 0
    # the native random start still draws from the same generator (the shared header changed no bit)
    from oni_ml_amd.ops import native
    cw = native.lib().random_ss(2, 5, 9, 1)
    s = R.splitmix64_int(9)
    assert cw[1, 3] == 1.0 / 5 + (R.splitmix64_int(s ^ 8) >> 11) * 2.0 ** -53


def loop_draw(counts, seed, thr):
    key = R.holdout_key(seed)
    out, g = [], 0
    for c in counts:
        n = 0
        for _ in range(c):
            n += (R.splitmix64_int(key ^ g) >> 11) < thr
            g += 1
        out.append(n)
    return out


def draw_case():
    """About 200 entries over 40 documents (one empty): counts 1, 63, 64, 65, a zero and one of 5,000."""
    rng = np.random.default_rng(5)
    counts = rng.choice([1, 63, 64, 65], size=200).tolist()
    counts[17], counts[101] = 5000, 0
    cuts = np.sort(rng.choice(np.arange(1, 200), size=38, replace=False)).tolist()
    ptr = [0] + cuts + [200, 200]
    return i64(ptr), i64(counts)


@pytest.mark.parametrize("F", [0.2, 0.5, 2.0 ** -8])
def test_draw_equals_a_python_loop_over_the_tokens(F):
    ptr, counts = draw_case()
    thr = R.holdout_thr(F)
    assert thr == int(F * 2 ** 53) and 0 < thr <= 2 ** 52
    want = loop_draw(counts.tolist(), 3, thr)
    got = R.holdout_draw(ptr, counts, 3, thr, rules=False)
    assert got.tolist() == want and got.dtype == torch.int64
    assert 0 < sum(want) < int(counts.sum()) and want[101] == 0
    assert R.holdout_draw(ptr, counts, 3, thr, rules=False, chunk=97).tolist() == want      # the walk's chunks
    assert R.holdout_draw(ptr, counts, 4, thr, rules=False).tolist() != want               # the seed takes part
    # nothing but (seed, F, corpus): the documents' cuts do not
    assert R.holdout_draw(i64([0, 200]), counts, 3, thr, rules=False).tolist() == want


def test_draw_refusals():
    ptr, counts = draw_case()
    thr = R.holdout_thr(0.2)
    ok = lambda **kw: R.holdout_draw(**{**dict(doc_ptr=ptr, counts=counts, seed=1, thr=thr), **kw})      # noqa: E731
    assert ok().numel() == 200      # the positive control
    assert ok(thr=2 ** 52).numel() == 200 and ok(thr=1).sum() == 0
    for bad in (dict(thr=0), dict(thr=2 ** 52 + 1), dict(thr=-1)):
        with pytest.raises(ValueError, match="thr"):
            ok(**bad)
    with pytest.raises(TypeError):
        ok(thr=0.5)
    with pytest.raises(ValueError, match="int64"):
        ok(counts=counts.int())
    with pytest.raises(ValueError, match="contiguous"):
        ok(counts=torch.stack([counts, counts], 1)[:, 0])
    neg = counts.clone()
    neg[3] = -1
    with pytest.raises(ValueError, match=">= 0"):
        ok(counts=neg)
    with pytest.raises(ValueError, match="doc_ptr"):
        ok(doc_ptr=ptr[:-2])
    down = ptr.clone()
    down[3], down[4] = ptr[4], ptr[3]
    with pytest.raises(ValueError, match="non-decreasing"):
        ok(doc_ptr=down)


# ------------------------------------------------------------------------------------- the document rules
def test_document_rules():
    n = 5000
    F = 0.5
    thr = R.holdout_thr(F)
    # 5,000 one-entry documents of exactly 10 tokens, then 300 of 9 tokens
    counts = i64([10] * n + [9] * 300)
    ptr = torch.arange(n + 301, dtype=torch.int64)
    raw = R.holdout_draw(ptr, counts, 0, thr, rules=False)
    got = R.holdout_draw(ptr, counts, 0, thr)
    whole = (raw[:n] == 10)
    assert int(whole.sum()) >= 1      # each with probability 2^-10: the draw made some
    assert int((got[:n] == 10).sum()) == 0 and torch.equal(got[:n][whole], torch.zeros_like(got[:n][whole]))
    assert torch.equal(got[:n][~whole], raw[:n][~whole])      # every other document keeps its draw
    assert int(raw[n:].sum()) > 0 and int(got[n:].sum()) == 0      # 9 tokens: untouched
    # the held-out share of the eligible tokens, five sigma.  (The rule removes the wholly drawn documents, 10 tokens
    # each with probability 2^-10: the raw draw is what the binomial bound is about.)
    N = 10 * n
    assert abs(int(raw[:n].sum()) / N - F) <= 5 * math.sqrt(F * (1 - F) / N)
    for F2 in (0.2, 0.05):
        r2 = R.holdout_draw(ptr, counts, 1, R.holdout_thr(F2), rules=False)
        assert abs(int(r2[:n].sum()) / N - F2) <= 5 * math.sqrt(F2 * (1 - F2) / N)
    # a document of several entries, all of them drawn: all given back; min_tokens counts tokens, not entries
    ptr2, c2 = i64([0, 3, 5, 5, 6]), i64([4, 4, 4, 2, 7, 20])
    t2 = i64([4, 4, 4, 1, 3, 20])
    assert R.holdout_rules(ptr2, c2, t2).tolist() == [0, 0, 0, 0, 0, 0]      # all drawn; 9 tokens; empty; all drawn
    assert R.holdout_rules(ptr2, c2, i64([4, 4, 3, 1, 3, 19])).tolist() == [4, 4, 3, 0, 0, 19]
    assert R.holdout_rules(ptr2, c2, i64([4, 4, 3, 1, 3, 19]), min_tokens=9).tolist() == [4, 4, 3, 1, 3, 19]


# ------------------------------------------------------------------------------------- the training corpus
def planted():
    from oni_ml_amd.synth.corpus import planted_corpus
    return planted_corpus(num_docs=600, num_terms=300, num_topics=8, mean_tokens=40, seed=3)


def test_training_corpus():
    c = planted()
    assert (c.num_docs, c.num_terms, int(c.counts.sum())) == (600, 293, 23997)
    train, t = HO.split(c, 0.2, 0, "cpu")
    t = t.numpy()
    assert isinstance(train, Corpus)      # its own checks ran in __post_init__
    Corpus(train.doc_ptr, train.word_idx, train.counts, train.num_terms)
    assert train.num_docs == c.num_docs and train.num_terms == c.num_terms
    assert (np.diff(train.doc_ptr) > 0).all() and (train.counts > 0).all()
    assert (t >= 0).all() and (t <= c.counts).all() and 0 < t.sum() < c.counts.sum()
    # train plus held-out is the original, entry by entry
    back = np.zeros((c.num_docs, c.num_terms), np.int64)
    orig = np.zeros_like(back)
    doc_of = np.repeat(np.arange(c.num_docs), np.diff(c.doc_ptr))
    np.add.at(orig, (doc_of, c.word_idx), c.counts)
    np.add.at(back, (doc_of, c.word_idx), t)
    np.add.at(back, (np.repeat(np.arange(train.num_docs), np.diff(train.doc_ptr)), train.word_idx), train.counts)
    assert (back == orig).all()
    # word order inside a document is kept
    keep = c.counts - t > 0
    assert (train.word_idx == c.word_idx[keep]).all() and (train.counts == (c.counts - t)[keep]).all()
    # documents under 10 tokens are whole
    from oni_ml_amd.synth.corpus import planted_corpus
    c2 = planted_corpus(num_docs=400, num_terms=100, num_topics=4, mean_tokens=12, seed=1)
    tr2, t2 = HO.split(c2, 0.3, 0, "cpu")
    per_doc = np.add.reduceat(t2.numpy(), c2.doc_ptr[:-1])
    small = c2.totals() < CFG.HOLDOUT_MIN_TOKENS
    assert small.sum() > 20 and (~small).sum() > 20 and (per_doc[small] == 0).all() and (per_doc[~small] > 0).any()
    assert (np.diff(tr2.doc_ptr) > 0).all() and (per_doc < c2.totals()).all()
    tal = HO.split_tallies(c, train, torch.from_numpy(t))
    assert tal["heldout_tokens"] + tal["train_tokens"] == tal["tokens"] == 23997
    # the split depends on the seed and on F
    assert not np.array_equal(HO.split(c, 0.2, 1, "cpu")[1].numpy(), t)
    for bad in (0.0, 0.51, -0.1, float("nan")):
        with pytest.raises(ValueError, match="holdout"):
            HO.split(c, bad, 0, "cpu")


def test_entries_twin_by_hand():
    th = torch.tensor([[0.25, 0.75], [0.5, 0.5]], dtype=torch.float64)
    ph = torch.tensor([[0.1, 0.2], [0.3, 0.4], [math.exp(-100.0), math.exp(-100.0)]], dtype=torch.float64)
    doc, word = torch.tensor([0, 0, 1, 1], dtype=torch.int32), torch.tensor([0, 1, 2, 1], dtype=torch.int32)
    t = i64([3, 0, 2, 5])
    seen = torch.tensor([1, 0, 1], dtype=torch.uint8)
    got = R.holdout_entries(th, ph, doc, word, t, seen)
    s0 = (0.0 + 0.25 * 0.1) + 0.75 * 0.2
    s2 = (0.0 + 0.5 * math.exp(-100.0)) + 0.5 * math.exp(-100.0)
    lg = lambda v: R.log_rn(torch.tensor([v], dtype=torch.float64)).item()      # noqa: E731
    assert got.tolist() == [3.0 * lg(s0), 0.0, 2.0 * lg(s2), 0.0]      # t = 0; a word unseen in training
    assert abs(got[2].item() - 2 * -100.0) < 1e-9


# --------------------------------------------------------------------------------------------- selection
def planted_cfg(lpath, **kw):
    from oni_ml_amd.models.lda.settings import LDASettings
    cfg = CFG.RunConfig(fdate="20160122", dsource="flow", lpath=str(lpath), flow_path="unused", backend="cpu",
                        compat="fixed", holdout=0.2, holdout_topics="4,8,32", verbose=False, **kw)
    cfg.settings = LDASettings()
    return cfg.validate()


def test_planted_corpus_selects_its_topic_count(tmp_path):
    c = planted()
    logs = []
    out = C.run_holdout(planted_cfg(tmp_path), c, device="cpu", log=logs.append)
    recs = out["records"]
    print("holdout on the planted corpus:", [(r["topics"], r["perplexity"], r["unseen_tokens"]) for r in recs])
    assert [r["topics"] for r in recs] == [4, 8, 32] and all(tuple(r) == HO.RECORD_KEYS for r in recs)
    held = out["split"]["heldout_tokens"]
    assert all(r["heldout_tokens"] == held and r["unseen_tokens"] <= 0.01 * held for r in recs)
    assert all(r["evaluated_tokens"] == held - r["unseen_tokens"] for r in recs)
    assert all(r["perplexity"] == math.exp(-r["loglik"] / r["evaluated_tokens"]) for r in recs)
    assert out["selected"] == 8
    assert out["key"] == dict(fraction=0.2, topics=[4, 8, 32], seed=0, alpha_init=2.5, start="random", compat="fixed",
                              docs=600, terms=293, nnz=c.nnz)
    assert len(logs) == 3
    lines = (tmp_path / "holdout" / "holdout.csv").read_text().split("\n")
    assert lines[0] == ",".join(C.HOLDOUT_CSV) and lines[-1] == "" and len(lines) == 5
    for ln, r in zip(lines[1:], recs):
        f = ln.split(",")
        assert int(f[0]) == r["topics"] and float(f[-1]) == r["perplexity"] and float(f[8]) == r["loglik"]
    assert json.loads((tmp_path / "holdout" / "holdout.json").read_text()) == json.loads(json.dumps(out))
    for K in (4, 8, 32):
        have = set(os.listdir(tmp_path / "holdout" / f"k{K}"))
        assert {"final.beta", "final.gamma", "final.other", "likelihood.dat", "final_model.npz"} <= have
        assert "word-assignments.dat" not in have and not [f for f in have if f[:3].isdigit() and f[:3] != "000"]
    # the record again from the fit's files: evaluate is a function of (corpus, split, gamma, log beta)
    from oni_ml_amd.models.lda.estimate import load_final
    train, t = HO.split(c, 0.2, 0, "cpu")
    g, lb = load_final(str(tmp_path / "holdout" / "k8"))
    again = HO.evaluate(c, train, t, g, lb, "cpu")
    assert again["loglik"] == recs[1]["loglik"] and again["perplexity"] == recs[1]["perplexity"]


def test_select_takes_the_lowest_and_on_a_tie_the_smaller():
    r = lambda k, p: dict(topics=k, perplexity=p)      # noqa: E731
    assert HO.select([r(4, 9.0), r(8, 7.0), r(32, 8.0)]) == 8
    assert HO.select([r(30, 7.0), r(10, 7.0), r(20, 7.5)]) == 10
    assert HO.select([r(30, None), r(10, 7.0)]) == 10 and HO.select([r(3, None)]) is None and HO.select([]) is None


# --------------------------------------------------------------------------------------------- pipeline
HOLD = dict(holdout=0.2, holdout_topics="10,20")
_DAY = {}


def get_day(tmp_path_factory):
    if "d" not in _DAY:
        _DAY["d"] = Day("flow", "fixed", tmp_path_factory.mktemp("holdout_flow"))
    return _DAY["d"]


def tree(lp):
    """``test_ensemble.tree`` with the ``seconds`` entries of holdout.json left out."""
    out = plain_tree(lp)
    k = os.path.join("holdout", "holdout.json")
    if k in out:
        j = json.loads(out[k])
        j["split"].pop("seconds")
        for r in j["records"]:
            r.pop("seconds")
        out[k] = j
    return out


def test_the_plain_runs_files_are_unchanged(tmp_path_factory):
    day = get_day(tmp_path_factory)
    plain, sp = day.run("plain")
    hold, sh = day.run("hold", **HOLD)
    a, b = plain_tree(plain), tree(hold)
    assert len(a) >= 12 and day.results in a and "final.beta" in a
    for f in a:
        assert a[f] == b[f], f
    extra = sorted(set(b) - set(a))
    assert extra and all(f.startswith("holdout" + os.sep) for f in extra), extra
    assert not (plain / "holdout").exists() and "holdout" not in sp
    lines = (hold / "holdout" / "holdout.csv").read_text().split("\n")
    assert len(lines) == 4 and lines[-1] == "" and [ln.split(",")[0] for ln in lines[1:3]] == ["10", "20"]
    h = sh["holdout"]
    assert set(h) == {"fraction", "topics", "perplexity", "selected", "select", "heldout_tokens", "split_documents",
                      "unseen_tokens", "seconds"}
    assert h["fraction"] == 0.2 and h["topics"] == [10, 20] and h["selected"] in (10, 20) and h["select"] is False
    assert all(p > 1.0 for p in h["perplexity"]) and h["heldout_tokens"] > 0 and h["split_documents"] > 0
    assert "holdout" in sh["stage_seconds"] and sh["lda"]["em_iterations"] == sp["lda"]["em_iterations"]
    j = json.loads((hold / "holdout" / "holdout.json").read_text())
    assert j["selected"] == h["selected"] and j["key"]["topics"] == [10, 20] and j["key"]["docs"] == sh["corpus"]["docs"]
    recs = [json.loads(ln) for ln in (hold / "metrics.jsonl").read_text().splitlines()]
    det = [r for r in recs if r["stage"] == "holdout_detail"]
    assert len(det) == 1 and [r["topics"] for r in det[0]["records"]] == [10, 20]
    stages = [r["stage"] for r in recs if r.get("status") == "ok" and "." not in r["stage"]]
    assert stages.index("lda_pre") < stages.index("holdout") < stages.index("lda")
    # the default list is the run's --topics alone
    one, so = day.run("hold_default", holdout=0.2)
    assert so["holdout"]["topics"] == [20] and so["holdout"]["selected"] == 20


def test_resume_at_every_stage_boundary(tmp_path_factory):
    day = get_day(tmp_path_factory)
    lp = day.root / "hold_resume"
    day.go(day.cfg(lp, **HOLD))
    want = tree(lp)
    assert want == tree(day.run("hold", **HOLD)[0])      # the uninterrupted run, twice: deterministic
    order = ["flow_pre", "lda_pre", "holdout", "lda", "lda_post", "flow_post"]
    from oni_ml_amd.pipeline import run
    for i in range(len(order)):
        for st in order[i:]:
            os.unlink(lp / ".stages" / f"{st}.done")
        logs = []
        run(day.cfg(lp, resume=True, **HOLD).validate(), device="cpu", log=logs.append)
        text = "\n".join(str(x) for x in logs)
        j = 0 if i == 1 else i      # the two corpus stages go together: without lda_pre's marker flow_pre runs again
        for st in order[:j]:
            assert f"[stage {st}] already complete" in text, (st, text)
        for st in order[j:]:
            assert f"[stage {st}] already complete" not in text and f"[stage {st}]" in text, (st, text)
        assert tree(lp) == want, order[i]
    # a finished run resumed does nothing, and still reports the record
    s = run(day.cfg(lp, resume=True, **HOLD).validate(), device="cpu", log=lambda *a, **k: None)
    assert s["holdout"]["topics"] == [10, 20] and tree(lp) == want


def test_select_is_the_plain_run_with_the_selected_topics(tmp_path_factory):
    day = get_day(tmp_path_factory)
    sel, ss = day.run("hold_select", holdout_select=True, **HOLD)
    k = ss["holdout"]["selected"]
    assert k in (10, 20) and ss["holdout"]["select"] is True
    assert k == json.loads((day.run("hold", **HOLD)[0] / "holdout" / "holdout.json").read_text())["selected"]
    plain, _ = day.run(f"plain_k{k}", topics=k)
    a, b = plain_tree(plain), tree(sel)
    assert len(a) >= 12
    for f in a:
        assert a[f] == b[f], f
    other = 30 - k      # and not the other count's run
    assert plain_tree(day.run(f"plain_k{other}", topics=other)[0])["final.beta"] != b["final.beta"]
    # a resume past the holdout stage reads the selection from holdout.json
    lp = day.root / "select_resume"
    day.go(day.cfg(lp, holdout_select=True, **HOLD))
    want = tree(lp)
    assert want == tree(sel)
    for st in ("lda", "lda_post", "flow_post"):
        os.unlink(lp / ".stages" / f"{st}.done")
    from oni_ml_amd.pipeline import run
    logs = []
    s = run(day.cfg(lp, resume=True, holdout_select=True, **HOLD).validate(), device="cpu", log=logs.append)
    assert any("[stage holdout] already complete" in str(x) for x in logs) and s["holdout"]["selected"] == k
    assert tree(lp) == want
    # a record made under another key is refused before any stage runs; the same resume under its own key is not
    marks = sorted(os.listdir(lp / ".stages"))
    for kw in (dict(holdout=0.3, holdout_topics="10,20"), dict(holdout=0.2, holdout_topics="10,20,30"),
               dict(seed=5, **HOLD), dict(alpha=1.5, **HOLD)):
        logs = []
        with pytest.raises(ValueError, match="made under"):
            run(day.cfg(lp, resume=True, **kw).validate(), device="cpu", log=logs.append)
        assert not logs and sorted(os.listdir(lp / ".stages")) == marks
    run(day.cfg(lp, resume=True, **HOLD).validate(), device="cpu", log=lambda *a, **k: None)
    # the lda stage complete without the holdout stage: nothing to select for
    os.unlink(lp / ".stages" / "holdout.done")
    with pytest.raises(ValueError, match="lda stage is complete"):
        run(day.cfg(lp, resume=True, holdout_select=True, **HOLD).validate(), device="cpu")
    run(day.cfg(lp, resume=True, **HOLD).validate(), device="cpu", log=lambda *a, **k: None)      # without: it runs
    assert tree(lp) == want


def test_refusals_write_nothing(tmp_path_factory, monkeypatch):
    day = get_day(tmp_path_factory)

    class Group:
        active, rank, world_size = True, 0, 2
    from oni_ml_amd.pipeline import run
    never = day.root / "never"

    def mk(**kw):      # Day.cfg names the backend and the compat mode itself
        late = {k: kw.pop(k) for k in ("backend", "compat") if k in kw}
        cfg = day.cfg(never, **kw)
        for k, v in late.items():
            setattr(cfg, k, v)
        return cfg
    assert CFG.RunConfig().holdout == 0.0 and CFG.RunConfig().holdout_select is False
    model = str(day.run("plain")[0] / "final")
    cases = [(dict(holdout=0.6), r"\(0, 0.5\]"), (dict(holdout=-0.1), r"\(0, 0.5\]"), (dict(holdout=float("nan")), r"\(0, 0.5\]"),
             (dict(holdout=0.2, holdout_topics="10,0"), "outside what"), (dict(holdout=0.2, holdout_topics="10,x"), "comma-separated"),
             (dict(holdout=0.2, holdout_topics="10,200", backend="hip"), "outside what"),
             (dict(holdout=0.2, holdout_topics="10,10"), "twice"),
             (dict(holdout=0.2, start=model), "fixes the topic count"), (dict(holdout=0.2, gpus=2), "one process"),
             (dict(holdout=0.2, hdfs=True), "one process"), (dict(holdout_select=True), "needs --holdout"),
             (dict(holdout=0.2, holdout_topics="10,20", holdout_select=True, compat="strict"), "strict")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            mk(**kw).validate()
        with pytest.raises(ValueError, match=msg):
            run(mk(**kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(mk(holdout=0.2), dist=Group(), device="cpu")
    assert CFG.HOLDOUT_ONE_PROCESS.startswith("--holdout")
    # the positive controls: the same options inside the rules
    for ok in (dict(holdout=0.5), dict(holdout=1e-6), dict(holdout=0.2, holdout_topics="10,200"),
               dict(holdout=0.2, holdout_topics="1,128", backend="hip"), dict(holdout=0.2, start="seeded"),
               dict(holdout=0.2, holdout_topics="20", holdout_select=True, compat="strict"),
               dict(holdout=0.2, holdout_topics="10,20", compat="strict"),
               dict(holdout=0.2, holdout_topics="10,20", holdout_select=True, compat="fixed")):
        assert mk(**dict(ok)).validate().holdout == ok["holdout"]
    # a proxy day has no strict scorer fixed at 20
    assert CFG.RunConfig.check_holdout(0.2, [10, 20], True, "random", "strict", "proxy") is None
    # the command line refuses before a process group is asked for and before the work directory is made
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    for v in ("WORLD_SIZE", "HOLDOUT", "HOLDOUT_TOPICS"):
        monkeypatch.delenv(v, raising=False)
    base = ["20160122", "flow", "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never), "--compat", "fixed",
            "--flow-path", day.paths["flow_path"]]
    for extra, msg in ((["--holdout", "0.6"], r"\(0, 0.5\]"), (["--holdout", "0"], None), (["--holdout", "-1"], r"\(0, 0.5\]"),
                       (["--holdout", "0.2", "--holdout-topics", "0,5"], "outside what"),
                       (["--holdout", "0.2", "--holdout-topics", "5,300", "--backend", "hip"], "outside what"),
                       (["--holdout", "0.2", "--start", model], "fixes the topic count"),
                       (["--holdout", "0.2", "--gpus", "2"], "one process"), (["--holdout", "0.2", "--hdfs"], "one process"),
                       (["--holdout-select"], "needs --holdout"),
                       (["--holdout", "0.2", "--holdout-topics", "10,20", "--holdout-select", "--compat", "strict"], "strict")):
        if msg is None:
            continue
        with pytest.raises(ValueError, match=msg):
            cli.cmd_ml_ops(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")      # a torchrun launch
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--holdout", "0.2"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("HOLDOUT", "0.2")       # set by the environment: the same refusal
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    assert not never.exists()


def test_cli_flag_environment_and_site_file_reach_the_config(monkeypatch, tmp_path):
    seen = {}

    def body(a, resolve):
        seen["cfg"] = resolve(1)
        return 0

    monkeypatch.setattr(cli, "_ml_ops_body", body)
    monkeypatch.setenv("ONI_PREFETCH", "0")
    for v in ("WORLD_SIZE", "HOLDOUT", "HOLDOUT_TOPICS"):
        monkeypatch.delenv(v, raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nHOLDOUT=0.1\nHOLDOUT_TOPICS=(5 15)\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a", "--compat", "fixed"]
    none = ["--conf", str(tmp_path / "none.conf")]
    got = lambda: (seen["cfg"].holdout, seen["cfg"].holdout_list(), seen["cfg"].holdout_select)      # noqa: E731
    assert cli.cmd_ml_ops(base + none) == 0 and got() == (0.0, [20], False)
    assert cli.cmd_ml_ops(base + none + ["--topics", "7", "--holdout", "0.25"]) == 0 and got() == (0.25, [7], False)
    assert cli.cmd_ml_ops(base + none + ["--holdout", "0.25", "--holdout-topics", "10,20,30", "--holdout-select"]) == 0
    assert got() == (0.25, [10, 20, 30], True)
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and got() == (0.1, [5, 15], False)
    monkeypatch.setenv("HOLDOUT", "0.3")
    monkeypatch.setenv("HOLDOUT_TOPICS", "8, 9")
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and got() == (0.3, [8, 9], False)      # environment over file
    assert cli.cmd_ml_ops(base + ["--conf", str(conf), "--holdout", "0.4", "--holdout-topics", "3"]) == 0
    assert got() == (0.4, [3], False)
    assert "HOLDOUT" in CFG.ENV_KEYS and "HOLDOUT_TOPICS" in CFG.ENV_KEYS


def test_a_fresh_run_removes_an_earlier_holdout(tmp_path, tmp_path_factory):
    k = tmp_path / "holdout" / "k20"
    k.mkdir(parents=True)
    (k / "final.beta").write_text("x")
    (tmp_path / "holdout" / "holdout.json").write_text("{}")
    (tmp_path / "flow_scores.csv").write_text("kept")
    cli.clean_workdir(str(tmp_path))
    assert not (tmp_path / "holdout").exists() and (tmp_path / "flow_scores.csv").read_text() == "kept"
    # and so does the pipeline itself when it is started without the flag in a directory that has one
    day = get_day(tmp_path_factory)
    lp = day.root / "hold_then_plain"
    day.go(day.cfg(lp, **HOLD))
    assert (lp / "holdout" / "holdout.csv").exists()
    s = day.go(day.cfg(lp))
    assert not (lp / "holdout").exists() and "holdout" not in s
    assert plain_tree(lp) == plain_tree(day.run("plain")[0]) and "lda_stats.json" in TIMED
