"""--tail on the CPU path: the torch twin ``ops.reference.tail_mass`` against a numpy / ``math.fsum`` oracle, its
exact properties (the most probable and the rarest word, ties, NaN, missing rows, the block order of the sums), and
the three pipelines end to end on the torch LDA backend -- nothing else changes, the tail file follows the results
file line for line, its values are the twin over the written tables bit for bit; MAXRESULTS, the ensemble,
--explain beside it, resume and the refusals."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import SIDES, Day, bits_equal, tree  # noqa: E402
from test_explain import _tables  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.pipeline.common import TAIL_DECADES as C_DECADES  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

f64 = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
i32 = lambda x: torch.tensor(x, dtype=torch.int32)        # noqa: E731
TAIL_KEYS = {"tail_words", "tail_pairs", "tail_hist", "tail_total_range"}


def tail_case(V, R_, K, n, D=37, seed=0, nan=False):
    """(theta [D, R, K], phi [V, R, K], doc int32 [n], word int32 [n]) on the CPU: phi rows over 8 decades, two
    pairs of identical rows, with ``nan`` a NaN in one row, a tenth of the docs and of the words -1."""
    g = torch.Generator().manual_seed(7919 * V + 100 * R_ + K + seed)
    th = torch.rand(D, R_, K, dtype=torch.float64, generator=g)
    ph = torch.rand(V, R_, K, dtype=torch.float64, generator=g) * \
        10.0 ** torch.randint(-8, 1, (V, 1, 1), generator=g).double()
    if V > 9:
        ph[7], ph[9] = ph[3], ph[4]
    if nan and V > 11:
        ph[11, R_ - 1, K - 1] = float("nan")

    def idx(rows):
        x = torch.randint(0, rows, (n,), generator=g, dtype=torch.int32)
        x[torch.rand(n, generator=g) < 0.1] = -1
        return x
    doc, word = idx(D), idx(V)
    if n >= 4:
        doc[:4] = i32([-1, -1, 0, 1])      # both missing, the document alone, the word alone, neither
        word[:4] = i32([-1, 0, -1, min(3, V - 1)])
    return th, ph, doc, word


def oracle(th, ph, doc, word):
    """Per side (le, tot, rarer, ties) or None: numpy dots in the same member and topic order with separate * and
    +, counts by direct comparison, sums by ``math.fsum``."""
    th, ph = th.numpy(), ph.numpy()
    V, R_, K = ph.shape
    out = []
    for d, w in zip(doc.tolist(), word.tolist()):
        if d < 0 or w < 0:
            out.append(None)
            continue
        p = np.zeros(V)
        for r in range(R_):
            acc = np.zeros(V)
            for k in range(K):
                acc = acc + th[d, r, k] * ph[:, r, k]
            p = p + acc
        p = p / float(R_)
        s = p[w]
        out.append((math.fsum(p[p <= s].tolist()), math.fsum(p.tolist()), int((p < s).sum()), int((p == s).sum())))
    return out


# ------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("V,R_,K,block", [(5003, 1, 20, None), (5003, 3, 7, None), (300, 1, 1, 64), (131, 3, 33, 4),
                                          (1, 1, 3, None)])
def test_twin_against_the_fsum_oracle(V, R_, K, block):
    """2e-12 relative: a blocked sequential sum of V <= 5,003 non-negative terms is off by at most about
    (V - 1) 2^-53 = 5.6e-13 relative, and the quotient adds two roundings."""
    th, ph, doc, word = tail_case(V, R_, K, 60)
    le, tot, rarer, ties = R.tail_mass(th, ph, doc, word, block=block)
    assert le.dtype == tot.dtype == torch.float64 and rarer.dtype == ties.dtype == torch.int32
    seen = 0
    for i, o in enumerate(oracle(th, ph, doc, word)):
        if o is None:
            assert math.isnan(le[i]) and math.isnan(tot[i]) and rarer[i] == -1 and ties[i] == -1
            continue
        assert (int(rarer[i]), int(ties[i])) == o[2:] and o[3] >= 1
        assert abs(le[i].item() - o[0]) <= 2e-12 * o[0] and abs(tot[i].item() - o[1]) <= 2e-12 * o[1]
        assert abs(le[i].item() / tot[i].item() - o[0] / o[1]) <= 2e-12 * (o[0] / o[1])
        seen += 1
    assert seen > 30 or V == 1


def _extremes(th, ph):
    """Per document the row of its most probable and of its rarest word (by the twin's own p, through rarer)."""
    V, D = ph.shape[0], th.shape[0]
    doc = torch.arange(D, dtype=torch.int32).repeat_interleave(V)
    word = torch.arange(V, dtype=torch.int32).repeat(D)
    le, tot, rarer, ties = R.tail_mass(th, ph, doc, word)
    rarer, ties = rarer.reshape(D, V), ties.reshape(D, V)
    return doc, word, le.reshape(D, V), tot.reshape(D, V), rarer, ties


def test_most_probable_and_rarest_word():
    th, ph, _, _ = tail_case(211, 1, 5, 0, D=9)
    ph[7], ph[9] = ph[8] * 1.5, ph[8] * 2.5      # (no duplicate rows here: ties == 1 everywhere)
    _, _, le, tot, rarer, ties = _extremes(th, ph)
    V = 211
    top, low = rarer.argmax(1), rarer.argmin(1)
    for d in range(9):
        # the most probable word: le and tot are the same sum
        assert bits_equal(le[d, top[d]], tot[d, top[d]]) and (le[d, top[d]] / tot[d, top[d]]).item() == 1.0
        assert int(rarer[d, top[d]] + ties[d, top[d]]) == V
        # the rarest: nothing below it, and le is its own score
        assert int(rarer[d, low[d]]) == 0 and int(ties[d, low[d]]) == 1
        s = R.score(th[:, 0], ph[:, 0], 5, 0.1, i32([d]), low[d:d + 1].to(torch.int32))[0]
        assert le[d, low[d]].item() == s.item()
    assert bool((ties == 1).all()) and bool(((le / tot) > 0).all()) and bool(((le / tot) <= 1).all())
    # rarer is the rank: per document a permutation of 0 .. V - 1
    assert all(sorted(rarer[d].tolist()) == list(range(V)) for d in range(9))


def test_identical_rows_tie():
    th, ph, _, _ = tail_case(50, 1, 4, 0, D=5)
    doc, word = i32([0, 0, 1, 2]), i32([3, 7, 4, 20])
    le, tot, rarer, ties = R.tail_mass(th, ph, doc, word)
    assert ties.tolist() == [2, 2, 2, 1]
    assert le[0].item() == le[1].item() and rarer[0] == rarer[1]      # rows 3 and 7 are the same word to the model


def test_a_nan_row_makes_the_total_nan_and_leaves_the_counts():
    th, ph, doc, word = tail_case(131, 3, 6, 200, nan=False)
    word[word == 11] = 12
    clean = R.tail_mass(th, ph, doc, word, block=64)
    ph[11, 1, 2] = float("nan")
    le, tot, rarer, ties = R.tail_mass(th, ph, doc, word, block=64)
    ok = (doc >= 0) & (word >= 0)
    assert int(ok.sum()) > 100 and bool(torch.isnan(tot[ok]).all()) and not bool(torch.isnan(le[ok]).any())
    assert torch.equal(ties, clean[3])
    # row 11 left the count of the sides it was rarer than, and entered le as 0.0
    zeros = ph.clone()
    zeros[11] = 0.0      # the row as a row of zeros: p = 0.0, below every side's score
    was = R.tail_mass(th, zeros, doc, word, block=64)
    assert torch.equal(rarer[ok] + 1, was[2][ok]) and bits_equal(le, was[0])
    assert bool((clean[2][ok] >= rarer[ok]).all())


def test_missing_rows_and_no_sides():
    th, ph, _, _ = tail_case(40, 1, 3, 0)
    le, tot, rarer, ties = R.tail_mass(th, ph, i32([-1, 2, -1, 2]), i32([5, -1, -1, 5]))
    assert torch.isnan(le[:3]).all() and torch.isnan(tot[:3]).all() and rarer[:3].tolist() == ties[:3].tolist() == [-1] * 3
    assert not math.isnan(le[3]) and ties[3] >= 1
    out = R.tail_mass(th, ph, i32([]), i32([]))
    assert all(tuple(t.shape) == (0,) for t in out) and out[0].dtype == torch.float64 and out[2].dtype == torch.int32
    with pytest.raises(ValueError, match="block"):
        R.tail_mass(th, ph, i32([0]), i32([0]), block=0)
    with pytest.raises(ValueError, match="out of range"):
        R.tail_mass(th, ph, i32([0]), i32([40]))
    with pytest.raises(ValueError, match="out of range"):
        R.tail_mass(th, ph, i32([-2]), i32([0]))


def test_block_order_is_observable():
    """p = (1, u, u, u) with u = 2^-53: blocks of two give (1 + u) + (u + u) = 1 + 2^-52, blocks of three
    ((1 + u) + u) + u = 1 (every step rounds to even)."""
    u = 2.0 ** -53
    th, ph = f64([[[1.0]]]), f64([[[1.0]], [[u]], [[u]], [[u]]])
    assert (1.0 + u) + (u + u) != ((1.0 + u) + u) + u
    for block, want in ((2, 1.0 + 2.0 ** -52), (3, 1.0), (1, 1.0), (4, 1.0)):
        le, tot, rarer, ties = R.tail_mass(th, ph, i32([0]), i32([0]), block=block)
        assert le.item() == tot.item() == want and (int(rarer), int(ties)) == (3, 1)
    le, tot, rarer, ties = R.tail_mass(th, ph, i32([0]), i32([2]), block=2)
    assert le.item() == (0.0 + u) + (u + u) and tot.item() == 1.0 + 2.0 ** -52 and (int(rarer), int(ties)) == (0, 3)


def test_one_model_is_one_member_and_the_score_is_the_ensembles():
    th, ph, doc, word = tail_case(97, 1, 20, 150)
    one = S.tail_mass(S.TopicModel(th[:, 0].contiguous(), ph[:, 0].contiguous(), 20, 0.05), doc, word)
    ens = S.tail_mass(S.EnsembleModel(th, ph, 1, 20, 0.05), doc, word)
    raw = R.tail_mass(th, ph, doc, word)
    for a, b, c in zip(one, ens, raw):
        assert bits_equal(a, b) and bits_equal(a, c)
    # R = 3: at a document's rarest word le is s itself -- score_ensemble's score bit for bit
    th, ph, _, _ = tail_case(97, 3, 20, 0, D=6)
    ph[7], ph[9] = ph[8] * 1.5, ph[8] * 2.5
    _, _, le, _, rarer, ties = _extremes(th, ph)
    low = rarer.argmin(1).to(torch.int32)
    s = R.score_ensemble(th, ph, 3, 20, 0.05, torch.arange(6, dtype=torch.int32), low)[0]
    assert bool((ties[torch.arange(6), low.long()] == 1).all())
    assert bits_equal(le[torch.arange(6), low.long()], s)


def test_the_slab_does_not_change_the_bits():
    th, ph, doc, word = tail_case(300, 3, 5, 200, nan=True)
    a = R.tail_mass(th, ph, doc, word, block=64)
    b = R.tail_mass(th, ph, doc, word, block=64, slab=7 * 300)      # 7 sides at a time
    assert all(bits_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------- end to end
ALL = ["flow-strict", "flow-fixed", "dns-strict", "proxy-fixed"]
_DAYS = {}


def get_day(which, tmp_path_factory):
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("tail_" + kind + compat))
    return _DAYS[which]


def read_tail(day, lp):
    """Per line: (key text, [per side (doc, word, score text, tail text, rarer text)])."""
    sep, sides = SIDES[day.kind]
    lines = (lp / f"{day.kind}_tail.csv").read_text(encoding="utf-8").split("\n")
    assert lines[-1] == ""
    out = []
    for ln in lines[:-1]:
        f = ln.split(sep)
        assert len(f) == 1 + 5 * len(sides)
        out.append((f[0], [tuple(f[1 + 5 * j:6 + 5 * j]) for j in range(len(sides))]))
    return out


def twin_tail_of_file(day, lp, members=1):
    """(parsed tail [sides], the twin's over the written tables, parsed rarer texts, the twin's as texts)."""
    dn, wn, th, ph = _tables(lp, members)
    rows = read_tail(day, lp)
    di = {n: i for i, n in enumerate(dn)}      # later duplicates win, as the scorers' maps
    wi = {n: i for i, n in enumerate(wn)}
    flat = [s for _, ss in rows for s in ss]
    doc, word = i32([di.get(s[0], -1) for s in flat]), i32([wi.get(s[1], -1) for s in flat])
    le, tot, rarer, _ = R.tail_mass(th, ph, doc, word)
    with np.errstate(invalid="ignore"):
        want = torch.from_numpy(le.numpy() / tot.numpy())
    got = f64([float(s[3]) if s[3] else float("nan") for s in flat])
    return got, want, [s[4] for s in flat], ["" if r < 0 else str(r) for r in rarer.tolist()]


def check_tail_file(day, lp, summary, members=1):
    """The tail file against the results file line for line, against the twin, and against the summary."""
    rows = read_tail(day, lp)
    sep, sides = SIDES[day.kind]
    res = [ln.split(sep) for ln in (lp / day.results).read_text(encoding="utf-8").split("\n")[:-1]]
    assert len(res) == len(rows) == summary["scored"] > 20
    for f, (key, ss) in zip(res, rows):
        assert [s[:3] for s in ss] == [(f[c[0]], f[c[1]], f[c[2]]) for c in sides]
        assert key in [s[2] for s in ss] and float(key) == min(float(s[2]) for s in ss)
    got, want, r_got, r_want = twin_tail_of_file(day, lp, members)
    assert bits_equal(got, want) and r_got == r_want
    good = got[~torch.isnan(got)]
    assert good.numel() > 20 and bool((good > 0).all()) and bool((good <= 1).all())
    hist = summary["tail_hist"]
    assert list(hist) == list(C_DECADES) + ["none"] and sum(hist.values()) == len(rows) * len(sides)
    assert hist["none"] == int(torch.isnan(got).sum()) and hist["<=1"] == int((good >= 0.1).sum())
    dn, wn, th, ph = _tables(lp, members)
    assert summary["tail_words"] == len(wn) == ph.shape[0]
    flat = [s for _, ss in rows for s in ss]
    assert summary["tail_pairs"] == len({(s[0], s[1]) for s in flat if s[3]})
    lo, hi = summary["tail_total_range"]
    assert lo <= hi and (day.compat == "strict" or (abs(lo - 1) < 1e-9 and abs(hi - 1) < 1e-9))
    return got


@pytest.mark.parametrize("which", ALL)
def test_day_with_tail(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    plain, sp = day.run("plain")
    lp, s = day.run("tail", tail=True)
    a, b = tree(plain), tree(lp)
    assert set(b) - set(a) == {f"{day.kind}_tail.csv"} and set(a) <= set(b)
    for f in a:
        assert a[f] == b[f], f
    assert not TAIL_KEYS & set(sp) and {k for k in s if k not in sp} == TAIL_KEYS
    recs = [json.loads(x) for x in (lp / "metrics.jsonl").read_text().splitlines()]
    det = [r for r in recs if r.get("stage") == f"{day.kind}_post_detail" and "tail_hist" in r]
    assert len(det) == 1 and det[0]["tail_hist"] == s["tail_hist"] and det[0]["tail_pairs"] == s["tail_pairs"]
    assert not any("tail_hist" in json.loads(x) for x in (plain / "metrics.jsonl").read_text().splitlines())
    got = check_tail_file(day, lp, s)
    assert which != "flow-strict" or bool(torch.isnan(got).any())      # a side without a row: empty cells


@pytest.mark.parametrize("which", ["flow-strict", "dns-strict", "proxy-fixed"])
def test_max_results_ensemble_and_explain(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp, s = day.run("tail", tail=True)
    name = f"{day.kind}_tail.csv"
    full = (lp / name).read_bytes().splitlines(keepends=True)
    N = s["scored"] // 3
    lim, sl = day.run("tail_lim", tail=True, max_results=N)
    assert (lim / name).read_bytes() == b"".join(full[:N]) and N > 5
    assert sum(sl["tail_hist"].values()) == N * len(SIDES[day.kind][1]) and sl["tail_pairs"] <= s["tail_pairs"]
    # --ensemble 3: the twin over the three written member tables; the results file is the ensemble's
    ens, se = day.run("tail_ens3", tail=True, ensemble=3)
    check_tail_file(day, ens, se, members=3)
    assert (ens / day.results).read_bytes() == (day.run("ens3", ensemble=3)[0] / day.results).read_bytes()
    # --explain and the host report beside it: each file is what it is alone
    both, sb = day.run("tail_explain", tail=True, explain=True, host_report=-1)
    alone, _ = day.run("explain_hosts", explain=True, host_report=-1)
    assert (both / name).read_bytes() == b"".join(full)
    for f in (f"{day.kind}_explain.csv", f"{day.kind}_hosts.csv", day.results):
        assert (both / f).read_bytes() == (alone / f).read_bytes()
    assert TAIL_KEYS <= set(sb) and "explain_why_hist" in sb


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_resume_writes_the_same_tail_file(which, tmp_path_factory):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)
    want = (day.run("tail", tail=True)[0] / f"{day.kind}_tail.csv").read_bytes()
    lp = day.root / "resume"
    day.go(day.cfg(lp, tail=True))
    post = f"{day.kind}_post"
    tf = lp / f"{day.kind}_tail.csv"
    assert tf.read_bytes() == want
    # at the scoring stage: nothing but the model tables is needed
    os.unlink(lp / ".stages" / f"{post}.done")
    os.unlink(tf)
    s = run(day.cfg(lp, tail=True, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert tf.read_bytes() == want and TAIL_KEYS <= set(s)
    # a run that had no flag, resumed with it
    plain = day.root / "resume_plain"
    day.go(day.cfg(plain))
    os.unlink(plain / ".stages" / f"{post}.done")
    run(day.cfg(plain, tail=True, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert (plain / f"{day.kind}_tail.csv").read_bytes() == want


@pytest.mark.parametrize("which", ["flow-strict", "proxy-fixed"])
def test_refusals_write_nothing(which, tmp_path_factory, monkeypatch):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)

    class Group:
        active, rank, world_size = True, 0, 2
    never = day.root / "never"
    assert CFG.RunConfig().tail is False and CFG.TAIL_ONE_PROCESS.startswith("--tail")
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="one process"):
            day.cfg(never, tail=True, **kw).validate()
        with pytest.raises(ValueError, match="one process"):
            run(day.cfg(never, tail=True, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, tail=True), dist=Group(), device="cpu")
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TAIL", raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    for extra in (["--tail", "--gpus", "2"], ["--tail", "--hdfs"]):
        with pytest.raises(ValueError, match="one process"):
            cli.cmd_ml_ops(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--tail"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("TAIL", "1")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    assert not never.exists()


def test_a_fresh_run_removes_a_stale_tail_file(tmp_path):
    for f in ("flow_tail.csv", "flow_scores.csv", "flow_results.csv"):
        (tmp_path / f).write_text("x")
    cli.clean_workdir(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["flow_results.csv", "flow_scores.csv"]


def test_cli_flag_environment_and_site_file_reach_the_config(monkeypatch, tmp_path):
    seen = {}

    def body(a, resolve):
        seen["cfg"] = resolve(1)
        return 0
    monkeypatch.setattr(cli, "_ml_ops_body", body)
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TAIL", raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nTAIL=1\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].tail is False
    assert cli.cmd_ml_ops(base + none + ["--tail"]) == 0 and seen["cfg"].tail is True
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].tail is True
    monkeypatch.setenv("TAIL", "0")
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].tail is False      # environment over file
    monkeypatch.setenv("TAIL", "1")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].tail is True
    assert "TAIL" in CFG.ENV_KEYS and CFG.TAIL_BLOCK == 1024
