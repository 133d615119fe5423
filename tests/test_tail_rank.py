"""--tail-tol on the CPU path: the three pipelines flagged and ranked by the tail p-value, end to end on the torch LDA
backend.  The oracle is code from before the option: the same day run with TOL = 1e300 and --tail writes every
scored event with its sides' tails, so the lines whose lowest tail is under P, ascending by it, are what --tail-tol P
has to write.  Also MAXRESULTS, the ensemble, resume, P = 1, the refusals, the three ways to set P, and
``pipeline.common.tail_keys`` on its own."""
import json
import math
import os
import sys
import types
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import SIDES, Day, bits_equal, tree  # noqa: E402
from test_tail import ALL, TAIL_KEYS, check_tail_file, read_tail, tail_case  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

RANK_KEYS = {"tail_tol", "tail_rank_pairs", "tail_rank_docs", "tail_rank_path", "tail_sides_skipped"}
_DAYS = {}


def get_day(which, tmp_path_factory):
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("tail_rank_" + kind + compat))
    return _DAYS[which]


def run_at(day, name, tol, **kw):
    """``day.run`` at another TOL (``Day.cfg`` fixes the day's own)."""
    if name not in day.runs:
        lp = day.root / name
        cfg = day.cfg(lp, **kw)
        cfg.tol = tol
        day.runs[name] = (lp, day.go(cfg))
    return day.runs[name]


def lines_of(path):
    text = path.read_text(encoding="utf-8").split("\n")
    assert text[-1] == ""
    return text[:-1]


def line_keys(day, lp):
    """Per line of the tail file its ranking key: the lowest of its non-empty ``tail`` cells (NaN: none)."""
    out = []
    for _, ss in read_tail(day, lp):
        t = [float(s[3]) for s in ss if s[3]]
        out.append(min(t) if t else float("nan"))
    return out


def oracle_of(day, name="oracle", **kw):
    """((results line, key) of every scored event, P): the day with TOL = 1e300 and --tail, and the key of rank
    ceil(n / 10), so that about a tenth of the day lies under P."""
    lp, s = run_at(day, name, 1e300, tail=True, **kw)
    lines, keys = lines_of(lp / day.results), line_keys(day, lp)
    assert len(lines) == len(keys) == s["scored"] > 1000
    good = sorted(k for k in keys if k == k)
    P = good[math.ceil(len(keys) / 10) - 1]
    assert 0.0 < P < 1.0
    return list(zip(lines, keys)), P


def check_ranked_by_tail(day, lp, s, oracle, P, members=1, limit=None):
    """The run's results file against the oracle's lines under P, its tail file, and its summary."""
    want = sorted(((k, ln) for ln, k in oracle if k < P), key=lambda x: x[0])
    got_lines, got_keys = lines_of(lp / day.results), line_keys(day, lp)
    assert 100 < len(want) < len(oracle) // 8 + 2
    assert s["below_tol"] == len(want) and s["scored"] == len(got_lines) == (limit or len(want))
    assert got_keys == [k for k, _ in want][:len(got_keys)]      # ascending by the key, the same keys
    assert all(k < P for k in got_keys)
    if limit is None:      # runs of equal keys as multisets: the oracle file is in score order
        by_key = lambda pairs: {k: Counter(ln for kk, ln in pairs if kk == k) for k in {kk for kk, _ in pairs}}  # noqa: E731
        assert by_key(list(zip(got_keys, got_lines))) == by_key(want)
    check_tail_file(day, lp, s, members=members)
    assert RANK_KEYS <= set(s) and TAIL_KEYS <= set(s) and s["tail_tol"] == P
    assert s["tail_rank_path"] == ("cpu" if day.device == "cpu" else s["tail_rank_path"])
    assert s["tail_rank_pairs"] >= s["tail_pairs"] > 0 and 0 < s["tail_rank_docs"] <= s["tail_rank_pairs"]
    recs = [json.loads(x) for x in (lp / "metrics.jsonl").read_text().splitlines()]
    det = [r for r in recs if r.get("stage") == f"{day.kind}_post_detail" and "tail_hist" in r]
    assert len(det) == 1 and all(det[0][k] == s[k] for k in RANK_KEYS)


# ---------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("which", ALL)
def test_day_ranked_by_tail(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    oracle, P = oracle_of(day)
    lp, s = day.run("tail_tol", tail_tol=P)
    check_ranked_by_tail(day, lp, s, oracle, P)
    # not the score's selection: the plain run writes other rows
    plain, sp = day.run("plain")
    assert not RANK_KEYS & set(sp) and (plain / day.results).read_bytes() != (lp / day.results).read_bytes()
    assert s["tail_sides_skipped"] > 0 or which != "flow-strict"      # a side without a row


@pytest.mark.parametrize("which", ALL)
def test_every_other_file_is_the_plain_runs(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    oracle, P = oracle_of(day)
    plain, _ = day.run("plain_hosts_explain", host_report=-1, explain=True)
    lp, s = day.run("tail_tol_hosts_explain", tail_tol=P, host_report=-1, explain=True)
    a, b = tree(plain), tree(lp)
    chosen = {day.results, f"{day.kind}_tail.csv", f"{day.kind}_explain.csv"}
    assert set(b) - set(a) == {f"{day.kind}_tail.csv"} and set(a) <= set(b) and f"{day.kind}_hosts.csv" in a
    for f in a:
        if f not in chosen:
            assert a[f] == b[f], f
    assert (lp / day.results).read_bytes() == (day.run("tail_tol", tail_tol=P)[0] / day.results).read_bytes()
    # --explain explains whatever rows are written: the lines of the run that writes every row, for these rows
    every, _ = run_at(day, "oracle_explain", 1e300, explain=True)
    why = dict(zip(lines_of(every / day.results), lines_of(every / f"{day.kind}_explain.csv")))
    got = list(zip(lines_of(lp / day.results), lines_of(lp / f"{day.kind}_explain.csv")))
    assert len(got) == s["scored"] > 100 and all(why[r] == e for r, e in got)
    both = dict(zip(lines_of(plain / day.results), lines_of(plain / f"{day.kind}_explain.csv")))
    assert all(both[r] == e for r, e in got if r in both)


@pytest.mark.parametrize("which", ["flow-strict", "dns-strict", "proxy-fixed"])
def test_max_results_writes_the_head(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    oracle, P = oracle_of(day)
    lp, s = day.run("tail_tol", tail_tol=P)
    N = s["scored"] // 3
    lim, sl = day.run("tail_tol_lim", tail_tol=P, max_results=N)
    assert N > 30 and sl["scored"] == N and sl["below_tol"] == s["below_tol"]
    for f in (day.results, f"{day.kind}_tail.csv"):      # the select's tie rule is the sort's
        assert (lim / f).read_bytes() == b"".join((lp / f).read_bytes().splitlines(keepends=True)[:N])
    check_ranked_by_tail(day, lim, sl, oracle, P, limit=N)


def test_ensemble(tmp_path_factory):
    day = get_day("flow-strict", tmp_path_factory)
    oracle, P = oracle_of(day, "oracle_ens3", ensemble=3)
    lp, s = day.run("tail_tol_ens3", tail_tol=P, ensemble=3)
    check_ranked_by_tail(day, lp, s, oracle, P, members=3)
    assert "ensemble_votes_hist" in s and sum(s["ensemble_votes_hist"]) == s["scored"]


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_resume_writes_the_same_files(which, tmp_path_factory):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)
    _, P = oracle_of(day)
    first, _ = day.run("tail_tol", tail_tol=P)
    files = (day.results, f"{day.kind}_tail.csv")
    want = [(first / f).read_bytes() for f in files]
    post = f"{day.kind}_post"
    lp = day.root / "tail_tol_resume"
    day.go(day.cfg(lp, tail_tol=P))
    assert [(lp / f).read_bytes() for f in files] == want
    # at the scoring stage: nothing but the model tables is needed
    os.unlink(lp / ".stages" / f"{post}.done")
    for f in files:
        os.unlink(lp / f)
    s = run(day.cfg(lp, tail_tol=P, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert [(lp / f).read_bytes() for f in files] == want and RANK_KEYS <= set(s)
    # a run that had no flag, resumed with it
    plain = day.root / "tail_tol_resume_plain"
    day.go(day.cfg(plain))
    os.unlink(plain / ".stages" / f"{post}.done")
    run(day.cfg(plain, tail_tol=P, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert [(plain / f).read_bytes() for f in files] == want


def test_p_of_one_writes_every_event_below_one(tmp_path_factory):
    """At P = 1.0 ties abound (a side at its host's most probable word has tail 1.0 exactly, and many events share
    a pair): every event whose key is < 1.0, in non-decreasing key order."""
    day = get_day("dns-strict", tmp_path_factory)
    oracle, _ = oracle_of(day)
    lp, s = day.run("tail_tol_one", tail_tol=1.0)
    want = sorted(k for _, k in oracle if k < 1.0)
    got = line_keys(day, lp)
    assert got == want and len(want) > len(oracle) // 2 and len(set(want)) < len(want)
    assert Counter(lines_of(lp / day.results)) == Counter(ln for ln, k in oracle if k < 1.0)
    assert s["below_tol"] == s["scored"] == len(want)


# ------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("which", ["flow-strict", "proxy-fixed"])
def test_refusals_write_nothing(which, tmp_path_factory, monkeypatch):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)

    class Group:
        active, rank, world_size = True, 0, 2
    never = day.root / "never"
    assert CFG.RunConfig().tail_tol is None
    for p in (0, -1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="tail-tol"):
            day.cfg(never, tail_tol=p).validate()
        with pytest.raises(ValueError, match="tail-tol"):
            run(day.cfg(never, tail_tol=p), device="cpu")
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="one process"):
            day.cfg(never, tail_tol=0.1, **kw).validate()
        with pytest.raises(ValueError, match="one process"):
            run(day.cfg(never, tail_tol=0.1, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, tail_tol=0.1), dist=Group(), device="cpu")
    assert day.cfg(never, tail_tol=0.1).validate().tail is True      # it implies --tail
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    for k in ("WORLD_SIZE", "TAIL", "TAIL_TOL"):
        monkeypatch.delenv(k, raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    for p in ("0", "-1", "1.5", "nan"):
        with pytest.raises(ValueError, match="tail-tol"):
            cli.cmd_ml_ops(base + ["--tail-tol", p])
    for extra in (["--tail-tol", "0.1", "--gpus", "2"], ["--tail-tol", "0.1", "--hdfs"]):
        with pytest.raises(ValueError, match="one process"):
            cli.cmd_ml_ops(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--tail-tol", "0.1"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("TAIL_TOL", "0.1")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    monkeypatch.setenv("TAIL_TOL", "2")
    with pytest.raises(ValueError, match="tail-tol"):
        cli.cmd_ml_ops(base)
    assert not never.exists()


def test_cli_flag_environment_and_site_file_reach_the_config(monkeypatch, tmp_path):
    seen = {}

    def body(a, resolve):
        seen["cfg"] = resolve(1)
        return 0
    monkeypatch.setattr(cli, "_ml_ops_body", body)
    monkeypatch.setenv("ONI_PREFETCH", "0")
    for k in ("WORLD_SIZE", "TAIL", "TAIL_TOL"):
        monkeypatch.delenv(k, raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nTAIL_TOL=0.25\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].tail_tol is None and seen["cfg"].tail is False
    assert cli.cmd_ml_ops(base + none + ["--tail-tol", "0.01"]) == 0 and seen["cfg"].tail_tol == 0.01
    assert seen["cfg"].validate().tail is True
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].tail_tol == 0.25
    monkeypatch.setenv("TAIL_TOL", "0.5")
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].tail_tol == 0.5      # environment over file
    assert cli.cmd_ml_ops(base + ["--conf", str(conf), "--tail-tol", "1"]) == 0 and seen["cfg"].tail_tol == 1.0
    monkeypatch.setenv("TAIL_TOL", "")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].tail_tol is None
    assert "TAIL_TOL" in CFG.ENV_KEYS and CFG.TAIL_DOCS_MIN_SHARE >= 1


# ------------------------------------------------------------------------------------------ tail_keys
def test_tail_keys_directly():
    th, ph, _, _ = tail_case(97, 1, 20, 0, D=9)
    model = S.TopicModel(th[:, 0].contiguous(), ph[:, 0].contiguous(), 20, 0.05)
    i64 = lambda x: torch.tensor(x, dtype=torch.int64)      # noqa: E731
    #            both   a only  b only  neither  no θ row  no φ row  a repeated pair
    da, wa = i64([0, 1, -1, -1, -1, 4, 0]), i64([5, 6, 7, -1, 8, -1, 5])
    db, wb = i64([2, -1, 3, -1, -1, 3, 2]), i64([10, 11, 12, -1, 13, -1, 10])
    cfg = types.SimpleNamespace(tail_tol=0.5, dsource="flow")
    said = []
    tr = C.tail_keys(cfg, model, (da, db), (wa, wb), log=said.append)
    assert len(said) == 1 and "0.5" in said[0] and "multiply-adds" in said[0]
    doc, word = torch.cat([da, db]), torch.cat([wa, wb])
    le, tot, rarer, _ = R.tail_mass(th, ph, doc.to(torch.int32), word.to(torch.int32))
    ok = (doc >= 0) & (word >= 0)
    le, tot, rarer = le[ok], tot[ok], rarer[ok]
    want = torch.full((14,), float("nan"), dtype=torch.float64)
    want[ok] = torch.from_numpy(le.numpy() / tot.numpy())
    a, b = want[:7], want[7:]
    assert bits_equal(tr.tail[0], a) and bits_equal(tr.tail[1], b)
    assert torch.isnan(a).tolist() == [False, False, True, True, True, True, False]
    assert torch.isnan(b).tolist() == [False, True, False, True, True, True, False]
    key = [min(x, y) if x == x and y == y else (x if x == x else y) for x, y in zip(a.tolist(), b.tolist())]
    assert bits_equal(tr.key, torch.tensor(key, dtype=torch.float64))
    assert torch.isnan(tr.key).tolist() == [False, False, False, True, True, True, False]
    assert tr.flag.tolist() == [k < 0.5 for k in key] and not any(tr.flag[3:6].tolist())
    assert tr.rarer[0].tolist()[2:6] == [-1] * 4 and tr.rarer[0][0] == tr.rarer[0][6] >= 0
    assert tr.pair[0][0] == tr.pair[0][6] and tr.pair[1][0] == tr.pair[1][6] and tr.pair[0][2] == -1
    # sides: 14, of which 6 have a pair -- 4 distinct pairs of 4 documents
    assert tr.stats == dict(tail_tol=0.5, tail_rank_pairs=4, tail_rank_docs=4, tail_rank_path="cpu",
                            tail_sides_skipped=8)
    # the threshold is strict, and 1.0 takes everything below it
    cfg.tail_tol = float(tr.key[0])
    assert not bool(C.tail_keys(cfg, model, (da, db), (wa, wb), log=said.append).flag[0])
    # one side, and no event at all
    one = C.tail_keys(cfg, model, (da,), (wa,), log=said.append)
    assert bits_equal(one.key, a) and one.stats["tail_sides_skipped"] == 4
    none = C.tail_keys(cfg, model, (da[:0],), (wa[:0],), log=said.append)
    assert none.key.numel() == 0 and none.flag.numel() == 0 and none.stats["tail_rank_pairs"] == 0
    nothing = C.tail_keys(cfg, model, (i64([-1, 2]),), (i64([3, -1]),), log=said.append)
    assert bool(torch.isnan(nothing.key).all()) and not bool(nothing.flag.any())
    assert nothing.stats["tail_rank_pairs"] == 0 and nothing.stats["tail_sides_skipped"] == 2
