"""--peers on the CPU path: the torch twin ``ops.reference.peer_topn`` against a brute-force oracle bit for bit (a
per-pair numpy fold in j order, then ``sorted`` by (L, row)), ties, NaN rows, the slab, ``scorer.peer_scores``, and
the three pipelines end to end on the torch LDA backend -- nothing else changes, the peers file follows the results
file line for line, every cell is the twin's over the written tables; MAXRESULTS, the ensemble, the other options
beside it, resume, the refusals and the clean-up."""
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
from oni_ml_amd.pipeline.common import PEER_LIFT_DECADES  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

f64 = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
i32 = lambda x: torch.tensor(x, dtype=torch.int32)        # noqa: E731
PEER_KEYS = {"peers", "peer_hosts", "peer_candidates", "peer_path", "peer_identical", "peer_lift_hist"}
INF = float("inf")


def peer_case(D, R_, K, Q, seed=0):
    """(theta [D, R, K] on the CPU, query int32 [Q] with repeats): rows normalised per member like a topic mixture,
    over several decades; rows 3 and 7 identical (D > 7), so distance 0 and a tie occur."""
    g = torch.Generator().manual_seed(7919 * D + 100 * R_ + K + seed)
    th = torch.rand(D, R_, K, dtype=torch.float64, generator=g) ** 4
    th = th / th.sum(2, keepdim=True)
    if D > 7:
        th[7] = th[3]
    q = torch.randint(0, D, (Q,), generator=g, dtype=torch.int32)
    if Q >= 2 and D > 7:
        q[:2] = i32([3, 7])
    return th, q


def tripled(D3=7, R_=1, K=5):
    """A table in which every row occurs three times: rows r, r + D3, r + 2 D3 are the same."""
    th, _ = peer_case(D3, R_, K, 0, seed=5)      # (D3 <= 7: no planted pair, the rows are distinct)
    return torch.cat([th, th, th]).contiguous()


def nan_table():
    """131 rows, three members: row 11 has a NaN, so has the query row 40."""
    th, q = peer_case(131, 3, 6, 200, seed=9)
    th[11, 1, 2] = float("nan")
    th[40, 2, 5] = float("nan")
    q[5], q[6] = 40, 11
    return th, q


def oracle(th, q, n):
    """Per query the list [(L, p)] of its peers: a numpy fold over j per pair, then ``sorted`` by (L, row)."""
    t = th.reshape(th.shape[0], -1).numpy()
    out = []
    for qi in q.tolist():
        acc = np.zeros(t.shape[0])
        for j in range(t.shape[1]):
            acc = acc + np.abs(t[qi, j] - t[:, j])
        cand = [(float(acc[p]), p) for p in range(t.shape[0]) if p != qi and not math.isnan(acc[p])]
        out.append(sorted(cand)[:n])
    return out


def check_against_oracle(got, th, q, n):
    rows, dist, count = got
    assert rows.dtype == torch.int32 and dist.dtype == torch.float64 and count.dtype == torch.int32
    assert tuple(rows.shape) == tuple(dist.shape) == (q.numel(), n) and tuple(count.shape) == (q.numel(),)
    for i, want in enumerate(oracle(th, q, n)):
        c = int(count[i])
        assert c == len(want)
        assert rows[i, :c].tolist() == [p for _, p in want]
        assert bits_equal(dist[i, :c], f64([L for L, _ in want]))
        assert rows[i, c:].tolist() == [-1] * (n - c) and dist[i, c:].tolist() == [INF] * (n - c)


# ------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("K,R_", [(1, 1), (3, 3), (20, 1), (33, 3)])
@pytest.mark.parametrize("D", [1, 2, 5, 17, 131])
def test_twin_against_the_brute_force_oracle(D, K, R_, n):
    th, q = peer_case(D, R_, K, 40)
    got = R.peer_topn(th, q, n)
    check_against_oracle(got, th, q, n)
    assert bool((got[2] == min(n, D - 1)).all())      # D - 1 < n: fewer peers than slots


def test_ties_go_to_the_lower_row_and_the_query_is_never_listed():
    th = tripled()
    D = th.shape[0]
    D3 = D // 3
    q = torch.arange(D, dtype=torch.int32)
    rows, dist, count = R.peer_topn(th, q, 5)
    for i in range(D):
        copies = [r for r in (i % D3, i % D3 + D3, i % D3 + 2 * D3) if r != i]
        assert rows[i, :2].tolist() == copies and dist[i, :2].tolist() == [0.0, 0.0] and dist[i, 2] > 0
        assert i not in rows[i].tolist() and int(count[i]) == 5
    rows1, dist1, _ = R.peer_topn(th, q, 1)
    assert rows1[:, 0].tolist() == [min(r for r in (i % D3, i % D3 + D3, i % D3 + 2 * D3) if r != i) for i in range(D)]
    assert bool((dist1 == 0.0).all())
    check_against_oracle((rows, dist, count), th, q, 5)


def test_a_nan_row_is_never_a_peer_and_a_nan_query_has_none():
    th, q = nan_table()
    rows, dist, count = R.peer_topn(th, q, 16)
    assert not bool((rows == 11).any()) and not bool((rows == 40).any()) and not bool(torch.isnan(dist).any())
    assert count[5] == 0 and count[6] == 0 and rows[5].tolist() == [-1] * 16 and dist[6].tolist() == [INF] * 16
    ok = (q != 40) & (q != 11)
    assert bool((count[ok] == 16).all())
    check_against_oracle((rows, dist, count), th, q, 16)
    # with n = 130 > 16 refused; with D - 3 valid candidates and n = 16 nothing is short
    with pytest.raises(ValueError, match="n must be"):
        R.peer_topn(th, q, 17)
    with pytest.raises(ValueError, match="n must be"):
        R.peer_topn(th, q, 0)
    with pytest.raises(ValueError, match="out of range"):
        R.peer_topn(th, i32([131]), 3)
    with pytest.raises(ValueError, match="out of range"):
        R.peer_topn(th, i32([-1]), 3)
    out = R.peer_topn(th, i32([]), 3)
    assert tuple(out[0].shape) == (0, 3) and tuple(out[1].shape) == (0, 3) and tuple(out[2].shape) == (0,)


def test_the_slab_does_not_change_the_bits():
    th, q = nan_table()
    a = R.peer_topn(th, q, 7)
    b = R.peer_topn(th, q, 7, slab=7 * 131)      # 7 queries at a time
    c = R.peer_topn(th, q, 7, slab=1)            # one
    assert all(bits_equal(x, y) and bits_equal(x, z) for x, y, z in zip(a, b, c))


@pytest.mark.parametrize("R_", [1, 3])
def test_peer_scores_are_the_scorers_mean_in_peer_order(R_):
    K, D, V, n, N = 20, 37, 50, 300, 5
    th, _ = peer_case(D, R_, K, 0)
    g = torch.Generator().manual_seed(3)
    ph = torch.rand(V, R_, K, dtype=torch.float64, generator=g) * 1e-3
    doc = torch.randint(-1, D, (n,), generator=g, dtype=torch.int32)
    word = torch.randint(-1, V, (n,), generator=g, dtype=torch.int32)
    rows_u, _, cnt_u = R.peer_topn(th, torch.arange(D, dtype=torch.int32), N)
    cnt_u[::4] = 2      # short lists: the slots past the count hold real rows here and must be masked all the same
    cnt_u[1::8] = 0
    at = doc.long().clamp_min(0)
    rows, count = rows_u[at], torch.where(doc >= 0, cnt_u[at], torch.zeros_like(cnt_u[at]))
    model = S.TopicModel(th[:, 0].contiguous(), ph[:, 0].contiguous(), K, 0.05) if R_ == 1 else \
        S.EnsembleModel(th, ph, R_, K, 0.05)
    got = S.peer_scores(model, rows, count, doc, word)
    want = torch.full((n,), float("nan"), dtype=torch.float64)
    seen = 0
    for i in range(n):
        c = int(count[i])
        if doc[i] < 0 or word[i] < 0 or c == 0:
            continue
        acc = torch.zeros((), dtype=torch.float64)
        for j in range(c):
            d, w = rows[i, j:j + 1], word[i:i + 1]
            s = R.score(th[:, 0], ph[:, 0], K, 0.05, d, w)[0] if R_ == 1 else \
                R.score_ensemble(th, ph, R_, K, 0.05, d, w)[0]
            acc = acc + s[0]
        want[i] = acc / float(c)
        seen += 1
    assert seen > 150 and int(torch.isnan(want).sum()) > 30 and bits_equal(got, want)


# ---------------------------------------------------------------------------------------- end to end
ALL = ["flow-strict", "flow-fixed", "dns-strict", "proxy-fixed"]
_DAYS = {}
NP = 4      # peers of the days' runs


def get_day(which, tmp_path_factory):
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("peers_" + kind + compat))
    return _DAYS[which]


def read_peers(day, lp):
    """Per line: (key text, [per side (doc, word, score, peers, peer_dist, peer_score, peer_lift) texts])."""
    sep, sides = SIDES[day.kind]
    lines = (lp / f"{day.kind}_peers.csv").read_text(encoding="utf-8").split("\n")
    assert lines[-1] == ""
    out = []
    for ln in lines[:-1]:
        f = ln.split(sep)
        assert len(f) == 1 + 7 * len(sides)
        out.append((f[0], [tuple(f[1 + 7 * j:8 + 7 * j]) for j in range(len(sides))]))
    return out


def num(texts):
    return f64([float(t) if t else float("nan") for t in texts])


def check_peer_files(day, lp, summary, members=1, n_peers=NP):
    """Both files against the results file line for line, against the twin over the written tables, and against the
    summary."""
    rows = read_peers(day, lp)
    sep, sides = SIDES[day.kind]
    res = [ln.split(sep) for ln in (lp / day.results).read_text(encoding="utf-8").split("\n")[:-1]]
    assert len(res) == len(rows) == summary["scored"] > 20
    for f, (key, ss) in zip(res, rows):
        assert [s[:3] for s in ss] == [(f[c[0]], f[c[1]], f[c[2]]) for c in sides]
        assert float(key) == min(float(s[2]) for s in ss)
    dn, wn, th, ph = _tables(lp, members)
    D, R_, K = th.shape
    di = {n: i for i, n in enumerate(dn)}      # later duplicates win, as the scorers' maps
    wi = {n: i for i, n in enumerate(wn)}
    flat = [s for _, ss in rows for s in ss]
    doc, word = i32([di.get(s[0], -1) for s in flat]), i32([wi.get(s[1], -1) for s in flat])
    ud = torch.unique(doc[doc >= 0])
    rows_u, dist_u, cnt_u = R.peer_topn(th, ud.to(torch.int32), n_peers)
    at = torch.searchsorted(ud, doc.clamp_min(0)).clamp_max(ud.numel() - 1)      # (a side without a document: masked)
    has = doc >= 0
    cnt = torch.where(has, cnt_u[at], torch.zeros_like(cnt_u[at]))
    assert [s[3] for s in flat] == ["" if not h else str(int(c)) for h, c in zip(has.tolist(), cnt.tolist())]
    last = torch.gather(dist_u[at], 1, (cnt.long() - 1).clamp_min(0).unsqueeze(1)).reshape(-1)
    far = torch.where(has & (cnt > 0), last / (2.0 * R_), torch.full_like(last, float("nan")))
    assert bits_equal(num([s[4] for s in flat]), far)
    model = S.TopicModel(th[:, 0].contiguous(), ph[:, 0].contiguous(), K, day.default(K)) if members == 1 else \
        S.EnsembleModel(th, ph, R_, K, day.default(K))
    ps = S.peer_scores(model, rows_u[at], cnt, doc, word)
    assert bits_equal(num([s[5] for s in flat]), ps)
    lift = ps / num([s[2] for s in flat])
    got_lift = num([s[6] for s in flat])
    assert bits_equal(got_lift, lift)
    good = got_lift[~torch.isnan(got_lift)]
    assert good.numel() > 20 and bool((good > 0).all())
    # the groups file: exactly the distinct documents of the written sides, ascending by row
    g = [ln.split(sep) for ln in (lp / f"{day.kind}_peer_groups.csv").read_text(encoding="utf-8").split("\n")[:-1]]
    assert [x[0] for x in g] == [dn[d] for d in ud.tolist()] and all(len(x) == 2 + 2 * n_peers for x in g)
    assert {x[0] for x in g} == {s[0] for s in flat if s[3]}
    for x, r, d, c in zip(g, rows_u.tolist(), dist_u, cnt_u.tolist()):
        assert x[1] == str(c)
        assert x[2::2] == [dn[p] if p >= 0 else "" for p in r]
        want = torch.where(torch.arange(n_peers) < c, d / (2.0 * R_), torch.full_like(d, float("nan")))
        assert bits_equal(num(x[3::2]), want)
    hist = summary["peer_lift_hist"]
    assert list(hist) == list(PEER_LIFT_DECADES) + ["none"] and sum(hist.values()) == len(flat)
    assert hist["none"] == int(torch.isnan(got_lift).sum())
    assert hist["<1e1"] == int(((good >= 1) & (good < 10)).sum())
    assert summary["peers"] == n_peers and summary["peer_hosts"] == ud.numel() and summary["peer_candidates"] == D
    assert summary["peer_path"] == ("cpu" if day.device == "cpu" else "registers")
    assert summary["peer_identical"] == int(((cnt_u > 0) & (dist_u[:, 0] == 0)).sum())
    return got_lift


@pytest.mark.parametrize("which", ALL)
def test_day_with_peers(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    plain, sp = day.run("plain")
    lp, s = day.run("peers", peers=NP)
    a, b = tree(plain), tree(lp)
    assert set(b) - set(a) == {f"{day.kind}_peers.csv", f"{day.kind}_peer_groups.csv"} and set(a) <= set(b)
    for f in a:
        assert a[f] == b[f], f      # the results file and every LDA file: byte for byte the plain run's
    assert not PEER_KEYS & set(sp) and {k for k in s if k not in sp} == PEER_KEYS
    recs = [json.loads(x) for x in (lp / "metrics.jsonl").read_text().splitlines()]
    det = [r for r in recs if r.get("stage") == f"{day.kind}_post_detail" and "peer_lift_hist" in r]
    assert len(det) == 1 and det[0]["peer_lift_hist"] == s["peer_lift_hist"] and det[0]["peer_hosts"] == s["peer_hosts"]
    got = check_peer_files(day, lp, s)
    assert which != "flow-strict" or bool(torch.isnan(got).any())      # a side without a row: empty cells


@pytest.mark.parametrize("which", ["flow-strict", "dns-strict", "proxy-fixed"])
def test_max_results_ensemble_and_the_other_options(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp, s = day.run("peers", peers=NP)
    name, gname = f"{day.kind}_peers.csv", f"{day.kind}_peer_groups.csv"
    full = (lp / name).read_bytes().splitlines(keepends=True)
    N = s["scored"] // 3
    lim, sl = day.run("peers_lim", peers=NP, max_results=N)
    assert (lim / name).read_bytes() == b"".join(full[:N]) and N > 5
    assert sum(sl["peer_lift_hist"].values()) == N * len(SIDES[day.kind][1]) and sl["peer_hosts"] <= s["peer_hosts"]
    check_peer_files(day, lim, sl)      # the groups file describes the head's documents
    # --ensemble 3 with the largest N: the twin over the three written member tables
    ens, se = day.run("peers_ens3", peers=16, ensemble=3)
    check_peer_files(day, ens, se, members=3, n_peers=16)
    a, b = tree(day.run("ens3", ensemble=3)[0]), tree(ens)      # the members' files and the results file: unchanged
    assert set(b) - set(a) == {name, gname} and all(a[f] == b[f] for f in a)
    # --explain, --tail-tol and the host report beside it: each file is what it is without the flag
    both, sb = day.run("peers_all", peers=NP, explain=True, tail_tol=0.5, host_report=-1)
    alone, sa = day.run("all_but_peers", explain=True, tail_tol=0.5, host_report=-1)
    a, b = tree(alone), tree(both)
    assert set(b) - set(a) == {name, gname} and all(a[f] == b[f] for f in a)
    check_peer_files(day, both, sb)
    assert PEER_KEYS <= set(sb) and "explain_why_hist" in sb and "tail_hist" in sb and not PEER_KEYS & set(sa)


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_resume_writes_the_same_files(which, tmp_path_factory):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)
    names = (f"{day.kind}_peers.csv", f"{day.kind}_peer_groups.csv")
    first = day.run("peers", peers=NP)[0]
    want = [(first / f).read_bytes() for f in names]
    lp = day.root / "resume"
    day.go(day.cfg(lp, peers=NP))
    post = f"{day.kind}_post"
    assert [(lp / f).read_bytes() for f in names] == want
    # at the scoring stage: nothing but the model tables is needed
    os.unlink(lp / ".stages" / f"{post}.done")
    for f in names:
        os.unlink(lp / f)
    s = run(day.cfg(lp, peers=NP, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert [(lp / f).read_bytes() for f in names] == want and PEER_KEYS <= set(s)
    # a run that had no flag, resumed with it
    plain = day.root / "resume_plain"
    day.go(day.cfg(plain))
    os.unlink(plain / ".stages" / f"{post}.done")
    run(day.cfg(plain, peers=NP, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert [(plain / f).read_bytes() for f in names] == want


@pytest.mark.parametrize("which", ["flow-strict", "proxy-fixed"])
def test_refusals_write_nothing(which, tmp_path_factory, monkeypatch):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)

    class Group:
        active, rank, world_size = True, 0, 2
    never = day.root / "never"
    assert CFG.RunConfig().peers == 0 and CFG.PEERS_ONE_PROCESS.startswith("--peers") and CFG.PEERS_MAX == 16
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="one process"):
            day.cfg(never, peers=3, **kw).validate()
        with pytest.raises(ValueError, match="one process"):
            run(day.cfg(never, peers=3, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, peers=3), dist=Group(), device="cpu")
    for bad in (17, -1):
        with pytest.raises(ValueError, match="--peers must be"):
            day.cfg(never, peers=bad).validate()
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("PEERS", raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    for extra in (["--peers", "3", "--gpus", "2"], ["--peers", "3", "--hdfs"]):
        with pytest.raises(ValueError, match="one process"):
            cli.cmd_ml_ops(base + extra)
    with pytest.raises(ValueError, match="--peers must be"):
        cli.cmd_ml_ops(base + ["--peers", "17"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--peers", "3"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("PEERS", "3")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    monkeypatch.setenv("PEERS", "17")
    with pytest.raises(ValueError, match="--peers must be"):
        cli.cmd_ml_ops(base)
    assert not never.exists()


def test_a_fresh_run_removes_stale_peer_files(tmp_path):
    for f in ("flow_peers.csv", "flow_peer_groups.csv", "flow_scores.csv", "flow_results.csv"):
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
    monkeypatch.delenv("PEERS", raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nPEERS=7\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].peers == 0
    assert cli.cmd_ml_ops(base + none + ["--peers", "5"]) == 0 and seen["cfg"].peers == 5
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].peers == 7
    monkeypatch.setenv("PEERS", "0")      # the environment over the file; 0 is off, not an error
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].peers == 0
    assert CFG.RunConfig.check_peers(0, gpus=2, hdfs=True, world=2) == 0
    monkeypatch.setenv("PEERS", "16")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].peers == 16
    assert cli.cmd_ml_ops(base + none + ["--peers", "2"]) == 0 and seen["cfg"].peers == 2      # the flag over both
    assert "PEERS" in CFG.ENV_KEYS and CFG.PEERS_BLOCK >= 1 and CFG.PEERS_SCRATCH_MB > 0
