"""--ensemble R on the CPU path: the torch twin ``ops.reference.score_ensemble`` (order of the member sum, votes,
misses, NaN), and the three pipelines end to end on the torch LDA backend -- member 0 is the plain run, the
written scores are exactly the twin over the members' written tables, resume, the host report, the refusals and
the three ways to set R.  Every comparison is exact.

"Byte-identical" leaves out what carries wall-clock times: metrics.jsonl, lda_stats.json, run_summary.json, the
completion markers (.stages/, a member's .done); a .npz file (a zip archive stamps its entries with the time) is
compared array by array, by bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_report_cases as HC  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.export import lda_post  # noqa: E402
from oni_ml_amd.models.lda.settings import LDASettings  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

f64 = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
i32 = lambda x: torch.tensor(x, dtype=torch.int32)        # noqa: E731


def bits_equal(a, b):
    """The same doubles bit for bit; a NaN matches any NaN (its payload is not part of the result)."""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype != torch.float64:
        return a.dtype == b.dtype and torch.equal(a, b)
    nan = torch.isnan(a)
    return (b.dtype == torch.float64 and a.shape == b.shape and torch.equal(nan, torch.isnan(b))
            and torch.equal(a[~nan].view(torch.int64), b[~nan].view(torch.int64)))


# ------------------------------------------------------------------------------------------ the twin
def _batch(n, D, V, R_, K, seed, two):
    g = torch.Generator().manual_seed(seed)
    th = torch.rand(D, R_, K, dtype=torch.float64, generator=g)
    ph = torch.rand(V, R_, K, dtype=torch.float64, generator=g) * 1e-3

    def idx(rows):
        x = torch.randint(0, rows, (n,), generator=g, dtype=torch.int32)
        x[torch.rand(n, generator=g) < 0.1] = -1
        return x

    def side():
        d, w = idx(D), idx(V)
        d[:3] = i32([-1, -1, 0])      # both missing, the document alone, the word alone
        w[:3] = i32([-1, 0, -1])
        return d, w
    return (th, ph) + side() + (side() if two else (None, None))


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("K", [1, 7, 20])
def test_twin_at_one_member_is_the_scorer(K, two):
    th, ph, da, wa, db, wb = _batch(501, 23, 31, 1, K, 5 + K, two)
    assert (da < 0).any() and (wa < 0).any() and ((da < 0) & (wa < 0)).any()
    tol = 0.1 * K * 1e-3
    want = R.score(th[:, 0].contiguous(), ph[:, 0].contiguous(), K, 0.05, da, wa, db, wb, tol)
    got = R.score_ensemble(th, ph, 1, K, 0.05, da, wa, db, wb, tol)
    assert all(bits_equal(g, w) for g, w in zip(got[:4], want))
    assert 0 < int(want[3].sum()) < 501 and torch.equal(got[4], want[3])      # one member: its vote is the flag
    # and through the dispatcher, votes on the model
    m = S.EnsembleModel(th, ph, 1, K, 0.05)
    out = S.score_votes(m, da, wa, db, wb, tol)
    assert len(out) == 5 and all(bits_equal(g, w) for g, w in zip(out[:4], want)) and torch.equal(out[4], want[3])
    assert all(bits_equal(g, w) for g, w in zip(S.score(m, da, wa, db, wb, tol), want))
    # one model through the same entry point: no votes
    t = S.TopicModel(th[:, 0].contiguous(), ph[:, 0].contiguous(), K, 0.05)
    one = S.score_votes(t, da, wa, db, wb, tol)
    assert one[4] is None and all(bits_equal(g, w) for g, w in zip(one[:4], want))


def test_member_sum_runs_in_member_order():
    th = torch.ones(1, 3, 1, dtype=torch.float64)
    ph = f64([[[0.1], [0.2], [0.3]]])
    z = i32([0])
    sa, sb, key, flag, votes = R.score_ensemble(th, ph, 3, 1, 0.5, z, z, None, None, 0.25)
    left = ((0.0 + 0.1) + 0.2) + 0.3
    other = 0.1 + (0.2 + 0.3)
    assert left != other      # the two associations round differently, so the case tells them apart
    assert sa.item() == left / 3 and left / 3 != other / 3
    assert sb is None and key.item() == sa.item() and flag.item() == 1 and votes.item() == 2
    # as many rounded adds as members, in order, at every R (a hand fold)
    g = torch.Generator().manual_seed(1)
    ph = torch.rand(1, 8, 1, dtype=torch.float64, generator=g)
    th = torch.ones(1, 8, 1, dtype=torch.float64)
    for R_ in (2, 5, 8):
        s = 0.0
        for r in range(R_):
            s = s + (0.0 + 1.0 * ph[0, r, 0].item())
        got = R.score_ensemble(th[:, :R_].contiguous(), ph[:, :R_].contiguous(), R_, 1, 0.5, z, z)[0]
        assert got.item() == s / R_, R_


def test_votes_count_the_members_own_keys():
    """Two sides, three members.  Member keys (the lower of the member's two sides): 0.01, 0.2, 0.03; tol 0.05
    lies between them: two votes.  The ensemble key is the lower side mean, not the mean of the member keys."""
    th = torch.ones(1, 3, 1, dtype=torch.float64)
    ph = f64([[[0.01], [0.9], [0.03]],        # word 0: side a
              [[0.5], [0.2], [0.6]]])         # word 1: side b
    z = i32([0])
    sa, sb, key, flag, votes = R.score_ensemble(th, ph, 3, 1, 0.5, z, i32([0]), z, i32([1]), 0.05)
    assert sa.item() == (((0.0 + 0.01) + 0.9) + 0.03) / 3 and sb.item() == (((0.0 + 0.5) + 0.2) + 0.6) / 3
    assert key.item() == sa.item() and flag.item() == 0 and votes.item() == 2
    # tol is a strict bound for the votes as for the flag
    assert R.score_ensemble(th, ph, 3, 1, 0.5, z, i32([0]), z, i32([1]), 0.03)[4].item() == 1
    assert R.score_ensemble(th, ph, 3, 1, 0.5, z, i32([0]), z, i32([1]), 1.0)[4].item() == 3


def test_misses_take_the_default_vector_in_every_member():
    g = torch.Generator().manual_seed(2)
    K, R_, dflt = 4, 3, 0.25
    th = torch.rand(2, R_, K, dtype=torch.float64, generator=g)
    ph = torch.rand(2, R_, K, dtype=torch.float64, generator=g)
    d = i32([1, -1, 1, -1])
    w = i32([0, 0, -1, -1])
    got = R.score_ensemble(th, ph, R_, K, dflt, d, w)[0]
    for i in range(4):
        s = 0.0
        for r in range(R_):
            m = 0.0
            for k in range(K):
                t = th[d[i], r, k].item() if d[i] >= 0 else dflt
                p = ph[w[i], r, k].item() if w[i] >= 0 else dflt
                m = m + t * p
            s = s + m
        assert got[i].item() == s / R_, i
    assert got[3].item() == K * dflt * dflt      # both missing: the default vector's own product (exact here)


def test_a_nan_in_one_member_makes_the_side_nan():
    th = torch.ones(2, 3, 2, dtype=torch.float64)
    ph = torch.full((2, 3, 2), 1e-3, dtype=torch.float64)
    ph[1, 1, 0] = float("nan")
    d = i32([0, 0])
    sa, _, key, flag, votes = R.score_ensemble(th, ph, 3, 2, 0.5, d, i32([0, 1]), None, None, 1.0)
    assert not np.isnan(sa[0].item()) and flag[0].item() == 1 and votes[0].item() == 3
    assert np.isnan(sa[1].item()) and np.isnan(key[1].item()) and flag[1].item() == 0 and votes[1].item() == 2
    # two-sided, the NaN on side b: the key is NaN (a < NaN is false) and the flag 0
    sa, sb, key, flag, votes = R.score_ensemble(th, ph, 3, 2, 0.5, d, i32([0, 0]), d, i32([0, 1]), 1.0)
    assert np.isnan(sb[1].item()) and np.isnan(key[1].item()) and flag.tolist() == [1, 0]


def test_twin_refuses_tables_of_another_shape():
    th, ph, da, wa, db, wb = _batch(9, 5, 6, 2, 3, 1, True)
    for bad in (dict(theta=th[:, 0]), dict(R=3), dict(K=2), dict(phi=ph[:, :1])):
        a = dict(theta=th, phi=ph, R=2, K=3)
        a.update(bad)
        with pytest.raises(ValueError):
            R.score_ensemble(a["theta"], a["phi"], a["R"], a["K"], 0.1, da, wa, db, wb)
    with pytest.raises(ValueError, match="go together"):
        R.score_ensemble(th, ph, 2, 3, 0.1, da, wa, db, None)


# ---------------------------------------------------------------------------------------- end to end
TOL = dict(flow=1e-3, dns=1e-2, proxy=1e-3)
TIMED = {"metrics.jsonl", "lda_stats.json", "run_summary.json", ".done", ".lock"}
# (separator, ip column, word column, score column) of every side of a results line
SIDES = {"flow": (",", ((8, 33, 35), (9, 34, 36))), "dns": (",", ((3, 14, 15),)), "proxy": ("\t", ((2, 19, 20),))}


def tree(lp):
    """relative path -> bytes of every file under ``lp`` that carries no wall-clock time (.npz: its arrays)."""
    out = {}
    for root, dirs, files in os.walk(lp):
        dirs[:] = [d for d in dirs if d != ".stages"]
        for f in files:
            if f in TIMED:
                continue
            p = os.path.join(root, f)
            if f.endswith(".npz"):
                with np.load(p, allow_pickle=False) as z:
                    out[os.path.relpath(p, lp)] = {k: (z[k].dtype.str, z[k].shape, z[k].tobytes()) for k in z.files}
            else:
                with open(p, "rb") as fh:
                    out[os.path.relpath(p, lp)] = fh.read()
    return out


class Day:
    """One synthetic day of a type and a compat mode, and its runs, each in a directory of its own (run once)."""

    def __init__(self, kind, compat, root, backend="torch", device="cpu", scale=1):
        self.kind, self.compat, self.root, self.backend, self.device, self.runs = kind, compat, root, backend, device, {}
        if kind == "flow":      # the day of tests/test_pipeline.py
            from oni_ml_amd.synth.flow import generate_flow_day
            generate_flow_day(str(root / "in") + "/", events=4000 * scale, seed=11, n_internal=300, n_external=600)
            self.gen, self.paths = str(root / "in"), dict(flow_path=str(root / "in"))
        elif kind == "dns":
            from oni_ml_amd.synth.dns import generate_dns_day
            g = generate_dns_day(str(root / "in"), events=6000 * scale, seed=3, files=3, n_names=800, n_clients=300)
            self.gen, self.paths = g, dict(dns_path=g["dns_path"], top1m=g["top1m"])
        else:
            from oni_ml_amd.synth.proxy import generate_proxy_day
            g = generate_proxy_day(str(root / "in"), events=3000 * scale, seed=5, files=2)
            self.gen, self.paths = g, dict(proxy_path=g["proxy_path"], top1m=g["top1m"])
        self.results = f"{kind}_results.csv"

    def cfg(self, lpath, **kw):
        cfg = CFG.resolve("20160122", self.kind, tol=TOL[self.kind], conf_path=None, environ={}, lpath=str(lpath),
                          backend=self.backend, threads=2, verbose=False, compat=self.compat, **self.paths, **kw)
        cfg.settings = LDASettings(em_max_iter=3)
        return cfg

    def go(self, cfg):
        from oni_ml_amd.pipeline import run
        return run(cfg.validate(), device=self.device, log=lambda *a, **k: None)

    def run(self, name, **kw):
        """(work directory, summary) of the run ``name`` with these options."""
        if name not in self.runs:
            lp = self.root / name
            self.runs[name] = (lp, self.go(self.cfg(lp, **kw)))
        return self.runs[name]

    def default(self, K):
        if self.kind == "proxy":
            return S.default_value("proxy", K, False)
        return S.default_value(self.kind, K, self.compat == "strict")


ALL = ["flow-strict", "flow-fixed", "dns-strict", "proxy-fixed"]
_DAYS = {}


def get_day(which, tmp_path_factory):
    """The day ``which`` ("<type>-<compat>"), made once for the module: its runs are shared by the tests."""
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("ens_" + kind + compat))
    return _DAYS[which]


def twin_scores_of_file(day, lp, members=3):
    """The score columns of the results file and the twin over the members' written tables, looked up by the
    names on every line: ([parsed side scores], [twin side scores]), each [sides][rows]."""
    dirs = [str(lp)] + [os.path.join(str(lp), "ensemble", f"m{r}") for r in range(1, members)]
    tabs = [(lda_post.read_results(os.path.join(d, "doc_results.csv")),
             lda_post.read_results(os.path.join(d, "word_results.csv"))) for d in dirs]
    (dn, _), (wn, _) = tabs[0]
    assert all(t[0][0] == dn and t[1][0] == wn for t in tabs)      # one corpus: the rows are shared
    th = torch.from_numpy(np.ascontiguousarray(np.stack([t[0][1] for t in tabs], 1)))
    ph = torch.from_numpy(np.ascontiguousarray(np.stack([t[1][1] for t in tabs], 1)))
    di = {n: i for i, n in enumerate(dn)}      # later duplicates win, as the scorers' maps
    wi = {n: i for i, n in enumerate(wn)}
    sep, sides = SIDES[day.kind]
    lines = (lp / day.results).read_text(encoding="utf-8").split("\n")
    assert lines[-1] == "" and len(lines) > 20
    rows = [ln.split(sep) for ln in lines[:-1]]
    idx, parsed = [], []
    for ip_c, w_c, s_c in sides:
        idx += [i32([di.get(f[ip_c], -1) for f in rows]), i32([wi.get(f[w_c], -1) for f in rows])]
        parsed.append(f64([float(f[s_c]) for f in rows]))
    K = th.shape[2]
    out = R.score_ensemble(th, ph, members, K, day.default(K), *idx, tol=TOL[day.kind])
    return parsed, [out[0]] + ([out[1]] if len(sides) == 2 else []), out


@pytest.mark.parametrize("which", ALL)
def test_member_0_is_the_plain_run(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    plain, _ = day.run("plain")
    ens, s = day.run("ens3", ensemble=3)
    a, b = tree(plain), tree(ens)
    assert len(a) >= 12 and day.results in a and "final_model.npz" in a and "final.beta" in a
    for f in a:
        if f != day.results:
            assert a[f] == b[f], f
    assert a[day.results] != b[day.results]
    for r in (1, 2):
        have = set(os.listdir(ens / "ensemble" / f"m{r}"))
        assert {"final.beta", "final.gamma", "final.other", "likelihood.dat", "final_model.npz", "doc_results.csv",
                "word_results.csv", ".done"} <= have, have
        assert not {"doc.dat", "words.dat", "model.dat", "word-assignments.dat"} & have
        assert not [f for f in have if f[:3].isdigit() and f[:3] != "000"]      # lag 0
        assert (ens / "ensemble" / f"m{r}" / "final.beta").read_bytes() != (ens / "final.beta").read_bytes()
    assert not (plain / "ensemble").exists()
    m = s["lda"]["members"]
    assert [x["member"] for x in m] == [0, 1, 2] and [x["seed"] for x in m] == [0, 1, 2]
    assert all(x["em_iterations"] >= 1 and x["likelihood"] < 0 and x["alpha"] > 0 and x["seconds"] > 0 for x in m)
    import json
    assert json.loads((ens / "lda_stats.json").read_text())["ensemble"] == json.loads(json.dumps(m))
    assert "ensemble" not in json.loads((plain / "lda_stats.json").read_text())


@pytest.mark.parametrize("which", ALL)
def test_written_scores_are_the_twin_over_the_written_member_tables(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    ens, s = day.run("ens3", ensemble=3)
    parsed, twin, out = twin_scores_of_file(day, ens)
    for p, t in zip(parsed, twin):
        assert bits_equal(p, t)
    key = out[2].tolist()
    assert key == sorted(key) and key[-1] < TOL[day.kind]      # ascending, all under TOL
    hist = s["ensemble_votes_hist"]
    assert hist == np.bincount(out[4].numpy(), minlength=4).tolist() and sum(hist) == s["scored"] == len(key)
    # a different result than any one member's: the plain run flags another set
    assert (ens / day.results).read_bytes() != (day.run("plain")[0] / day.results).read_bytes()


@pytest.mark.parametrize("which", ALL)
def test_max_results_writes_the_head(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    ens, s = day.run("ens3", ensemble=3)
    N = s["scored"] // 3
    lim, sl = day.run("ens3_lim", ensemble=3, max_results=N)
    assert sl["scored"] == N and sl["below_tol"] == s["scored"] and sum(sl["ensemble_votes_hist"]) == N
    full = (ens / day.results).read_bytes().splitlines(keepends=True)
    assert (lim / day.results).read_bytes() == b"".join(full[:N])


@pytest.mark.parametrize("which", ["flow-strict"])
def test_one_member_is_the_run_without_the_option(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    plain, sp = day.run("plain")
    one, so = day.run("ens1", ensemble=1)
    assert tree(plain) == tree(one) and not (one / "ensemble").exists()
    assert "ensemble_votes_hist" not in so and "members" not in so["lda"]


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_resume_writes_the_same_files(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp = day.root / "resume"
    day.go(day.cfg(lp, ensemble=3))
    want = tree(lp)
    assert want == tree(day.run("ens3", ensemble=3)[0])      # the uninterrupted run, twice: deterministic
    post = f"{day.kind}_post"
    member_csv = [lp / "ensemble" / f"m{r}" / f for r in (1, 2) for f in ("doc_results.csv", "word_results.csv")]

    def resume(expect_skipped, expect_run):
        logs = []
        from oni_ml_amd.pipeline import run
        run(day.cfg(lp, ensemble=3, resume=True).validate(), device=day.device, log=logs.append)
        text = "\n".join(str(x) for x in logs)
        for st in expect_skipped:
            assert f"[stage {st}] already complete" in text, (st, text)
        for st in expect_run:
            assert f"[stage {st}] already complete" not in text and f"[stage {st}]" in text, (st, text)
        assert tree(lp) == want

    # after lda: the tables of every member and the scores are made again from the model files
    for p in [lp / ".stages" / "lda_post.done", lp / ".stages" / f"{post}.done", lp / day.results,
              lp / "doc_results.csv", lp / "word_results.csv"] + member_csv:
        os.unlink(p)
    resume(["lda"], ["lda_post", post])
    # after lda_post: the member tables are read back from their files
    os.unlink(lp / ".stages" / f"{post}.done")
    os.unlink(lp / day.results)
    resume(["lda", "lda_post"], [post])
    # a member without its marker is fitted again from its seed, then exported and scored again
    os.unlink(lp / "ensemble" / "m1" / ".done")
    before = (lp / "ensemble" / "m2" / "final.beta").stat().st_mtime_ns
    resume(["lda"], ["lda_members", "lda_post", post])
    assert (lp / "ensemble" / "m2" / "final.beta").stat().st_mtime_ns == before      # member 2 was kept
    assert (lp / "ensemble" / "m1" / ".done").exists()
    assert not (lp / ".stages" / "lda_members.done").exists()      # the members' own markers are the record
    # and a finished run resumed does nothing
    resume(["lda", "lda_post", post], [])


def test_a_member_of_another_seed_or_topic_count_is_fitted_again(tmp_path_factory):
    """A member's marker names what it was fitted with: a resume that asks for something else does not keep it."""
    import json
    from oni_ml_amd.pipeline import common as C
    day = get_day("flow-fixed", tmp_path_factory)
    lp = day.root / "reseed"
    (lp / "ensemble" / "m7").mkdir(parents=True)      # left by an earlier, larger ensemble
    day.go(day.cfg(lp, ensemble=3))
    assert sorted(os.listdir(lp / "ensemble")) == ["m1", "m2"]      # a fresh run keeps nothing of it
    cfg = day.cfg(lp, ensemble=3, resume=True)
    assert C.members_to_fit(cfg) == [] and C.member_done(cfg, 1)
    assert C.members_to_fit(day.cfg(lp, ensemble=3, resume=True, seed=4)) == [1, 2]
    assert C.members_to_fit(day.cfg(lp, ensemble=3, resume=True, topics=7)) == [1, 2]
    assert C.members_to_fit(day.cfg(lp, ensemble=3, resume=True, start="seeded")) == [1, 2]
    assert C.members_to_fit(day.cfg(lp, ensemble=3)) == [1, 2]      # not a resume: all of them
    mark = lp / "ensemble" / "m2" / ".done"
    m = json.loads(mark.read_text())
    assert m["seed"] == 2 and m["topics"] == 20 and m["compat"] == "fixed"
    m["seed"] = 9      # as if member 2 came from a run with another --seed
    mark.write_text(json.dumps(m))
    before = (lp / "ensemble" / "m1" / "final.beta").stat().st_mtime_ns
    logs = []
    from oni_ml_amd.pipeline import run
    s = run(cfg.validate(), device="cpu", log=logs.append)
    assert json.loads(mark.read_text())["seed"] == 2 and any("[stage lda_members]" in str(x) for x in logs)
    assert (lp / "ensemble" / "m1" / "final.beta").stat().st_mtime_ns == before
    assert tree(lp) == tree(day.run("ens3", ensemble=3)[0])
    assert [x["seed"] for x in s["lda"]["members"]] == [0, 1, 2]


def test_a_plain_run_resumed_as_an_ensemble_reports_member_0(tmp_path_factory):
    import json
    day = get_day("flow-fixed", tmp_path_factory)
    lp = day.root / "plain_then_ens"
    day.go(day.cfg(lp))
    plain = json.loads((lp / "lda_stats.json").read_text())
    s = day.go(day.cfg(lp, ensemble=2, resume=True))
    m0, m1 = s["lda"]["members"]
    assert m0["member"] == 0 and m0["em_iterations"] == plain["em_iterations"] and m0["alpha"] == plain["alpha"]
    assert m0["seconds"] == plain["seconds"] and m0["likelihood"] < 0
    last = (lp / "likelihood.dat").read_text().split("\n")[-2].split()[0]
    assert m0["likelihood"] == float(last)
    assert m1["member"] == 1 and m1["em_iterations"] >= 1 and set(m1) == set(m0)
    assert json.loads((lp / "lda_stats.json").read_text())["ensemble"] == json.loads(json.dumps([m0, m1]))
    assert not (lp / "lda_stats.json.tmp").exists()
    # the scores are those of the uninterrupted two-member run
    two, _ = day.run("ens2", ensemble=2)
    assert (lp / day.results).read_bytes() == (two / day.results).read_bytes()


@pytest.mark.parametrize("which", ["flow-fixed", "dns-fixed", "proxy-fixed"])      # the recount reads every input row
def test_hosts_file_is_a_recount_of_the_ensemble_results_file(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp, s = day.run("hosts", ensemble=3, host_report=-1)
    counts = HC.input_counts(day.kind, day.gen)
    lines = HC.check_hosts_file(day.kind, str(lp), TOL[day.kind], counts)
    assert len(lines) >= 20 and s["hosts"] == len(lines)
    assert (lp / day.results).read_bytes() == (day.run("ens3", ensemble=3)[0] / day.results).read_bytes()


@pytest.mark.parametrize("which", ALL)
def test_refusals_write_nothing(which, tmp_path_factory, monkeypatch):
    day = get_day(which, tmp_path_factory)
    class Group:
        active, rank, world_size = True, 0, 2
    from oni_ml_amd.pipeline import run
    never = day.root / "never"
    assert CFG.RunConfig().ensemble == 1
    model = str(day.run("plain")[0] / "final")
    cases = [(dict(ensemble=0), r"\[1, 64\]"), (dict(ensemble=65), r"\[1, 64\]"), (dict(ensemble=-3), r"\[1, 64\]"),
             (dict(ensemble=3, start=model), "same model"), (dict(ensemble=3, gpus=2), "one process"),
             (dict(ensemble=3, hdfs=True), "one process")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            day.cfg(never, **kw).validate()
        with pytest.raises(ValueError, match=msg):
            run(day.cfg(never, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, ensemble=3), dist=Group(), device="cpu")
    assert CFG.ENSEMBLE_ONE_PROCESS.startswith("--ensemble")
    # the command line refuses before a process group is asked for and before the work directory is made
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("ENSEMBLE", raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    for extra, msg in ((["--ensemble", "0"], r"\[1, 64\]"), (["--ensemble", "65"], r"\[1, 64\]"),
                       (["--ensemble", "3", "--start", model], "same model"),
                       (["--ensemble", "3", "--gpus", "2"], "one process"),
                       (["--ensemble", "3", "--hdfs"], "one process")):
        with pytest.raises(ValueError, match=msg):
            cli.cmd_ml_ops(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")      # a torchrun launch
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--ensemble", "3"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("ENSEMBLE", "3")        # set by the environment: the same refusal
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    assert not never.exists()
    for ok in (1, 2, 64):
        assert day.cfg(never, ensemble=ok).validate().ensemble == ok
    assert day.cfg(never, ensemble=2, start="seeded").validate().start == "seeded"


def test_cli_flag_environment_and_site_file_reach_the_config(monkeypatch, tmp_path):
    seen = {}

    def body(a, resolve):
        seen["cfg"] = resolve(1)
        return 0

    monkeypatch.setattr(cli, "_ml_ops_body", body)
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("ENSEMBLE", raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nENSEMBLE=4\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].ensemble == 1
    assert cli.cmd_ml_ops(base + none + ["--ensemble", "8"]) == 0 and seen["cfg"].ensemble == 8
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].ensemble == 4
    monkeypatch.setenv("ENSEMBLE", "5")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].ensemble == 5
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].ensemble == 5      # environment over file
    assert cli.cmd_ml_ops(base + ["--conf", str(conf), "--ensemble", "2"]) == 0 and seen["cfg"].ensemble == 2
    assert "ENSEMBLE" in CFG.ENV_KEYS
    c = CFG.resolve("20160122", "flow", conf_path=str(conf), environ={})
    assert c.ensemble == 4 and CFG.resolve("20160122", "flow", conf_path=None, environ={"ENSEMBLE": "7"}).ensemble == 7


def test_a_fresh_run_removes_the_members_of_an_earlier_one(tmp_path):
    m = tmp_path / "ensemble" / "m1"
    m.mkdir(parents=True)
    (m / "final.beta").write_text("x")
    (tmp_path / "flow_scores.csv").write_text("kept")
    cli.clean_workdir(str(tmp_path))
    assert not (tmp_path / "ensemble").exists() and (tmp_path / "flow_scores.csv").read_text() == "kept"
