"""--host-report on the CPU path: the torch twin ``ops.reference.host_summary`` against a literal oracle (a
Python loop over the sides, tests/host_report_cases.py) over key sets x sizes x document shapes, ``rank_hosts``,
the twin's refusals, and the three pipelines end to end on the CPU backend -- the hosts file checked against the
results file's text and the input only.  Every comparison is exact: counts, minima and side numbers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_report_cases as HC  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.models.lda.settings import LDASettings  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402


# ------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("shape", HC.SHAPES)
@pytest.mark.parametrize("keyset", HC.KEYSETS)
def test_twin_equals_the_oracle(keyset, shape):
    for n in HC.SIZES:
        for two in (False, True):
            c = HC.case(keyset, shape, n, two)
            got = R.host_summary(*HC.tensors(c))
            assert all(t.dtype == d for t, d in zip(got[:4], (torch.int64, torch.int64, torch.float64, torch.int64)))
            HC.same(got, HC.oracle(*c))
            HC.same(S.host_summary(*HC.tensors(c)), got)      # the dispatcher, on CPU tensors


def test_the_a_side_wins_a_tie_at_the_minimum():
    """Event 3 has both sides on document 1 at the document's lowest score; event 5's a side ties it later."""
    doc_a = torch.tensor([0, 1, 0, 1, 2, 1], dtype=torch.int32)
    doc_b = torch.tensor([1, 0, 2, 1, -1, 0], dtype=torch.int32)
    sa = torch.tensor([5e-3, 4e-3, 1e-3, 1e-6, 2e-3, 1e-6], dtype=torch.float64)
    sb = torch.tensor([3e-3, 6e-3, float("nan"), 1e-6, 1e-9, 7e-3], dtype=torch.float64)
    ev, fl, ms, worst, skipped = R.host_summary(doc_a, sa, doc_b, sb, 4, 1e-4)
    assert ev.tolist() == [4, 5, 2, 0] and fl.tolist() == [0, 3, 0, 0] and skipped == 1
    assert ms.tolist() == [1e-3, 1e-6, 2e-3, float("inf")]
    assert worst.tolist() == [2 * 2, 2 * 3, 2 * 4, -1]      # document 1: side a of event 3, not its side b
    HC.same((ev, fl, ms, worst, skipped), HC.oracle(doc_a.numpy(), sa.numpy(), doc_b.numpy(), sb.numpy(), 4, 1e-4))


def test_cases_hold_what_they_promise():
    c = HC.case("all_equal", "zipf", HC.RAGGED, True)
    hot = c[4] // 2
    assert (c[0] == hot).mean() > 0.45 and (c[0] == c[2]).sum() >= HC.RAGGED // 5
    both = (c[0] == c[2]) & (c[1] == c[3])
    assert both.sum() >= HC.RAGGED // 10
    c = HC.case("nan_mix", "third", 2049, False)
    assert np.isnan(c[1]).sum() > 500 and np.signbit(c[1][np.isnan(c[1])]).any()
    c = HC.case("signed_mix", "unnamed", 2049, False)
    assert set(np.unique(c[0]) % 2) == {0} and c[4] > c[0].max() + 2
    assert HC.order_key(-0.0) + 1 == HC.order_key(0.0) and HC.order_key(-np.inf) < HC.order_key(-1.5)


def test_rank_hosts():
    rng = np.random.default_rng(11)
    D = 3000
    ms = rng.choice(np.array([-0.0, 0.0, 1e-7, 3e-6, np.nextafter(3e-6, 1.0), 2e-4]), D)      # long tie runs
    mix = rng.random(D) < 0.3
    ms[mix] = 10.0 ** rng.uniform(-9, -3, int(mix.sum()))
    fl = rng.integers(0, 3, D)
    want = sorted((d for d in range(D) if fl[d] >= 1), key=lambda d: (HC.order_key(ms[d]), d))
    got = S.rank_hosts(torch.from_numpy(ms), torch.from_numpy(fl))
    assert got.dtype == np.int64 and got.tolist() == want and 0 < len(want) < D
    for limit in (1, 10, len(want) - 1, len(want), len(want) + 5):
        assert S.rank_hosts(torch.from_numpy(ms), torch.from_numpy(fl), limit).tolist() == want[:limit], limit
    assert S.rank_hosts(torch.from_numpy(ms), torch.zeros(D, dtype=torch.int64)).size == 0


def test_twin_validation():
    da, sa, db, sb, D, tol = HC.tensors(HC.case("log_uniform", "third", 65, True))
    HC.same(R.host_summary(da, sa, db, sb, D, tol, max_blocks=3), R.host_summary(da, sa, db, sb, D, tol))
    with pytest.raises(ValueError):
        R.host_summary(da.to(torch.int64), sa, db, sb, D, tol)
    with pytest.raises(ValueError):
        R.host_summary(da, sa.to(torch.float32), db, sb, D, tol)
    with pytest.raises(ValueError):
        R.host_summary(da, sa[:-1], db, sb, D, tol)
    with pytest.raises(ValueError):
        R.host_summary(da, sa, db[:-1], sb[:-1], D, tol)
    with pytest.raises(ValueError, match="go together"):
        R.host_summary(da, sa, None, sb, D, tol)
    with pytest.raises(ValueError, match="go together"):
        R.host_summary(da, sa, db, None, D, tol)
    with pytest.raises(ValueError, match="out of range"):
        R.host_summary(da, sa, db, sb, int(da.max()), tol)
    bad = da.clone()
    bad[7] = -2
    with pytest.raises(ValueError, match="out of range"):
        R.host_summary(bad, sa, db, sb, D, tol)
    with pytest.raises(ValueError):
        R.host_summary(da, sa, db, sb, -1, tol)
    with pytest.raises(ValueError):
        R.host_summary(da, sa, db, sb, D, tol, max_blocks=1.5)
    with pytest.raises(TypeError):
        R.host_summary(da, sa, db, sb, 2.5, tol)
    # no events, or no documents: the initial result
    e = torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64)
    ev, fl, ms, worst, skipped = R.host_summary(e[0], e[1], None, None, 3, tol)
    assert ev.tolist() == [0] * 3 and fl.tolist() == [0] * 3 and ms.tolist() == [np.inf] * 3 and worst.tolist() == [-1] * 3
    assert skipped == 0
    out = R.host_summary(torch.full((4,), -1, dtype=torch.int32), sa[:4], None, None, 0, tol)
    assert all(t.numel() == 0 for t in out[:4]) and out[4] == 4


# ---------------------------------------------------------------------------------------- end to end
TOL = dict(flow=1e-3, dns=1e-2, proxy=1e-3)


class Day:
    """One synthetic day of a type and its runs, each in a directory of its own (run once, shared)."""

    def __init__(self, kind, root, backend="cpu", device="cpu", scale=1):
        self.kind, self.root, self.backend, self.device, self.runs = kind, root, backend, device, {}
        if kind == "flow":
            from oni_ml_amd.synth.flow import generate_flow_day
            generate_flow_day(str(root / "in") + "/", events=5000 * scale, seed=3, n_internal=300, n_external=700, files=3)
            self.gen, self.paths = str(root / "in"), dict(flow_path=str(root / "in"))
        elif kind == "dns":
            from oni_ml_amd.synth.dns import generate_dns_day
            g = generate_dns_day(str(root / "in"), events=6000 * scale, seed=4, files=4, n_names=700, n_clients=250)
            self.gen, self.paths = g, dict(dns_path=g["dns_path"], top1m=g["top1m"])
        else:
            from oni_ml_amd.synth.proxy import generate_proxy_day
            g = generate_proxy_day(str(root / "in"), events=3000 * scale, seed=5, files=2)
            self.gen, self.paths = g, dict(proxy_path=g["proxy_path"], top1m=g["top1m"])
        self.counts = HC.input_counts(kind, self.gen)

    def cfg(self, lpath, **kw):
        cfg = CFG.resolve("20160122", self.kind, tol=TOL[self.kind], conf_path=None, environ={}, lpath=str(lpath),
                          backend=self.backend, threads=2, verbose=False, compat="fixed", **self.paths, **kw)
        cfg.settings = LDASettings(em_max_iter=4)
        return cfg

    def go(self, cfg):
        from oni_ml_amd.pipeline import run
        return run(cfg.validate(), device=self.device, log=lambda *a, **k: None)

    def run(self, host_report, max_results=-1):
        """(work directory, summary) of the run with these two options."""
        key = (host_report, max_results)
        if key not in self.runs:
            lp = self.root / f"h{host_report}_m{max_results}"
            self.runs[key] = (lp, self.go(self.cfg(lp, host_report=host_report, max_results=max_results)))
        return self.runs[key]

    def hosts(self, lp):
        return (lp / f"{self.kind}_hosts.csv").read_bytes()

    def results(self, lp):
        return (lp / f"{self.kind}_results.csv").read_bytes()


@pytest.fixture(scope="module", params=["flow", "dns", "proxy"])
def day(request, tmp_path_factory):
    return Day(request.param, tmp_path_factory.mktemp("hosts_" + request.param))


def test_hosts_file_is_a_recount_of_the_results_file(day):
    lp, summary = day.run(-1)
    lines = HC.check_hosts_file(day.kind, str(lp), TOL[day.kind], day.counts)
    assert len(lines) >= 20 and summary["hosts"] == len(lines) and summary["host_sides_skipped"] == 0
    import json
    done = json.loads((lp / ".stages" / f"{day.kind}_post.done").read_text())
    assert done["hosts"] == len(lines) and done["host_sides_skipped"] == 0
    if day.kind == "flow":      # both sides show up as the worst one
        assert {ln.split(",")[4] for ln in lines} == {"src", "dst"}


def test_max_results_does_not_change_the_hosts_file(day):
    full, _ = day.run(-1)
    lim, s = day.run(-1, 50)
    assert s["scored"] == 50 and len(day.results(lim).splitlines()) == 50
    assert day.hosts(lim) == day.hosts(full)


def test_a_limit_writes_the_head(day):
    full, _ = day.run(-1)
    top, s = day.run(10)
    assert s["hosts"] == 10
    assert day.hosts(top) == b"".join(day.hosts(full).splitlines(keepends=True)[:10])
    assert day.results(top) == day.results(full)
    HC.check_hosts_file(day.kind, str(top), TOL[day.kind], day.counts, limit=10)


def test_resume_rewrites_the_same_hosts_file(day):
    full, _ = day.run(-1)
    raw, res = day.hosts(full), day.results(full)
    os.unlink(full / f"{day.kind}_hosts.csv")
    os.unlink(full / f"{day.kind}_results.csv")
    os.unlink(full / ".stages" / f"{day.kind}_post.done")
    day.go(day.cfg(full, host_report=-1, resume=True))
    assert day.hosts(full) == raw and day.results(full) == res
    assert "skipped" in (full / "metrics.jsonl").read_text()


def test_option_off_changes_nothing(day):
    full, _ = day.run(-1)
    off, s = day.run(0)
    assert not (off / f"{day.kind}_hosts.csv").exists() and "hosts" not in s and "host_sides_skipped" not in s
    assert day.results(off) == day.results(full)
    import json
    assert "hosts" not in json.loads((off / ".stages" / f"{day.kind}_post.done").read_text())


def test_refusals_make_nothing(day):
    class Group:
        active, rank, world_size = True, 0, 2
    from oni_ml_amd.pipeline import run
    never = day.root / "never"
    assert CFG.RunConfig().host_report == 0
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="host-report" if day.kind != "proxy" else "one process"):
            day.cfg(never, host_report=-1, **kw).validate()
        with pytest.raises(ValueError, match="host-report" if day.kind != "proxy" else "one process"):
            run(day.cfg(never, host_report=5, **kw), device="cpu")
    for bad in (-2, -100):
        with pytest.raises(ValueError, match="host-report"):
            day.cfg(never, host_report=bad).validate()
        with pytest.raises(ValueError, match="host-report"):
            run(day.cfg(never, host_report=bad), device="cpu")
    with pytest.raises(ValueError, match="host-report" if day.kind != "proxy" else "one process"):
        run(day.cfg(never, host_report=-1), dist=Group(), device="cpu")
    assert not never.exists()
    for ok in (0, -1, 1, 250):
        assert day.cfg(never, host_report=ok).validate().host_report == ok


def test_cli_flag_reaches_the_config(monkeypatch, tmp_path):
    seen = {}

    def body(a, resolve):
        seen["cfg"] = resolve(1)
        return 0

    monkeypatch.setattr(cli, "_ml_ops_body", body)
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["20160122", "flow", "1e-3", "--conf", str(tmp_path / "none.conf"), "--lpath", "/w", "--flow-path", "/a"]
    assert cli.cmd_ml_ops(base) == 0 and seen["cfg"].host_report == 0
    assert cli.cmd_ml_ops(base + ["--host-report", "25"]) == 0 and seen["cfg"].host_report == 25
    assert cli.cmd_ml_ops(base + ["--host-report", "-1"]) == 0 and seen["cfg"].host_report == -1
    seen.clear()
    for extra in (["--gpus", "2"], ["--hdfs"]):
        with pytest.raises(ValueError, match="host-report"):
            cli.cmd_ml_ops(base + ["--host-report", "5"] + extra)
    assert not seen
