"""MAXRESULTS end to end on the CPU path: configuration layering and the command line, the one-process flow and
DNS pipelines (the limited results file is the head of the unlimited one, every other file unchanged), 2 and 3
gloo ranks against one process, and ``shardio.merge_sorted_rows(limit=...)`` on a hand-made input."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dist import _free_port  # noqa: E402
from test_sharded_pipeline import DNS_FILES, FLOW_FILES, _cfg, _dns_feedback  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402


# ------------------------------------------------------------------------- configuration, command line
def test_max_results_layering(tmp_path):
    conf = tmp_path / "duxbay.conf"
    conf.write_text("LPATH=/w\nFLOW_PATH=/a\nTOL=1e-5\nMAXRESULTS=500\n")
    r = lambda **kw: CFG.resolve("20160122", "flow", conf_path=str(conf), **kw)      # noqa: E731
    assert "MAXRESULTS" in CFG.ENV_KEYS
    assert CFG.RunConfig().max_results == -1
    assert CFG.resolve("20160122", "flow", conf_path=None, environ={}).max_results == -1
    assert r(environ={}).max_results == 500
    assert r(environ={"MAXRESULTS": "400"}).max_results == 400
    assert r(environ={"MAXRESULTS": "400"}, max_results=300).max_results == 300
    assert r(environ={"MAXRESULTS": ""}).max_results == 500
    for ok in (-1, 1, 250):
        assert r(environ={}, max_results=ok).validate().max_results == ok
    for bad in (0, -2):
        with pytest.raises(ValueError, match="MAXRESULTS"):
            r(environ={}, max_results=bad).validate()


def _parsed(monkeypatch, argv, conf, environ):
    """The RunConfig that ``ml_ops <argv>`` resolves (the run itself is not started)."""
    seen = {}

    def body(a, resolve):
        seen["cfg"] = resolve(1)
        return 0

    monkeypatch.setattr(cli, "_ml_ops_body", body)
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("MAXRESULTS", raising=False)
    for k, v in environ.items():
        monkeypatch.setenv(k, v)
    assert cli.cmd_ml_ops(argv + ["--conf", str(conf)]) == 0
    return seen["cfg"]


def test_cli_positional_and_flag(monkeypatch, tmp_path):
    conf = tmp_path / "duxbay.conf"
    conf.write_text("LPATH=/w\nFLOW_PATH=/a\nMAXRESULTS=500\n")
    base = ["20160122", "flow", "1e-3"]
    env = {"MAXRESULTS": "400"}
    assert _parsed(monkeypatch, base, conf, {}).max_results == 500                       # the conf file
    assert _parsed(monkeypatch, base, conf, env).max_results == 400                      # the environment
    c = _parsed(monkeypatch, base + ["300"], conf, env)                                  # the positional
    assert c.max_results == 300 and c.tol == 1e-3
    assert _parsed(monkeypatch, base + ["300", "--max-results", "200"], conf, env).max_results == 200
    assert _parsed(monkeypatch, base + ["-1"], conf, env).max_results == -1
    none = tmp_path / "none.conf"
    c = _parsed(monkeypatch, ["20160122", "flow", "1e-3", "250"], none, {})
    assert c.max_results == 250 and c.tol == 1e-3 and c.fdate == "20160122" and c.dsource == "flow"
    assert _parsed(monkeypatch, ["20160122", "flow"], none, {}).max_results == -1
    assert "./ml_ops.sh YYYYMMDD TYPE [TOL] [MAXRESULTS]" in cli.SYNTAX
    assert cli.SYNTAX.splitlines()[0] == "ml_ops.sh syntax error"


# ----------------------------------------------------------------------------------------- pipelines
def _worker(rank, world, port, kind, indir, lpath, extra, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), ONI_DIST_DETERMINISTIC="chain")
    torch.set_num_threads(1)
    try:
        from oni_ml_amd.parallel import dist as D
        from oni_ml_amd.pipeline import run
        ctx = D.init_from_env(backend="gloo")
        cfg = _cfg(kind, indir, lpath, extra)
        cfg.max_results = extra.get("max_results", -1)
        lines = []
        s = run(cfg.validate(), dist=ctx if world > 1 else None, device="cpu",
                log=lambda *a, **k: lines.append(" ".join(map(str, a))))
        q.put((rank, dict(scored=s.get("scored"), below_tol=s.get("below_tol"),
                          log=[x for x in lines if "_post:" in x])))
        ctx.shutdown()
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def _run(world, kind, indir, lpath, extra):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, kind, indir, lpath, extra, q)) for r in range(world)]
    for p in ps:
        p.start()
    out = sorted([q.get(timeout=600) for _ in ps], key=lambda x: x[0])
    for p in ps:
        p.join(timeout=60)
    for r, o in out:
        assert not isinstance(o, str), o
    return [o for _, o in out]


class _Day:
    """One synthetic day and its runs, each in a directory of its own (run once, shared by the tests)."""

    def __init__(self, kind, root):
        self.kind, self.root, self.runs = kind, root, {}
        if kind == "flow":
            from oni_ml_amd.synth.flow import generate_flow_day, generate_flow_feedback
            generate_flow_day(str(root / "in") + "/", events=5000, seed=3, n_internal=300, n_external=700, files=3)
            rows = (root / "in" / "part-00000.csv").read_text().splitlines()[1:300]
            generate_flow_feedback(str(root / "fb.csv"), rows, seed=2, n=12)
            self.indir, self.extra, self.files = str(root / "in"), dict(tol=1e-3, compat="fixed"), FLOW_FILES
        else:
            from oni_ml_amd.synth.dns import generate_dns_day
            g = generate_dns_day(str(root / "in"), events=6000, seed=4, files=4, n_names=700, n_clients=250)
            self.indir, self.files = None, DNS_FILES
            self.extra = dict(tol=1e-2, compat="fixed", dns_path=g["dns_path"], top1m=g["top1m"])
        self.results = f"{kind}_results.csv"

    def run(self, world, max_results):
        """(work directory, per-rank summaries) of the run with that many ranks and that limit."""
        if (world, max_results) not in self.runs:
            lp = self.root / f"w{world}_m{max_results}"
            lp.mkdir()
            if self.kind == "flow":
                os.link(self.root / "fb.csv", lp / "flow_scores.csv")
            else:
                _dns_feedback(str(lp / "dns_scores.csv"), self.extra["dns_path"])
            out = _run(world, self.kind, self.indir, str(lp), dict(self.extra, max_results=max_results))
            self.runs[world, max_results] = (lp, out)
        return self.runs[world, max_results]

    def flagged(self):
        lp, out = self.run(1, -1)
        F = out[0]["scored"]
        assert F >= 3 and len((lp / self.results).read_bytes().splitlines()) == F
        return F


@pytest.fixture(scope="module", params=["flow", "dns"])
def day(request, tmp_path_factory):
    return _Day(request.param, tmp_path_factory.mktemp("maxres_" + request.param))


def test_limited_results_are_the_head_of_the_unlimited_file(day):
    F = day.flagged()
    N = F // 3
    full_dir, full = day.run(1, -1)
    lim_dir, lim = day.run(1, N)
    assert full[0]["below_tol"] == F
    assert lim[0]["scored"] == N and lim[0]["below_tol"] == F
    full_lines = (full_dir / day.results).read_bytes().splitlines(keepends=True)
    assert (lim_dir / day.results).read_bytes() == b"".join(full_lines[:N])
    for f in day.files:
        if f != day.results:
            assert (full_dir / f).read_bytes() == (lim_dir / f).read_bytes(), f
    done = json.loads((lim_dir / ".stages" / f"{day.kind}_post.done").read_text())
    assert done["flagged"] == N and done["below_tol"] == F
    # the log line names both counts when a limit is set, and is the old one without
    assert any(f"{N} of the {F} " in x and f"MAXRESULTS {N}" in x for x in lim[0]["log"]), lim[0]["log"]
    assert any(f"_post: {F} " in x and "MAXRESULTS" not in x for x in full[0]["log"]), full[0]["log"]


def test_a_limit_past_the_flagged_count_changes_nothing(day):
    F = day.flagged()
    full_dir, _ = day.run(1, -1)
    big_dir, big = day.run(1, F + 7)
    assert big[0]["scored"] == F and big[0]["below_tol"] == F
    for f in day.files:
        assert (full_dir / f).read_bytes() == (big_dir / f).read_bytes(), f


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_limit_equals_one_process(day, world):
    F = day.flagged()
    N = F // 3
    one_dir, _ = day.run(1, N)
    lp, out = day.run(world, N)
    assert all(o["scored"] == N and o["below_tol"] == F for o in out), out
    assert (lp / day.results).read_bytes() == (one_dir / day.results).read_bytes()
    assert not [p for p in os.listdir(lp) if ".part" in p]


# --------------------------------------------------------------------------------- merge_sorted_rows
# rank -> (ascending keys, one text line per row); 0.25 and 0.5 tie across the ranks, 0.5 also within rank 1
_MERGE = {0: ([0.125, 0.25, 0.5, 2.0], ["a0", "a1", "a2", "a3"]),
          1: ([0.25, 0.5, 0.5, 0.75, 4.0], ["b0", "b1", "b2", "b3", "b4"]),
          2: ([], [])}
# one stable sort over the rows in rank order, then local order
_MERGED = ["a0", "a1", "b0", "a2", "b1", "b2", "b3", "a3", "b4"]


def _merge_worker(rank, world, port, lpath, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    try:
        from oni_ml_amd.parallel import dist as D
        from oni_ml_amd.parallel import shardio as S
        ctx = D.init_from_env(backend="gloo")
        keys, rows = _MERGE[rank]
        text = np.frombuffer("".join(r + "\n" for r in rows).encode(), np.uint8)
        ends = np.cumsum([len(r) + 1 for r in rows]).astype(np.int64)
        got = {}
        for name, kw in (("default", {}), ("none", dict(limit=None)), ("4", dict(limit=4)), ("5", dict(limit=5)),
                         ("1", dict(limit=1)), ("9", dict(limit=9)), ("50", dict(limit=50))):
            got[name] = S.merge_sorted_rows(ctx, np.asarray(keys, np.float64), text, ends,
                                            os.path.join(lpath, name + ".csv"), **kw)
        q.put((rank, got))
        ctx.shutdown()
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, traceback.format_exc()))


def test_merge_sorted_rows_limit(tmp_path):
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_merge_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in ps:
        p.start()
    out = dict(q.get(timeout=300) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    for r in range(world):
        assert isinstance(out[r], dict), out[r]
    text = lambda rows: "".join(x + "\n" for x in rows)      # noqa: E731
    for name, k in (("default", 9), ("none", 9), ("4", 4), ("5", 5), ("1", 1), ("9", 9), ("50", 9)):
        assert all(out[r][name] == k for r in range(world)), (name, out)
        assert (tmp_path / (name + ".csv")).read_text() == text(_MERGED[:k]), name


def test_merge_sorted_rows_limit_one_process(tmp_path):
    from oni_ml_amd.parallel import shardio as S
    keys, rows = _MERGE[1]
    text = np.frombuffer("".join(r + "\n" for r in rows).encode(), np.uint8)
    ends = np.cumsum([len(r) + 1 for r in rows]).astype(np.int64)
    for limit, k in ((None, 5), (2, 2), (5, 5), (8, 5)):
        p = str(tmp_path / f"{limit}.csv")
        assert S.merge_sorted_rows(None, np.asarray(keys), text, ends, p, limit=limit) == k
        assert open(p).read() == "".join(r + "\n" for r in rows[:k])
