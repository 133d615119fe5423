"""Proxy suspicious-connects on the CPU: the entropy twin against the textbook sum, the word strings against a
literal transcription of the word table, the row rules, the file contract of a small day end to end, the CLI."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oni_ml_amd import config as CFG
from oni_ml_amd.features import proxy as FP
from oni_ml_amd.features import proxy_io as PIO
from oni_ml_amd.models.lda.settings import LDASettings
from oni_ml_amd.ops.reference import entropy_table, string_entropy
from oni_ml_amd.synth import proxy as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3


def _batch(strings):
    data = b"".join(strings)
    off = np.zeros(len(strings) + 1, np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return np.frombuffer(data, np.uint8) if data else np.zeros(0, np.uint8), off


def _textbook(s: bytes) -> float:
    """-sum p log2 p with math.fsum."""
    n = len(s)
    if n <= 1:
        return 0.0
    c = np.bincount(np.frombuffer(s, np.uint8), minlength=256)
    return -math.fsum((int(k) / n) * math.log2(int(k) / n) for k in c if k)


def test_entropy_twin_known_values_are_exact():
    known = [(b"", 0.0), (b"a", 0.0), (b"aaaa", 0.0), (b"ab", 1.0), (b"aabc", 1.5), (b"abcd", 2.0),
             (b"abcdefgh", 3.0), (bytes(range(256)), 8.0)]
    got = string_entropy(*_batch([s for s, _ in known]))
    assert got.dtype == np.float64 and got.tolist() == [h for _, h in known]
    assert string_entropy(np.zeros(0, np.uint8), np.zeros(1, np.int64)).shape == (0,)
    t = entropy_table(8)
    assert t[:3].tolist() == [0.0, 0.0, 2.0] and t[8] == 24.0 and entropy_table(0).size == 2


def test_entropy_twin_matches_the_textbook_sum():
    """|twin - textbook| <= 1e-12: both are sums of at most 257 terms of magnitude <= log2 n with a
    relative error of a few 2^-53 each, so the difference is bounded by about (terms + 2) 2^-53 log2 n
    (n = 100,000: 259 x 1.1e-16 x 17 = 5e-13)."""
    rng = np.random.default_rng(11)
    strings = []
    for i in range(400):
        n = int(rng.integers(0, 400)) if i % 8 else int(rng.integers(400, 100_001))
        k = int(rng.choice([1, 2, 16, 95, 256]))
        alphabet = rng.choice(256, size=k, replace=False).astype(np.uint8)
        p = rng.dirichlet(np.full(k, 0.5))
        strings.append(alphabet[rng.choice(k, size=n, p=p)].tobytes())
    got = string_entropy(*_batch(strings))
    want = np.array([_textbook(s) for s in strings])
    err = np.abs(got - want)
    print("twin vs textbook: max abs error", err.max())
    assert err.max() <= 1e-12
    assert (got >= 0).all() and (got <= 8.0).all()


def test_entropy_twin_chunks_do_not_change_bits(monkeypatch):
    from oni_ml_amd.ops import reference as R
    rng = np.random.default_rng(3)
    strings = [rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 300, size=500)]
    data, off = _batch(strings)
    whole = string_entropy(data, off)
    monkeypatch.setattr(R, "ENTROPY_CHUNK_ROWS", 7)
    monkeypatch.setattr(R, "ENTROPY_CHUNK_BYTES", 256)
    assert np.array_equal(R.string_entropy(data, off), whole)
    with pytest.raises(ValueError):
        string_entropy(data, off[::-1].copy())
    with pytest.raises(ValueError):
        string_entropy(data[:-1], off)


# ------------------------------------------------------------------ words ---
def _word_py(row, top_set, agent_count, agent_cuts):
    """The word of one kept row, written out from the word table (hosts of the synthetic day are
    ``[sub.]domain.tld`` names with one-label TLDs: the domain is the label before the last)."""
    host = row["host"].split(":")[0]
    labels = host.split(".")
    domain = labels[-2] if len(labels) >= 2 else labels[0]
    top = 2 if domain == "intel" else (1 if domain in top_set else 0)
    hour = int(row["p_time"].split(":")[0])
    method = row["reqmethod"] if row["reqmethod"] != "" else "unknown_method"
    h = _textbook(row["fulluri"].encode("utf-8"))
    ecuts = [0.0, 0.3, 0.6, 0.9, 1.2, 1.5, 1.8, 2.1, 2.4, 2.7, 3.0, 3.3, 3.6, 3.9, 4.2, 4.5, 4.8, 5.1, 5.4, 20.0]
    assert all(abs(h - c) > 1e-9 for c in ecuts[1:]), "a test URI sits on an entropy cut"
    ebin = sum(1 for c in ecuts if h > c)
    ctype = row["resconttype"].split("/")[0] if row["resconttype"] != "" else "unknown_content_type"
    abin = sum(1 for c in agent_cuts if agent_count[row["useragent"]] > c)
    resp = row["respcode"][0] if row["respcode"] != "" else "unknown_response_code"
    return f"{top}_{hour}_{method}_{ebin}_{ctype}_{abin}_{resp}"


@pytest.fixture(scope="module")
def day(tmp_path_factory):
    d = tmp_path_factory.mktemp("proxy_day")
    g = SP.generate_proxy_day(str(d / "in"), events=3000, seed=5, files=2)
    return d, g


def test_row_rules_and_drop_reasons(day):
    _, g = day
    assert g["edge_rows"] == SP.EDGE_ROWS
    tab = PIO.load_proxy(g["proxy_path"])
    assert tab.n_input == 3000 and tab.dropped == 8 and tab.n == 2992
    assert tab.drop_reasons == dict(null=5, time=2, control=1) == g["edge_dropped"]
    cols = tab.cols
    assert list(cols) == PIO.COLUMNS and len(PIO.COLUMNS) == 19
    assert all(isinstance(v, str) for c in PIO.COLUMNS for v in cols[c][:40])
    assert not any(ch in v for c in PIO.COLUMNS for v in cols[c] for ch in "\t\r\n")
    # the 14 rows with a null in an optional column are kept and print it empty (rows 0 .. 18, less the 5)
    kept_null = [c for c in PIO.COLUMNS if c not in PIO.REQUIRED]
    for i, c in enumerate(kept_null):
        assert cols[c][i] == "", c
    # integers in decimal
    assert cols["respcode"][20].isdigit() and cols["scbytes"][20].isdigit()
    assert PIO.hour_of("07:01:02") == 7 and PIO.hour_of("7:1") == 7 and PIO.hour_of("23:") == 23
    assert [PIO.hour_of(x) for x in ("24:00:00", "noon", ":10", "", "-1:00", "1 :00")] == [-1] * 6


def test_words_match_the_written_out_table(day):
    _, g = day
    tab = PIO.load_proxy(g["proxy_path"])
    top = FP.load_top_domains(g["top1m"])
    feat = FP.featurize(tab, "cpu", top)
    words = FP.ProxyWordSpace(feat).decode(feat.word_key.numpy())
    cols = tab.cols
    rows = [{c: cols[c][i] for c in PIO.COLUMNS} for i in range(tab.n)]
    agent_count = {}
    for r in rows:
        agent_count[r["useragent"]] = agent_count.get(r["useragent"], 0) + 1
    from oni_ml_amd.features.quantiles import QUINTILES, ecdf_cuts_reference
    acuts = ecdf_cuts_reference([agent_count[r["useragent"]] for r in rows], QUINTILES)
    assert np.array_equal(feat.cuts["agent"], acuts) and len(acuts) == 5
    want = [_word_py(r, set(top), agent_count, acuts) for r in rows]
    assert words == want
    # the edge rows took part: an empty method / content type / response code, the :443 host, the empty agent
    assert any(w.split("_")[2:4] == ["unknown", "method"] for w in words)
    assert any("unknown_content_type" in w for w in words) and any(w.endswith("unknown_response_code") for w in words)
    i443 = cols["host"].index("login.google.com:443")
    assert words[i443].startswith("1_") and "_CONNECT_" in words[i443]
    assert "" in agent_count
    # entropy of the edge URIs: empty -> 0 (bin 0), 5,000 bytes, UTF-8 and low bytes counted as unsigned bytes
    ent = dict(zip(cols["fulluri"], feat.host["entropy"].tolist()))
    assert ent[""] == 0.0
    for u in cols["fulluri"][:30]:
        assert abs(ent[u] - _textbook(u.encode("utf-8"))) <= 1e-12
    assert max(len(u.encode()) for u in cols["fulluri"]) == 5000
    assert feat.ip_names == list(dict.fromkeys(cols["clientip"]))
    # the persisted cuts reproduce the keys
    again = FP.featurize(tab, "cpu", top, cuts={"agent": feat.cuts["agent"].tolist()})
    assert np.array_equal(again.word_key.numpy(), feat.word_key.numpy())
    reused = FP.featurize(tab, "cpu", top, cuts={"agent": feat.cuts["agent"].tolist()}, host=feat.host)
    assert np.array_equal(reused.word_key.numpy(), feat.word_key.numpy()) and reused.ip_names == feat.ip_names
    assert np.array_equal(reused.ip.numpy(), feat.ip.numpy())
    # a dictionary column full of garbage cannot wrap the int64 key
    FP.check_radices(10, 10, 10, 6)
    with pytest.raises(ValueError, match="int64"):
        FP.check_radices(1 << 20, 1 << 20, 1 << 12, 6)


def test_synthetic_day_plants_what_it_says(day):
    _, g = day
    import pyarrow.parquet as pq
    import pyarrow as pa
    t = pa.concat_tables([pq.read_table(p) for p in g["paths"]]).to_pydict()
    assert t["respcode"][100] is not None and isinstance(t["respcode"][100], int)
    assert len(g["planted"]) == 6 and (g["planted"] >= SP.EDGE_ROWS).all()
    top = set(FP.load_top_domains(g["top1m"]))
    agents = {}
    for a in t["useragent"]:
        agents[a] = agents.get(a, 0) + 1
    for i, kind in zip(g["planted"].tolist(), g["planted_kinds"]):
        if kind == "long_query":
            assert 400 <= len(t["uriquery"][i]) <= 2000 and t["fulluri"][i].endswith(t["uriquery"][i])
        elif kind == "rare_agent":
            assert agents[t["useragent"][i]] == 1
        elif kind == "off_list_host":
            assert t["host"][i].split(".")[-2] not in top
        else:
            others = {int(t["p_time"][j].split(":")[0]) for j in range(SP.EDGE_ROWS, 3000)
                      if j != i and t["clientip"][j] == t["clientip"][i]}
            assert others and int(t["p_time"][i].split(":")[0]) not in others
    lens = [len(u) for u in t["fulluri"][SP.EDGE_ROWS:] if u is not None]
    normal = [n for j, n in enumerate(lens) if j + SP.EDGE_ROWS not in set(g["planted"].tolist())]
    assert min(normal) >= 20 and max(normal) <= 300
    assert any("," in a for a in agents if a)
    g2 = SP.generate_proxy_day(str(day[0] / "again"), events=3000, seed=5, files=2)
    assert np.array_equal(g2["planted"], g["planted"])
    t2 = pa.concat_tables([pq.read_table(p) for p in g2["paths"]])
    assert t2.equals(pa.concat_tables([pq.read_table(p) for p in g["paths"]]))


# ------------------------------------------------------------- end to end ---
def _cfg(g, lpath, max_results=-1, **kw):
    cfg = CFG.resolve("20160122", "proxy", tol=TOL, conf_path=None, environ={}, lpath=str(lpath),
                      proxy_path=g["proxy_path"], top1m=g["top1m"], backend="cpu", threads=2, verbose=False,
                      max_results=max_results, **kw)
    cfg.settings = LDASettings(em_max_iter=5)
    return cfg.validate()


def _run(cfg):
    from oni_ml_amd.pipeline import run
    return run(cfg, device="cpu", log=lambda *a, **k: None)


@pytest.fixture(scope="module")
def full_run(day):
    d, g = day
    summary = _run(_cfg(g, d / "full"))
    return d / "full", summary


def test_results_file_contract(day, full_run):
    lp, summary = full_run
    assert {"input", "corpus", "lda", "scored", "below_tol"} <= set(summary)
    assert summary["input"] == dict(rows=2992, dropped=8)
    raw = (lp / "proxy_results.csv").read_bytes()
    lines = raw.split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 == summary["scored"] == summary["below_tol"] > 50
    scores = []
    for ln in lines[:-1]:
        f = ln.decode("utf-8").split("\t")
        assert len(f) == 21
        scores.append(float(f[20]))
        assert len(f[19].split("_")) >= 7
    assert scores == sorted(scores) and scores[-1] < TOL
    assert json.load(open(lp / "proxy_cuts.json"))["cuts"]["agent"]
    # words longer than 20 bytes are written whole
    words = [ln.split(",", 1)[1] for ln in (lp / "words.dat").read_text().splitlines()]
    assert max(len(w) for w in words) > 20
    # compat is ignored: "strict" (the default) and "fixed" give the same bytes
    d, g = day
    _run(_cfg(g, d / "fixed", compat="fixed"))
    assert (d / "fixed" / "proxy_results.csv").read_bytes() == raw


def test_same_seed_same_bytes_and_max_results_head(day, full_run):
    d, g = day
    lp, summary = full_run
    raw = (lp / "proxy_results.csv").read_bytes()
    g2 = SP.generate_proxy_day(str(d / "in2"), events=3000, seed=5, files=2)
    _run(_cfg(g2, d / "same"))
    assert (d / "same" / "proxy_results.csv").read_bytes() == raw
    lim = _run(_cfg(g, d / "lim", max_results=50))
    assert lim["scored"] == 50 and lim["below_tol"] == summary["scored"]
    assert (d / "lim" / "proxy_results.csv").read_bytes() == b"".join(raw.splitlines(keepends=True)[:50])


def test_resume_rewrites_the_same_results(day, full_run):
    d, g = day
    lp, _ = full_run
    raw = (lp / "proxy_results.csv").read_bytes()
    os.unlink(lp / "proxy_results.csv")
    os.unlink(lp / ".stages" / "proxy_post.done")
    _run(_cfg(g, lp, resume=True))
    assert (lp / "proxy_results.csv").read_bytes() == raw
    assert "skipped" in (lp / "metrics.jsonl").read_text()


def test_scores_are_theta_dot_phi_of_the_written_tables(full_run):
    from oni_ml_amd.pipeline.common import load_model_tables
    lp, _ = full_run
    mt = load_model_tables(str(lp))
    assert mt.K == 20
    di, wi = mt.doc_index(), mt.word_index()
    lines = (lp / "proxy_results.csv").read_text(encoding="utf-8").split("\n")[:200]
    assert len(lines) == 200
    for ln in lines:
        f = ln.split("\t")
        want = float(np.dot(mt.theta[di[f[2]]], mt.phi[wi[f[19]]]))
        assert abs(float(f[20]) - want) <= 1e-9 * abs(want), (f[2], f[19])


def test_config_and_one_process_rule(day):
    d, g = day
    c = CFG.resolve("20160122", "proxy", conf_path=None, environ={"PROXY_PATH": "/p/a,/p/b", "LPATH": "/tmp/x"})
    assert c.proxy_path == "/p/a,/p/b" and "PROXY_PATH" in CFG.ENV_KEYS
    conf = d / "duxbay.conf"
    conf.write_text('PROXY_PATH=/hive/proxy/y=${YR}\nLPATH=/tmp/y\n')
    assert CFG.resolve("20160122", "proxy", conf_path=str(conf), environ={}).proxy_path == "/hive/proxy/y=2016"
    with pytest.raises(ValueError, match="PROXY_PATH"):
        CFG.resolve("20160122", "proxy", conf_path=None, environ={}, lpath="/tmp/x").validate()
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="one process"):
            _cfg(g, d / "never", **kw)

    class Group:
        active, rank, world_size = True, 0, 2
    from oni_ml_amd.pipeline import run
    with pytest.raises(ValueError, match="one process"):
        run(_cfg(g, d / "never"), dist=Group(), device="cpu")
    assert not (d / "never").exists()
    # the input prefetch has nothing to start for proxy, and says nothing
    from oni_ml_amd.pipeline import prefetch
    prefetch.start_for(_cfg(g, d / "never"), fork=False)
    assert prefetch.take(("proxy",)) is None


def test_cli_runs_a_proxy_day_and_refuses_two_gpus(day, tmp_path):
    _, g = day
    st = tmp_path / "settings.txt"
    st.write_text(LDASettings(em_max_iter=2).dumps())
    env = dict(os.environ, ONI_CONF=str(tmp_path / "none.conf"))
    cmd = [sys.executable, "-m", "oni_ml_amd", "ml_ops", "20160122", "proxy", "1e-3", "--proxy-path", g["proxy_path"],
           "--top1m", g["top1m"], "--backend", "cpu", "--settings", str(st), "--threads", "2", "--quiet"]
    r = subprocess.run(cmd + ["--lpath", str(tmp_path / "ml")], cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    summ = json.load(open(tmp_path / "ml" / "run_summary.json"))
    assert summ["scored"] > 0 and (tmp_path / "ml" / "proxy_results.csv").exists()
    r = subprocess.run(cmd + ["--lpath", str(tmp_path / "ml2"), "--gpus", "2"], cwd=ROOT, capture_output=True,
                       text=True, env=env)
    assert r.returncode != 0 and "proxy runs on one process" in r.stderr
    assert not (tmp_path / "ml2" / "proxy_results.csv").exists()
