"""--explain on the CPU path: the torch twins ``ops.reference.group_rows_sum`` / ``explain_sides`` (the block order
of the sums, ties, NaN), the word spaces' field tables, and the three pipelines end to end on the torch LDA backend
-- nothing else changes, the explain file follows the results file line for line, its conditionals are the twin
over the written tables bit for bit and agree with an oracle built from the written files alone (a Python dict
for the groups, ``math.fsum`` for the sums); MAXRESULTS, the ensemble, the host report, resume and the refusals."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import SIDES, TOL, Day, bits_equal, tree  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.export import lda_post  # noqa: E402
from oni_ml_amd.io import ldac  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402

f64 = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
i32 = lambda x: torch.tensor(x, dtype=torch.int32)        # noqa: E731
i64 = lambda x: torch.tensor(x, dtype=torch.int64)        # noqa: E731


# ------------------------------------------------------------------------------------------ the twins
def test_group_sum_follows_the_block_rule():
    g = torch.Generator().manual_seed(3)
    n = 600
    t = torch.rand(n, 2, dtype=torch.float64, generator=g) * 10.0 ** torch.randint(-8, 1, (n, 1), generator=g).double()
    order = torch.randperm(n, generator=g).to(torch.int32)
    got = R.group_rows_sum(t, order, i64([0]), i64([n]))
    assert CFG.GROUP_BLOCK == 256
    for c in range(2):
        total = 0.0
        for b0 in range(0, n, 256):
            blk = 0.0
            for m in range(b0, min(b0 + 256, n)):
                blk = blk + t[order[m], c].item()
            total = total + blk
        assert got[0, c].item() == total
    seq = [0.0, 0.0]
    for m in range(n):
        for c in range(2):
            seq[c] = seq[c] + t[order[m], c].item()
    # the positive control: the order is observable
    assert got[0].tolist() != seq and got[0].tolist() != t[order.long()].sum(0).tolist()
    # another block size is another set of bits, and segments are independent of each other
    assert R.group_rows_sum(t, order, i64([0]), i64([n]), block=64)[0].tolist() != got[0].tolist()
    two = R.group_rows_sum(t, order, i64([5, 0, 9]), i64([5, n, 10]))
    assert two[0].tolist() == [0.0, 0.0] and bits_equal(two[1], got[0]) and two[2].tolist() == t[order[9]].tolist()


def test_singleton_gives_one_and_conditionals_never_exceed_one():
    g = torch.Generator().manual_seed(4)
    D, V, K = 7, 40, 5
    th = torch.rand(D, 1, K, dtype=torch.float64, generator=g)
    ph = torch.rand(V, 1, K, dtype=torch.float64, generator=g) * 1e-3
    order = torch.randperm(V, generator=g).to(torch.int32)
    s, e = i64([0, 10, 11, 30]), i64([10, 11, 30, 40])
    gs = R.group_rows_sum(ph.reshape(V, K), order, s, e).reshape(-1, 1, K)
    seg = torch.empty(V, dtype=torch.int32)
    for j in range(4):
        seg[order[s[j]:e[j]].long()] = j
    word = torch.arange(V, dtype=torch.int32)
    doc = torch.randint(-1, D, (V,), generator=g, dtype=torch.int32)
    cond, why = R.explain_sides(th, ph, gs, doc, word, seg.reshape(-1, 1), 0.2)
    assert bool((cond <= 1.0).all()) and bool((cond > 0).all()) and (doc < 0).any()
    assert cond[order[10], 0].item() == 1.0 and bool((why == 0).all())
    # R = 1: s is the scorer's score -- a group of the row itself gives exactly 1
    c1, _ = R.explain_sides(th, ph, ph, doc, word, word.reshape(-1, 1), 0.2)
    assert bool((c1 == 1.0).all())
    s_ref = R.score(th[:, 0], ph[:, 0], K, 0.2, doc, word)[0]
    ones = torch.ones(1, 1, K, dtype=torch.float64)      # m = sum of theta: cond * m is the score back
    cm, _ = R.explain_sides(th, ph, ones, doc, word, torch.zeros(V, 1, dtype=torch.int32), 0.2)
    m = R.score(th[:, 0], ones[:, 0], K, 0.2, doc, torch.zeros(V, dtype=torch.int32))[0]
    assert bits_equal(cm[:, 0], s_ref / m)


def test_ties_nan_and_member_order():
    th = torch.ones(1, 1, 1, dtype=torch.float64)
    ph = f64([[[0.25]], [[0.5]]])
    gs = f64([[[0.5]], [[1.0]], [[float("nan")]]])
    z = i32([0, 0, 0, 0, -1])
    word = i32([0, 0, 0, -1, 0])
    grow = i32([[0, 0, 1], [1, 0, 0], [2, -1, 2], [0, 0, 0], [1, 1, 0]])
    cond, why = R.explain_sides(th, ph, gs, z, word, grow, 0.5)
    assert cond[0].tolist() == [0.5, 0.5, 0.25] and why[0].item() == 2
    assert cond[1].tolist() == [0.25, 0.5, 0.5] and why[1].item() == 0
    assert torch.isnan(cond[2]).all() and why[2].item() == 255      # NaN group, no group, NaN group
    assert torch.isnan(cond[3]).all() and why[3].item() == 255      # no phi row
    assert cond[4].tolist() == [0.125 / 0.5, 0.125 / 0.5, 0.125 / 0.25] and why[4].item() == 0      # default theta; tie
    # members are added in member order, then divided by R (as score_ensemble)
    th3 = torch.ones(1, 3, 1, dtype=torch.float64)
    ph3 = f64([[[0.1], [0.2], [0.3]]])
    gs3 = f64([[[0.7], [0.1], [0.9]]])
    c3, _ = R.explain_sides(th3, ph3, gs3, i32([0]), i32([0]), i32([[0]]), 0.5)
    assert c3.item() == ((((0.0 + 0.1) + 0.2) + 0.3) / 3) / ((((0.0 + 0.7) + 0.1) + 0.9) / 3)


# ------------------------------------------------------------------------------------- the field tables
def _digits(kind, name):
    """The key's digits of a word name, as texts, most significant first."""
    if kind == "flow":
        side = name.startswith("-1_")
        return (name[3:] if side else name).split("_") + ["1" if side else "0"]
    if kind == "dns":
        return name.split("_", 6)      # the query pair holds a "_" of its own
    from oni_ml_amd.features import proxy as FP      # proxy: the names of the empty values hold "_" of their own
    for u in (FP.UNKNOWN_METHOD, FP.UNKNOWN_CTYPE, FP.UNKNOWN_RESP):
        name = name.replace(u, u.replace("_", "\0"))
    return [p.replace("\0", "_") for p in name.split("_")]


def _key_of(fields, digits):
    key = 0
    for (_, r, _), d in zip(fields, digits):
        key = key * r + d
    return key


def test_fields_re_encode_the_decoded_names():
    from oni_ml_amd.features.dns import DnsWordSpace
    from oni_ml_amd.features.flow import FlowWordSpace
    from oni_ml_amd.features.proxy import ProxyWordSpace
    rng = np.random.default_rng(0)
    ws = FlowWordSpace(np.asarray([22.0, 80.0, 443.0, 333333.0]), 11, 11, 6)
    fl = ws.fields()
    assert [n for n, _, _ in fl] == ["port", "time", "ibyt", "ipkt", "side"] and [e for _, _, e in fl][-1] is False
    keys = rng.integers(0, 4 * 11 * 11 * 6 * 2, 300)
    ports = {"22.0": 0, "80.0": 1, "443.0": 2, "333333.0": 3}
    for k, name in zip(keys.tolist(), ws.decode_py(keys)):
        d = _digits("flow", name)
        assert _key_of(fl, [ports[d[0]]] + [int(float(x)) for x in d[1:]]) == k
    cuts = dict(frame_len=np.zeros(10), unix_tstamp=np.zeros(9), subdomain_length=np.zeros(4), entropy=np.zeros(5),
                num_periods=np.zeros(3))
    qp = ["1_0", "28_0", "33_3"]
    ds = DnsWordSpace(cuts, qp)
    fd = ds.fields()
    assert [n for n, _, _ in fd] == ["top", "frame_len", "unix_tstamp", "subdomain_length", "entropy", "num_periods",
                                     "qpair"] and all(e for _, _, e in fd)
    keys = rng.integers(0, 3 * 11 * 10 * 5 * 6 * 4 * 3, 300)
    for k, name in zip(keys.tolist(), ds.decode_py(keys)):
        d = _digits("dns", name)
        assert _key_of(fd, [int(x) for x in d[:6]] + [qp.index(d[6])]) == k

    class Feat:
        methods, ctypes, resps, cuts = ["GET", "POST"], ["text", "image", "app"], ["2", "3", "4", "5"], dict(agent=np.zeros(4))
    ps = ProxyWordSpace(Feat)
    fp = ps.fields()
    assert [n for n, _, _ in fp] == ["top", "hour", "method", "ebin", "ctype", "abin", "resp"]
    keys = rng.integers(0, 3 * 24 * 2 * 21 * 3 * 5 * 4, 300)
    for k, name in zip(keys.tolist(), ps.decode(keys)):
        d = _digits("proxy", name)
        assert _key_of(fp, [int(d[0]), int(d[1]), Feat.methods.index(d[2]), int(d[3]), Feat.ctypes.index(d[4]),
                            int(d[5]), Feat.resps.index(d[6])]) == k


# ---------------------------------------------------------------------------------------- end to end
ALL = ["flow-strict", "flow-fixed", "dns-strict", "dns-fixed", "proxy-fixed"]
_DAYS = {}


def get_day(which, tmp_path_factory):
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("exp_" + kind + compat))
    return _DAYS[which]


def read_explain(day, lp):
    """Per line: (key text, [per side (doc, word, score text, why, [c_f texts])]) and the explained field names."""
    _, fields = C.load_word_fields(str(lp))
    names = [n for n, _, e in fields if e]
    F = len(names)
    sep = SIDES[day.kind][0]
    lines = (lp / f"{day.kind}_explain.csv").read_text(encoding="utf-8").split("\n")
    assert lines[-1] == ""
    out = []
    for ln in lines[:-1]:
        f = ln.split(sep)
        n_sides = len(SIDES[day.kind][1])
        assert len(f) == 1 + n_sides * (4 + F)
        out.append((f[0], [(f[1 + j * (4 + F)], f[2 + j * (4 + F)], f[3 + j * (4 + F)], f[4 + j * (4 + F)],
                            f[5 + j * (4 + F):5 + (j + 1) * (4 + F) - 4]) for j in range(n_sides)]))
    return out, names


def _tables(lp, members=1):
    dirs = [str(lp)] + [os.path.join(str(lp), "ensemble", f"m{r}") for r in range(1, members)]
    tabs = [(lda_post.read_results(os.path.join(d, "doc_results.csv")),
             lda_post.read_results(os.path.join(d, "word_results.csv"))) for d in dirs]
    (dn, _), (wn, _) = tabs[0]
    th = torch.from_numpy(np.ascontiguousarray(np.stack([t[0][1] for t in tabs], 1)))
    ph = torch.from_numpy(np.ascontiguousarray(np.stack([t[1][1] for t in tabs], 1)))
    return dn, wn, th, ph


def twin_conditionals_of_file(day, lp, members=1):
    """(parsed c_f [sides, F], the twin's over the written tables and word_fields.npz, parsed why, the twin's):
    the groups from a Python dict over the masked keys, their sums and the conditionals from the twins."""
    dn, wn, th, ph = _tables(lp, members)
    keys, fields = C.load_word_fields(str(lp))
    assert keys.size == len(wn)
    rows, names = read_explain(day, lp)
    di = {n: i for i, n in enumerate(dn)}      # later duplicates win, as the scorers' maps
    wi = {n: i for i, n in enumerate(wn)}
    doc = [di.get(s[0], -1) for _, sides in rows for s in sides]
    word = [wi.get(s[1], -1) for _, sides in rows for s in sides]
    stride = [1] * len(fields)
    for i in range(len(fields) - 2, -1, -1):
        stride[i] = stride[i + 1] * fields[i + 1][1]
    order, seg, grow = [], {}, []
    members_of = {}
    for i, (_, r, e) in enumerate(fields):
        if e:
            for row, k in enumerate(keys.tolist()):
                dgt = k // stride[i] if i == 0 else (k // stride[i]) % r
                members_of.setdefault((i, k - dgt * stride[i]), []).append(row)
    for w in word:
        g = []
        for i, (_, r, e) in enumerate(fields):
            if not e:
                continue
            if w < 0:
                g.append(-1)
                continue
            k = int(keys[w])
            dgt = k // stride[i] if i == 0 else (k // stride[i]) % r
            gid = (i, k - dgt * stride[i])
            if gid not in seg:
                seg[gid] = (len(seg), len(order), len(order) + len(members_of[gid]))
                order += members_of[gid]
            g.append(seg[gid][0])
        grow.append(g)
    V, R_, K = ph.shape
    segs = sorted(seg.values())
    gs = R.group_rows_sum(ph.reshape(V, R_ * K), i32(order), i64([s[1] for s in segs]), i64([s[2] for s in segs]))
    want, why = R.explain_sides(th, ph, gs.reshape(-1, R_, K), i32(doc), i32(word), i32(grow).reshape(len(word), -1),
                                day.default(K))
    got = f64([[float(x) if x else float("nan") for x in s[4]] for _, sides in rows for s in sides])
    why_got = [s[3] for _, sides in rows for s in sides]
    return got, want, why_got, ["" if w == 255 else names[w] for w in why.tolist()]


def check_day_against_oracle(day, lp, summary):
    """(b), (c) and (e): the explain file against the results file line for line, and against an oracle that reads
    only the written files: fields by position in the words.dat names, groups in a dict, sums by math.fsum."""
    rows, names = read_explain(day, lp)
    sep, sides = SIDES[day.kind]
    res = [ln.split(sep) for ln in (lp / day.results).read_text(encoding="utf-8").split("\n")[:-1]]
    assert len(res) == len(rows) == summary["scored"] > 20
    for f, (key, ss) in zip(res, rows):
        assert [s[2] for s in ss] == [f[c[2]] for c in sides] and [s[1] for s in ss] == [f[c[1]] for c in sides]
        assert [s[0] for s in ss] == [f[c[0]] for c in sides]
        assert key in [s[2] for s in ss] and float(key) == min(float(s[2]) for s in ss)
    hist = summary["explain_why_hist"]
    assert summary["explain_fields"] == names and list(hist) == names + ["none"]
    assert sum(hist.values()) == len(rows) * len(sides)
    flat = [s for _, ss in rows for s in ss]
    for nm in names + ["none"]:
        assert hist[nm] == sum(1 for s in flat if s[3] == ("" if nm == "none" else nm))
    # the oracle
    dn, wn, th, ph = _tables(lp)
    th, ph = th[:, 0].numpy(), ph[:, 0].numpy()
    K = th.shape[1]
    full = ldac.read_index_file(str(lp / "words.dat"))
    assert len(full) == len(wn)
    digits = [_digits(day.kind, w) for w in full]
    nf = len(digits[0])
    explained = [i for i in range(nf) if not (day.kind == "flow" and i == nf - 1)]
    assert len(explained) == len(names)
    groups = {}
    for row, d in enumerate(digits):
        assert len(d) == nf
        for i in explained:
            groups.setdefault((i, tuple(d[:i] + d[i + 1:])), []).append(row)
    di = {n: i for i, n in enumerate(dn)}
    wi = {n: i for i, n in enumerate(wn)}      # the names as written (truncated in strict mode); later rows win
    dflt = day.default(K)
    checked = largest = 0
    for s in flat:
        w = wi.get(s[1], -1)
        if w < 0:
            assert s[3] == "" and all(x == "" for x in s[4])
            continue
        t = th[di[s[0]]] if s[0] in di else np.full(K, dflt)
        sc = math.fsum((t * ph[w]).tolist())
        c, bound = [], []
        for i in explained:
            mem = groups[(i, tuple(digits[w][:i] + digits[w][i + 1:]))]
            big = [math.fsum(ph[mem, k].tolist()) for k in range(K)]
            c.append(sc / math.fsum((t * np.asarray(big)).tolist()))
            bound.append(2 * (len(mem) + K + 2) * 2.0 ** -53)
            largest = max(largest, len(mem))
        for x, cf, b in zip(s[4], c, bound):
            assert abs(float(x) - cf) <= b * cf, (s, cf)
        lo = sorted(range(len(c)), key=lambda j: c[j])
        if len(c) == 1 or c[lo[1]] - c[lo[0]] > 2 * max(bound) * c[lo[1]]:
            assert s[3] == names[lo[0]]
        checked += 1
    assert checked > 20
    assert largest == max(summary["explain_max_group"].values()) and list(summary["explain_max_group"]) == names
    return largest


@pytest.mark.parametrize("which", ALL)
def test_day_with_explain(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    plain, sp = day.run("plain")
    lp, s = day.run("explain", explain=True)
    a, b = tree(plain), tree(lp)
    assert set(b) - set(a) == {"word_fields.npz", f"{day.kind}_explain.csv"} and set(a) <= set(b)      # (a)
    for f in a:
        assert a[f] == b[f], f
    assert "explain_fields" not in sp and "explain_why_hist" not in sp
    assert {k for k in s if k not in sp} == {"explain_fields", "explain_why_hist", "explain_max_group"}
    recs = [json.loads(x) for x in (lp / "metrics.jsonl").read_text().splitlines()]
    det = [r for r in recs if r.get("stage") == f"{day.kind}_post_detail" and "explain_why_hist" in r]
    assert len(det) == 1 and det[0]["explain_why_hist"] == s["explain_why_hist"]
    assert not any("explain_why_hist" in json.loads(x) for x in (plain / "metrics.jsonl").read_text().splitlines())
    check_day_against_oracle(day, lp, s)      # (b), (c), (e)
    got, want, why_got, why_want = twin_conditionals_of_file(day, lp)
    assert bits_equal(got, want) and why_got == why_want
    assert bool((got[~torch.isnan(got)] <= 1.0).all())
    keys, fields = C.load_word_fields(str(lp))
    assert keys.dtype == np.int64 and len(fields) == len(_digits(day.kind, ldac.read_index_file(str(lp / "words.dat"))[0]))


# (d) a day whose explained sides refer to a group of more than GROUP_BLOCK members.  The default days have none
# (flow port groups: at most 15 words at 4,000 events, 28 at 20,000, 60 at 100,000 -- a day scaled up alone would
# need millions of events), so the flow day is scaled 5 x and binned coarsely through the CUT option (two byte
# cuts, one packet cut, two time cuts): 18 bin triples over ~300 ports, port groups of up to ~290 words.
BIG = dict(scale=5, cuts="0 1000,0,0 12")


@pytest.mark.parametrize("compat", ["strict", "fixed"])
def test_a_day_whose_sides_refer_to_a_group_past_one_block(compat, tmp_path_factory):
    day = Day("flow", compat, tmp_path_factory.mktemp("exp_big_" + compat), scale=BIG["scale"])
    lp, s = day.run("explain", explain=True, cuts=BIG["cuts"])
    assert max(s["explain_max_group"].values()) > CFG.GROUP_BLOCK == 256
    assert check_day_against_oracle(day, lp, s) > CFG.GROUP_BLOCK      # the oracle's own count of the group
    got, want, why_got, why_want = twin_conditionals_of_file(day, lp)
    assert bits_equal(got, want) and why_got == why_want
    plain, _ = day.run("plain", cuts=BIG["cuts"])
    assert (plain / day.results).read_bytes() == (lp / day.results).read_bytes()


def test_a_fresh_run_removes_what_an_earlier_explain_run_left(tmp_path):
    for f in ("flow_explain.csv", "word_fields.npz", "flow_scores.csv", "flow_results.csv"):
        (tmp_path / f).write_text("x")
    cli.clean_workdir(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["flow_results.csv", "flow_scores.csv"]


@pytest.mark.parametrize("which", ["flow-strict", "dns-fixed", "proxy-fixed"])
def test_max_results_host_report_and_ensemble(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp, s = day.run("explain", explain=True)
    N = s["scored"] // 3
    lim, sl = day.run("explain_lim", explain=True, max_results=N)
    full = (lp / f"{day.kind}_explain.csv").read_bytes().splitlines(keepends=True)
    assert (lim / f"{day.kind}_explain.csv").read_bytes() == b"".join(full[:N]) and N > 5
    assert sum(sl["explain_why_hist"].values()) == N * len(SIDES[day.kind][1])
    # the host report is what it is without the flag
    h0, _ = day.run("hosts", host_report=-1)
    h1, _ = day.run("hosts_explain", host_report=-1, explain=True)
    assert (h0 / f"{day.kind}_hosts.csv").read_bytes() == (h1 / f"{day.kind}_hosts.csv").read_bytes()
    assert (h1 / f"{day.kind}_explain.csv").read_bytes() == b"".join(full)
    # --ensemble 3: the twin over the three written member tables
    ens, se = day.run("explain_ens3", explain=True, ensemble=3)
    got, want, why_got, why_want = twin_conditionals_of_file(day, ens, members=3)
    assert got.shape[0] > 20 and bits_equal(got, want) and why_got == why_want
    assert (ens / day.results).read_bytes() == (day.run("ens3", ensemble=3)[0] / day.results).read_bytes()


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_resume_writes_the_same_explain_file(which, tmp_path_factory):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)
    want = (day.run("explain", explain=True)[0] / f"{day.kind}_explain.csv").read_bytes()
    lp = day.root / "resume"
    day.go(day.cfg(lp, explain=True))
    post = f"{day.kind}_post"
    ex = lp / f"{day.kind}_explain.csv"
    assert ex.read_bytes() == want
    # at the scoring stage
    os.unlink(lp / ".stages" / f"{post}.done")
    os.unlink(ex)
    run(day.cfg(lp, explain=True, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert ex.read_bytes() == want
    # at lda_post
    for p in (lp / ".stages" / f"{post}.done", lp / ".stages" / "lda_post.done", ex, lp / "word_results.csv"):
        os.unlink(p)
    run(day.cfg(lp, explain=True, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert ex.read_bytes() == want
    # without word_fields.npz: refused before any stage runs, nothing written
    os.unlink(lp / ".stages" / f"{post}.done")
    os.unlink(lp / "word_fields.npz")
    os.unlink(ex)
    before = tree(lp)
    marks = sorted(os.listdir(lp / ".stages"))
    with pytest.raises(ValueError, match="word_fields.npz"):
        run(day.cfg(lp, explain=True, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert tree(lp) == before and sorted(os.listdir(lp / ".stages")) == marks and not ex.exists()
    # a rerun from scratch produces it
    day.go(day.cfg(lp, explain=True))
    assert ex.read_bytes() == want and (lp / "word_fields.npz").exists()


@pytest.mark.parametrize("which", ["flow-strict", "proxy-fixed"])
def test_refusals_write_nothing(which, tmp_path_factory, monkeypatch):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)

    class Group:
        active, rank, world_size = True, 0, 2
    never = day.root / "never"
    assert CFG.RunConfig().explain is False and CFG.EXPLAIN_ONE_PROCESS.startswith("--explain")
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="one process"):
            day.cfg(never, explain=True, **kw).validate()
        with pytest.raises(ValueError, match="one process"):
            run(day.cfg(never, explain=True, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, explain=True), dist=Group(), device="cpu")
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("EXPLAIN", raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    for extra in (["--explain", "--gpus", "2"], ["--explain", "--hdfs"]):
        with pytest.raises(ValueError, match="one process"):
            cli.cmd_ml_ops(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--explain"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("EXPLAIN", "1")
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
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("EXPLAIN", raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nEXPLAIN=1\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].explain is False
    assert cli.cmd_ml_ops(base + none + ["--explain"]) == 0 and seen["cfg"].explain is True
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].explain is True
    monkeypatch.setenv("EXPLAIN", "0")
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].explain is False      # environment over file
    monkeypatch.setenv("EXPLAIN", "1")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].explain is True
    assert "EXPLAIN" in CFG.ENV_KEYS
