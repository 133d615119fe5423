"""--topic-report on the CPU path: the torch twins ``ops.reference.column_topn`` / ``row_dominant`` / ``topic_sides``
against brute-force oracles bit for bit (Python ``sorted`` by (-value, row) over a column's non-NaN entries;
per-element Python loops in IEEE double), ties, signed zeros, NaN, the slab, and the three pipelines end to end on
the torch LDA backend -- nothing else changes, the per-event file follows the results file line for line, every
cell of the four files is the twins' over the written tables; MAXRESULTS, the ensemble, the other options beside
it, resume, the refusals and the clean-up."""
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
from oni_ml_amd.pipeline.common import TOPIC_REPORT_FILES, TOPIC_REPORT_KEYS, TOPIC_RESP_BUCKETS  # noqa: E402

f64 = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
i32 = lambda x: torch.tensor(x, dtype=torch.int32)        # noqa: E731
TOPIC_KEYS = set(TOPIC_REPORT_KEYS)
NINF = float("-inf")
NAN = float("nan")


def topn_case(rows, R_, K, seed=0):
    """A table [rows, R K] on the CPU: rows normalised per member like a topic mixture, over several decades; where
    the table is tall enough, rows 3 and 7 are identical (a tie in every column) and column 0 holds a NaN."""
    g = torch.Generator().manual_seed(7919 * rows + 100 * R_ + K + seed)
    t = torch.rand(rows, R_, K, dtype=torch.float64, generator=g) ** 4
    t = t / t.sum(2, keepdim=True)
    if rows > 7:
        t[7] = t[3]
        t[5, 0, 0] = NAN
    return t.reshape(rows, R_ * K).contiguous()


def tripled(rows3=7, W=5):
    """A table in which every row occurs three times: rows r, r + rows3, r + 2 rows3 are the same."""
    t = topn_case(rows3, 1, W, seed=5)      # (rows3 <= 7: nothing planted, the rows are distinct)
    return torch.cat([t, t, t]).contiguous()


def edge_table():
    """131 x 6: column 1 all equal, column 2 holds -0.0 (row 9) before +0.0 (row 20) among negatives, column 3 a NaN
    at its greatest row's neighbour, column 4 NaN only, column 5 +inf and -inf."""
    t = topn_case(131, 1, 6, seed=9)
    t[:, 1] = 0.25
    t[:, 2] = -t[:, 2]
    t[9, 2], t[20, 2] = -0.0, 0.0
    t[(int(t[:, 3].argmax()) + 1) % 131, 3] = NAN
    t[:, 4] = NAN
    t[17, 5], t[18, 5] = float("inf"), NINF
    return t


def oracle(t, n):
    """Per column the list [(value, row)]: ``sorted`` by (-value, row) over the non-NaN entries."""
    out = []
    for j in range(t.shape[1]):
        c = [(-v, r) for r, v in enumerate(t[:, j].tolist()) if not math.isnan(v)]
        out.append([(t[r, j].item(), r) for _, r in sorted(c)[:n]])
    return out


def check_against_oracle(got, t, n):
    rows, vals, count = got
    assert rows.dtype == torch.int32 and vals.dtype == torch.float64 and count.dtype == torch.int32
    assert tuple(rows.shape) == tuple(vals.shape) == (t.shape[1], n) and tuple(count.shape) == (t.shape[1],)
    for j, want in enumerate(oracle(t, n)):
        c = int(count[j])
        assert c == len(want)
        assert rows[j, :c].tolist() == [r for _, r in want]
        assert bits_equal(vals[j, :c], f64([v for v, _ in want]))      # bits: a listed -0.0 stays -0.0
        assert rows[j, c:].tolist() == [-1] * (n - c) and vals[j, c:].tolist() == [NINF] * (n - c)


# ------------------------------------------------------------------------------------------ the twins
@pytest.mark.parametrize("n", [1, 5, 32])
@pytest.mark.parametrize("K,R_", [(1, 1), (3, 3), (20, 1), (33, 3)])
@pytest.mark.parametrize("rows", [1, 2, 5, 17, 131])
def test_column_topn_against_the_brute_force_oracle(rows, K, R_, n):
    t = topn_case(rows, R_, K)
    got = R.column_topn(t, n)
    check_against_oracle(got, t, n)
    nans = torch.isnan(t).sum(0).to(torch.int32)
    assert bool((got[2] == torch.clamp(rows - nans, max=n)).all())      # rows < n: short lists


def test_ties_go_to_the_lower_row():
    t = tripled()
    rows3 = t.shape[0] // 3
    rows, vals, count = R.column_topn(t, 5)
    for j in range(t.shape[1]):
        best = int(t[:rows3, j].argmax())
        assert rows[j, :3].tolist() == [best, best + rows3, best + 2 * rows3]
        assert vals[j, 0] == vals[j, 1] == vals[j, 2] > vals[j, 3] and int(count[j]) == 5
    assert R.column_topn(t, 1)[0][:, 0].tolist() == [int(t[:rows3, j].argmax()) for j in range(t.shape[1])]
    check_against_oracle((rows, vals, count), t, 5)


def test_equal_values_signed_zeros_and_nans():
    t = edge_table()
    for n in (1, 5, 32):
        rows, vals, count = R.column_topn(t, n)
        check_against_oracle((rows, vals, count), t, n)
        assert rows[1].tolist() == list(range(n))                            # all equal: the lowest rows
        assert int(count[4]) == 0 and rows[4].tolist() == [-1] * n           # NaN only
        assert not bool(torch.isnan(vals).any())
    rows, vals, count = R.column_topn(t, 5)
    assert rows[2, :2].tolist() == [9, 20]                                   # -0.0 and +0.0 tie: the lower row first
    assert math.copysign(1.0, vals[2, 0].item()) == -1.0 and math.copysign(1.0, vals[2, 1].item()) == 1.0
    assert int(torch.isnan(t[:, 3]).nonzero()[0]) not in R.column_topn(t, 32)[0][3].tolist()      # never listed
    assert rows[5, 0] == 17 and vals[5, 0] == float("inf")
    assert R.column_topn(t, 32)[0][5].tolist().count(18) == 0                # -inf is a value, but 130 others beat it
    assert R.column_topn(t[16:19], 5)[0][5].tolist() == [1, 0, 2, -1, -1]    # ... and is listed where there is room
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="n must be"):
            R.column_topn(t, bad)
    with pytest.raises(ValueError, match="float64"):
        R.column_topn(t.float(), 3)
    out = R.column_topn(t[:0], 3)
    assert tuple(out[0].shape) == (6, 3) and out[2].tolist() == [0] * 6 and out[1][0].tolist() == [NINF] * 3


def dominant_case(rows, R_, K, seed=0):
    """[rows, R, K] with an all-equal row (row 1), a NaN among values (row 2), an all-NaN member (row 4) and a
    signed-zero tie (row 6), where the table has those rows."""
    t = topn_case(rows, R_, K, seed=seed + 1).reshape(rows, R_, K).clone()
    if rows > 7:
        t[5, 0, 0] = 0.1
        t[1] = 0.3
        t[2, 0, K // 2] = NAN
        t[4, R_ - 1] = NAN
        t[6, 0] = -0.0
        t[6, 0, K - 1] = 0.0
    return t


def first_max(vals):
    """The first index attaining the maximum under IEEE ``>``, a NaN never; -1: all NaN."""
    best, bv = -1, 0.0
    for k, v in enumerate(vals):
        if not math.isnan(v) and (best < 0 or v > bv):
            best, bv = k, v
    return best


@pytest.mark.parametrize("K,R_", [(1, 1), (3, 3), (20, 1), (20, 3), (33, 3)])
def test_row_dominant_against_python_loops(K, R_):
    for rows in (0, 1, 131):
        t = dominant_case(rows, R_, K)
        arg, counts = R.row_dominant(t)
        assert arg.dtype == torch.int32 and counts.dtype == torch.int64
        assert tuple(arg.shape) == (rows, R_) and tuple(counts.shape) == (R_, K)
        want = [[first_max(t[i, r].tolist()) for r in range(R_)] for i in range(rows)]
        assert arg.tolist() == want
        assert counts.tolist() == [[sum(1 for i in range(rows) if want[i][r] == k) for k in range(K)]
                                   for r in range(R_)]
        if rows == 131:
            assert arg[4, R_ - 1] == -1 and int(counts.sum()) == int((arg >= 0).sum()) < rows * R_
            assert arg[6, 0] == 0 and arg[1].tolist() == [0] * R_      # ties, -0.0 and +0.0 among them: the first k
        for slab in (1, R_ * K):
            a, c = R.row_dominant(t, slab=slab)
            assert torch.equal(a, arg) and torch.equal(c, counts)


def sides_case(n, D, V, R_, K, seed=0):
    """(theta [D, R, K], phi [V, R, K], doc, word): misses on either side and both, a side with tied products
    (θ row 1 and φ row 1 constant), an all-NaN side (θ row 2), one NaN product among real ones (φ row 3)."""
    g = torch.Generator().manual_seed(31 * n + 7 * R_ + K + seed)
    th = dominant_case(D, R_, K, seed=seed + 2) if D > 7 else topn_case(D, R_, K).reshape(D, R_, K)
    ph = torch.rand(V, R_, K, dtype=torch.float64, generator=g) ** 3 * 1e-3
    th[1], ph[1] = 0.125, 0.5
    th[2] = NAN
    ph[3, 0, 0] = NAN
    doc = torch.randint(-1, D, (n,), generator=g, dtype=torch.int32)
    word = torch.randint(-1, V, (n,), generator=g, dtype=torch.int32)
    m = min(n, 6)
    doc[:m] = i32([-1, -1, 0, 1, 2, 0][:m])
    word[:m] = i32([-1, 0, -1, 1, 0, 3][:m])
    return th, ph, doc, word


def sides_oracle(th, ph, doc, word):
    """Per side (col, resp, host_share, host_topic) from Python floats, one rounded operation per step."""
    D, R_, K = th.shape
    out = []
    for d, w in zip(doc.tolist(), word.tolist()):
        if d < 0 or w < 0:
            out.append((-1, NAN, NAN, -1))
            continue
        t, p = th[d].reshape(-1).tolist(), ph[w].reshape(-1).tolist()
        prod = [a * b for a, b in zip(t, p)]
        best = first_max(prod)
        if best < 0:
            out.append((-1, NAN, NAN, -1))
            continue
        total = 0.0
        for r in range(R_):
            s = 0.0
            for k in range(K):
                s = s + prod[r * K + k]
            total = total + s
        with np.errstate(divide="ignore", invalid="ignore"):      # IEEE: x / 0 is an infinity or a NaN
            score = np.float64(total) / np.float64(R_)
            resp = float(np.float64(prod[best]) / (score * np.float64(R_)))      # the stated two operations
        r = best // K
        out.append((best, resp, t[best], first_max(t[r * K:(r + 1) * K])))
    return out


def check_sides(got, th, ph, doc, word):
    col, resp, share, ht = got
    assert col.dtype == ht.dtype == torch.int32 and resp.dtype == share.dtype == torch.float64
    want = sides_oracle(th, ph, doc, word)
    assert col.tolist() == [x[0] for x in want] and ht.tolist() == [x[3] for x in want]
    assert bits_equal(resp, f64([x[1] for x in want])) and bits_equal(share, f64([x[2] for x in want]))
    return want


@pytest.mark.parametrize("K,R_", [(1, 1), (3, 3), (20, 1), (20, 3), (33, 3)])
def test_topic_sides_against_python_loops(K, R_):
    th, ph, doc, word = sides_case(300, 37, 50, R_, K)
    got = R.topic_sides(th, ph, doc, word)
    want = check_sides(got, th, ph, doc, word)
    assert want[3][0] == 0 and want[4][0] == -1 and want[0][0] == want[1][0] == want[2][0] == -1
    assert want[5][0] > 0 or K * R_ == 1      # the NaN product at j = 0 never wins
    assert sum(1 for x in want if x[0] >= 0) > 150
    # the score is the scorers': resp x score x R gives the product back only through the same two operations
    s = R.score_ensemble(th, ph, R_, K, 0.05, doc, word)[0]
    j = got[0].long().clamp_min(0)
    prod = th.reshape(37, -1)[doc.long().clamp_min(0), j] * ph.reshape(50, -1)[word.long().clamp_min(0), j]
    ok = got[0] >= 0
    assert bits_equal(got[1][ok], (prod / (s * float(R_)))[ok])
    for slab in (1, R_ * K):
        assert all(bits_equal(a, b) for a, b in zip(R.topic_sides(th, ph, doc, word, slab=slab), got))
    empty = R.topic_sides(th, ph, i32([]), i32([]))
    assert all(x.numel() == 0 for x in empty)
    with pytest.raises(ValueError, match="out of range"):
        R.topic_sides(th, ph, i32([37]), i32([0]))
    with pytest.raises(ValueError, match="out of range"):
        R.topic_sides(th, ph, i32([0]), i32([-2]))


def test_the_slab_does_not_change_the_bits():
    t = edge_table()
    a = R.column_topn(t, 7)
    for slab in (1, 6, 6 * 40):      # one value, one row's worth, 40 rows
        assert all(bits_equal(x, y) for x, y in zip(a, R.column_topn(t, 7, slab=slab)))
    t = tripled()
    assert all(bits_equal(x, y) for x, y in zip(R.column_topn(t, 5), R.column_topn(t, 5, slab=5)))


# ---------------------------------------------------------------------------------------- end to end
ALL = ["flow-strict", "flow-fixed", "dns-strict", "proxy-fixed"]
_DAYS = {}
NT = 4      # N of the days' runs


def get_day(which, tmp_path_factory):
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("topics_" + kind + compat))
    return _DAYS[which]


def names_of(day):
    return [f"{day.kind}_{x}.csv" for x in TOPIC_REPORT_FILES]


def read(day, lp, name):
    lines = (lp / f"{day.kind}_{name}.csv").read_text(encoding="utf-8").split("\n")
    assert lines[-1] == ""
    return [ln.split(SIDES[day.kind][0]) for ln in lines[:-1]]


def num(texts):
    return f64([float(t) if t else NAN for t in texts])


def check_topic_files(day, lp, summary, members=1, n=NT):
    """The four files against the results file line for line, against the twins over the written tables, and
    against the summary.  Returns the per-event file's ``resp`` column."""
    sep, sides = SIDES[day.kind]
    dn, wn, th, ph = _tables(lp, members)
    D, R_, K = th.shape
    V, W = ph.shape[0], R_ * K
    # the word and host lists
    top_mass = []
    for name, tab, names in (("topic_words", ph, wn), ("topic_hosts", th, dn)):
        rows, vals, cnt = R.column_topn(tab.reshape(tab.shape[0], W).contiguous(), n)
        got = read(day, lp, name)
        at = [(j, s) for j in range(W) for s in range(int(cnt[j]))]
        assert len(got) == len(at) and all(len(x) == (6 if name == "topic_words" else 5) for x in got)
        assert [x[:3] for x in got] == [[str(j // K), str(j % K), str(s + 1)] for j, s in at]
        assert [x[3] for x in got] == [names[int(rows[j, s])] for j, s in at]
        assert bits_equal(num([x[4] for x in got]), f64([vals[j, s].item() for j, s in at]))
        if name == "topic_words":
            want = []
            for j, s in at:
                tot = 0.0
                for v in ph[int(rows[j, s]), j // K].tolist():
                    tot = tot + v
                want.append(vals[j, s].item() / tot)
            assert bits_equal(num([x[5] for x in got]), f64(want))
            for j in range(W):
                acc = 0.0
                for s in range(int(cnt[j])):
                    acc = acc + vals[j, s].item()
                top_mass.append(acc)
            assert bool((cnt == min(n, V)).all())
    # the per-event file
    res = [ln.split(sep) for ln in (lp / day.results).read_text(encoding="utf-8").split("\n")[:-1]]
    ev = read(day, lp, "topic")
    assert len(res) == len(ev) == summary["scored"] > 20 and all(len(x) == 1 + 8 * len(sides) for x in ev)
    flat = []
    for f, x in zip(res, ev):
        ss = [x[1 + 8 * j:9 + 8 * j] for j in range(len(sides))]
        assert [s[:3] for s in ss] == [[f[c[0]], f[c[1]], f[c[2]]] for c in sides]
        assert float(x[0]) == min(float(s[2]) for s in ss)
        flat += ss
    di = {nm: i for i, nm in enumerate(dn)}      # later duplicates win, as the scorers' maps
    wi = {nm: i for i, nm in enumerate(wn)}
    doc, word = i32([di.get(s[0], -1) for s in flat]), i32([wi.get(s[1], -1) for s in flat])
    col, resp, share, ht = R.topic_sides(th, ph, doc, word)
    txt = lambda v: "" if v < 0 else str(v)      # noqa: E731
    assert [s[3] for s in flat] == [txt(c // K if c >= 0 else -1) for c in col.tolist()]
    assert [s[4] for s in flat] == [txt(c % K if c >= 0 else -1) for c in col.tolist()]
    got_resp = num([s[5] for s in flat])
    assert bits_equal(got_resp, resp) and bits_equal(num([s[6] for s in flat]), share)
    assert [s[7] for s in flat] == [txt(v) for v in ht.tolist()]
    good = got_resp[~torch.isnan(got_resp)]
    assert good.numel() > 20 and bool((good > 0).all()) and bool((good <= 1.0000001).all())
    # the topics file
    has = col >= 0
    written = torch.bincount(col[has].long(), minlength=W)
    minor = torch.bincount(col[has & (ht != col % K)].long(), minlength=W)
    mass = R.group_rows_sum(th.reshape(D, W).contiguous(), torch.arange(D), torch.zeros(1, dtype=torch.int64),
                            torch.full((1,), D, dtype=torch.int64)).reshape(-1)
    hosts_dom, words_dom = R.row_dominant(th)[1].reshape(-1), R.row_dominant(ph)[1].reshape(-1)
    tp = read(day, lp, "topics")
    assert len(tp) == W and all(len(x) == 9 for x in tp)
    assert [x[:2] for x in tp] == [[str(j // K), str(j % K)] for j in range(W)]
    assert bits_equal(num([x[2] for x in tp]), mass) and bits_equal(num([x[3] for x in tp]), mass / float(D))
    assert [x[4] for x in tp] == [str(v) for v in hosts_dom.tolist()]
    assert [x[5] for x in tp] == [str(v) for v in words_dom.tolist()]
    assert bits_equal(num([x[6] for x in tp]), f64(top_mass))
    assert [x[7] for x in tp] == [str(v) for v in written.tolist()]
    assert [x[8] for x in tp] == [str(v) for v in minor.tolist()]
    assert int(hosts_dom.sum()) == D * R_ and int(words_dom.sum()) == V * R_
    assert sum(int(x[7]) for x in tp) == int(has.sum())      # written_sides: the sides with a topic
    # the summary
    assert summary["topic_report"] == n and summary["topic_rows"] == [D, V] and summary["topic_columns"] == W
    lanes = 256 if n <= 16 else 128
    assert summary["topic_path"] == ("cpu" if day.device == "cpu" else
                                     f"subgroups{lanes // W}" if W <= lanes // 2 else "columns")
    ts = summary["topic_sides"]
    assert ts["members"] == written.reshape(R_, K).tolist() and ts["none"] == len(flat) - int(has.sum())
    assert summary["topic_minor_sides"] == int(minor.sum())
    hist = summary["topic_resp_hist"]
    assert list(hist) == list(TOPIC_RESP_BUCKETS) + ["none"] and sum(hist.values()) == len(flat)
    assert hist["none"] == ts["none"] and hist["<0.5"] == int((good < 0.5).sum())
    assert hist[">=0.99"] == int((good >= 0.99).sum())
    return got_resp


@pytest.mark.parametrize("which", ALL)
def test_day_with_the_topic_report(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    plain, sp = day.run("plain")
    lp, s = day.run("topics", topic_report=NT)
    a, b = tree(plain), tree(lp)
    assert set(b) - set(a) == set(names_of(day)) and set(a) <= set(b)
    for f in a:
        assert a[f] == b[f], f      # the results file and every LDA file: byte for byte the plain run's
    assert not TOPIC_KEYS & set(sp) and {k for k in s if k not in sp} == TOPIC_KEYS
    recs = [json.loads(x) for x in (lp / "metrics.jsonl").read_text().splitlines()]
    det = [r for r in recs if r.get("stage") == f"{day.kind}_post_detail" and "topic_resp_hist" in r]
    assert len(det) == 1 and all(det[0][k] == s[k] for k in TOPIC_KEYS)
    got = check_topic_files(day, lp, s)
    assert which != "flow-strict" or bool(torch.isnan(got).any())      # a side without a row: empty cells


@pytest.mark.parametrize("which", ["flow-strict", "dns-strict", "proxy-fixed"])
def test_max_results_ensemble_and_the_other_options(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp, s = day.run("topics", topic_report=NT)
    topics, words, hosts, event = names_of(day)
    full = (lp / event).read_bytes().splitlines(keepends=True)
    N = s["scored"] // 3
    lim, sl = day.run("topics_lim", topic_report=NT, max_results=N)
    assert (lim / event).read_bytes() == b"".join(full[:N]) and N > 5
    for f in (words, hosts):      # the model's description does not depend on what is written
        assert (lim / f).read_bytes() == (lp / f).read_bytes()
    sep = SIDES[day.kind][0].encode()
    cut = lambda p: [ln.split(sep)[:7] for ln in (p / topics).read_bytes().splitlines()]      # noqa: E731
    assert cut(lim) == cut(lp)      # ... except the two side counts
    assert sum(sl["topic_resp_hist"].values()) == N * len(SIDES[day.kind][1])
    check_topic_files(day, lim, sl)
    # --ensemble 3 with the largest N: the twins over the three written member tables
    ens, se = day.run("topics_ens3", topic_report=32, ensemble=3)
    check_topic_files(day, ens, se, members=3, n=32)
    assert len(se["topic_sides"]["members"]) == 3
    a, b = tree(day.run("ens3", ensemble=3)[0]), tree(ens)      # the members' files and the results file: unchanged
    assert set(b) - set(a) == set(names_of(day)) and all(a[f] == b[f] for f in a)
    # every other option beside it: each other file is what it is without the flag; under --tail-tol the per-event
    # file follows the tail-ranked rows
    opts = dict(explain=True, expect=True, tail_tol=0.5, peers=3, host_report=-1)
    both, sb = day.run("topics_all", topic_report=NT, **opts)
    alone, sa = day.run("all_but_topics", **opts)
    a, b = tree(alone), tree(both)
    assert set(b) - set(a) == set(names_of(day)) and all(a[f] == b[f] for f in a)
    check_topic_files(day, both, sb)
    assert TOPIC_KEYS <= set(sb) and "explain_why_hist" in sb and "tail_hist" in sb and "peer_lift_hist" in sb
    assert not TOPIC_KEYS & set(sa)
    for f in (words, hosts):
        assert (both / f).read_bytes() == (lp / f).read_bytes()


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_resume_writes_the_same_files(which, tmp_path_factory):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)
    names = names_of(day)
    first = day.run("topics", topic_report=NT)[0]
    want = [(first / f).read_bytes() for f in names]
    lp = day.root / "resume"
    day.go(day.cfg(lp, topic_report=NT))
    post = f"{day.kind}_post"
    assert [(lp / f).read_bytes() for f in names] == want
    # at the scoring stage: nothing but the model tables is needed
    os.unlink(lp / ".stages" / f"{post}.done")
    for f in names:
        os.unlink(lp / f)
    s = run(day.cfg(lp, topic_report=NT, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert [(lp / f).read_bytes() for f in names] == want and TOPIC_KEYS <= set(s)
    # a run that had no flag, resumed with it
    plain = day.root / "resume_plain"
    day.go(day.cfg(plain))
    os.unlink(plain / ".stages" / f"{post}.done")
    run(day.cfg(plain, topic_report=NT, resume=True).validate(), device="cpu", log=lambda *a: None)
    assert [(plain / f).read_bytes() for f in names] == want


@pytest.mark.parametrize("which", ["flow-strict", "proxy-fixed"])
def test_refusals_write_nothing(which, tmp_path_factory, monkeypatch):
    from oni_ml_amd.ops import hip as H
    from oni_ml_amd.pipeline import run
    from oni_ml_amd.score import scorer as S
    day = get_day(which, tmp_path_factory)

    class Group:
        active, rank, world_size = True, 0, 2
    never = day.root / "never"
    assert CFG.RunConfig().topic_report == 0 and CFG.TOPIC_REPORT_ONE_PROCESS.startswith("--topic-report")
    assert CFG.TOPIC_REPORT_MAX == 32
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="one process"):
            day.cfg(never, topic_report=3, **kw).validate()
        with pytest.raises(ValueError, match="one process"):
            run(day.cfg(never, topic_report=3, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, topic_report=3), dist=Group(), device="cpu")
    for bad in (33, -1):
        with pytest.raises(ValueError, match="--topic-report must be"):
            day.cfg(never, topic_report=bad).validate()
    # N = 0 is "off" to the configuration; the functions themselves refuse it
    t = edge_table()
    for fn in (R.column_topn, lambda x, n: S.column_topn(x, n), H.column_topn):
        with pytest.raises(ValueError, match="n must be"):
            fn(t, 0)
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TOPIC_REPORT", raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    for extra in (["--topic-report", "3", "--gpus", "2"], ["--topic-report", "3", "--hdfs"]):
        with pytest.raises(ValueError, match="one process"):
            cli.cmd_ml_ops(base + extra)
    for bad in ("33", "-1"):
        with pytest.raises(ValueError, match="--topic-report must be"):
            cli.cmd_ml_ops(base + ["--topic-report", bad])
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--topic-report", "3"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("TOPIC_REPORT", "3")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    monkeypatch.setenv("TOPIC_REPORT", "33")
    with pytest.raises(ValueError, match="--topic-report must be"):
        cli.cmd_ml_ops(base)
    assert not never.exists()


def test_a_fresh_run_removes_stale_topic_files(tmp_path):
    stale = ["flow_topics.csv", "flow_topic_words.csv", "flow_topic_hosts.csv", "flow_topic.csv"]
    for f in stale + ["flow_scores.csv", "flow_results.csv"]:
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
    monkeypatch.delenv("TOPIC_REPORT", raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nTOPIC_REPORT=7\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].topic_report == 0
    assert cli.cmd_ml_ops(base + none + ["--topic-report", "5"]) == 0 and seen["cfg"].topic_report == 5
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].topic_report == 7
    monkeypatch.setenv("TOPIC_REPORT", "0")      # the environment over the file; 0 is off, not an error
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].topic_report == 0
    assert CFG.RunConfig.check_topic_report(0, gpus=2, hdfs=True, world=2) == 0
    monkeypatch.setenv("TOPIC_REPORT", "32")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].topic_report == 32
    assert cli.cmd_ml_ops(base + none + ["--topic-report", "2"]) == 0 and seen["cfg"].topic_report == 2
    assert "TOPIC_REPORT" in CFG.ENV_KEYS and CFG.TOPIC_BLOCK >= 1 and CFG.TOPIC_SCRATCH_MB > 0
