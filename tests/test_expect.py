"""--expect on the CPU path: the torch twin ``ops.reference.expect_sides`` against an oracle of plain loops (groups
from the keys' digits, every dot in topic order in Python floats: no code shared with ``field_segments`` or the
twin), its invariants, and the three pipelines end to end on the torch LDA backend -- the expect file follows the
results file line for line and passes the oracle over the written tables bit for bit, nothing else changes;
MAXRESULTS, the host report, the ensemble, --tail-tol, resume, the refusals and the ways the flag reaches the
config."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import SIDES, Day, tree  # noqa: E402
from test_explain import BIG, _tables  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

NAN = float("nan")


# ------------------------------------------------------------------------------------------ the oracle
def groups_of(keys, fields):
    """{(field position, key with that digit zeroed): [phi rows, ascending]} for the explained fields."""
    stride = [1] * len(fields)
    for i in range(len(fields) - 2, -1, -1):
        stride[i] = stride[i + 1] * fields[i + 1][1]
    out = {}
    for row, k in enumerate(int(x) for x in keys):
        for i, (_, r, e) in enumerate(fields):
            if e:
                dgt = k // stride[i] if i == 0 else (k // stride[i]) % r
                out.setdefault((i, k - dgt * stride[i]), []).append(row)
    return out, stride


def group_of(groups, stride, fields, keys, w, i):
    k = int(keys[w])
    dgt = k // stride[i] if i == 0 else (k // stride[i]) % fields[i][1]
    return groups[(i, k - dgt * stride[i])]


def dot_py(th, ph):
    """The scorers' dot of [R][K] rows in Python floats: topic order, members in order, / R."""
    total = 0.0
    for tr, pr in zip(th, ph):
        acc = 0.0
        for t, p in zip(tr, pr):
            acc = acc + t * p
        total = total + acc
    return total / float(len(th))


def dots_np(th, ph_rows):
    """``dot_py`` of one theta row [R, K] against many phi rows [m, R, K]: the same operations, elementwise."""
    total = np.zeros(ph_rows.shape[0])
    for r in range(th.shape[0]):
        acc = np.zeros(ph_rows.shape[0])
        for k in range(th.shape[1]):
            acc = acc + th[r, k] * ph_rows[:, r, k]
        total = total + acc
    return total / float(th.shape[0])


def pick(mem, p, s):
    """(best, pbest, above, lift) of the definition, from the members' rows and scores."""
    best, pb, above = -1, NAN, 0
    for v, x in zip(mem, p):
        if x > s:
            above += 1
        if x == x and (best < 0 or x > pb or (x == pb and v < best)):
            best, pb = v, x
    with np.errstate(invalid="ignore", divide="ignore"):
        lift = float(np.float64(pb) / np.float64(s))
    return best, pb, above, lift


def oracle_side(th3, ph3, dflt, groups, stride, fields, keys, d, w, python=False):
    """Per explained field (best, pbest, above, lift) of the side (d, w), None without a phi row."""
    if w < 0:
        return None
    R_, K = ph3.shape[1:]
    th = th3[d] if d >= 0 else np.full((R_, K), dflt)
    s = dot_py(th.tolist(), ph3[w].tolist())
    out = []
    for i, (_, _, e) in enumerate(fields):
        if not e:
            continue
        mem = group_of(groups, stride, fields, keys, w, i)
        if python:
            p = [dot_py(th.tolist(), ph3[v].tolist()) for v in mem]
        else:
            p = dots_np(th, ph3[mem]).tolist()
        out.append(pick(mem, p, s))
    return out


def same(a, b):
    return a == b or (a != a and b != b)


# ------------------------------------------------------------------------------------------- the twin
FIELDS = [("a", 3, True), ("b", 4, True), ("c", 5, False), ("d", 2, True)]


def small_tables(R_=1, seed=0):
    g = np.random.default_rng(seed)
    V, D, K = 70, 9, 4
    keys = g.choice(3 * 4 * 5 * 2, V, replace=False).astype(np.int64)
    th = g.random((D, R_, K))
    ph = g.random((V, R_, K)) * 1e-2
    grp, stride = groups_of(keys, FIELDS)
    big = max((m for (i, _), m in grp.items() if i == 1), key=len)      # a group of field b with several members
    assert len(big) >= 3
    ph[big[2]] = ph[big[0]]                                  # duplicate rows: the lowest row wins the tie
    solo = [m for m in grp.values() if len(m) == 1]
    assert solo
    other = [m for (i, _), m in grp.items() if i == 0 and len(m) >= 2 and not set(m) & set(big)]
    ph[other[0][0]] = NAN                                    # a NaN row: never best, counts nothing
    ph[other[1][0]] = -0.0                                   # a row of -0.0
    return keys, th, ph, grp, stride, big, solo, other


@pytest.mark.parametrize("R_", [1, 3])
def test_twin_against_the_oracle(R_):
    keys, th, ph, grp, stride, big, solo, other = small_tables(R_)
    V = ph.shape[0]
    g = np.random.default_rng(5)
    word = np.concatenate([np.arange(V), g.integers(0, V, 60), [-1, -1]]).astype(np.int64)
    doc = g.integers(-1, th.shape[0], word.size).astype(np.int64)
    doc[:3] = -1                                             # the default theta
    rows = torch.from_numpy(np.unique(word[word >= 0]))
    seg = S.field_segments(V, torch.from_numpy(keys), FIELDS, rows, "cpu")
    at = np.searchsorted(rows.numpy(), np.maximum(word, 0))
    grow = np.where(word[:, None] >= 0, seg.grow.numpy()[at], -1)
    grow[5, 1] = -1                                          # a field without a group
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)      # noqa: E731
    best, pbest, above = R.expect_sides(t(th, torch.float64), t(ph, torch.float64), seg.order, seg.seg_start,
                                        seg.seg_end, t(doc, torch.int32), t(word, torch.int32), t(grow, torch.int32),
                                        0.25)
    assert best.dtype == torch.int32 and above.dtype == torch.int32 and pbest.dtype == torch.float64
    ex_pos = [i for i, f in enumerate(FIELDS) if f[2]]
    seen = dict(tie=0, nan=0, zero=0, dflt=0, solo=0, modal=0, beaten=0)
    for i, (d, w) in enumerate(zip(doc.tolist(), word.tolist())):
        want = oracle_side(th, ph, 0.25, grp, stride, FIELDS, keys, d, w, python=True)
        if want is None:
            assert best[i].tolist() == [-1] * 3 and above[i].tolist() == [-1] * 3 and torch.isnan(pbest[i]).all()
            continue
        fast = oracle_side(th, ph, 0.25, grp, stride, FIELDS, keys, d, w)
        s = dot_py((th[d] if d >= 0 else np.full(th.shape[1:], 0.25)).tolist(), ph[w].tolist())
        sc = R.score_ensemble(t(th, torch.float64), t(ph, torch.float64), R_, 4, 0.25, t(doc[i:i + 1], torch.int32),
                              t(word[i:i + 1], torch.int32))[0].item()
        assert same(s, sc)                                   # the oracle's dot is the scorer's
        for f in range(3):
            if i == 5 and f == 1:
                assert best[i, f].item() == -1 and above[i, f].item() == -1 and pbest[i, f].item() != pbest[i, f].item()
                continue
            b, pb, ab, lift = want[f]
            assert all(same(x, y) for x, y in zip(want[f], fast[f]))      # the two forms of the oracle agree
            assert (best[i, f].item(), above[i, f].item()) == (b, ab) and same(pbest[i, f].item(), pb), (i, f)
            mem = group_of(grp, stride, FIELDS, keys, w, ex_pos[f])
            if s != s:                                       # the word's own row is the NaN row
                assert ab == 0 and lift != lift
                seen["nan"] += 1
                continue
            if s == 0.0:                                     # the row of -0.0: a lift over 0 is inf or NaN
                assert (ab == 0) == (pb == 0.0) and not lift < 1.0
                seen["zero"] += 1
                continue
            # the invariants
            assert (ab == 0) == (pb == s) == (lift == 1.0) and lift >= 1.0
            assert b in mem and w in mem
            kb, kw = int(keys[b]), int(keys[w])
            for j in range(len(FIELDS)):                     # best differs from w in digit f only
                if j != ex_pos[f]:
                    assert (kb // stride[j]) % FIELDS[j][1] == (kw // stride[j]) % FIELDS[j][1]
            if len(mem) == 1:
                assert b == w and ab == 0
                seen["solo"] += 1
            seen["modal" if ab == 0 else "beaten"] += 1
            seen["dflt"] += d < 0
            if mem == big and f == 1 and b in (big[0], big[2]):
                assert b == big[0]                           # the duplicate rows tie: the lowest row
                seen["tie"] += 1
            if other[0][0] in mem and f == 0:
                assert b != other[0][0]
            if other[1][0] in mem and f == 0:
                assert pb > 0.0 and b != other[1][0]         # the group's other rows beat its zero
    assert all(v > 0 for k, v in seen.items() if k != "tie"), seen
    # the tie, made certain: a document whose best member of the big group is the duplicated row
    pd = dots_np(th[0], ph[big])
    ph[big[0]] = ph[big[2]] = ph[big[int(np.argmax(pd))]] * 2.0
    best2, _, above2 = R.expect_sides(t(th, torch.float64), t(ph, torch.float64), seg.order, seg.seg_start,
                                      seg.seg_end, t([0, 0], torch.int32), t([big[2], big[1]], torch.int32),
                                      t(seg.grow.numpy()[[big[2], big[1]]], torch.int32), 0.25)
    assert best2[:, 1].tolist() == [big[0], big[0]] and above2[0, 1].item() == 0 and above2[1, 1].item() == 2
    # slabs change nothing
    small = R.expect_sides(t(th, torch.float64), t(ph, torch.float64), seg.order, seg.seg_start, seg.seg_end,
                           t(doc, torch.int32), t(word, torch.int32), t(grow, torch.int32), 0.25, slab=7)
    full = R.expect_sides(t(th, torch.float64), t(ph, torch.float64), seg.order, seg.seg_start, seg.seg_end,
                          t(doc, torch.int32), t(word, torch.int32), t(grow, torch.int32), 0.25)
    for a, b in zip(small, full):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                  b.view(torch.int64) if b.dtype == torch.float64 else b)


def test_twin_edges():
    th = torch.ones(1, 1, 1, dtype=torch.float64)
    ph = torch.tensor([[[0.5]], [[NAN]], [[-0.0]], [[0.0]], [[0.5]]], dtype=torch.float64)
    order = torch.tensor([4, 0, 1, 2, 3], dtype=torch.int32)      # not ascending: the tie rule is by row
    s, e = torch.tensor([0, 2, 3, 5, 2]), torch.tensor([2, 3, 5, 5, 5])
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)      # noqa: E731
    doc, word = i32([0, 0, 0, 0, -1, 0]), i32([4, 1, 3, 0, 2, -1])
    grow = i32([[0], [1], [2], [3], [4], [0]])
    best, pbest, above = R.expect_sides(th, ph, order, s, e, doc, word, grow, 2.0)
    assert best[:, 0].tolist() == [0, -1, 2, -1, 2, -1]      # tie 4 / 0 -> 0; all NaN; -0.0 ties +0.0 -> row 2; empty
    assert above[:, 0].tolist() == [0, 0, 0, 0, 0, -1]
    assert pbest[0, 0].item() == 0.5 and pbest[1, 0].item() != pbest[1, 0].item() and pbest[3, 0].item() != pbest[3, 0].item()
    assert pbest[2, 0].item() == 0.0 and pbest[4, 0].item() == 0.0      # default theta 2.0 * -0.0: a zero
    none = R.expect_sides(th, ph, order, s, e, doc[:0], word[:0], grow[:0], 2.0)
    assert [tuple(x.shape) for x in none] == [(0, 1)] * 3
    for bad in (dict(doc=i32([1])), dict(word=i32([5])), dict(grow=i32([[5]])), dict(word=i32([-2]))):
        kw = dict(doc=i32([0]), word=i32([0]), grow=i32([[0]]))
        kw.update(bad)
        with pytest.raises(ValueError):
            R.expect_sides(th, ph, order, s, e, kw["doc"], kw["word"], kw["grow"], 2.0)
    with pytest.raises(ValueError):
        R.expect_sides(th, ph, order, torch.tensor([3]), torch.tensor([2]), i32([0]), i32([0]), i32([[0]]), 2.0)
    with pytest.raises(ValueError):
        R.expect_sides(th, ph, i32([5]), torch.tensor([0]), torch.tensor([1]), i32([0]), i32([0]), i32([[0]]), 2.0)


def test_field_groups_is_field_segments_summed():
    keys, th, ph, *_ = small_tables()
    ph = np.nan_to_num(ph)
    model = S.TopicModel.build(th[:, 0], ph[:, 0], 0.25, "cpu")
    rows = torch.arange(0, 70, 3)
    gsum, grow, sizes = S.field_groups(model, torch.from_numpy(keys), FIELDS, rows)
    seg = S.field_segments(70, torch.from_numpy(keys), FIELDS, rows, "cpu")
    g2, grow2, sizes2 = S.field_groups(model, None, FIELDS, rows, segments=seg)
    assert torch.equal(grow, seg.grow) and torch.equal(sizes, seg.sizes) and torch.equal(grow, grow2)
    assert torch.equal(gsum.view(torch.int64), g2.view(torch.int64)) and torch.equal(sizes, sizes2)
    grp, stride = groups_of(keys, FIELDS)
    for i, w in enumerate(rows.tolist()):
        for f, pos in enumerate([0, 1, 3]):
            g = int(grow[i, f])
            mem = seg.order[int(seg.seg_start[g]):int(seg.seg_end[g])].tolist()
            assert [m for m in mem] == group_of(grp, stride, FIELDS, keys, w, pos) and int(sizes[i, f]) == len(mem)


# ---------------------------------------------------------------------------------------- end to end
ALL = ["flow-strict", "flow-fixed", "dns-strict", "dns-fixed", "proxy-fixed"]
_DAYS = {}


def get_day(which, tmp_path_factory):
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("expect_" + kind + compat))
    return _DAYS[which]


def read_expect(day, lp):
    """Per line: (key text, [per side (doc, word, score text, [(expected, lift text, above text)] per field)]) and
    the explained field names."""
    _, fields = C.load_word_fields(str(lp))
    names = [n for n, _, e in fields if e]
    F = len(names)
    sep, sides = SIDES[day.kind]
    lines = (lp / f"{day.kind}_expect.csv").read_text(encoding="utf-8").split("\n")
    assert lines[-1] == ""
    out = []
    w = 3 + 3 * F
    for ln in lines[:-1]:
        f = ln.split(sep)
        assert len(f) == 1 + len(sides) * w
        out.append((f[0], [(f[1 + j * w], f[2 + j * w], f[3 + j * w],
                            [tuple(f[4 + j * w + 3 * k:7 + j * w + 3 * k]) for k in range(F)])
                           for j in range(len(sides))]))
    return out, names


def check_day(day, lp, summary, members=1):
    """The expect file against the results file line for line, and against the oracle over the written tables and
    word_fields.npz: names, lifts (the parsed text is the oracle's double) and counts.  Returns the largest group."""
    rows, names = read_expect(day, lp)
    sep, sides = SIDES[day.kind]
    res = [ln.split(sep) for ln in (lp / day.results).read_text(encoding="utf-8").split("\n")[:-1]]
    assert len(res) == len(rows) == summary["scored"] > 20
    for f, (key, ss) in zip(res, rows):
        assert [s[:3] for s in ss] == [(f[c[0]], f[c[1]], f[c[2]]) for c in sides]
        assert float(key) == min(float(s[2]) for s in ss)
    dn, wn, th, ph = _tables(lp, members)
    th, ph = th.numpy(), ph.numpy()
    K = th.shape[2]
    keys, fields = C.load_word_fields(str(lp))
    assert keys.size == len(wn) and [n for n, _, e in fields if e] == names == summary["expect_fields"]
    grp, stride = groups_of(keys, fields)
    di = {n: i for i, n in enumerate(dn)}      # later duplicates win, as the scorers' maps
    wi = {n: i for i, n in enumerate(wn)}
    modal = [0] * len(names)
    pairs, dots, largest, checked, cache = set(), 0, 0, 0, {}
    for _, ss in rows:
        for doc, word, score, cells in ss:
            w, d = wi.get(word, -1), di.get(doc, -1)
            if w < 0:
                assert all(c == ("", "", "") for c in cells)
                continue
            if (d, w) not in cache:
                cache[(d, w)] = oracle_side(th, ph, day.default(K), grp, stride, fields, keys, d, w)
                dots += sum(len(group_of(grp, stride, fields, keys, w, i)) for i, f in enumerate(fields) if f[2])
            s = float(score)
            for k, ((b, pb, ab, _), (name, lift, above)) in enumerate(zip(cache[(d, w)], cells)):
                assert name == wn[b] and int(above) == ab, (doc, word, k)
                assert float(lift) == pb / s and float(lift) >= 1.0 and (ab == 0) == (float(lift) == 1.0) == (pb == s)
                modal[k] += ab == 0
            largest = max([largest] + [len(group_of(grp, stride, fields, keys, w, i))
                                       for i, f in enumerate(fields) if f[2]])
            checked += 1
    assert checked > 20
    assert summary["expect_modal_hist"] == dict(zip(names, modal)) and list(summary["expect_modal_hist"]) == names
    assert summary["expect_pairs"] == len(cache) and summary["expect_member_dots"] == dots
    return largest


NEW = {"expect_fields", "expect_modal_hist", "expect_pairs", "expect_member_dots", "expect_path"}


@pytest.mark.parametrize("which", ALL)
def test_day_with_expect(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    plain, sp = day.run("plain")
    ex, se = day.run("explain", explain=True)
    lp, s = day.run("expect", expect=True)
    a, b = tree(ex), tree(lp)
    assert set(b) - set(a) == {f"{day.kind}_expect.csv"} and set(a) <= set(b)
    for f in a:      # <type>_explain.csv and every other file: the --explain run's bytes
        assert a[f] == b[f], f
    assert not list(plain.glob("*_expect.csv")) and not list(ex.glob("*_expect.csv"))
    assert not NEW & set(sp) and not NEW & set(se) and {k for k in s if k not in se} == NEW
    assert s["expect_path"] == "cpu"
    recs = [json.loads(x) for x in (lp / "metrics.jsonl").read_text().splitlines()]
    det = [r for r in recs if r.get("stage") == f"{day.kind}_post_detail" and "expect_pairs" in r]
    assert len(det) == 1 and det[0]["expect_modal_hist"] == s["expect_modal_hist"]
    post = [r for r in recs if r.get("stage") == f"{day.kind}_post"]
    assert post and post[-1]["expect_member_dots"] == s["expect_member_dots"] > 0
    assert not any("expect_pairs" in json.loads(x) for x in (ex / "metrics.jsonl").read_text().splitlines())
    check_day(day, lp, s)
    # --explain together with --expect is --expect
    both, sb = day.run("both", explain=True, expect=True)
    assert tree(both) == b


@pytest.mark.parametrize("compat", ["strict", "fixed"])
def test_a_day_whose_groups_pass_one_block(compat, tmp_path_factory):
    day = Day("flow", compat, tmp_path_factory.mktemp("expect_big_" + compat), scale=BIG["scale"])
    lp, s = day.run("expect", expect=True, cuts=BIG["cuts"])
    assert check_day(day, lp, s) > CFG.GROUP_BLOCK == 256
    assert max(s["explain_max_group"].values()) > CFG.GROUP_BLOCK
    ex, _ = day.run("explain", explain=True, cuts=BIG["cuts"])
    assert (ex / "flow_explain.csv").read_bytes() == (lp / "flow_explain.csv").read_bytes()
    assert (ex / day.results).read_bytes() == (lp / day.results).read_bytes()


@pytest.mark.parametrize("which", ["flow-strict", "dns-fixed", "proxy-fixed"])
def test_max_results_host_report_ensemble_and_tail_tol(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp, s = day.run("expect", expect=True)
    name = f"{day.kind}_expect.csv"
    full = (lp / name).read_bytes().splitlines(keepends=True)
    N = s["scored"] // 3
    lim, sl = day.run("expect_lim", expect=True, max_results=N)
    assert (lim / name).read_bytes() == b"".join(full[:N]) and N > 5
    assert all(v <= N * len(SIDES[day.kind][1]) for v in sl["expect_modal_hist"].values())
    # the host report is what it is without the flag, and its rows are not described
    h0, _ = day.run("hosts", host_report=-1)
    h1, _ = day.run("hosts_expect", host_report=-1, expect=True)
    assert (h0 / f"{day.kind}_hosts.csv").read_bytes() == (h1 / f"{day.kind}_hosts.csv").read_bytes()
    assert (h1 / name).read_bytes() == b"".join(full)
    # --ensemble 3: p_v is the members' mean, as the score is
    ens, se = day.run("expect_ens3", expect=True, ensemble=3)
    check_day(day, ens, se, members=3)
    assert (ens / day.results).read_bytes() == (day.run("ens3", ensemble=3)[0] / day.results).read_bytes()
    # --tail-tol: other rows, in another order; the same definition
    tt, st = day.run("expect_tailtol", expect=True, tail_tol=1.0, max_results=150)
    check_day(day, tt, st)
    assert st["scored"] == 150
    t0, _ = day.run("tailtol", tail_tol=1.0, max_results=150)
    assert (t0 / day.results).read_bytes() == (tt / day.results).read_bytes()
    assert (t0 / f"{day.kind}_tail.csv").read_bytes() == (tt / f"{day.kind}_tail.csv").read_bytes()


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_resume_writes_the_same_expect_file(which, tmp_path_factory):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)
    name = f"{day.kind}_expect.csv"
    want = (day.run("expect", expect=True)[0] / name).read_bytes()
    lp = day.root / "resume"
    day.go(day.cfg(lp, expect=True))
    post = f"{day.kind}_post"
    ex = lp / name
    assert ex.read_bytes() == want
    go = lambda **kw: run(day.cfg(lp, resume=True, **kw).validate(), device="cpu", log=lambda *a: None)      # noqa: E731
    stages = [post, "lda_post", "lda", "lda_pre", f"{day.kind}_pre"]
    for upto in range(1, len(stages) + 1):      # resumed at the scoring stage, at lda_post, at lda, ...
        for st in stages[:upto]:
            p = lp / ".stages" / f"{st}.done"
            if p.exists():
                os.unlink(p)
        os.unlink(ex)
        go(expect=True)
        assert ex.read_bytes() == want, stages[upto - 1]
    # a run with --explain alone, resumed at the scoring stage with --expect: word_fields.npz is there
    lp2 = day.root / "resume_add"
    day.go(day.cfg(lp2, explain=True))
    assert not (lp2 / name).exists()
    os.unlink(lp2 / ".stages" / f"{post}.done")
    run(day.cfg(lp2, resume=True, expect=True).validate(), device="cpu", log=lambda *a: None)
    assert (lp2 / name).read_bytes() == want
    # a plain run has no word_fields.npz: refused before any stage runs, nothing written
    lp3 = day.root / "resume_plain"
    day.go(day.cfg(lp3))
    os.unlink(lp3 / ".stages" / f"{post}.done")
    before, marks = tree(lp3), sorted(os.listdir(lp3 / ".stages"))
    with pytest.raises(ValueError, match="word_fields.npz"):
        run(day.cfg(lp3, resume=True, expect=True).validate(), device="cpu", log=lambda *a: None)
    assert tree(lp3) == before and sorted(os.listdir(lp3 / ".stages")) == marks and not (lp3 / name).exists()


@pytest.mark.parametrize("which", ["flow-strict", "proxy-fixed"])
def test_refusals_write_nothing(which, tmp_path_factory, monkeypatch):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)

    class Group:
        active, rank, world_size = True, 0, 2
    never = day.root / "never"
    assert CFG.RunConfig().expect is False and CFG.EXPECT_ONE_PROCESS.startswith("--expect")
    for kw in (dict(gpus=2), dict(hdfs=True)):
        with pytest.raises(ValueError, match="one process"):
            day.cfg(never, expect=True, **kw).validate()
        with pytest.raises(ValueError, match="one process"):
            run(day.cfg(never, expect=True, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, expect=True), dist=Group(), device="cpu")
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("EXPECT", raising=False)
    monkeypatch.delenv("EXPLAIN", raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    mine = "one process" if day.kind == "proxy" else "--expect runs on one process"      # (proxy refuses first)
    for extra in (["--expect", "--gpus", "2"], ["--expect", "--hdfs"]):
        with pytest.raises(ValueError, match=mine):
            cli.cmd_ml_ops(base + extra)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match=mine):
        cli.cmd_ml_ops(base + ["--expect"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("EXPECT", "1")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    assert not never.exists()


def test_a_fresh_run_removes_what_an_earlier_expect_run_left(tmp_path):
    for f in ("flow_expect.csv", "dns_expect.csv", "flow_explain.csv", "flow_scores.csv", "flow_results.csv"):
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
    monkeypatch.delenv("EXPECT", raising=False)
    monkeypatch.delenv("EXPLAIN", raising=False)
    conf = tmp_path / "duxbay.conf"
    conf.write_text("FLOW_PATH=/a\nEXPECT=1\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].expect is False
    assert cli.cmd_ml_ops(base + none + ["--expect"]) == 0 and seen["cfg"].expect is True
    assert seen["cfg"].explain is False and seen["cfg"].validate().explain is True      # implied once validated
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].expect is True
    monkeypatch.setenv("EXPECT", "0")
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0 and seen["cfg"].expect is False      # environment over file
    monkeypatch.setenv("EXPECT", "1")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].expect is True
    assert "EXPECT" in CFG.ENV_KEYS
