"""--topic-match / --topic-match-day on the CPU: the ``column_l1`` twin against a literal double loop of its
definition, ``native.assign_min`` against brute force over all permutations, a planted alignment, and small flow,
DNS and proxy days (the days of tests/test_ensemble.py): an ensemble's members matched to member 0, a copy of the
run's own work directory as the previous day (identity, every distance and drift exactly 0.0), another seed, another
topic count, the run without the flags, a resumed scoring stage, stale files and the refusals."""
import itertools
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble import Day, bits_equal, tree  # noqa: E402

from oni_ml_amd import cli  # noqa: E402
from oni_ml_amd import config as CFG  # noqa: E402
from oni_ml_amd.ops import native  # noqa: E402
from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.pipeline import common as C  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

FILES = ("topic_match", "topic_stability", "host_drift")


# ---------------------------------------------------------------------------------------- the twin
def literal(A, B, ia, ib, block):
    """The definition in numpy scalars: blocks of ``block`` pairs, each from 0.0 in pair order, the block sums from
    0.0 in block order."""
    A, B = A.numpy(), B.numpy()
    M = A.shape[0] if ia is None else len(ia)
    out = np.zeros((A.shape[1], B.shape[1]), np.float64)
    with np.errstate(invalid="ignore"):
        for a in range(A.shape[1]):
            for b in range(B.shape[1]):
                total = np.float64(0.0)
                for m0 in range(0, M, block):
                    part = np.float64(0.0)
                    for m in range(m0, min(m0 + block, M)):
                        x = A[m if ia is None else int(ia[m]), a]
                        y = B[m if ib is None else int(ib[m]), b]
                        part = part + np.abs(np.float64(x - y))
                    total = total + part
                out[a, b] = total
    return torch.from_numpy(out)


def l1_case(M, Wa, Wb, seed=0, Va=None, Vb=None, special=True):
    """Tables and index arrays with repeats and no order; ``special``: signed zeros, an inf pair (inf - inf: NaN) and
    a NaN in the last columns' first rows (only where the table is wide enough to keep a clean column)."""
    g = torch.Generator().manual_seed(1000 * M + 10 * Wa + Wb + seed)
    Va, Vb = Va or max(M, 1) + 2, Vb or max(M, 1) + 3
    A = torch.randn(Va, Wa, generator=g, dtype=torch.float64)
    B = torch.randn(Vb, Wb, generator=g, dtype=torch.float64)
    ia = torch.randint(0, Va, (M,), generator=g, dtype=torch.int64)
    ib = torch.randint(0, Vb, (M,), generator=g, dtype=torch.int64)
    if special and M:
        A[int(ia[0]), 0] = -0.0
        B[int(ib[0]), 0] = 0.0
        if Wa > 1 and Wb > 1:
            A[int(ia[-1]), Wa - 1] = float("inf")
            B[int(ib[-1]), Wb - 1] = float("inf")
        if Wa > 2:
            A[int(ia[M // 2]), Wa - 2] = float("nan")
    return A, B, ia, ib


@pytest.mark.parametrize("block", [1, 4])
@pytest.mark.parametrize("M", [0, 1, 5, 9])
def test_twin_against_the_literal_definition(M, block):
    seen_nan = False
    for Wa, Wb in itertools.product((1, 2, 3), repeat=2):
        A, B, ia, ib = l1_case(M, Wa, Wb)
        got = R.column_l1(A, B, ia, ib, block=block)
        assert got.shape == (Wa, Wb) and got.dtype == torch.float64
        assert bits_equal(got, literal(A, B, ia, ib, block)), (M, Wa, Wb, block)
        seen_nan |= bool(torch.isnan(got).any())
        # the identity form: both tables of M rows
        A2, B2 = A[:M].contiguous(), B[:M].contiguous()
        assert bits_equal(R.column_l1(A2, B2, block=block), literal(A2, B2, None, None, block))
    assert seen_nan == (M > 0)      # the inf pair and the NaN reach the sums
    if M == 0:
        assert not R.column_l1(*l1_case(0, 3, 2), block=block).any()


def test_twin_block_is_part_of_the_bits_and_the_slab_is_not():
    A, B, ia, ib = l1_case(300, 5, 4, special=False)
    want = R.column_l1(A, B, ia, ib, block=7)
    for slab in (1, 20, 41, 1 << 22):
        assert bits_equal(R.column_l1(A, B, ia, ib, block=7, slab=slab), want)
    assert bits_equal(want, literal(A, B, ia, ib, 7))
    assert not bits_equal(want, R.column_l1(A, B, ia, ib, block=300))      # another block: other roundings
    assert torch.allclose(want, R.column_l1(A, B, ia, ib, block=300), rtol=1e-12)
    assert bits_equal(R.column_l1(A, B, ia, ib), R.column_l1(A, B, ia, ib, block=CFG.MATCH_BLOCK))


def test_twin_and_dispatch_refusals():
    A, B, ia, ib = l1_case(5, 2, 2)
    for bad in (lambda: R.column_l1(A.float(), B, ia, ib), lambda: R.column_l1(A, B, ia, None),
                lambda: R.column_l1(A, B, ia, ib[:3]), lambda: R.column_l1(A, B), lambda: R.column_l1(A, B, ia + 100, ib),
                lambda: R.column_l1(A, B, ia, ib - 100), lambda: R.column_l1(A, B, ia, ib, block=0)):
        with pytest.raises(ValueError):
            bad()
    got, path = S.column_l1(A, B, ia, ib)
    assert path == "cpu" and bits_equal(got, R.column_l1(A, B, ia, ib))


# ---------------------------------------------------------------------------------------- assign_min
def brute(cost):
    n = cost.shape[0]
    c = np.where(np.isnan(cost), native.ASSIGN_NAN_COST, cost)
    return min(sum(c[i, p[i]] for i in range(n)) for p in itertools.permutations(range(n)))


def total_of(cost, match):
    c = np.where(np.isnan(cost), native.ASSIGN_NAN_COST, cost)
    return sum(c[i, int(match[i])] for i in range(cost.shape[0]))


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7])
def test_assign_min_against_brute_force(n):
    rng = np.random.default_rng(n)
    cases = [rng.random((n, n)) for _ in range(4)]
    cases += [rng.integers(0, 3, (n, n)).astype(np.float64) * 0.25 for _ in range(4)]      # many exact ties
    cases += [np.zeros((n, n)), np.ones((n, n)), np.eye(n), 1.0 - np.eye(n)]
    withnan = rng.random((n, n))
    withnan[rng.random((n, n)) < 0.3] = np.nan
    cases.append(withnan)
    for cost in cases:
        m = native.assign_min(cost)
        assert m.dtype == np.int64 and sorted(m.tolist()) == list(range(n))
        # quarters and random doubles of this size add without a rounding that could reorder two totals by more
        assert abs(total_of(cost, m) - brute(cost)) <= 1e-12
        assert np.array_equal(m, native.assign_min(cost.copy()))      # deterministic


def test_assign_min_edges_and_nan():
    assert native.assign_min(np.zeros((0, 0))).shape == (0,)
    assert native.assign_min(np.asarray([[3.5]])).tolist() == [0]
    assert native.assign_min(np.asarray([[np.nan]])).tolist() == [0]
    # a NaN counts as 2.0: above any distance, so it is avoided where a real cost is to be had ...
    assert native.assign_min(np.asarray([[np.nan, 0.9], [0.9, np.nan]])).tolist() == [1, 0]
    assert native.assign_min(np.asarray([[np.nan, 1.0], [1.0, 0.1]])).tolist() == [1, 0]      # 2.0 < 2.1
    # ... and below a pair of costs that add to more
    assert native.assign_min(np.asarray([[np.nan, 1.5], [1.5, 0.1]])).tolist() == [0, 1]      # 2.1 < 3.0
    assert native.assign_min(np.full((3, 3), np.nan)).tolist() == [0, 1, 2]
    assert native.assign_min(np.zeros((4, 4))).tolist() == [0, 1, 2, 3]      # ties: the lower column
    for bad in (np.zeros((2, 3)), np.zeros(4), np.asarray([[np.inf, 0.0], [0.0, 1.0]])):
        with pytest.raises(ValueError):
            native.assign_min(bad)


def test_match_topics_unmatched_nearest_and_mutual():
    # today's 2 topics, the other's 3: one of the other's goes to a dummy row
    cost = np.asarray([[0.1, 0.5, 0.1], [0.6, 0.2, 0.05]])
    match, nearest, mutual = C.match_topics(cost)
    assert match.tolist() == [0, -1, 1]           # 0.1 + 0.05 is the least total
    assert nearest.tolist() == [0, 1, 1]
    assert mutual.tolist() == [True, False, True]
    # ties: nearest to the lower a, the row's lowest column to the lower b
    match, nearest, mutual = C.match_topics(np.zeros((2, 2)))
    assert match.tolist() == [0, 1] and nearest.tolist() == [0, 0] and mutual.tolist() == [True, False]
    # a NaN is never the nearest; a column of NaN has none
    match, nearest, mutual = C.match_topics(np.asarray([[np.nan, np.nan], [0.3, np.nan]]))
    assert nearest.tolist() == [1, -1] and sorted(match.tolist()) == [0, 1]
    # the other has fewer topics: one of today's stays unmatched
    match, _, _ = C.match_topics(np.asarray([[0.9], [0.1], [0.5]]))
    assert match.tolist() == [1]


@pytest.mark.parametrize("K,V", [(5, 40), (20, 300)])
def test_planted_alignment(K, V):
    g = torch.Generator().manual_seed(K)
    A = torch.rand(V, K, generator=g, dtype=torch.float64) ** 4
    A = A / A.sum(0, keepdim=True)
    perm = torch.randperm(K, generator=g)
    B = A[:, perm].contiguous()      # the other's topic b is today's perm[b]
    cost = (R.column_l1(A, B) * 0.5).numpy()
    match, nearest, mutual = C.match_topics(cost)
    assert match.tolist() == perm.tolist() and nearest.tolist() == perm.tolist() and mutual.all()
    assert all(cost[int(perm[b]), b] == 0.0 for b in range(K))
    noisy = B * (1.0 + 0.01 * torch.rand(V, K, generator=g, dtype=torch.float64))
    noisy = (noisy / noisy.sum(0, keepdim=True)).contiguous()
    cost = (R.column_l1(A, noisy) * 0.5).numpy()
    match, _, mutual = C.match_topics(cost)
    assert match.tolist() == perm.tolist() and mutual.all()
    assert all(0.0 < cost[int(perm[b]), b] < 0.02 for b in range(K))


# ---------------------------------------------------------------------------------------- days
ALL = ["flow-fixed", "dns-strict", "proxy-fixed"]
_DAYS = {}


def get_day(which, tmp_path_factory):
    if which not in _DAYS:
        kind, compat = which.split("-")
        _DAYS[which] = Day(kind, compat, tmp_path_factory.mktemp("match_" + kind + compat))
    return _DAYS[which]


def rows_of(path, sep):
    with open(path) as f:
        return [line.rstrip("\n").split(sep) for line in f if line.rstrip("\n")]


def sep_of(day):
    return "\t" if day.kind == "proxy" else ","


def read_files(day, lp):
    """{name: rows} of the three files that exist."""
    return {f: rows_of(lp / f"{day.kind}_{f}.csv", sep_of(day)) for f in FILES if (lp / f"{day.kind}_{f}.csv").exists()}


def check_match_file(rows, others, K, Kp=None):
    """Shapes and ranges of <type>_topic_match.csv; returns {other: (match list with None, dist list)}."""
    out = {}
    assert [r[0] for r in rows[::1]] == [o for o in others for _ in range(Kp[o] if Kp else K)]
    for o in others:
        mine = [r for r in rows if r[0] == o]
        assert all(len(r) == 8 for r in mine)
        assert [int(r[1]) for r in mine] == list(range(len(mine)))
        match = [int(r[2]) if r[2] else None for r in mine]
        dist = [float(r[3]) if r[3] else None for r in mine]
        assert all((m is None) == (d is None) for m, d in zip(match, dist))
        assert all(0.0 <= d <= 1.0 for d in dist if d is not None)
        assert all(0.0 <= float(r[5]) <= 1.0 and 0 <= int(r[4]) < K for r in mine)
        assert all(float(r[5]) <= d for r, d in zip(mine, dist) if d is not None)      # the nearest is no farther
        assert all(r[6] in ("0", "1") for r in mine)
        assert all(r[6] == "0" or (m is not None and int(r[4]) == m) for r, m in zip(mine, match))
        assert all(0.0 <= float(r[7]) <= 1.0 + 1e-9 for r in mine)
        out[o] = (match, dist)
    return out


@pytest.mark.parametrize("which", ALL)
def test_members_are_matched_to_member_0(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    lp, s = day.run("ens3m", ensemble=3, topic_match=True)
    files = read_files(day, lp)
    assert sorted(files) == ["topic_match", "topic_stability"]      # no day: no drift file
    K = 20
    got = check_match_file(files["topic_match"], ["m1", "m2"], K)
    for o in ("m1", "m2"):
        assert sorted(got[o][0]) == list(range(K))      # a bijection on the topics
    st = files["topic_stability"]
    assert len(st) == K and all(len(r) == 9 for r in st) and [int(r[0]) for r in st] == list(range(K))
    assert all(r[1] == "2" and 0 <= int(r[2]) <= 2 for r in st)
    assert all(0.0 <= float(r[3]) <= float(r[4]) <= 1.0 for r in st)
    assert all(r[5:] == ["", "", "", ""] for r in st)      # no previous day
    for a in range(K):      # mean and max over the members' matched distances, added in member order
        d = [got[o][1][got[o][0].index(a)] for o in ("m1", "m2")]
        assert float(st[a][3]) == ((0.0 + d[0]) + d[1]) / 2.0 and float(st[a][4]) == max(d)
    assert int(sum(int(r[2]) for r in st)) == sum(s["topic_match_mutual"])
    assert s["topic_match"] is True and s["topic_match_day"] == "" and s["topic_match_path"] == "cpu"
    assert len(s["topic_match_pairs"]) == 2 and s["topic_match_pairs"][0] == s["topic_match_pairs"][1] > 0
    assert s["topic_match_shared_words"] is None and s["topic_match_shared_hosts"] is None
    assert s["host_drift_hist"] == {}
    # the distances are the twin's over the written member tables
    t0, t1 = C.load_model_tables(str(lp)), C.load_model_tables(C.member_dir(str(lp), 1))
    cost = (R.column_l1(torch.from_numpy(t0.phi), torch.from_numpy(t1.phi)) * 0.5).numpy()
    for b, (m, d) in enumerate(zip(*got["m1"])):
        assert d == cost[m, b]


@pytest.mark.parametrize("which", ALL)
def test_a_copy_of_the_run_is_the_identity(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    first, _ = day.run("ens3m", ensemble=3, topic_match=True)
    copy = day.root / "copy"
    if not copy.exists():
        shutil.copytree(first, copy)
    lp, s = day.run("ens3day", ensemble=3, topic_match_day=str(copy))
    files = read_files(day, lp)
    assert sorted(files) == sorted(FILES)
    K = 20
    got = check_match_file(files["topic_match"], ["m1", "m2", "prev"], K)
    match, dist = got["prev"]
    assert match == list(range(K)) and all(d == 0.0 for d in dist)
    prev = [r for r in files["topic_match"] if r[0] == "prev"]
    assert all(r[4] == r[1] and float(r[5]) == 0.0 and r[6] == "1" for r in prev)
    # shared_mass: every word is shared, so it is the column total in row order
    t = C.load_model_tables(str(lp))
    V = t.phi.shape[0]
    tot = R.group_rows_sum(torch.from_numpy(t.phi), torch.arange(V), torch.zeros(1, dtype=torch.int64),
                           torch.full((1,), V, dtype=torch.int64)).reshape(-1)
    assert [float(r[7]) for r in prev] == tot.tolist()
    st = files["topic_stability"]
    assert all(r[5] == r[0] and float(r[6]) == 0.0 and r[7] == "1" and float(r[8]) == x for r, x in zip(st, tot.tolist()))
    # the members' lines do not depend on the day
    assert [r for r in files["topic_match"] if r[0] != "prev"] == read_files(day, first)["topic_match"]
    drift = files["host_drift"]
    assert all(len(r) == 4 for r in drift)
    assert sorted(r[0] for r in drift) == sorted(set(t.doc_names))
    assert all(float(r[1]) == 0.0 and r[2] == r[3] for r in drift)
    order = {n: i for i, n in enumerate(t.doc_names)}
    rows = [order[r[0]] for r in drift]
    assert rows == sorted(rows)      # ties follow today's row order
    dom = [int(np.argmax(t.theta[i])) for i in rows]
    assert [int(r[2]) for r in drift] == dom
    assert s["topic_match_day"] == str(copy) and s["topic_match_mutual"][-1] == K
    assert s["topic_match_shared_words"] == s["topic_match_pairs"][-1] == V
    assert s["topic_match_shared_hosts"] == len(drift) and s["topic_match_new_hosts"] == 0
    assert s["host_drift_hist"]["<1e-6"] == len(drift) and sum(s["host_drift_hist"].values()) == len(drift)


@pytest.mark.parametrize("which", ["flow-fixed", "proxy-fixed"])
def test_another_seed_and_another_topic_count(which, tmp_path_factory):
    day = get_day(which, tmp_path_factory)
    K = 20
    other, _ = day.run("seed99", seed=99)
    lp, s = day.run("vs_seed", topic_match_day=str(other))
    files = read_files(day, lp)
    match, dist = check_match_file(files["topic_match"], ["prev"], K)["prev"]
    assert sorted(match) == list(range(K)) and any(d > 0.0 for d in dist)
    drift = [float(r[1]) for r in files["host_drift"]]
    assert drift and all(0.0 <= d <= 1.0 for d in drift) and drift == sorted(drift, reverse=True) and drift[0] > 0.0
    assert all(0 <= int(r[2]) < K and 0 <= int(r[3]) < K for r in files["host_drift"])
    # the drift of the first host, from the written tables and the written matching
    t, p = C.load_model_tables(str(lp)), C.load_model_tables(str(other))
    b_of = {a: b for b, a in enumerate(match)}
    host = files["host_drift"][0][0]
    x, y = t.theta[t.doc_index()[host]], p.theta[p.doc_index()[host]]
    acc = np.float64(0.0)
    for a in range(K):
        acc = acc + np.abs(x[a] - y[b_of[a]])
    assert drift[0] == acc * 0.5
    st = files["topic_stability"]
    assert all(r[1] == "0" and r[2:5] == ["", "", ""] for r in st)      # R = 1: the member cells are empty
    assert [int(r[5]) for r in st] == [b_of[a] for a in range(K)]
    assert s["topic_match_pairs"] == [s["topic_match_shared_words"]] and s["topic_match_new_hosts"] == 0
    # another topic count: |K - K'| topics stay unmatched
    for Kp, name in ((15, "k15"), (23, "k23")):
        if Kp == 23 and day.kind != "flow":
            continue
        odir, _ = day.run(name, topics=Kp)
        lp2, s2 = day.run("vs_" + name, topic_match_day=str(odir))
        f2 = read_files(day, lp2)
        m2, _ = check_match_file(f2["topic_match"], ["prev"], K, Kp={"prev": Kp})["prev"]
        real = [m for m in m2 if m is not None]
        assert len(m2) == Kp and len(real) == min(K, Kp) and len(set(real)) == len(real)
        st2 = f2["topic_stability"]
        assert sum(1 for r in st2 if r[5] == "") == max(0, K - Kp)
        assert all((r[5] == "") == (r[6] == "") == (r[7] == "") for r in st2)
        d2 = [float(r[1]) for r in f2["host_drift"]]
        assert all(0.0 <= d <= 1.0 + 1e-12 for d in d2)
        if Kp > K:      # a host whose previous dominant topic went unmatched has an empty cell
            unmatched = {b for b, m in enumerate(m2) if m is None}
            p2 = C.load_model_tables(str(odir))
            for r in f2["host_drift"]:
                assert (r[3] == "") == (int(np.argmax(p2.theta[p2.doc_index()[r[0]]])) in unmatched)


def test_a_day_with_other_words_and_hosts(tmp_path_factory):
    """The previous day is another synthetic day: words and hosts are joined by name, the rest is unshared mass."""
    day = get_day("dns-strict", tmp_path_factory)
    from oni_ml_amd.synth.dns import generate_dns_day
    g = generate_dns_day(str(day.root / "in2"), events=5000, seed=4, files=2, n_names=700, n_clients=320)
    other = Day.__new__(Day)
    other.__dict__.update(day.__dict__)
    other.paths, other.runs = dict(dns_path=g["dns_path"], top1m=g["top1m"]), {}
    odir, _ = other.run("yesterday")
    lp, s = day.run("vs_yesterday", topic_match_day=str(odir))
    t, p = C.load_model_tables(str(lp)), C.load_model_tables(str(odir))
    files = read_files(day, lp)
    check_match_file(files["topic_match"], ["prev"], 20)
    shared = [n for n in t.word_names if n in p.word_index()]
    assert s["topic_match_shared_words"] == len(shared) and 0 < len(shared)
    hosts = set(t.doc_names) & set(p.doc_names)
    assert s["topic_match_shared_hosts"] == len(hosts) == len(files["host_drift"])
    assert s["topic_match_new_hosts"] == len(set(t.doc_names) - set(p.doc_names))
    assert {r[0] for r in files["host_drift"]} == hosts
    # a distance by hand: shared rows paired by name, the unshared mass of both columns added
    ia = torch.tensor([t.word_index()[n] for n in shared])
    ib = torch.tensor([p.word_index()[n] for n in shared])
    Cm = R.column_l1(torch.from_numpy(t.phi), torch.from_numpy(p.phi), ia, ib)

    def rest(tab, names, known):
        rows = torch.tensor([i for i, n in enumerate(names) if n not in known], dtype=torch.int64)
        return R.group_rows_sum(torch.from_numpy(tab.phi), rows, torch.zeros(1, dtype=torch.int64),
                                torch.full((1,), rows.numel(), dtype=torch.int64)).reshape(-1)
    ua, ub = rest(t, t.word_names, p.word_index()), rest(p, p.word_names, t.word_index())
    cost = ((Cm + ua.unsqueeze(1)) + ub.unsqueeze(0)) * 0.5
    for r in files["topic_match"]:
        assert float(r[3]) == float(cost[int(r[2]), int(r[1])])
        assert float(r[5]) == float(cost[int(r[4]), int(r[1])]) == float(cost[:, int(r[1])].min())


def test_without_the_flags_nothing_changes(tmp_path_factory):
    day = get_day("dns-strict", tmp_path_factory)
    plain, sp = day.run("plain")
    flagged, sf = day.run("plain_match", topic_match=True)
    assert read_files(day, plain) == {}
    tp, tf = tree(plain), tree(flagged)
    new = {f"{day.kind}_topic_match.csv", f"{day.kind}_topic_stability.csv"}
    assert set(tf) - set(tp) == new and {k: v for k, v in tf.items() if k not in new} == tp
    assert set(sf) - set(sp) == set(C.TOPIC_MATCH_KEYS) and not set(sp) & set(C.TOPIC_MATCH_KEYS)
    assert sf["scored"] == sp["scored"] and sf["below_tol"] == sp["below_tol"]
    # no ensemble and no day: no other model, today's topics with empty cells; not an error
    files = read_files(day, flagged)
    assert files["topic_match"] == [] and len(files["topic_stability"]) == 20
    assert all(r[1:] == ["0"] + [""] * 7 for r in files["topic_stability"])
    assert sf["topic_match_pairs"] == [] and sf["topic_match_mutual"] == []
    # nor do they depend on TOL or MAXRESULTS
    few = day.root / "few_match"
    cfg = day.cfg(few, topic_match=True, max_results=5)
    cfg.tol = 1e-4
    day.go(cfg)
    assert read_files(day, few) == files and len(rows_of(few / day.results, sep_of(day))) <= 5


@pytest.mark.parametrize("which", ["flow-fixed", "dns-strict"])
def test_a_resumed_scoring_stage_adds_the_files(which, tmp_path_factory):
    from oni_ml_amd.pipeline import run
    day = get_day(which, tmp_path_factory)
    first, _ = day.run("ens3m", ensemble=3, topic_match=True)
    copy = day.root / "copy"
    if not copy.exists():
        shutil.copytree(first, copy)
    want, _ = day.run("ens3day", ensemble=3, topic_match_day=str(copy))
    lp = day.root / "resumed"
    day.go(day.cfg(lp, ensemble=3))      # a run without the flags ...
    assert read_files(day, lp) == {}
    os.unlink(lp / ".stages" / f"{day.kind}_post.done")      # ... resumed at the scoring stage with them
    os.unlink(lp / day.results)
    logs = []
    run(day.cfg(lp, ensemble=3, topic_match_day=str(copy), resume=True).validate(), device="cpu", log=logs.append)
    text = "\n".join(str(x) for x in logs)
    assert "[stage lda] already complete" in text and "[stage lda_post] already complete" in text
    for f in FILES + (None,):
        name = day.results if f is None else f"{day.kind}_{f}.csv"
        assert (lp / name).read_bytes() == (want / name).read_bytes(), name
    assert "pairs x Wa x Wb" in text


def test_a_fresh_run_removes_stale_files(tmp_path):
    for f in FILES:
        (tmp_path / f"dns_{f}.csv").write_text("x")
    (tmp_path / "dns_scores.csv").write_text("kept")
    cli.clean_workdir(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["dns_scores.csv"]


def test_refusals_write_nothing(tmp_path_factory, monkeypatch):
    from oni_ml_amd.pipeline import run
    day = get_day("dns-strict", tmp_path_factory)
    done, _ = day.run("plain")

    class Group:
        active, rank, world_size = True, 0, 2
    never = day.root / "never"
    empty = day.root / "empty_dir"
    empty.mkdir(exist_ok=True)
    half = day.root / "half_dir"
    half.mkdir(exist_ok=True)
    shutil.copy(done / "doc_results.csv", half / "doc_results.csv")
    cases = [(dict(topic_match=True, gpus=2), "one process"), (dict(topic_match=True, hdfs=True), "one process"),
             (dict(topic_match_day=str(done), gpus=2), "one process"),
             (dict(topic_match_day=str(empty)), "doc_results.csv"), (dict(topic_match_day=str(half)), "word_results.csv"),
             (dict(topic_match_day=str(day.root / "nowhere")), "not found"),
             (dict(topic_match_day=str(never)), "not found")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            day.cfg(never, **kw).validate()
        with pytest.raises(ValueError, match=msg):
            run(day.cfg(never, **kw), device="cpu")
    with pytest.raises(ValueError, match="one process"):
        run(day.cfg(never, topic_match=True), dist=Group(), device="cpu")
    # DIR is the work directory itself, under another spelling too; refused before any stage runs
    before = tree(done)
    for spelling in (str(done), str(done) + "/", str(done / ".." / done.name)):
        with pytest.raises(ValueError, match="own work directory"):
            run(day.cfg(done, topic_match_day=spelling, resume=True), device="cpu")
    assert tree(done) == before
    assert CFG.TOPIC_MATCH_ONE_PROCESS.startswith("--topic-match")
    # the command line refuses before a process group is asked for and before the work directory is made
    monkeypatch.setattr(cli, "_ml_ops_body", lambda a, resolve: pytest.fail("the run was started"))
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TOPIC_MATCH", raising=False)
    monkeypatch.delenv("TOPIC_MATCH_DAY", raising=False)
    base = ["20160122", day.kind, "1e-3", "--conf", str(day.root / "none.conf"), "--lpath", str(never)]
    base += [x for k, v in day.paths.items() for x in ("--" + k.replace("_", "-"), v)]
    for extra, msg in ((["--topic-match", "--gpus", "2"], "one process"), (["--topic-match", "--hdfs"], "one process"),
                       (["--topic-match-day", str(empty)], "doc_results.csv"),
                       (["--topic-match-day", str(never)], "not found")):
        with pytest.raises(ValueError, match=msg):
            cli.cmd_ml_ops(base + extra)
    with pytest.raises(ValueError, match="own work directory"):
        cli.cmd_ml_ops(base[:5] + ["--lpath", str(done)] + base[7:] + ["--topic-match-day", str(done)])
    monkeypatch.setenv("WORLD_SIZE", "2")      # a torchrun launch
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--topic-match"])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.setenv("TOPIC_MATCH", "1")      # set by the environment: the same refusal
    with pytest.raises(ValueError, match="one process"):
        cli.cmd_ml_ops(base + ["--hdfs"])
    assert not never.exists()
    assert day.cfg(never, topic_match_day=str(done)).validate().topic_match is True      # the day implies the option


def test_cli_flag_environment_and_site_file_reach_the_config(monkeypatch, tmp_path):
    seen = {}

    def body(a, resolve):
        seen["cfg"] = resolve(1)
        return 0

    monkeypatch.setattr(cli, "_ml_ops_body", body)
    monkeypatch.setenv("ONI_PREFETCH", "0")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("TOPIC_MATCH", raising=False)
    monkeypatch.delenv("TOPIC_MATCH_DAY", raising=False)
    prev = tmp_path / "prev"
    prev.mkdir()
    for f in ("doc_results.csv", "word_results.csv"):
        (prev / f).write_text("")
    conf = tmp_path / "duxbay.conf"
    conf.write_text(f"FLOW_PATH=/a\nTOPIC_MATCH=1\nTOPIC_MATCH_DAY={prev}\n")
    base = ["20160122", "flow", "1e-3", "--lpath", "/w", "--flow-path", "/a"]
    none = ["--conf", str(tmp_path / "none.conf")]
    assert cli.cmd_ml_ops(base + none) == 0 and not seen["cfg"].topic_match and seen["cfg"].topic_match_day == ""
    assert cli.cmd_ml_ops(base + none + ["--topic-match"]) == 0 and seen["cfg"].topic_match is True
    assert cli.cmd_ml_ops(base + none + ["--topic-match-day", str(prev)]) == 0
    assert seen["cfg"].topic_match_day == str(prev) and seen["cfg"].validate().topic_match is True
    assert cli.cmd_ml_ops(base + ["--conf", str(conf)]) == 0
    assert seen["cfg"].topic_match is True and seen["cfg"].topic_match_day == str(prev)
    monkeypatch.setenv("TOPIC_MATCH", "0")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].topic_match is False
    monkeypatch.setenv("TOPIC_MATCH", "1")
    assert cli.cmd_ml_ops(base + none) == 0 and seen["cfg"].topic_match is True
    assert "TOPIC_MATCH" in CFG.ENV_KEYS and "TOPIC_MATCH_DAY" in CFG.ENV_KEYS
    c = CFG.resolve("20160122", "flow", conf_path=None, environ={"TOPIC_MATCH_DAY": str(prev)})
    assert c.topic_match_day == str(prev)
