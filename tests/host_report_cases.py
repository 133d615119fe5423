"""Shared by tests/test_host_report.py (CPU) and tests/test_host_report_gpu.py: the seeded inputs of
``host_summary`` (key sets x sizes x document shapes, one- and two-sided), the literal oracle, and the checks of
a ``<type>_hosts.csv`` against the results file and the input.  Not a test module."""
import os

import numpy as np
import torch

KEYSETS = ["log_uniform", "five_values", "all_equal", "low_bits", "signed_mix", "nan_mix"]
SHAPES = ["one", "seven", "third", "zipf", "tenth_skipped", "all_skipped", "unnamed"]
RAGGED = 34 * 2048 + 371           # ~70 k events: many workgroups, the last one partial
SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, RAGGED]


def _bits(x):
    return np.asarray(x, np.uint64).view(np.float64)


def _scores(name, n, rng):
    """(scores float64 [n], TOL) of one key set."""
    if name == "log_uniform":                                    # scaled like the scorers' keys
        return 10.0 ** rng.uniform(-9, -2, n), 1e-4
    if name == "five_values":                                    # minima tie
        return rng.choice(np.array([1e-7, 3e-6, np.nextafter(3e-6, 1.0), 2e-4, 5e-3]), n), 1e-4
    if name == "all_equal":
        return np.full(n, 1.25e-5), 1e-4
    if name == "low_bits":                                       # only the lowest mantissa bits separate the keys
        return 1.0 + rng.integers(0, max(n, 1), n) * 2.0 ** -52, 1.0 + (n // 2) * 2.0 ** -52
    if name == "signed_mix":
        vals = np.array([-0.0, 0.0, -1.5, -1e-300, 5e-324, -5e-324, 1.1e-308, -1.1e-308, 1.0, 7e-4, np.inf, -np.inf])
        return rng.choice(vals, n), 1e-4
    if name == "nan_mix":                                        # NaN of either sign: never under TOL, never a minimum
        s = 10.0 ** rng.uniform(-9, -2, n)
        nan = rng.random(n) < 0.4
        s[nan] = np.where(rng.random(int(nan.sum())) < 0.5, np.nan, _bits(np.uint64(0xFFF8000000000123)))
        return s, 1e-4
    raise KeyError(name)


def _docs(shape, n, rng):
    """(doc int32 [n], D) of one document shape."""
    if shape == "one":
        return np.zeros(n, np.int32), 1
    if shape == "seven":
        return rng.integers(0, 7, n).astype(np.int32), 7
    D = max(1, n // 3)
    if shape == "third":
        return rng.integers(0, D, n).astype(np.int32), D
    if shape == "zipf":                                          # one document takes half of the sides
        d = rng.integers(0, D, n)
        d[rng.random(n) < 0.5] = D // 2
        return d.astype(np.int32), D
    if shape == "tenth_skipped":
        d = rng.integers(0, D, n)
        d[rng.random(n) < 0.1] = -1
        return d.astype(np.int32), D
    if shape == "all_skipped":
        return np.full(n, -1, np.int32), 5
    if shape == "unnamed":                                       # the odd rows and the tail are documents no side names
        return (2 * rng.integers(0, D, n)).astype(np.int32), 2 * D + 3
    raise KeyError(shape)


def case(keyset, shape, n, two):
    """(doc_a, score_a, doc_b | None, score_b | None, D, tol) as numpy arrays, seeded by the case.  Two-sided: every
    fifth event has both sides on one document, every tenth of them also the same score on both."""
    rng = np.random.default_rng([KEYSETS.index(keyset), SHAPES.index(shape), n, int(two)])
    sa, tol = _scores(keyset, n, rng)
    da, D = _docs(shape, n, rng)
    if not two:
        return da, np.ascontiguousarray(sa), None, None, D, float(tol)
    sb, _ = _scores(keyset, n, rng)
    db, _ = _docs(shape, n, rng)
    i = np.arange(n)
    db = np.where(i % 5 == 0, da, db).astype(np.int32)
    sb = np.where(i % 10 == 0, sa, sb)
    return da, np.ascontiguousarray(sa), db, np.ascontiguousarray(sb), D, float(tol)


def order_key(x: float) -> int:
    """The order of the scores as a Python int: IEEE bits, negatives with every bit flipped, the others with the
    sign bit set (-0.0 just below +0.0)."""
    b = int(np.float64(x).view(np.uint64))
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def oracle(doc_a, score_a, doc_b, score_b, D, tol):
    """The definition applied side by side, in side-number order: (events, flagged, min_score, worst, skipped)."""
    events, flagged = np.zeros(D, np.int64), np.zeros(D, np.int64)
    min_score, worst = np.full(D, np.inf), np.full(D, -1, np.int64)
    best = [None] * D
    skipped = 0
    sides = [(doc_a, score_a)] + ([(doc_b, score_b)] if doc_b is not None else [])
    for i in range(len(doc_a)):
        for side, (doc, score) in enumerate(sides):
            d, s = int(doc[i]), float(score[i])
            if d == -1:
                skipped += 1
                continue
            events[d] += 1
            if s < tol:
                flagged[d] += 1
            if s != s:
                continue
            k = order_key(s)
            if best[d] is None or k < best[d]:      # an equal key keeps the earlier side
                best[d], min_score[d], worst[d] = k, s, 2 * i + side
    return events, flagged, min_score, worst, skipped


def tensors(c, device="cpu"):
    """The torch arguments of ``host_summary`` for a ``case``."""
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)      # noqa: E731
    return t(c[0]), t(c[1]), t(c[2]), t(c[3]), c[4], c[5]


def same(got, want):
    """Exact equality of two host_summary results (min_score by its bits: -0.0 is not +0.0)."""
    for name, g, w in zip(("events", "flagged", "min_score", "worst"), got[:4], want[:4]):
        g = g.cpu().numpy() if torch.is_tensor(g) else np.asarray(g)
        w = w.cpu().numpy() if torch.is_tensor(w) else np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.int64) != w.view(np.int64))
        assert bad.size == 0, (name, bad[:5], g[bad[:5]], w[bad[:5]])
    assert int(got[4]) == int(want[4]), ("skipped", got[4], want[4])


# --------------------------------------------------------------------------------------- the hosts file
# per type: separator, fields of a results line, (ip field, score field) of every side
LAYOUT = {"flow": (",", 37, ((8, 35), (9, 36))), "dns": (",", 16, ((3, 15),)), "proxy": ("\t", 21, ((2, 20),))}


def input_counts(kind, gen) -> dict:
    """ip -> sides in the day's input (the rows the loader keeps), read with the loaders only."""
    from collections import Counter
    c = Counter()
    if kind == "flow":
        from oni_ml_amd.features import flow as FF
        ft = FF.load_flow(gen, None, 1000, 2)
        for ln in _flow_rows(gen):
            f = ln.split(",")
            c[f[8]] += 1
            c[f[9]] += 1
        assert sum(c.values()) == 2 * ft.n_raw
    elif kind == "dns":
        from oni_ml_amd.features import dns as FD
        tab = FD.load_dns(gen["dns_path"], None, 1000, strict=False)
        c.update(tab.column("ip_dst", tab.n_raw).to_pylist())
    else:
        from oni_ml_amd.features import proxy as FP
        c.update(FP.load_proxy(gen["proxy_path"]).column("clientip").to_pylist())
    return c


def _flow_rows(indir):
    """The data lines of the day's CSV parts (27 fields; the header of every part skipped)."""
    for name in sorted(os.listdir(indir)):
        with open(os.path.join(indir, name)) as f:
            header = f.readline()
            for ln in f:
                if ln != header and ln.count(",") == 26:
                    yield ln.rstrip("\n")


def check_hosts_file(kind, lpath, tol, counts, limit=None):
    """The hosts file of an unlimited-results run against the results file's text and the input: lines ascend
    and are under TOL, every tail is a results line, ``flagged`` and the minimum equal a recount of the results
    file, ``events`` the input's count, and the listed hosts are exactly the IPs with a side under TOL (the
    first ``limit`` of them).  Returns the hosts file's lines."""
    sep, width, sides = LAYOUT[kind]
    res = open(os.path.join(lpath, f"{kind}_results.csv"), encoding="utf-8").read().split("\n")
    assert res[-1] == ""
    res = res[:-1]
    flagged, lowest = {}, {}
    for ln in res:
        f = ln.split(sep)
        assert len(f) == width, (len(f), ln)
        for ip_col, sc_col in sides:
            s = float(f[sc_col])
            if s < tol:
                ip = f[ip_col]
                flagged[ip] = flagged.get(ip, 0) + 1
                lowest[ip] = min(lowest.get(ip, np.inf), s)
    lines = open(os.path.join(lpath, f"{kind}_hosts.csv"), encoding="utf-8").read().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    head = 4 + (len(sides) == 2)
    rows = set(res)
    seen, scores = [], []
    for ln in lines:
        f = ln.split(sep, head)
        assert len(f) == head + 1, ln
        ip, ev, fl, lo = f[0], int(f[1]), int(f[2]), float(f[3])
        assert f[head] in rows, ln
        assert fl == flagged.get(ip) and lo == lowest[ip], (ip, fl, lo, flagged.get(ip), lowest.get(ip))
        assert ev == counts[ip] and ev >= fl >= 1, (ip, ev, counts[ip])
        w = f[head].split(sep)
        if len(sides) == 2:      # the worst event's own side scored the minimum, on this host
            ip_col, sc_col = sides[("src", "dst").index(f[4])]
            assert w[ip_col] == ip and float(w[sc_col]) == lo, ln
        else:
            assert w[sides[0][0]] == ip and float(w[sides[0][1]]) == lo, ln
        seen.append(ip)
        scores.append(lo)
    assert scores == sorted(scores) and (not scores or scores[-1] < tol)
    assert len(set(seen)) == len(seen)
    if limit is None:
        assert set(seen) == set(flagged), (len(seen), len(flagged))
    else:
        assert len(seen) == min(limit, len(flagged)) and set(seen) <= set(flagged)
    return lines
