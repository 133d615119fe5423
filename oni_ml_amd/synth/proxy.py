"""Synthetic web-proxy day in the 19-column parquet schema of `features/proxy_io.py`, plus the synthetic
top-1m.csv of `synth/dns.py`.

Clients, hosts and user agents are Zipf-distributed; every client browses inside its own window of hours;
hosts are subdomains of the top-list domains; URIs are 20-300 bytes and nearly all distinct (a random session
id in the query); user agents are real-looking strings, commas included.  A small share of requests is
planted as anomalous -- a base64-like 400-2,000-byte query string, a user agent seen once, a host outside the
top list, or an hour the client never uses -- and their row indices are returned.  With ``with_edge_rows`` the
first rows exercise the row rules and the entropy kernel's edge cases (``EDGE_ROWS``).
"""
from __future__ import annotations

import os

import numpy as np

from .dns import POPULAR, SUBS, _rand_label, write_top1m

# the schema of features/proxy_io.py; duration, respcode, uriport, scbytes and csbytes are written as integers
COLUMNS = ["p_date", "p_time", "clientip", "host", "reqmethod", "useragent", "resconttype", "duration", "username",
           "webcat", "referer", "respcode", "uriport", "uripath", "uriquery", "serverip", "scbytes", "csbytes",
           "fulluri"]
REQUIRED = ("p_date", "p_time", "clientip", "host", "fulluri")
METHODS = ["GET", "POST", "CONNECT", "HEAD", "PUT"]
CTYPES = ["text/html", "image/png", "application/json", "text/css", "application/javascript", "image/jpeg",
          "video/mp4", "application/octet-stream"]
WEBCATS = ["Search Engines", "Social Networking", "News", "Business", "Technology", "Shopping", "Streaming Media"]
WORDS = ["index", "images", "static", "api", "v1", "v2", "assets", "js", "css", "user", "account", "search", "news",
         "article", "product", "cart", "media", "video", "thumb", "download", "content", "en", "us", "2016", "01"]
B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
KINDS = ("long_query", "rare_agent", "off_list_host", "odd_hour")

# edge rows (rows 0 .. EDGE_ROWS - 1 when with_edge_rows): row i < 19 has a null in column i (the five
# required columns drop the row, the others print empty), then
EDGE_TAB, EDGE_TIME_RANGE, EDGE_TIME_TEXT, EDGE_EMPTY_URI, EDGE_PORT_HOST, EDGE_LONG_URI, EDGE_UTF8, EDGE_LOW = \
    range(19, 27)
EDGE_ROWS = 27
EDGE_DROPPED = dict(null=len(REQUIRED), time=2, control=1)


def _zipf(rng, n, size, s):
    p = 1.0 / np.arange(1, n + 1) ** s
    p /= p.sum()
    return rng.choice(n, size=size, p=p)


def _agents(rng, n):
    out = []
    for i in range(n):
        v = 40 + i
        kind = i % 3
        if kind == 0:
            out.append(f"Mozilla/5.0 (Windows NT 10.0; Win64; x64) AppleWebKit/537.36 (KHTML, like Gecko) "
                       f"Chrome/{v}.0.{2000 + 7 * i}.{i % 200} Safari/537.36")
        elif kind == 1:
            out.append(f"Mozilla/5.0 (Macintosh; Intel Mac OS X 10_{9 + i % 4}_{i % 6}) AppleWebKit/601.{i % 7}.{i % 9} "
                       f"(KHTML, like Gecko) Version/9.0.{i % 4} Safari/601.{i % 7}.{i % 9}")
        else:
            out.append(f"Mozilla/5.0 (X11; Linux x86_64; rv:{v}.0) Gecko/20100101 Firefox/{v}.0")
    return out


def _paths(rng, n):
    """n URI paths of 2 .. 230 bytes (the whole URI stays within 20 .. 300)."""
    out = []
    for _ in range(n):
        target = int(rng.integers(2, 40)) if rng.random() < 0.7 else int(rng.integers(40, 225))
        p = ""
        while len(p) < target:
            p += "/" + (WORDS[int(rng.integers(len(WORDS)))] if rng.random() < 0.7
                        else _rand_label(rng, int(rng.integers(3, 12))))
        out.append(p[:225] + (".html" if rng.random() < 0.3 else ""))
    return out


def _edge_rows(base: dict) -> dict:
    """The EDGE_ROWS edge rows as {column: list}: copies of ``base`` (a valid row) with one change each."""
    rows = [dict(base) for _ in range(EDGE_ROWS)]
    for i, c in enumerate(COLUMNS):
        rows[i][c] = None
    rows[EDGE_TAB]["useragent"] = "Mozilla/5.0\t(tab inside)"
    rows[EDGE_TIME_RANGE]["p_time"] = "25:00:00"
    rows[EDGE_TIME_TEXT]["p_time"] = "noon"
    rows[EDGE_EMPTY_URI]["fulluri"] = ""
    rows[EDGE_PORT_HOST]["host"] = "login.google.com:443"
    rows[EDGE_PORT_HOST]["reqmethod"] = "CONNECT"
    rows[EDGE_LONG_URI]["fulluri"] = "http://cdn.akamaihd.com/" + "a/" * 2480 + "x" * 16     # 5,000 bytes
    rows[EDGE_UTF8]["fulluri"] = "http://www.wikipedia.org/wiki/café/日本語?q=üß"
    rows[EDGE_LOW]["fulluri"] = "http://www.example.com/a%00b%0a?x=\x01\x02\x7f&y=%ff"
    return {c: [r[c] for r in rows] for c in COLUMNS}


def generate_proxy_day(path: str, events: int = 100_000, seed: int = 0, files: int = 1, n_clients: int = None,
                       n_hosts: int = None, n_agents: int = 60, anomaly_share: float = 0.002,
                       date=(2016, 1, 22), with_edge_rows: bool = True) -> dict:
    import pyarrow as pa
    import pyarrow.compute as pc
    import pyarrow.parquet as pq
    rng = np.random.default_rng(seed)
    n_clients = n_clients or max(100, events // 40)
    n_hosts = n_hosts or max(200, events // 50)
    clients = [f"10.{(i >> 8) & 255}.{i & 255}.{(i * 7) % 250 + 1}" for i in range(n_clients)]
    hosts = [f"{SUBS[i % len(SUBS)]}{i // len(SUBS) or ''}.{POPULAR[int(rng.integers(20))]}.com" for i in range(n_hosts)]
    agents = _agents(rng, n_agents)
    paths = _paths(rng, min(max(events // 4, 50), 50_000))
    cl = _zipf(rng, n_clients, events, 0.9)
    ho = _zipf(rng, n_hosts, events, 1.1)
    # a client keeps to a few agents: its own offset into the Zipf-ranked list
    ag = (_zipf(rng, n_agents, events, 1.2) + (cl % 3)) % n_agents
    pi = rng.integers(0, len(paths), size=events)
    start = rng.integers(6, 11, size=n_clients)               # each client's 10-hour window
    hour = (start[cl] + rng.integers(0, 10, size=events)) % 24
    minute, second = rng.integers(0, 60, size=events), rng.integers(0, 60, size=events)
    method = rng.choice(len(METHODS), size=events, p=[.78, .15, .04, .02, .01])
    ctype = rng.choice(len(CTYPES), size=events, p=[.3, .15, .2, .08, .1, .1, .02, .05])
    resp = rng.choice([200, 304, 302, 404, 500, 403], size=events, p=[.8, .08, .05, .04, .01, .02])
    sid = rng.integers(0, 1 << 62, size=events)

    take = lambda vals, idx: pc.take(pa.array(vals, pa.string()), pa.array(np.asarray(idx, np.int64)))  # noqa: E731
    const = lambda s: pa.array([s], pa.string()).take(pa.array(np.zeros(events, np.int64)))            # noqa: E731
    dec = lambda a: pc.cast(pa.array(np.asarray(a, np.int64)), pa.string())                              # noqa: E731
    two = lambda a: pc.utf8_lpad(dec(a), 2, "0")                                                         # noqa: E731
    join = lambda *xs: pc.binary_join_element_wise(*xs, "")                                              # noqa: E731
    host_a, path_a = take(hosts, ho), take(paths, pi)
    query_a = join(const("sid="), dec(sid), const("&p="), dec(sid % 97))
    cols = dict(
        p_date=const(f"{date[0]:04d}-{date[1]:02d}-{date[2]:02d}"),
        p_time=join(two(hour), const(":"), two(minute), const(":"), two(second)),
        clientip=take(clients, cl),
        host=host_a,
        reqmethod=take(METHODS, method),
        useragent=take(agents, ag),
        resconttype=take(CTYPES, ctype),
        duration=pa.array(rng.integers(1, 3000, size=events).astype(np.int32)),
        username=take([f"user{i}" for i in range(n_clients)], cl),
        webcat=take(WEBCATS, ho % len(WEBCATS)),
        referer=join(const("http://"), host_a, const("/")),
        respcode=pa.array(resp.astype(np.int32)),
        uriport=pa.array(np.where(method == 2, 443, 80).astype(np.int32)),
        uripath=path_a,
        uriquery=query_a,
        serverip=take([f"93.184.{i & 255}.{(i * 13) % 250 + 1}" for i in range(n_hosts)], ho),
        scbytes=pa.array(rng.integers(200, 2_000_000, size=events).astype(np.int64)),
        csbytes=pa.array(rng.integers(100, 4000, size=events).astype(np.int64)),
        fulluri=join(const("http://"), host_a, path_a, const("?"), query_a),
    )
    table = pa.table({c: cols[c] for c in COLUMNS})

    # planted anomalies: whole rows rebuilt in Python (a few per thousand) and put back by index
    first = EDGE_ROWS if with_edge_rows and events >= 2 * EDGE_ROWS else 0
    n_plant = min(int(round(events * anomaly_share)), max(events - first, 0))
    planted = np.sort(rng.choice(np.arange(first, events), size=n_plant, replace=False)) if n_plant else \
        np.zeros(0, np.int64)
    kinds = [KINDS[i % len(KINDS)] for i in range(n_plant)]
    patches = {}
    if n_plant:
        rows = table.take(pa.array(planted)).to_pylist()
        for j, (r, kind) in enumerate(zip(rows, kinds)):
            if kind == "long_query":
                q = "d=" + "".join(B64[i] for i in rng.integers(0, 64, size=int(rng.integers(400, 2001)) - 2))
                r["uriquery"] = q
                r["fulluri"] = f"http://{r['host']}{r['uripath']}?{q}"
            elif kind == "rare_agent":
                r["useragent"] = f"{_rand_label(rng, 8)}/{int(rng.integers(1, 9))}.{j} (compatible, one-off)"
            elif kind == "off_list_host":
                h = f"{_rand_label(rng, int(rng.integers(8, 16)), 'abcdefghijklmnopqrstuvwxyz')}.biz"
                r["host"] = h
                r["referer"] = f"http://{h}/"
                r["fulluri"] = f"http://{h}{r['uripath']}?{r['uriquery']}"
            else:   # odd_hour: three hours before the client's window opens
                c = int(cl[planted[j]])
                r["p_time"] = f"{(int(start[c]) - 3) % 24:02d}{r['p_time'][2:]}"
            patches[int(planted[j])] = r
    if first:
        edge = _edge_rows(table.slice(EDGE_ROWS, 1).to_pylist()[0])
        for i in range(EDGE_ROWS):
            patches[i] = {c: edge[c][i] for c in COLUMNS}
    if patches:
        idx = np.fromiter(sorted(patches), np.int64, count=len(patches))
        ptab = pa.table({c: pa.array([patches[int(i)][c] for i in idx], table.schema.field(c).type) for c in COLUMNS})
        # row i of the day: the patch when there is one, else the generated row
        src = np.arange(events, dtype=np.int64)
        src[idx] = events + np.arange(idx.size)
        table = pa.concat_tables([table, ptab]).take(pa.array(src))

    os.makedirs(path, exist_ok=True)
    out = []
    bounds = np.linspace(0, events, files + 1).astype(np.int64)
    for i in range(files):
        d = os.path.join(path, f"h={i:02d}")
        os.makedirs(d, exist_ok=True)
        pq.write_table(table.slice(bounds[i], bounds[i + 1] - bounds[i]), os.path.join(d, "part-00000.parquet"))
        out.append(d)
    return dict(paths=out, proxy_path=",".join(out), top1m=write_top1m(path), events=events,
                planted=planted.astype(np.int64), planted_kinds=kinds, edge_rows=first,
                edge_dropped=dict(EDGE_DROPPED) if first else dict(null=0, time=0, control=0))
