"""Web-proxy input ingest without torch (like `dns_io.py`): the 19 columns of the proxy parquet day as
strings, with the row rules of `ml_ops YYYYMMDD proxy`.

PROXY_PATH is one or more comma-separated parquet paths (files or directory datasets).  Every column is
read as its string form (integers in decimal).  A row is dropped, and counted in ``dropped``, if

* p_date, p_time, clientip, host or fulluri is null (``drop_reasons["null"]``);
* p_time does not start with ``H+:``, an integer hour 0-23 (``"time"``);
* any field contains a tab, CR or LF -- the results file is tab-separated (``"control"``).

A row that breaks several rules counts under the first in that order.  Other nulls print as the empty string.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np

from .dns_io import _offsets, _pa, arrow_dictionary_encode  # noqa: F401  (re-exported)

COLUMNS = ["p_date", "p_time", "clientip", "host", "reqmethod", "useragent", "resconttype", "duration", "username",
           "webcat", "referer", "respcode", "uriport", "uripath", "uriquery", "serverip", "scbytes", "csbytes",
           "fulluri"]
REQUIRED = ("p_date", "p_time", "clientip", "host", "fulluri")

_HOUR = re.compile(r"^([0-9]+):")


def hour_of(p_time: str) -> int:
    """The integer before the first ':' of ``p_time`` if it is an hour 0-23, else -1."""
    m = _HOUR.match(p_time)
    if not m:
        return -1
    d = m.group(1).lstrip("0") or "0"
    return int(d) if len(d) <= 2 and int(d) <= 23 else -1


@dataclass
class ProxyTable:
    """The kept rows' 19 columns as Arrow large_string arrays (one chunk each) and their hour."""
    arrays: Dict[str, object]
    hour: np.ndarray               # int64 [n]
    n_input: int = 0               # rows read, before the row rules
    dropped: int = 0
    drop_reasons: Dict[str, int] = field(default_factory=dict)

    @property
    def n(self) -> int:
        return int(self.hour.size)

    def column(self, name: str):
        return self.arrays[name]

    def take_encoded(self, name: str, rows):
        """(first-appearance ids int32, distinct values) of column ``name`` at ``rows`` (DnsTable.take_encoded)."""
        pa, pc, _ = _pa()
        t = pc.take(self.arrays[name], pa.array(np.asarray(rows, np.int64)))
        if isinstance(t, pa.ChunkedArray):
            t = t.combine_chunks()
        d = pc.dictionary_encode(t)
        return np.asarray(d.indices.to_numpy(zero_copy_only=False), np.int32), d.dictionary.to_pylist()

    @property
    def cols(self) -> Dict[str, list]:
        """All columns as Python lists (tests / small tables only)."""
        return {c: a.to_pylist() for c, a in self.arrays.items()}


def select_paths(proxy_path: str) -> List[str]:
    return [p for p in proxy_path.split(",") if p]


def load_proxy(proxy_path: str) -> ProxyTable:
    _, _, pq = _pa()
    tables = []
    for p in select_paths(proxy_path):
        tables.append(pq.ParquetFile(p).read(columns=COLUMNS) if os.path.isfile(p) else pq.read_table(p, columns=COLUMNS))
    if not tables:
        raise FileNotFoundError(f"no proxy input in {proxy_path!r}")
    return table_from_arrow(tables)


def _strings(pa, pc, col):
    """``col`` as one large_string array, nulls kept."""
    if not pa.types.is_large_string(col.type):
        col = pc.cast(col, pa.large_string())
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks() if col.num_chunks != 1 else col.chunk(0)
    return col


def table_from_arrow(tables) -> ProxyTable:
    """The row rules on the read tables (in order)."""
    pa, pc, _ = _pa()
    missing = [c for t in tables for c in COLUMNS if c not in t.column_names]
    if missing:
        raise ValueError(f"proxy input lacks the columns {sorted(set(missing))}")
    tables = [t.select(COLUMNS) for t in tables]
    t = pa.concat_tables(tables, promote_options="permissive") if len(tables) > 1 else tables[0]
    n_in = len(t)
    strs = {c: _strings(pa, pc, t[c]) for c in COLUMNS}
    null = np.zeros(n_in, bool)
    for c in REQUIRED:
        null |= pc.is_null(strs[c]).to_numpy(zero_copy_only=False)
    strs = {c: (v if c in REQUIRED else pc.fill_null(v, "")) for c, v in strs.items()}
    # the hour of every distinct p_time (at most 86,400 of them), mapped back through the dictionary
    tid, tnames = arrow_dictionary_encode(pc.fill_null(strs["p_time"], ""))
    hours = np.fromiter((hour_of(x) for x in tnames), np.int64, count=len(tnames))
    hour = hours[tid] if n_in else np.zeros(0, np.int64)
    bad_time = ~null & (hour < 0)
    ctl = np.zeros(n_in, bool)
    for c in COLUMNS:
        ctl |= pc.fill_null(pc.match_substring_regex(strs[c], "[\t\r\n]"), False).to_numpy(zero_copy_only=False)
    ctl &= ~null & ~bad_time
    keep = ~(null | bad_time | ctl)
    mask = pa.array(keep)
    arrays = {}
    for c in COLUMNS:
        a = pc.filter(strs[c], mask)
        arrays[c] = a.combine_chunks() if isinstance(a, pa.ChunkedArray) else a
    reasons = dict(null=int(null.sum()), time=int(bad_time.sum()), control=int(ctl.sum()))
    return ProxyTable(arrays, hour[keep].astype(np.int64), n_input=n_in, dropped=int(n_in - keep.sum()),
                      drop_reasons=reasons)
