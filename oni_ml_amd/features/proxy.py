"""Proxy featurization: parquet -> per-request words -> (clientip, word) counts.

The document is ``clientip``; the word is

    <top>_<hour>_<method>_<ebin>_<ctype>_<abin>_<resp>

* top    -- ``host`` cut at its first ':', through the native domain parser + top-1m flag of the DNS front end
            (``dns_features``: 0 / 1 / 2 for "intel"), over the distinct hosts only;
* hour   -- the integer before the first ':' of ``p_time``;
* method -- ``reqmethod``, or ``unknown_method`` if empty;
* ebin   -- #{cut : H(fulluri) > cut} with the fixed ``ENTROPY_CUTS``; H is the Shannon entropy of the URI's
            bytes (csrc/hip/string_entropy.hip on the GPU, its bitwise twin ops/reference.py on the host);
* ctype  -- ``resconttype`` before its first '/', or ``unknown_content_type`` if empty;
* abin   -- #{cut : a > cut}, a = the number of kept requests with exactly this ``useragent`` (the empty agent
            is an agent), cuts = ecdf_cuts(a per request, QUINTILES, weight);
* resp   -- the first character of ``respcode``, or ``unknown_response_code`` if empty.

The int64 word key packs these mixed-radix in that order (radices 3, 24, |method|, 21, |ctype|, 6, |resp|);
``ProxyWordSpace`` decodes it.  Proxy has no strict mode: cuts are persisted and reused when scoring, and word
names are never truncated.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from ..ops import native
from .dns_data import COUNTRY_CODES, SPECIAL_DOMAIN
from .dns_io import load_top_domains  # noqa: F401  (re-exported)
from .proxy_io import COLUMNS, ProxyTable, _offsets, arrow_dictionary_encode, load_proxy  # noqa: F401
from .quantiles import QUINTILES, ecdf_cuts

# 19 literals in steps of 0.3, then 20.0 (above any byte entropy, <= 8): radix 21
ENTROPY_CUTS = (0.0, 0.3, 0.6, 0.9, 1.2, 1.5, 1.8, 2.1, 2.4, 2.7, 3.0, 3.3, 3.6, 3.9, 4.2, 4.5, 4.8, 5.1, 5.4, 20.0)
TOP_RADIX, HOUR_RADIX = 3, 24
UNKNOWN_METHOD, UNKNOWN_CTYPE, UNKNOWN_RESP = "unknown_method", "unknown_content_type", "unknown_response_code"


@dataclass
class ProxyFeatures:
    rows: np.ndarray                  # table rows featurized
    ip: torch.Tensor                  # int64 clientip dictionary id
    ip_names: List[str]
    word_key: torch.Tensor            # int64
    weight: torch.Tensor
    bins: Dict[str, torch.Tensor]     # entropy, agent
    cuts: Dict[str, np.ndarray]       # agent
    host: dict                        # what does not depend on the cuts (``featurize(host=...)`` reuses it)
    methods: List[str]
    ctypes: List[str]
    resps: List[str]


def encode_mapped(arr, fn: Callable[[str], str]):
    """First-appearance ids + names of ``fn(value)`` over an Arrow string array: Arrow's dictionary of the raw
    values (first appearance), ``fn`` on the distinct values only, equal results merged in that order."""
    ids, raw = arrow_dictionary_encode(arr)
    d: Dict[str, int] = {}
    remap = np.empty(len(raw), np.int32)
    for i, v in enumerate(raw):
        remap[i] = d.setdefault(fn(v), len(d))
    return (remap[ids] if len(raw) else ids.astype(np.int32)), list(d)


def host_tops(hosts, top_domains: Sequence[str], threads: int = 8) -> np.ndarray:
    """top flag (0 / 1 / 2) per row of the Arrow ``hosts`` column: the distinct hosts, cut at the first ':',
    parsed by the native ``dns_features``."""
    ids, names = arrow_dictionary_encode(hosts)
    if not names:
        return np.zeros(0, np.int64)
    data, off = _offsets([h.split(":", 1)[0] for h in names])
    F = native.lib().dns_features(data, off, list(COUNTRY_CODES), list(top_domains), SPECIAL_DOMAIN, threads)
    return np.asarray(F["top_domain"], np.int64)[ids]


def uri_entropy(uris, device: torch.device) -> torch.Tensor:
    """float64 [n] on ``device``: H of every URI's bytes.  The GPU gets one upload of the column's bytes
    (through a pinned buffer) and runs the HIP kernel; the CPU pipeline runs the twin."""
    data, off = _offsets(uris)
    lo, hi = (int(off[0]), int(off[-1])) if off.size else (0, 0)
    buf = np.frombuffer(data, dtype=np.uint8)[lo:hi]
    off = off - lo
    if device.type != "cuda":
        from ..ops.reference import string_entropy
        return torch.from_numpy(string_entropy(buf, off))
    from ..ops import hip as H
    pin = torch.empty(buf.size, dtype=torch.uint8, pin_memory=True)
    pin.numpy()[:] = buf
    return H.string_entropy(pin.to(device, non_blocking=True), torch.from_numpy(off))


def _bins(values: List[torch.Tensor], cuts: List[torch.Tensor], device: torch.device) -> List[torch.Tensor]:
    if device.type == "cuda":
        from ..ops import hip as H
        b = H.bin_columns([v.contiguous() for v in values], [c.contiguous() for c in cuts]).to(torch.int64)
        return [b[:, i] for i in range(len(values))]
    return [(v.unsqueeze(-1) > c.unsqueeze(0)).sum(-1) for v, c in zip(values, cuts)]


def check_radices(n_method: int, n_ctype: int, n_resp: int, n_abin: int) -> None:
    """The mixed-radix key must fit an int64: garbage in a dictionary column would otherwise wrap and merge words."""
    space = TOP_RADIX * HOUR_RADIX * max(1, n_method) * (len(ENTROPY_CUTS) + 1) * max(1, n_ctype) * n_abin * max(1, n_resp)
    if space >= 1 << 63:
        raise ValueError(f"proxy word space of {space} keys does not fit an int64: {n_method} distinct reqmethod, "
                         f"{n_ctype} content-type and {n_resp} response-code values")


def featurize(tab: ProxyTable, device, top: Sequence[str], cuts: Optional[Dict[str, np.ndarray]] = None,
              threads: int = 8, host: Optional[dict] = None) -> ProxyFeatures:
    """``cuts``: the persisted agent cuts (proxy_post); None computes them from this table (proxy_pre).
    ``host``: ``ProxyFeatures.host`` of an earlier call on the same table (proxy_pre's, handed to proxy_post in
    the same process): the dictionaries, the top flags, the URI entropy and the agent counts are taken from it
    instead of being computed, and uploaded, again.  ``device`` "cpu" and "cuda" give identical word keys, cuts
    and client ids."""
    from ..ops import sortgroup as SG
    device = torch.device(device)
    n = tab.n
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(device)     # noqa: E731
    w = torch.ones(n, dtype=torch.int64, device=device)
    if host is not None and len(host["entropy"]) == n:
        mid, methods, cid, ctypes, rid, resps = (host[k] for k in ("mid", "methods", "cid", "ctypes", "rid", "resps"))
        ip_ids, ip_names, top_h = host["ip_ids"], host["ip_names"], host["top"]
        ent = torch.from_numpy(host["entropy"]).to(device)
        a = torch.from_numpy(host["agent_count"]).to(device)
    else:
        mid, methods = encode_mapped(tab.column("reqmethod"), lambda s: s or UNKNOWN_METHOD)
        cid, ctypes = encode_mapped(tab.column("resconttype"), lambda s: s.split("/", 1)[0] if s else UNKNOWN_CTYPE)
        rid, resps = encode_mapped(tab.column("respcode"), lambda s: s[0] if s else UNKNOWN_RESP)
        aid, _ = arrow_dictionary_encode(tab.column("useragent"))
        ip_ids, ip_names = arrow_dictionary_encode(tab.column("clientip"))
        top_h = host_tops(tab.column("host"), top, threads)
        ent = uri_entropy(tab.column("fulluri"), device)
        # requests per agent, per request: sorted distinct agent ids, their counts, gathered back
        if n:
            _, inv, cnt = SG.unique(dev(aid), return_inverse=True, return_counts=True)
            a = SG.gather(cnt, inv).to(torch.float64)
        else:
            a = torch.zeros(0, dtype=torch.float64, device=device)
    if cuts is None:
        acuts = ecdf_cuts(a, QUINTILES, w)
    else:
        acuts = torch.as_tensor(np.asarray(cuts["agent"], np.float64), device=device)
    ecuts = torch.tensor(ENTROPY_CUTS, dtype=torch.float64, device=device)
    ebin, abin = _bins([ent, a], [ecuts, acuts], device)
    check_radices(len(methods), len(ctypes), len(resps), int(acuts.numel()) + 1)

    key = dev(top_h)                   # < TOP_RADIX
    key = key * HOUR_RADIX + dev(tab.hour)
    key = key * max(1, len(methods)) + dev(mid)
    key = key * (len(ENTROPY_CUTS) + 1) + ebin
    key = key * max(1, len(ctypes)) + dev(cid)
    key = key * (int(acuts.numel()) + 1) + abin
    key = key * max(1, len(resps)) + dev(rid)
    if host is None or len(host["entropy"]) != n:
        host = dict(entropy=ent.cpu().numpy(), top=top_h, hour=tab.hour, agent_count=a.cpu().numpy(), mid=mid,
                    methods=methods, cid=cid, ctypes=ctypes, rid=rid, resps=resps, ip_ids=ip_ids, ip_names=ip_names)
    return ProxyFeatures(rows=np.arange(n, dtype=np.int64), ip=dev(ip_ids), ip_names=ip_names, word_key=key, weight=w,
                         bins=dict(entropy=ebin, agent=abin), cuts=dict(agent=acuts.cpu().numpy()), host=host,
                         methods=methods, ctypes=ctypes, resps=resps)


class ProxyWordSpace:
    """Decodes proxy word keys to their word strings."""

    def __init__(self, feat: ProxyFeatures):
        self.methods, self.ctypes, self.resps = list(feat.methods), list(feat.ctypes), list(feat.resps)
        self.n_abin = len(feat.cuts["agent"]) + 1

    def fields(self):
        """(name, radix, explained) of every digit of a key, most significant first (--explain)."""
        return [("top", TOP_RADIX, True), ("hour", HOUR_RADIX, True), ("method", max(1, len(self.methods)), True),
                ("ebin", len(ENTROPY_CUTS) + 1, True), ("ctype", max(1, len(self.ctypes)), True),
                ("abin", self.n_abin, True), ("resp", max(1, len(self.resps)), True)]

    def decode(self, keys: np.ndarray) -> List[str]:
        """In Python, column-wise as ``DnsWordSpace.decode_py``: method and content-type names sit inside the word."""
        k = np.asarray(keys, np.int64)
        parts = []
        for r in (max(1, len(self.resps)), self.n_abin, max(1, len(self.ctypes)), len(ENTROPY_CUTS) + 1,
                  max(1, len(self.methods)), HOUR_RADIX):
            parts.append(k % r)
            k = k // r
        resp, abin, ctype, ebin, method, hour = (p.tolist() for p in parts)
        s = lambda xs: list(map(str, xs))      # noqa: E731
        cols = [s(k.tolist()), s(hour), [self.methods[i] for i in method], s(ebin), [self.ctypes[i] for i in ctype],
                s(abin), [self.resps[i] for i in resp]]
        return ["_".join(t) for t in zip(*cols)]
