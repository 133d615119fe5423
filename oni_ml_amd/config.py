"""Typed run configuration.

The reference spreads configuration over five layers: positional CLI
(ml_ops.sh:4-6), the bash-sourced site file /etc/duxbay.conf (ml_ops.sh:36),
environment variables read by the Scala stages (System.getenv), hard-coded
constants (K=20, 20 MPI ranks, alpha 2.5, DUPFACTOR=1000, quantile grids) and
the lda-c settings.txt.  Here they collapse into one dataclass, resolved in
this order (later wins):

    defaults < duxbay.conf-style file < environment < explicit CLI flags

`parse_duxbay` understands the bash subset such site files use: comments,
``KEY=value`` / ``KEY="value"`` / ``KEY='value'``, arrays ``KEY=(a b c)``,
``export``, and ``$VAR`` / ``${VAR}`` expansion against earlier keys plus the
run variables FDATE, YR, MH, DY and DSOURCE that ml_ops.sh defines before
sourcing the file (ml_ops.sh:4-9).
"""
from __future__ import annotations

import os
import re
import shlex
from dataclasses import asdict, dataclass, field
from typing import Dict, List, Optional

from .models.lda.settings import LDASettings

ENV_KEYS = ("FLOW_PATH", "DNS_PATH", "PROXY_PATH", "HPATH", "LPATH", "LUSER", "TOL", "DUPFACTOR", "KRB_AUTH", "NODES",
            "UINODE", "RPATH", "LDAPATH", "SPK_EXEC", "SPK_EXEC_MEM", "TOP1M", "CUT", "MAXRESULTS", "ENSEMBLE", "EXPLAIN",
            "HOLDOUT", "HOLDOUT_TOPICS", "TAIL", "TAIL_TOL", "EXPECT", "PEERS",
            "TOPIC_REPORT", "TOPIC_MATCH", "TOPIC_MATCH_DAY")

# proxy has no multi-rank, sharded or HDFS-staged form
PROXY_ONE_PROCESS = "proxy runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"

# the host report folds one process's scored sides: no multi-rank, sharded or HDFS-staged form yet
HOST_REPORT_ONE_PROCESS = "--host-report runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"

# the ensemble's members are fitted and scored by one process: no multi-rank, sharded or HDFS-staged form
ENSEMBLE_ONE_PROCESS = "--ensemble runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"
ENSEMBLE_MAX = 64

# the explain file is made from one process's scored sides and its vocabulary's keys: no multi-rank, sharded or
# HDFS-staged form
EXPLAIN_ONE_PROCESS = "--explain runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"
EXPLAIN_MAX_FIELDS = 8     # explained fields of a word space (csrc/hip/kernels.h kExplainMaxFields)
# members of one block of a group sum (ops.hip / ops.reference group_rows_sum): a group's rows are summed block by
# block in member order, then the block sums in block order; the value is part of the result's bits
GROUP_BLOCK = 256
WORD_FIELDS = "word_fields.npz"      # <LPATH>/word_fields.npz: the vocabulary's keys and fields, under --explain

# the expect file is made from the explain file's groups and sides: the same one-process rule
EXPECT_ONE_PROCESS = "--expect runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"

# the tail file is made from one process's scored sides and its model tables: no multi-rank, sharded or HDFS-staged
# form
TAIL_ONE_PROCESS = "--tail runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"
# rows of one vocabulary block of a tail sum (ops.hip / ops.reference tail_mass): a side's p_v are summed block by
# block in row order, then the block sums in block order; the value is part of the result's bits, not a knob
# (256 / 1024 / 4096 measured on an MI355X: profiles/tail_mass.md)
TAIL_BLOCK = 1024
TAIL_SCRATCH_MB = 256      # cap on the per-block partials of one launch of ops.hip.tail_mass; more sides: batches
# --tail-tol: pairs per distinct document from which score.scorer.tail_pairs takes ops.hip.tail_mass_docs (p once per
# document of a tile) instead of ops.hip.tail_mass (p once per pair).  Both give the same bits: the value moves time
# only.  Measured on an MI355X at 1 / 2 / 4 / 8 / 16 pairs per document (profiles/tail_rank.md section 2): at 1 the
# shared-vector kernel loses (49 ms against 33 ms), from 2 on it wins (27 ms against 33 ms)
TAIL_DOCS_MIN_SHARE = 2.0

# the peers files are made from one process's written sides and its whole theta table: no multi-rank, sharded or
# HDFS-staged form
PEERS_ONE_PROCESS = "--peers runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"
PEERS_MAX = 16             # largest N of --peers (csrc/hip/kernels.h kPeersMax)
# candidate rows of one block of ops.hip.peer_topn and the cap on its per-block lists (N x 12 bytes per query and
# block; more queries: batches).  Neither changes a bit of the result: the values move time only (measured on an
# MI355X: profiles/peers.md)
PEERS_BLOCK = 4096
PEERS_SCRATCH_MB = 256

# the topic report is made from one process's written sides and its whole theta and phi tables: no multi-rank,
# sharded or HDFS-staged form
TOPIC_REPORT_ONE_PROCESS = ("--topic-report runs on one process: launch it without torchrun, with --gpus 1 and "
                            "without --hdfs")
TOPIC_REPORT_MAX = 32      # largest N of --topic-report (csrc/hip/kernels.h kTopicReportMax)
# rows of one block of ops.hip.column_topn and the cap on its per-block lists (N x 12 bytes per column and block; more
# columns: batches).  Neither changes a bit of the result: the values move time only (measured on an MI355X:
# profiles/topic_report.md)
TOPIC_BLOCK = 4096
TOPIC_SCRATCH_MB = 256
# rows of the strided sample whose N-th value per column lets the pass over all rows skip what lies below it (a
# table of fewer than twice as many rows is not sampled).  No bit of the result depends on it either
TOPIC_SAMPLE = 8192

# topics are matched from one process's whole phi and theta tables: no multi-rank, sharded or HDFS-staged form
TOPIC_MATCH_ONE_PROCESS = ("--topic-match runs on one process: launch it without torchrun, with --gpus 1 and "
                           "without --hdfs")
# pairs of one block of ops.hip.column_l1 / ops.reference.column_l1.  The block sums are added in block order, so
# the value is part of the bits of every distance, as GROUP_BLOCK is of a group sum (the reasoning, and what is not
# measured yet: profiles/topic_match.md)
MATCH_BLOCK = 1024
# cap on the blocks' partials of ops.hip.column_l1 (Wa x Wb x 8 bytes per block; more blocks: batches that continue
# the running sums).  It changes no bit of the result
MATCH_SCRATCH_MB = 256

# --holdout: the split and the K fits are one process's: no multi-rank, sharded or HDFS-staged form
HOLDOUT_ONE_PROCESS = "--holdout runs on one process: launch it without torchrun, with --gpus 1 and without --hdfs"
HOLDOUT_DIR = "holdout"              # <LPATH>/holdout/: holdout.csv, holdout.json, k<K>/ (the K's training fit)
HOLDOUT_MAX_F = 0.5
HOLDOUT_MIN_TOKENS = 10              # a document of fewer tokens is not split
# tokens of a corpus entry one lane draws (ops.hip.holdout_draw); a longer entry is shared by waves, 64 lanes x
# this many tokens each.  The split does not depend on it.
HOLDOUT_LANE_TOKENS = 64
HOLDOUT_SALT = 0x686F6C646F757421    # "holdout!": key = splitmix64(seed ^ HOLDOUT_SALT)
HOLDOUT_HIP_MAX_TOPICS = 128         # largest topic count of the HIP engine (ops.hip.padded_topics)

_VAR = re.compile(r"\$\{([A-Za-z_][A-Za-z0-9_]*)\}|\$([A-Za-z_][A-Za-z0-9_]*)")


def _expand(s: str, env: Dict[str, str]) -> str:
    return _VAR.sub(lambda m: env.get(m.group(1) or m.group(2), ""), s)


def parse_duxbay(text: str, run_vars: Optional[Dict[str, str]] = None) -> Dict[str, object]:
    """Parse a duxbay.conf-like bash file into {KEY: str | list[str]}."""
    env: Dict[str, str] = dict(run_vars or {})
    out: Dict[str, object] = {}
    for raw in text.splitlines():
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        if line.startswith("export "):
            line = line[len("export "):].strip()
        m = re.match(r"^([A-Za-z_][A-Za-z0-9_]*)=(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip()
        if val.startswith("("):
            inner = val[1:val.rfind(")")] if ")" in val else val[1:]
            items = [_expand(x, env) for x in shlex.split(inner, comments=True)]
            out[key] = items
            env[key] = items[0] if items else ""
            continue
        try:
            toks = shlex.split(val, comments=True)
        except ValueError:
            toks = [val]
        if val.startswith("'"):
            v = toks[0] if toks else ""
        else:
            v = _expand(toks[0] if toks else "", env)
        out[key] = v
        env[key] = v
    return out


def run_vars(fdate: str, dsource: str) -> Dict[str, str]:
    return dict(FDATE=fdate, YR=fdate[0:4], MH=fdate[4:6], DY=fdate[6:8], DSOURCE=dsource)


@dataclass
class RunConfig:
    fdate: str = ""
    dsource: str = "flow"                 # flow | dns | proxy
    tol: float = 1e-20
    max_results: int = -1                 # MAXRESULTS: write only the N lowest scores under TOL; -1: no limit
    ensemble: int = 1                     # --ensemble / ENSEMBLE: score by the mean of this many models fitted from
                                          # the seeds seed, seed + 1, ...; 1: one model, as ever
    host_report: int = 0                  # --host-report: also write <type>_hosts.csv; 0: off, -1: every host with a
                                          # side under TOL, N >= 1: the N hosts with the lowest scores
    explain: bool = False                 # --explain / EXPLAIN: also write <type>_explain.csv, per written side the
                                          # field of its word that makes it rare
    expect: bool = False                  # --expect / EXPECT: also write <type>_expect.csv, per written side and
                                          # explained field the value the host would normally show there (implies
                                          # explain)
    tail: bool = False                    # --tail / TAIL: also write <type>_tail.csv, per written side the host's
                                          # probability mass at or below the event's word
    tail_tol: Optional[float] = None      # --tail-tol / TAIL_TOL: flag and rank the events by their tail p-value, the
                                          # lower of the sides' tails, under this threshold (0 < P <= 1; implies
                                          # tail); None: by the score under TOL, as ever
    peers: int = 0                        # --peers / PEERS: also write <type>_peers.csv and <type>_peer_groups.csv,
                                          # every written side scored at its host's N nearest hosts in topic space
                                          # (1 <= N <= PEERS_MAX); 0: off
    topic_report: int = 0                 # --topic-report / TOPIC_REPORT: also write <type>_topics.csv,
                                          # <type>_topic_words.csv, <type>_topic_hosts.csv (the N words and hosts that
                                          # carry every topic) and <type>_topic.csv (the topic that explains every
                                          # written side); 1 <= N <= TOPIC_REPORT_MAX; 0: off
    topic_match: bool = False             # --topic-match / TOPIC_MATCH: also write <type>_topic_match.csv and
                                          # <type>_topic_stability.csv, the topics of an ensemble's members (and of
                                          # topic_match_day's model) aligned to member 0's
    topic_match_day: str = ""             # --topic-match-day / TOPIC_MATCH_DAY: the work directory of a previous run
                                          # whose model is aligned too, with <type>_host_drift.csv; implies
                                          # topic_match
    holdout: float = 0.0                  # --holdout / HOLDOUT: hold this fraction of every document's tokens out, fit
                                          # on the rest and report the held-out perplexity per topic count; 0: off
    holdout_topics: str = ""              # --holdout-topics / HOLDOUT_TOPICS: "K1,K2,..." to evaluate; "": topics alone
    holdout_select: bool = False          # --holdout-select: fit the day with the evaluated K of lowest perplexity
    lpath: str = ""                       # local working dir (reference: ${LUSER}/ml/${FDATE})
    hpath: str = ""                       # HDFS dir in the reference; unused unless set (optional copy target)
    flow_path: str = ""
    dns_path: str = ""
    proxy_path: str = ""                  # one or more comma-separated parquet paths
    top1m: str = "top-1m.csv"
    dupfactor: int = 1000
    topics: int = 20
    alpha: float = 2.5
    process_count: int = 20               # reference MPI ranks; CPU backend shards
    gpus: int = 1
    backend: str = "auto"                 # hip | torch | cpu | auto
    compat: str = "strict"                # strict | fixed
    seed: int = 0
    start: str = "random"                 # random | seeded | <model prefix>
    resume: bool = False
    threads: int = 0      # host threads of the stage pools; 0: knobs.threads(8), this rank's CPU budget
    write_doc_wc: bool = True
    word_assignments: bool = True          # lda-c writes word-assignments.dat on every `lda est`
    rank_gamma: Optional[bool] = None      # <rank>.gamma / <rank>.beta; None: multi-rank runs of K x V <= 2^26
    verbose: bool = True
    cuts: str = ""                        # fixed flow cuts in flow_qtiles form ("ibyt,ipkt,time"; the
                                          # reference's commented-out CUT consumer, flow_pre_lda.scala:95-98)
    hdfs: bool = False                    # stage hdfs:// inputs locally and publish results to HPATH
    hadoop: str = "hadoop"                # hadoop CLI used for the HDFS steps
    settings: LDASettings = field(default_factory=LDASettings)
    extra: Dict[str, object] = field(default_factory=dict)

    def fixed_cuts(self):
        """Cuts from `cuts` (flow_qtiles text or a path to such a file), else None."""
        if not self.cuts:
            return None
        from .features.quantiles import parse_qtiles
        text = self.cuts
        if os.path.exists(text):
            with open(text) as f:
                text = f.read()
        return parse_qtiles(text)

    @property
    def strict(self) -> bool:
        return self.compat == "strict"

    def feedback_path(self) -> str:
        return os.path.join(self.lpath, f"{self.dsource}_scores.csv")

    def validate(self):
        if self.dsource not in ("flow", "dns", "proxy"):
            raise ValueError("TYPE must be flow, dns or proxy")
        if self.fdate and (len(self.fdate) != 8 or not self.fdate.isdigit()):
            raise ValueError("FDATE must be YYYYMMDD")
        if self.compat not in ("strict", "fixed"):
            raise ValueError("compat must be strict or fixed")
        if not self.lpath:
            raise ValueError("LPATH (working directory) is not set")
        if self.dsource == "flow" and not self.flow_path:
            raise ValueError("FLOW_PATH is not set")
        if self.dsource == "dns" and not self.dns_path:
            raise ValueError("DNS_PATH is not set")
        if self.dsource == "proxy":
            if not self.proxy_path:
                raise ValueError("PROXY_PATH is not set")
            if self.gpus > 1 or self.hdfs:
                raise ValueError(PROXY_ONE_PROCESS)
        if self.topics < 1:
            raise ValueError("topics must be >= 1")
        if self.max_results != -1 and self.max_results < 1:
            raise ValueError(f"MAXRESULTS must be -1 (no limit) or >= 1, got {self.max_results}")
        if self.host_report < -1:
            raise ValueError(f"--host-report must be 0 (off), -1 (every flagged host) or >= 1, got {self.host_report}")
        if self.host_report and (self.gpus > 1 or self.hdfs):
            raise ValueError(HOST_REPORT_ONE_PROCESS)
        if self.expect:
            if self.gpus > 1 or self.hdfs:
                raise ValueError(EXPECT_ONE_PROCESS)
            self.explain = True      # the expect file describes the explain file's sides through its groups
        if self.explain and (self.gpus > 1 or self.hdfs):
            raise ValueError(EXPLAIN_ONE_PROCESS)
        if self.tail_tol is not None:
            self.tail_tol = self.check_tail_tol(self.tail_tol)
            self.tail = True      # the tail file describes the rows the threshold chose
        if self.tail and (self.gpus > 1 or self.hdfs):
            raise ValueError(TAIL_ONE_PROCESS)
        self.peers = self.check_peers(self.peers, self.gpus, self.hdfs)
        self.topic_report = self.check_topic_report(self.topic_report, self.gpus, self.hdfs)
        self.topic_match = self.check_topic_match(self.topic_match, self.topic_match_day, self.lpath, self.gpus,
                                                  self.hdfs)
        self.check_ensemble(self.ensemble, self.start, self.gpus, self.hdfs)
        self.check_holdout(self.holdout, self.holdout_list(), self.holdout_select, self.start, self.compat,
                           self.dsource, self.backend, self.gpus, self.hdfs)
        return self

    def holdout_list(self) -> List[int]:
        """The topic counts --holdout evaluates, in the order given: ``holdout_topics``, else ``topics`` alone."""
        return parse_topic_list(self.holdout_topics) or [int(self.topics)]

    @staticmethod
    def check_tail_tol(p) -> float:
        """The --tail-tol rule, also applied by the command line before anything is written."""
        p = float(p)
        if not 0.0 < p <= 1.0:      # (a NaN fails both comparisons)
            raise ValueError(f"--tail-tol must be in (0, 1], got {p}")
        return p

    @staticmethod
    def check_peers(n, gpus: int = 1, hdfs: bool = False, world: int = 1) -> int:
        """The --peers rules, also applied by the command line before anything is written."""
        n = int(n)
        if n == 0:
            return 0
        if not 1 <= n <= PEERS_MAX:
            raise ValueError(f"--peers must be 0 (off) or in [1, {PEERS_MAX}], got {n}")
        if gpus > 1 or hdfs or world > 1:
            raise ValueError(PEERS_ONE_PROCESS)
        return n

    @staticmethod
    def check_topic_report(n, gpus: int = 1, hdfs: bool = False, world: int = 1) -> int:
        """The --topic-report rules, also applied by the command line before anything is written."""
        n = int(n)
        if n == 0:
            return 0
        if not 1 <= n <= TOPIC_REPORT_MAX:
            raise ValueError(f"--topic-report must be 0 (off) or in [1, {TOPIC_REPORT_MAX}], got {n}")
        if gpus > 1 or hdfs or world > 1:
            raise ValueError(TOPIC_REPORT_ONE_PROCESS)
        return n

    @staticmethod
    def check_topic_match(on, day: str = "", lpath: str = "", gpus: int = 1, hdfs: bool = False,
                          world: int = 1) -> bool:
        """The --topic-match / --topic-match-day rules, also applied by the command line before anything is written:
        one process; the day's directory holds both results files and is not the work directory itself."""
        day = str(day or "")
        if not on and not day:
            return False
        if gpus > 1 or hdfs or world > 1:
            raise ValueError(TOPIC_MATCH_ONE_PROCESS)
        if day:
            for f in ("doc_results.csv", "word_results.csv"):
                if not os.path.isfile(os.path.join(day, f)):
                    raise ValueError(f"--topic-match-day: {os.path.join(day, f)} not found: the directory must hold "
                                     f"a finished run's doc_results.csv and word_results.csv")
            if lpath and os.path.realpath(day) == os.path.realpath(lpath):
                raise ValueError(f"--topic-match-day: {day} is this run's own work directory (LPATH)")
        return True

    @staticmethod
    def check_holdout(holdout: float, topics: List[int], select: bool, start: str, compat: str, dsource: str,
                      backend: str = "auto", gpus: int = 1, hdfs: bool = False, world: int = 1):
        """The --holdout rules, also applied by the command line before anything is written."""
        holdout = float(holdout)
        if holdout == 0.0:
            if select:
                raise ValueError("--holdout-select needs --holdout F")
            return
        if not 0.0 < holdout <= HOLDOUT_MAX_F:      # (a NaN fails both comparisons)
            raise ValueError(f"--holdout must be in (0, {HOLDOUT_MAX_F}], got {holdout}")
        if gpus > 1 or world > 1 or hdfs:
            raise ValueError(HOLDOUT_ONE_PROCESS)
        if start not in ("random", "seeded"):
            raise ValueError(f"--holdout needs a random or seeded start: the model {start!r} fixes the topic count")
        if len(set(topics)) != len(topics):
            raise ValueError(f"--holdout-topics names a topic count twice: {topics}")
        hip = backend == "hip"
        if backend == "auto" and any(k > HOLDOUT_HIP_MAX_TOPICS for k in topics):
            import torch
            hip = torch.cuda.is_available()
        for k in topics:
            if k < 1 or (hip and k > HOLDOUT_HIP_MAX_TOPICS):
                raise ValueError(f"--holdout-topics: {k} is outside what the {backend} backend fits "
                                 f"(1 .. {HOLDOUT_HIP_MAX_TOPICS if hip else 'any'})")
        if select and compat == "strict" and dsource in ("flow", "dns") and any(k != 20 for k in topics):
            raise ValueError("--holdout-select under --compat strict: the strict flow and dns scorers are fixed at 20 "
                             f"topics, the list {topics} could select another; use --compat fixed")

    @staticmethod
    def check_ensemble(ensemble: int, start: str, gpus: int = 1, hdfs: bool = False, world: int = 1):
        """The --ensemble rules, also applied by the command line before anything is written."""
        if not 1 <= ensemble <= ENSEMBLE_MAX:
            raise ValueError(f"--ensemble must be in [1, {ENSEMBLE_MAX}], got {ensemble}")
        if ensemble == 1:
            return
        if gpus > 1 or world > 1 or hdfs:
            raise ValueError(ENSEMBLE_ONE_PROCESS)
        if start not in ("random", "seeded"):
            raise ValueError("--ensemble needs a random or seeded start: every member would begin from the model "
                             f"{start!r} and be the same model")

    def to_dict(self) -> dict:
        d = asdict(self)
        return d


def parse_topic_list(x) -> List[int]:
    """"10,20,30" (or a list) -> [10, 20, 30]; "" / None -> []."""
    if x is None or x == "":
        return []
    items = x.split(",") if isinstance(x, str) else list(x)
    try:
        return [int(str(i).strip()) for i in items if str(i).strip() != ""]
    except ValueError:
        raise ValueError(f"--holdout-topics must be a comma-separated list of topic counts, got {x!r}") from None


def resolve(fdate: str, dsource: str, tol: Optional[float] = None, conf_path: Optional[str] = None,
            environ: Optional[Dict[str, str]] = None, max_results: Optional[int] = None, **overrides) -> RunConfig:
    """Build a RunConfig from the duxbay file, the environment and explicit overrides."""
    env = dict(os.environ if environ is None else environ)
    cfg = RunConfig(fdate=fdate, dsource=dsource)
    layers: List[Dict[str, object]] = []
    if conf_path and os.path.exists(conf_path):
        with open(conf_path) as f:
            layers.append(parse_duxbay(f.read(), run_vars(fdate, dsource)))
    layers.append({k: env[k] for k in ENV_KEYS if k in env})
    for layer in layers:
        _apply(cfg, layer)
    if tol is not None:
        cfg.tol = float(tol)
    if max_results is not None:
        cfg.max_results = int(max_results)
    if not cfg.lpath and isinstance(layers[0].get("LUSER") if layers else None, str):
        cfg.lpath = os.path.join(str(layers[0]["LUSER"]), "ml", fdate)
    for k, v in overrides.items():
        if v is None:
            continue
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config key {k}")
        setattr(cfg, k, v)
    if cfg.threads <= 0:
        from . import knobs
        cfg.threads = knobs.threads(8)
    return cfg


def _apply(cfg: RunConfig, layer: Dict[str, object]):
    m = dict(FLOW_PATH="flow_path", DNS_PATH="dns_path", PROXY_PATH="proxy_path", HPATH="hpath", LPATH="lpath",
             TOP1M="top1m")
    for k, attr in m.items():
        if k in layer and isinstance(layer[k], str) and layer[k]:
            setattr(cfg, attr, layer[k])
    if "TOL" in layer and layer["TOL"] not in ("", None):
        cfg.tol = float(layer["TOL"])
    if "MAXRESULTS" in layer and layer["MAXRESULTS"] not in ("", None):
        cfg.max_results = int(layer["MAXRESULTS"])
    if "ENSEMBLE" in layer and layer["ENSEMBLE"] not in ("", None):
        cfg.ensemble = int(layer["ENSEMBLE"])
    if "EXPLAIN" in layer and layer["EXPLAIN"] not in ("", None):
        cfg.explain = str(layer["EXPLAIN"]).strip().lower() not in ("0", "false", "no", "off")
    if "EXPECT" in layer and layer["EXPECT"] not in ("", None):
        cfg.expect = str(layer["EXPECT"]).strip().lower() not in ("0", "false", "no", "off")
    if "TAIL" in layer and layer["TAIL"] not in ("", None):
        cfg.tail = str(layer["TAIL"]).strip().lower() not in ("0", "false", "no", "off")
    if "TAIL_TOL" in layer and layer["TAIL_TOL"] not in ("", None):
        cfg.tail_tol = float(layer["TAIL_TOL"])
    if "PEERS" in layer and layer["PEERS"] not in ("", None):
        cfg.peers = int(layer["PEERS"])
    if "TOPIC_REPORT" in layer and layer["TOPIC_REPORT"] not in ("", None):
        cfg.topic_report = int(layer["TOPIC_REPORT"])
    if "TOPIC_MATCH" in layer and layer["TOPIC_MATCH"] not in ("", None):
        cfg.topic_match = str(layer["TOPIC_MATCH"]).strip().lower() not in ("0", "false", "no", "off")
    if "TOPIC_MATCH_DAY" in layer and isinstance(layer["TOPIC_MATCH_DAY"], str) and layer["TOPIC_MATCH_DAY"]:
        cfg.topic_match_day = layer["TOPIC_MATCH_DAY"]
    if "HOLDOUT" in layer and layer["HOLDOUT"] not in ("", None):
        cfg.holdout = float(layer["HOLDOUT"])
    if "HOLDOUT_TOPICS" in layer and layer["HOLDOUT_TOPICS"] not in ("", None):
        t = layer["HOLDOUT_TOPICS"]
        cfg.holdout_topics = ",".join(t) if isinstance(t, list) else str(t)      # a bash array or "10,20"
    if "DUPFACTOR" in layer and layer["DUPFACTOR"] not in ("", None):
        cfg.dupfactor = int(layer["DUPFACTOR"])
    if "CUT" in layer and isinstance(layer["CUT"], str) and layer["CUT"].strip():
        cfg.cuts = layer["CUT"]
    for k in ("NODES", "UINODE", "RPATH", "LDAPATH", "LUSER", "KRB_AUTH", "SPK_EXEC", "SPK_EXEC_MEM"):
        if k in layer:
            cfg.extra[k] = layer[k]
