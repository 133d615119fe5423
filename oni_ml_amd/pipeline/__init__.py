"""End-to-end suspicious-connects pipelines (flow / dns / proxy), the ml_ops.sh replacement."""
from __future__ import annotations


def run(cfg, dist=None, device=None, log=print) -> dict:
    cfg.validate()
    import os
    if cfg.host_report and dist is not None and dist.active:      # before any file or directory is made
        from ..config import HOST_REPORT_ONE_PROCESS
        raise ValueError(HOST_REPORT_ONE_PROCESS)
    if cfg.ensemble > 1 and dist is not None and dist.active:
        from ..config import ENSEMBLE_ONE_PROCESS
        raise ValueError(ENSEMBLE_ONE_PROCESS)
    if cfg.expect and dist is not None and dist.active:
        from ..config import EXPECT_ONE_PROCESS
        raise ValueError(EXPECT_ONE_PROCESS)
    if cfg.explain and dist is not None and dist.active:
        from ..config import EXPLAIN_ONE_PROCESS
        raise ValueError(EXPLAIN_ONE_PROCESS)
    if cfg.tail and dist is not None and dist.active:
        from ..config import TAIL_ONE_PROCESS
        raise ValueError(TAIL_ONE_PROCESS)
    if cfg.peers and dist is not None and dist.active:
        from ..config import PEERS_ONE_PROCESS
        raise ValueError(PEERS_ONE_PROCESS)
    if cfg.topic_report and dist is not None and dist.active:
        from ..config import TOPIC_REPORT_ONE_PROCESS
        raise ValueError(TOPIC_REPORT_ONE_PROCESS)
    if (cfg.topic_match or cfg.topic_match_day) and dist is not None and dist.active:
        from ..config import TOPIC_MATCH_ONE_PROCESS
        raise ValueError(TOPIC_MATCH_ONE_PROCESS)
    if cfg.holdout > 0 and dist is not None and dist.active:
        from ..config import HOLDOUT_ONE_PROCESS
        raise ValueError(HOLDOUT_ONE_PROCESS)
    if cfg.dsource == "proxy":     # one process, no HDFS staging (pipeline/proxy.py raises for either)
        from .proxy import run as _run
        return _run(cfg, dist=dist, device=device, log=log)
    if dist is None or dist.rank == 0:
        os.makedirs(cfg.lpath, exist_ok=True)
    rank0 = dist is None or dist.rank == 0
    hd = None
    if cfg.hdfs:
        from ..io.hdfs import Hdfs
        hd = Hdfs(cfg.hadoop)
        if rank0:   # featurization and scoring run on rank 0 (ml_ops.sh:57-62 staging)
            stage = os.path.join(cfg.lpath, ".hdfs_in")
            if cfg.dsource == "flow":
                cfg.flow_path = hd.stage_inputs(cfg.flow_path, stage)
            else:
                cfg.dns_path = hd.stage_inputs(cfg.dns_path, stage)
    if cfg.dsource == "flow":
        from .flow import run as _run
    else:
        from .dns import run as _run
    summary = _run(cfg, dist=dist, device=device, log=log)
    if hd is not None and rank0:
        if not cfg.hpath:
            raise ValueError("--hdfs needs HPATH")
        hd.publish(cfg.lpath, cfg.hpath, cfg.dsource)     # ml_ops.sh:93-101,110-115
        summary["hdfs_published"] = cfg.hpath
    return summary
