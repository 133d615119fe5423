"""MAXRESULTS on the GPU (gfx950): the pipelines' limited results file is the head of the unlimited one, and
``rank_flagged(key, flag, limit)`` on keys scored by the HIP kernel equals the head of the unlimited ranking."""
import numpy as np
import pytest
import torch

from oni_ml_amd import config as CFG
from oni_ml_amd.models.lda.settings import LDASettings
from oni_ml_amd.score import scorer as S

pytestmark = pytest.mark.gpu


def _run(cfg, iters):
    from oni_ml_amd.pipeline import run
    cfg.settings = LDASettings(em_max_iter=iters)
    return run(cfg.validate(), device="cuda", log=lambda *a, **k: None)


def _head_check(tmp_path, make_cfg, results, iters):
    full = _run(make_cfg(tmp_path / "full", -1), iters)
    F = full["scored"]
    assert F >= 3 and full["below_tol"] == F
    N = F // 3
    lim = _run(make_cfg(tmp_path / "lim", N), iters)
    assert lim["scored"] == N and lim["below_tol"] == F
    lines = (tmp_path / "full" / results).read_bytes().splitlines(keepends=True)
    assert len(lines) == F
    assert (tmp_path / "lim" / results).read_bytes() == b"".join(lines[:N])
    big = _run(make_cfg(tmp_path / "big", F + 5), iters)
    assert big["scored"] == F and big["below_tol"] == F
    assert (tmp_path / "big" / results).read_bytes() == b"".join(lines)


def test_flow_day_limited_is_the_head_of_the_unlimited_file(tmp_path):
    from oni_ml_amd.synth.flow import generate_flow_day
    generate_flow_day(str(tmp_path / "in") + "/", events=20000, seed=4, n_internal=1500, n_external=3000)

    def make_cfg(lp, max_results):
        return CFG.resolve("20160122", "flow", tol=1e-4, conf_path=None, environ={}, lpath=str(lp),
                           flow_path=str(tmp_path / "in"), backend="hip", threads=4, verbose=False,
                           max_results=max_results)
    _head_check(tmp_path, make_cfg, "flow_results.csv", 6)


def test_dns_day_limited_is_the_head_of_the_unlimited_file(tmp_path):
    from oni_ml_amd.synth.dns import generate_dns_day
    r = generate_dns_day(str(tmp_path / "in"), events=30000, seed=1, files=2)

    def make_cfg(lp, max_results):
        return CFG.resolve("20160122", "dns", tol=1e-3, conf_path=None, environ={}, lpath=str(lp),
                           dns_path=r["dns_path"], top1m=r["top1m"], backend="hip", threads=4, verbose=False,
                           max_results=max_results)
    _head_check(tmp_path, make_cfg, "dns_results.csv", 5)


def test_rank_flagged_limit_on_scored_keys(hip):
    rng = np.random.default_rng(7)
    D, V, K, n = 500, 300, 20, 50_001
    theta = torch.from_numpy(rng.dirichlet(np.full(K, 0.3), D)).cuda()
    phi = torch.from_numpy(rng.dirichlet(np.full(V, 0.1), K).T.copy()).cuda()
    idx = lambda hi: torch.from_numpy(rng.integers(-1, hi, n).astype(np.int32)).cuda()      # noqa: E731
    sa, sb, key, flag = hip.score_events(theta, phi, K, 1.0 / K, idx(D), idx(V), idx(D), idx(V), 1e-3)
    full = S.rank_flagged(key.cpu(), flag.cpu())
    F = full.size
    assert 0 < F < n and F == int(flag.sum())
    for limit in (1, 100, F - 1, F, F + 1):
        got, below = S.rank_flagged_counted(key, flag, limit)
        assert below == F and got.dtype == np.int64 and np.array_equal(got, full[:limit]), limit
        assert np.array_equal(S.rank_flagged(key, flag, limit), full[:limit]), limit
