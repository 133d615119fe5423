"""--host-report on the GPU (gfx950): ``ops.hip.host_summary`` (csrc/hip/host_summary.hip) exactly the torch twin
in all five outputs -- the key sets, sizes and document shapes of tests/test_host_report.py: wave and workgroup
edges, one hot address, documents no side names, both sides of an event on one document -- with the grid-stride
loops wrapping, with and without the wave fold, twice in one process; the wrapper's refusals; and a flow, a DNS
and a proxy day on the HIP backend."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_report_cases as HC  # noqa: E402
from test_host_report import TOL, Day  # noqa: E402

from oni_ml_amd.ops import reference as R  # noqa: E402
from oni_ml_amd.score import scorer as S  # noqa: E402

pytestmark = pytest.mark.gpu

_TWIN = {}


def _twin(keyset, shape, n, two):
    """The twin's result on CPU tensors, computed once per case and shared."""
    key = (keyset, shape, n, two)
    if key not in _TWIN:
        _TWIN[key] = R.host_summary(*HC.tensors(HC.case(*key)))
    return _TWIN[key]


@pytest.mark.parametrize("shape", HC.SHAPES)
@pytest.mark.parametrize("keyset", HC.KEYSETS)
def test_kernel_equals_the_twin(hip, keyset, shape):
    for n in HC.SIZES:
        for two in (False, True):
            args = HC.tensors(HC.case(keyset, shape, n, two), "cuda")
            got = hip.host_summary(*args)
            assert all(t.is_cuda for t in got[:4]) and isinstance(got[4], int)
            assert [t.dtype for t in got[:4]] == [torch.int64, torch.int64, torch.float64, torch.int64]
            HC.same(got, _twin(keyset, shape, n, two))


@pytest.mark.parametrize("keyset", HC.KEYSETS)
def test_grid_stride_wraps_and_the_fold_changes_nothing(hip, keyset):
    """3 workgroups over ~70 k events: both passes go round 91 times, with the wave fold (a pending entry carried
    over the rounds) and with one atomic per side."""
    for shape in ("third", "zipf", "tenth_skipped"):
        for two in (False, True):
            args = HC.tensors(HC.case(keyset, shape, HC.RAGGED, two), "cuda")
            want = _twin(keyset, shape, HC.RAGGED, two)
            HC.same(hip.host_summary(*args, max_blocks=3), want)
            HC.same(hip.host_summary(*args, fold=False), want)
            HC.same(hip.host_summary(*args, max_blocks=5, fold=False), want)


def test_hot_document_twice_in_one_process(hip):
    """Every side on one document, then half of them: the second call of each starts from outputs the launcher
    initialised again, and gives identical tensors."""
    for keyset, shape in (("all_equal", "one"), ("log_uniform", "zipf"), ("five_values", "zipf")):
        args = HC.tensors(HC.case(keyset, shape, HC.RAGGED, True), "cuda")
        first = hip.host_summary(*args)
        second = hip.host_summary(*args)
        HC.same(second, first)
        HC.same(first, _twin(keyset, shape, HC.RAGGED, True))
        ev, fl, ms, worst, skipped, stats = hip.host_summary(*args, stats=True)
        HC.same((ev, fl, ms, worst, skipped), first)
        sides = 2 * HC.RAGGED
        assert 0 < stats[0] <= 2 * sides and 0 < stats[1] <= sides and 0 < stats[2] <= sides
    # the scorer's dispatcher takes int64 rows, as the pipelines hold them
    da, sa, db, sb, D, tol = args
    HC.same(S.host_summary(da.long(), sa, db.long(), sb, D, tol), first)


def test_wrapper_accepts_what_the_refusals_below_vary(hip):
    """The positive control of the next test: the same arguments, unspoilt, launch and agree with the twin."""
    HC.same(hip.host_summary(*HC.tensors(HC.case("log_uniform", "third", 65, True), "cuda"), max_blocks=2),
            _twin("log_uniform", "third", 65, True))


def test_wrapper_refuses_bad_arguments_before_any_launch(hip):
    """Host-side checks only: every call below raises before a launch."""
    da, sa, db, sb, D, tol = HC.tensors(HC.case("log_uniform", "third", 65, True), "cuda")
    with pytest.raises(TypeError):
        hip.host_summary(da.long(), sa, db, sb, D, tol)
    with pytest.raises(TypeError):
        hip.host_summary(da, sa.float(), db, sb, D, tol)
    with pytest.raises(TypeError):
        hip.host_summary(da, sa, db, sb.float(), D, tol)
    with pytest.raises(ValueError, match="GPU tensor"):
        hip.host_summary(da, sa.cpu(), db, sb, D, tol)
    with pytest.raises(ValueError, match="GPU tensor"):
        hip.host_summary(da.cpu(), sa, db, sb, D, tol)
    with pytest.raises(ValueError, match="contiguous"):
        hip.host_summary(da, torch.cat([sa, sa])[::2], db, sb, D, tol)
    with pytest.raises(ValueError):
        hip.host_summary(da, sa[:-1], db, sb, D, tol)
    with pytest.raises(ValueError):
        hip.host_summary(da, sa, db[:-1], sb[:-1], D, tol)
    with pytest.raises(ValueError, match="out of range"):
        hip.host_summary(da, sa, db, sb, int(da.max()), tol)
    bad = db.clone()
    bad[11] = -2
    with pytest.raises(ValueError, match="out of range"):
        hip.host_summary(da, sa, bad, sb, D, tol)
    with pytest.raises(ValueError, match="go together"):
        hip.host_summary(da, sa, None, sb, D, tol)
    with pytest.raises(ValueError, match="go together"):
        hip.host_summary(da, sa, db, None, D, tol)
    with pytest.raises(ValueError, match="max_blocks"):
        hip.host_summary(da, sa, db, sb, D, tol, max_blocks=1.5)
    with pytest.raises(ValueError, match="max_blocks"):
        hip.host_summary(da, sa, db, sb, D, tol, max_blocks=-1)
    with pytest.raises(ValueError):
        hip.host_summary(da, sa, db, sb, -1, tol)
    # no documents: nothing is launched, every side is skipped
    none = torch.full_like(da, -1)
    out = hip.host_summary(none, sa, none, sb, 0, tol)
    assert all(t.numel() == 0 and t.is_cuda for t in out[:4]) and out[4] == 130


@pytest.fixture(scope="module", params=["flow", "dns", "proxy"])
def day(request, tmp_path_factory):
    return Day(request.param, tmp_path_factory.mktemp("hosts_gpu_" + request.param), backend="hip", device="cuda",
               scale=4)


def test_day_on_the_hip_backend(day):
    lp, summary = day.run(-1)
    lines = HC.check_hosts_file(day.kind, str(lp), TOL[day.kind], day.counts)
    assert len(lines) >= 20 and summary["hosts"] == len(lines)
    lim, s = day.run(-1, 50)
    assert s["scored"] == 50 and day.hosts(lim) == day.hosts(lp)
