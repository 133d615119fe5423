"""MAXRESULTS selection: ``select_lowest(key, flag, limit)`` -- the torch twin (ops/reference.py) on the CPU and
the HIP radix select (csrc/hip/select_lowest.hip) on the GPU -- and ``rank_flagged(key, flag, limit)``.

The oracle everywhere is the unlimited path on CPU tensors, ``rank_flagged(key, flag)`` sliced to ``[:limit]``:
the selection must be exactly ``np.sort(oracle[:limit])`` and the limited ranking ``oracle[:limit]`` itself,
as int64 arrays.  One oracle per (key set, size), computed once and shared by the CPU and the GPU cases.
"""
import numpy as np
import pytest
import torch

from oni_ml_amd.ops import hip as H
from oni_ml_amd.ops import reference as R
from oni_ml_amd.score import scorer as S

TILE = H.SELECT_TILE
RAGGED = 34 * TILE + 333            # ~70 k rows: 35 tiles, the last one partial
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, RAGGED]
SETS = ["uniform", "five_values", "all_equal", "low_digits", "top_exponent", "signed_mix", "none_flagged",
        "all_flagged", "nan_unflagged"]


def _bits(x):
    return np.asarray(x, np.uint64).view(np.float64)


def _case(name, n):
    """(key float64 [n], flag uint8 [n]) of one key set, seeded by its name and size."""
    rng = np.random.default_rng([SETS.index(name), n])
    scores = lambda: 10.0 ** rng.uniform(-9, -2, n)           # noqa: E731 -- scaled like the scorers' keys
    if name == "uniform":                                        # ~30 % under a TOL
        key = scores()
        flag = key < np.quantile(key, 0.3) if n else np.zeros(0, bool)
    elif name == "five_values":                                  # the cut falls inside a long tie run
        key = rng.choice(np.array([1e-7, 3e-6, np.nextafter(3e-6, 1.0), 2e-4, 5e-3]), n)
        flag = rng.random(n) < 0.8
    elif name == "all_equal":
        key = np.full(n, 1.25e-5)
        flag = rng.random(n) < 0.7
    elif name == "low_digits":                                   # only the lowest digits separate the keys
        key = 1.0 + rng.permutation(n) * 2.0 ** -52
        flag = rng.random(n) < 0.5
    elif name == "top_exponent":                                 # two keys, apart in the top exponent bits only
        lo = np.uint64(0x0018000000000001)
        key = np.where(rng.random(n) < 0.5, _bits(lo), _bits(lo | np.uint64(1 << 62)))
        flag = rng.random(n) < 0.6
    elif name == "signed_mix":                                   # flags by hand: negatives and zeros are selected
        vals = np.array([-0.0, 0.0, -1.5, -1e-300, 5e-324, -5e-324, 1.1e-308, -1.1e-308, 1.0, 7e-4, np.inf, -np.inf])
        key = rng.choice(vals, n)
        flag = rng.random(n) < 0.5
    elif name == "none_flagged":
        key, flag = scores(), np.zeros(n, bool)
    elif name == "all_flagged":
        key, flag = scores(), np.ones(n, bool)
    elif name == "nan_unflagged":                                # NaN of either sign, never under the TOL
        key = scores()
        nan = rng.random(n) < 0.2
        key[nan] = np.where(rng.random(int(nan.sum())) < 0.5, np.nan, _bits(np.uint64(0xFFF8000000000123)))
        with np.errstate(invalid="ignore"):
            flag = key < 1e-4
    else:
        raise KeyError(name)
    return np.ascontiguousarray(key, np.float64), np.ascontiguousarray(flag, np.uint8)


_ORACLE = {}


def _oracle(name, n):
    """(key, flag, the unlimited ranking of the flagged rows) -- the behaviour without a limit, on the CPU."""
    if (name, n) not in _ORACLE:
        key, flag = _case(name, n)
        full = S.rank_flagged(torch.from_numpy(key), torch.from_numpy(flag))
        full = np.ascontiguousarray(full, np.int64)
        full.setflags(write=False)
        _ORACLE[name, n] = (key, flag, full)
    return _ORACLE[name, n]


def _limits(n, F):
    return sorted({x for x in (1, 63, 64, 65, F - 1, F, F + 1, 10 * n) if x >= 1})


def _check(name, n, device, select):
    key, flag, full = _oracle(name, n)
    F = int(flag.astype(bool).sum())
    assert full.size == F
    k, f = torch.from_numpy(key).to(device), torch.from_numpy(flag).to(device)
    for limit in _limits(n, F):
        want = full[:limit]
        got = select(k, f, limit)
        assert got.dtype == torch.int64 and got.device.type == k.device.type
        got = got.cpu().numpy()
        assert np.array_equal(got, np.sort(want)), (name, n, limit, got[:8], np.sort(want)[:8])
        ranked = S.rank_flagged(k, f, limit)
        assert ranked.dtype == np.int64 and np.array_equal(ranked, want), (name, n, limit)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", SETS)
def test_twin_selects_the_head_of_the_full_ranking(name, n):
    _check(name, n, "cpu", R.select_lowest)


def test_twin_counts_and_validation():
    key, flag, full = _oracle("uniform", TILE + 1)
    k, f = torch.from_numpy(key), torch.from_numpy(flag)
    sel, flagged = R.select_lowest(k, f, 10, with_count=True)
    assert flagged == full.size and sel.numel() == 10
    order, below = S.rank_flagged_counted(k, f, 10)
    assert below == full.size and np.array_equal(order, full[:10])
    for bad in (0, -1):
        with pytest.raises(ValueError):
            R.select_lowest(k, f, bad)
    with pytest.raises(TypeError):
        R.select_lowest(k, f, 2.5)
    with pytest.raises(ValueError):
        R.select_lowest(k.to(torch.float32), f, 3)
    with pytest.raises(ValueError):
        R.select_lowest(k, f[:-1], 3)


def test_tile_size_is_exported():
    assert H.SELECT_TILE == 2048 and RAGGED > 8 * TILE and RAGGED % TILE


# ----------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", SETS)
def test_hip_selects_the_head_of_the_full_ranking(hip, name, n):
    _check(name, n, "cuda", hip.select_lowest)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_hip_grid_stride_wraps(hip, name):
    """3 workgroups over 35 tiles: every grid-stride loop of the kernels goes round 11 or 12 times."""
    _check(name, RAGGED, "cuda", lambda k, f, limit: hip.select_lowest(k, f, limit, max_blocks=3))


@pytest.mark.gpu
def test_hip_counts_and_validation(hip):
    key, flag, full = _oracle("uniform", RAGGED)
    k, f = torch.from_numpy(key).cuda(), torch.from_numpy(flag).cuda()
    assert hip.lib().select_tile() == TILE
    sel, flagged = hip.select_lowest(k, f, 100, with_count=True)
    assert flagged == full.size and np.array_equal(sel.cpu().numpy(), np.sort(full[:100]))
    with pytest.raises(ValueError):
        hip.select_lowest(k, f, 0)
    with pytest.raises(TypeError):
        hip.select_lowest(k, f, 1.5)
    with pytest.raises(TypeError):
        hip.select_lowest(k.float(), f, 3)
    with pytest.raises(TypeError):
        hip.select_lowest(k, f.bool(), 3)
    with pytest.raises(ValueError):
        hip.select_lowest(k, f[:-1], 3)
    with pytest.raises(ValueError):
        hip.select_lowest(k.cpu(), f, 3)
    with pytest.raises(ValueError):
        hip.select_lowest(k[::2], f[::2], 3)
