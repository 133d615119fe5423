"""Proxy suspicious-connects on the GPU (gfx950): the string-entropy kernel bit for bit against its numpy twin,
the wrapper's host checks, featurize on the device against the host, and a day end to end on the HIP backend."""
import numpy as np
import pytest
import torch

from oni_ml_amd import config as CFG
from oni_ml_amd.models.lda.settings import LDASettings
from oni_ml_amd.ops.reference import string_entropy as twin

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097]
LONG = 70_001


def _edge_batch():
    """One batch: every length x every byte set, the starts running through every residue mod 16 (a 1-byte
    string after each group shifts the phase), the 70,001-byte single-value run in the middle, and the last
    string ending the buffer."""
    rng = np.random.default_rng(0)
    printable = np.arange(32, 127, dtype=np.uint8)
    sets = [np.array([0x00], np.uint8), np.array([0xFF], np.uint8), np.array([0x61], np.uint8),
            np.array([0x00, 0xFF], np.uint8), printable, np.arange(256, dtype=np.uint8)]
    strings = []
    for phase in range(16):
        for n in LENGTHS:
            if n > 300 and phase % 4:          # the long ones at four phases
                continue
            a = sets[(phase + len(strings)) % len(sets)]
            strings.append(a[rng.integers(0, a.size, size=n)].tobytes())
        strings.append(b"\x80")                # shifts every later start by one more byte
        if phase == 7:
            strings.append(b"\xfe" * LONG)
    for a in sets:                             # every byte set at every length, whatever the phase
        for n in LENGTHS:
            strings.append(a[rng.integers(0, a.size, size=n)].tobytes())
    strings.append(bytes(range(256)) * 3 + b"tail")      # ends the buffer, not a multiple of 16
    off = np.zeros(len(strings) + 1, np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return np.frombuffer(b"".join(strings), np.uint8).copy(), off, strings


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_kernel_is_bitwise_the_twin_on_the_edge_batch(hip):
    data, off, strings = _edge_batch()
    starts = {int(o) % 16 for o, s in zip(off[:-1], strings) if len(s) > 16}
    assert starts == set(range(16)) and off[-1] == data.size and data.size % 16 != 0
    assert max(len(s) for s in strings) == LONG
    want = twin(data, off)
    got = hip.string_entropy(torch.from_numpy(data).cuda(), torch.from_numpy(off))
    assert got.dtype == torch.float64 and got.is_cuda
    g = got.cpu().numpy()
    bad = np.flatnonzero(g.view(np.int64) != want.view(np.int64))
    assert bad.size == 0, [(int(i), len(strings[i]), g[i], want[i]) for i in bad[:5]]
    i = [len(s) for s in strings].index(LONG)
    assert g[i] == 0.0                                   # 70,001 of one value: 32-bit counters
    assert g[-1] == want[-1] and abs(g[-1] - 8.0) < 0.01
    # a view that starts at an odd address inside a larger allocation
    pad = torch.zeros(data.size + 3, dtype=torch.uint8, device="cuda")
    pad[3:] = torch.from_numpy(data).cuda()
    assert _same_bits(hip.string_entropy(pad[3:], torch.from_numpy(off)).cpu().numpy(), want)


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 257])
def test_kernel_row_counts(hip, rows):
    rng = np.random.default_rng(rows)
    lens = rng.integers(0, 200, size=rows)
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    data = rng.integers(0, 256, size=int(off[-1]), dtype=np.uint8)
    got = hip.string_entropy(torch.from_numpy(data).cuda(), torch.from_numpy(off))
    assert got.shape == (rows,) and _same_bits(got.cpu().numpy(), twin(data, off))


def test_kernel_grid_stride_wrap(hip):
    rng = np.random.default_rng(9)
    rows = 70_003
    lens = rng.integers(0, 40, size=rows)
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789/?=&.%-_", np.uint8)
    data = letters[rng.integers(0, letters.size, size=int(off[-1]))]
    want = twin(data, off)
    d = torch.from_numpy(data).cuda()
    for max_blocks in (3, 0):                  # 12 waves take 70,003 strings; then the default grid
        got = hip.string_entropy(d, torch.from_numpy(off), max_blocks=max_blocks)
        assert _same_bits(got.cpu().numpy(), want), max_blocks


def test_wrapper_accepts_what_the_refusals_below_vary(hip):
    """The positive control of the next test: the same arguments, unspoilt, launch and agree with the twin."""
    data = torch.arange(64, dtype=torch.uint8)
    ok = torch.tensor([0, 10, 10, 64], dtype=torch.int64)
    assert _same_bits(hip.string_entropy(data.cuda(), ok).cpu().numpy(), twin(data.numpy(), ok.numpy()))


def test_wrapper_refuses_bad_arguments_before_any_launch(hip):
    """Host-side checks only: every call below raises before a launch."""
    data = torch.arange(64, dtype=torch.uint8).cuda()
    ok = torch.tensor([0, 10, 10, 64], dtype=torch.int64)
    with pytest.raises(ValueError, match="non-decreasing"):
        hip.string_entropy(data, torch.tensor([0, 20, 10, 64], dtype=torch.int64))
    with pytest.raises(ValueError, match="outside"):
        hip.string_entropy(data, torch.tensor([0, 10, 65], dtype=torch.int64))
    with pytest.raises(ValueError, match="outside"):
        hip.string_entropy(data, torch.tensor([-1, 10, 64], dtype=torch.int64))
    with pytest.raises(TypeError):
        hip.string_entropy(data, ok.to(torch.int32))
    with pytest.raises(TypeError):
        hip.string_entropy(data.to(torch.int8), ok)
    with pytest.raises(ValueError):
        hip.string_entropy(data.cpu(), ok)
    with pytest.raises(ValueError):
        hip.string_entropy(torch.arange(128, dtype=torch.uint8).cuda()[::2], ok)
    with pytest.raises(ValueError):
        hip.string_entropy(data, ok, max_blocks=-1)
    with pytest.raises(ValueError, match="on the host"):
        hip.string_entropy(data, ok.cuda())
    with pytest.raises(ValueError):
        hip.string_entropy(data, torch.zeros(0, dtype=torch.int64))


@pytest.fixture(scope="module")
def day(tmp_path_factory):
    from oni_ml_amd.synth.proxy import generate_proxy_day
    d = tmp_path_factory.mktemp("proxy_gpu_day")
    return d, generate_proxy_day(str(d / "in"), events=20_000, seed=3, files=2)


def test_featurize_on_the_device_equals_the_host(day):
    from oni_ml_amd.features import proxy as FP
    _, g = day
    tab = FP.load_proxy(g["proxy_path"])
    top = FP.load_top_domains(g["top1m"])
    assert tab.dropped == 8
    c = FP.featurize(tab, "cpu", top)
    d = FP.featurize(tab, "cuda", top)
    assert d.word_key.is_cuda and np.array_equal(d.word_key.cpu().numpy(), c.word_key.numpy())
    assert np.array_equal(d.ip.cpu().numpy(), c.ip.numpy()) and d.ip_names == c.ip_names
    assert _same_bits(d.cuts["agent"], c.cuts["agent"])
    assert _same_bits(d.host["entropy"], c.host["entropy"])
    assert (d.methods, d.ctypes, d.resps) == (c.methods, c.ctypes, c.resps)
    # with persisted cuts too (proxy_post's call)
    d2 = FP.featurize(tab, "cuda", top, cuts={"agent": c.cuts["agent"].tolist()})
    assert np.array_equal(d2.word_key.cpu().numpy(), c.word_key.numpy())


def test_proxy_day_on_the_hip_backend(day):
    from oni_ml_amd.pipeline import run
    d, g = day

    def go(lp, max_results):
        cfg = CFG.resolve("20160122", "proxy", tol=1e-3, conf_path=None, environ={}, lpath=str(lp),
                          proxy_path=g["proxy_path"], top1m=g["top1m"], backend="hip", threads=4, verbose=False,
                          max_results=max_results)
        cfg.settings = LDASettings(em_max_iter=5)
        return run(cfg.validate(), device="cuda", log=lambda *a, **k: None)

    full = go(d / "full", -1)
    F = full["scored"]
    assert F >= 3 and full["below_tol"] == F and full["input"] == dict(rows=19_992, dropped=8)
    lines = (d / "full" / "proxy_results.csv").read_bytes().splitlines(keepends=True)
    assert len(lines) == F
    scores = []
    for ln in lines:
        f = ln.decode("utf-8").rstrip("\n").split("\t")
        assert len(f) == 21
        scores.append(float(f[20]))
    assert scores == sorted(scores) and scores[-1] < 1e-3
    N = F // 3
    lim = go(d / "lim", N)
    assert lim["scored"] == N and lim["below_tol"] == F
    assert (d / "lim" / "proxy_results.csv").read_bytes() == b"".join(lines[:N])
