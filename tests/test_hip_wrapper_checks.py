"""The host-side rules that the scoring wrappers of ``ops/hip.py`` share, without a GPU: the scratch batch and the
list-scratch size against the expressions the wrappers carried inline before they shared them, every wrapper's
refusal of CPU tensors before it asks for the extension, and ``tail_mass``'s refusals of its scalar arguments."""
import pytest
import torch

from oni_ml_amd.ops import hip as H


def inline_batch(n, per_item, cap_mb, tile):
    """The batch arithmetic as tail_mass, peer_topn and column_topn each wrote it out."""
    batch = max(1, min(n, int(cap_mb * (1 << 20)) // per_item))
    if batch < n and batch >= tile:
        batch -= batch % tile
    return batch


@pytest.mark.parametrize("n, per_item, cap_mb, tile, want", [
    (1000, 72, 0.03, 256, 256),                              # 436 fit: whole tiles
    (1000, 72, 0.01, 256, 145),                              # below a tile: not rounded
    (1000, 72, 1e-9, 256, 1),                                # nothing fits: one item all the same
    (100, 72, 64, 256, 100),                                 # everything fits
    (1000, 576, 400 * 3 * 16 * 12 / 2 ** 20, 256, 256),      # test_peers_gpu.py's cap at N = 16, three blocks
    (1000, 72, 512 * 72 / 2 ** 20, 256, 512),                # exactly two tiles
    (300, 72, 299 * 72 / 2 ** 20, 256, 256),                 # one short of everything
])
def test_scratch_batch(n, per_item, cap_mb, tile, want):
    assert H._scratch_batch(n, per_item, cap_mb, tile) == want == inline_batch(n, per_item, cap_mb, tile)


def test_scratch_batch_without_tile():
    """column_l1's form: blocks of pairs, no tile rule."""
    assert H._scratch_batch(10, 8 * 50 * 50, 0.05) == 2 == max(1, min(10, int(0.05 * (1 << 20)) // (8 * 50 * 50)))
    assert H._scratch_batch(10, 8 * 50 * 50, 64) == 10
    assert H._scratch_batch(10, 8 * 50 * 50, 1e-9) == 1


@pytest.mark.parametrize("cells", [0, 1, 2, 7])
def test_list_scratch_doubles(cells):
    """The doubles, then as many ints rounded up to whole doubles."""
    assert H._list_scratch_doubles(cells) == cells + (cells + 1) // 2
    assert 8 * H._list_scratch_doubles(cells) >= 12 * cells


def _cpu_calls():
    """Every scoring wrapper with CPU tensors that are otherwise what it takes."""
    f64 = lambda *s: torch.rand(*s, dtype=torch.float64)                    # noqa: E731
    zeros = lambda dt, *s: torch.zeros(*s, dtype=dt)                        # noqa: E731
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    th, ph, gs = f64(4, 2, 3), f64(5, 2, 3), f64(2, 2, 3)
    d, w, grow = zeros(i32, 6), zeros(i32, 6), zeros(i32, 6, 2)
    order, s0, s1 = zeros(i32, 5), zeros(i64, 2), torch.ones(2, dtype=i64)
    return {
        "score_ensemble": lambda: H.score_ensemble(th, ph, 2, 3, 0.1, d, w, None, None, 1.0),
        "select_lowest": lambda: H.select_lowest(f64(6), zeros(u8, 6), 3),
        "host_summary": lambda: H.host_summary(d, f64(6), None, None, 4, 1.0),
        "group_rows_sum": lambda: H.group_rows_sum(f64(5, 6), order, s0, s1),
        "explain_sides": lambda: H.explain_sides(th, ph, gs, d, w, grow, 0.1),
        "expect_sides": lambda: H.expect_sides(th, ph, order, s0, s1, d, w, grow, 0.1),
        "tail_mass": lambda: H.tail_mass(th, ph, d, w),
        "tail_mass_docs": lambda: H.tail_mass_docs(th, ph, d, w),
        "peer_topn": lambda: H.peer_topn(th, zeros(i32, 3), 2),
        "column_topn": lambda: H.column_topn(f64(5, 6), 2),
        "topic_sides": lambda: H.topic_sides(th, ph, d, w),
        "column_l1": lambda: H.column_l1(f64(5, 3), f64(5, 4)),
        "holdout_draw": lambda: H.holdout_draw(torch.tensor([0, 2, 3]), torch.ones(3, dtype=i64), 1, 1 << 50),
        "holdout_entries": lambda: H.holdout_entries(f64(4, 3), f64(5, 3), d, w, zeros(i64, 6), zeros(u8, 5)),
        "string_entropy": lambda: H.string_entropy(zeros(u8, 8), torch.tensor([0, 3, 8])),
    }


@pytest.mark.parametrize("wrapper", sorted(_cpu_calls()))
def test_cpu_tensors_are_refused_before_the_extension_is_asked_for(wrapper, monkeypatch):
    """``ValueError ... must be a GPU tensor``, not the loader's ``RuntimeError``: as on a machine without the
    extension, ``lib()`` raises here."""
    def no_lib():
        raise RuntimeError("_onihip is not built")
    monkeypatch.setattr(H, "lib", no_lib)
    with pytest.raises(ValueError, match="GPU tensor"):
        _cpu_calls()[wrapper]()


def test_tail_mass_scalar_refusals(monkeypatch):
    monkeypatch.setattr(H, "lib", lambda: pytest.fail("a refused call asked for the extension"))
    th, ph = torch.rand(4, 2, 3, dtype=torch.float64), torch.rand(5, 2, 3, dtype=torch.float64)
    d = w = torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="tail_mass: block must be >= 1"):
        H.tail_mass(th, ph, d, w, block=0)
    with pytest.raises(ValueError, match="tail_mass: scratch_mb must be > 0, got 0"):
        H.tail_mass(th, ph, d, w, scratch_mb=0)
    with pytest.raises(ValueError, match="max_blocks must be a non-negative int, got -1"):
        H.tail_mass(th, ph, d, w, max_blocks=-1)
    with pytest.raises(ValueError, match="theta: expected torch.float64, got torch.float32"):
        H.tail_mass(th.float(), ph, d, w)
    # a bool is no block count, in these two as everywhere
    with pytest.raises(ValueError, match="max_blocks must be a non-negative int, got True"):
        H.select_lowest(th, ph, 3, max_blocks=True)
    with pytest.raises(ValueError, match="max_blocks must be a non-negative int, got True"):
        H.string_entropy(th, ph, max_blocks=True)
