"""The slotted particle-store layout (engine.store_layout, slot_capacity, slot_rule): host
arithmetic only, no device."""
import numpy as np
import pytest
import torch

from ccmpc import engine


def test_layout_invariants_packed_and_slotted():
    counts = [300, 0, 1025, 40, 256]
    po, pb, pld = engine.store_layout(counts)
    assert po == [0, 320, 320, 1376, 1440] and pb == 1696 and pld == 1696
    cap = engine.slot_capacity(counts)
    so, sb, sld = engine.store_layout(counts, slot_cap=cap)
    assert cap == 1280 and so == [j * cap for j in range(len(counts))]
    assert sb == pb                                   # n_bound: the packed walk's end, unchanged
    assert sld >= len(counts) * cap and sld % engine.STORE_ALIGN == 0
    assert all(n <= cap for n in counts)
    # a capacity raises n_bound alike, and ld holds both the bound and the slots
    for capacity in (8000, 2 ** 15):
        _, b0, _ = engine.store_layout(counts, capacity=capacity)
        _, b1, ld1 = engine.store_layout(counts, capacity=capacity, slot_cap=cap)
        assert b0 == b1 == capacity and ld1 >= max(capacity, len(counts) * cap)


@pytest.mark.parametrize("bad", [-256, 100, 288, 1024])
def test_layout_rejects_a_bad_slot(bad):
    with pytest.raises(ValueError):                   # sign, alignment, chunk, a cell too large
        engine.store_layout([300, 1025], slot_cap=bad)


@pytest.mark.parametrize("top,cap", [(0, 256), (1, 256), (255, 256), (256, 256), (257, 512),
                                     (5000, 5120), (8448, 8448), (8449, 8704)])
def test_slot_cap_rounding(top, cap):
    assert engine.slot_capacity([top, 0, min(top, 7)]) == cap
    assert engine.slot_capacity([top], align=4) == cap       # the chunk is the coarser unit
    assert engine.slot_capacity([top], align=96) % 768 == 0  # a multiple of both


def _bound(counts):
    return engine.store_layout(counts)[1]


def test_auto_rule_edges():
    full = [256] * 64
    assert engine.slot_rule(full, 8, _bound(full)) == 256
    assert engine.slot_rule([256] * 65, 8, _bound([256] * 65)) == 0          # 65 cells
    c256 = [4096] * 16                                                       # 16 x 16 = 256 items
    assert engine.slot_rule(c256, 8, _bound(c256)) == 4096
    c257 = [4096] * 16 + [256]                                               # 17 x 16 = 272
    assert engine.slot_rule(c257, 8, _bound(c257)) == 0
    c257b = [4097] * 15 + [4096]                                             # 16 x 17 items
    assert engine.slot_rule(c257b, 8, _bound(c257b)) == 0
    assert engine.slot_rule(full, 9, _bound(full)) == 0                      # T = 9: not RB = 1's
    assert engine.slot_rule(full, 1, _bound(full)) == 256
    assert engine.slot_rule(full, 8, 2 ** 18) == 256                         # a capacity, still
    assert engine.slot_rule(full, 8, 2 ** 18 + 32) == 0                      # balanced mode
    assert engine.slot_rule([], 8, 0) == 0


def test_auto_rule_fill():
    """Slots at least SLOT_MIN_FILL full on average; the bench's C2 shape is inside."""
    c2 = [5000, 1391, 3609, 2220, 1474, 1306, 5000, 600, 3400]
    assert engine.slot_rule(c2, 8, _bound(c2)) == 5120
    assert 9 * 5120 // 256 == 180
    assert engine.slot_rule([5000], 8, _bound([5000])) == 5120
    assert engine.slot_rule([1000], 8, _bound([1000])) == 1024
    assert engine.slot_rule([20000], 8, _bound([20000])) == 20224
    assert engine.slot_rule([100000], 8, _bound([100000])) == 0              # 391 items
    sparse = [1280, 96, 96, 96]                       # 1568 of 5120 columns
    assert engine.slot_rule(sparse, 8, _bound(sparse)) == 0
    edge = [1000, 1000, 48]                           # 2048 of 3072: 0.667; and just under 0.4
    assert engine.slot_rule(edge, 8, _bound(edge)) == 1024
    assert engine.slot_rule([1024, 100, 104], 8, _bound([1024, 100, 104])) == 0   # 1228 / 3072
    assert engine.slot_rule([1024, 100, 105], 8, _bound([1024, 100, 105])) == 1024  # 1229


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("slots", [False, True])
def test_round_trip_through_cell_positions(dtype, slots):
    rng = np.random.default_rng(7)
    counts, T = [300, 0, 1025, 40], 5
    cells = [100 + rng.normal(size=(n, T, 2)) for n in counts]
    origin = np.array([[100.0 + j, 99.0 - j] for j in range(len(counts))])
    org = origin if dtype == torch.float32 else None
    cap = engine.slot_capacity(counts) if slots else 0
    offs, n_bound, ld = engine.store_layout(counts, slot_cap=cap)
    host = engine.cells_image(cells, offs, ld, dtype, org)
    assert host.shape == (2 * T, ld)
    st = engine.ParticleStore.__new__(engine.ParticleStore)      # a host image: no device
    st.T, st.counts, st.offsets, st.dtype = T, counts, offs, dtype
    st.pos = torch.from_numpy(host)
    st.origin = None if org is None else torch.from_numpy(org)
    used = np.zeros(ld, bool)
    for j, c in enumerate(cells):
        got = st.cell_positions(j)
        assert got.shape == c.shape
        if dtype == torch.float64:
            np.testing.assert_array_equal(got, c)
        else:
            np.testing.assert_allclose(got, c, atol=1e-6, rtol=0)
        assert not used[offs[j]:offs[j] + counts[j]].any()       # cells do not overlap
        used[offs[j]:offs[j] + counts[j]] = True
    assert not host[:, ~used].any()                              # nothing outside the cells
