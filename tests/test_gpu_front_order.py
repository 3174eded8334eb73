"""The front of the non-balanced RB = 1 kernels (moments.hip: locate_item_straight for up to 64
cells, CCMPC_LOCATE_STRAIGHT, and the first load group requested ahead of everything else a wave
sets up, CCMPC_LOADS_FIRST), at the smallest shapes where a wrong cell, a wrong address, a wrong
clamp or a wrong mask shows.  Neither changes a value, so every check here holds on the library
without them too.

  clamp and masks   One OV whose cells hold 1, 3, 63, 64, 65, 255, 256, 257, 1024 and 1025
                    particles: a lone quad, one under / on / over a wave's group (64) and an
                    item (256), the whole-cell cap (one item of 16 round-robin groups, the ring
                    loop) and one particle over it (five items, the last of one particle) -- and
                    an EMPTY cell between two of them (its one item has no particles in any
                    wave: NaN moments, as np.cov's).
  n_cells           1, 9 and 64 cells (the straight locate; 64 fills every lane) and 65 (the
                    loop it falls back to), ragged counts.
  capacity          A store sized for more particles than it holds: the grid's workgroups past
                    the last item find no item and leave.
  the last column   Alignment 4 and a last cell that ends with the store's last column, so that
                    the clamped loads of its last, ragged group are the allocation's last bytes
                    in row 2T - 1 (results only: an unclamped address is not observable here).

Every case at T = 8 (the instances that know their horizon) and T = 5 (the generic ones, ten of
sixteen rows live), f64 and f32 store.  Checks, at the suite's tolerances: moments against NumPy
(ddof = 1), means rtol 1e-13, covariances rtol 1e-10 / atol 1e-12; the fused launch against a
second launch on the same workspace (the arrival counters are back at zero) and against the
two-call path (ccmpc_moments: the MINK = false instances; then ccmpc_minkowski), bit for bit.
"""
import warnings

import numpy as np
import pytest
import torch

from test_gpu_block_const import _moments_match_numpy, _run_all

pytestmark = pytest.mark.gpu

STORES = [(8, torch.float64), (8, torch.float32), (5, torch.float64), (5, torch.float32)]
STORE_IDS = ["T8-f64", "T8-f32", "T5-f64", "T5-f32"]

# the issue's counts, with an empty cell between two non-empty ones
CLAMP_COUNTS = [1, 3, 63, 64, 0, 65, 255, 256, 257, 1024, 1025]

_CELLS = {}


def _cells(T, counts, seed):
    """One OV's cells of the given counts (an empty cell is a (0, T, 2) array), its reference
    trajectory; built once per shape and left unchanged."""
    key = (T, tuple(counts), seed)
    if key not in _CELLS:
        from ccmpc import synthetic
        rng = np.random.default_rng(np.random.Philox(seed))
        p0 = np.array([190.0, -80.0])
        cells = [synthetic.mode_cloud(rng, n, T, p0) for n in counts]
        for c in cells:
            c.setflags(write=False)
        _CELLS[key] = (cells, synthetic.ego_ref(seed, T))
    return _CELLS[key]


def _store(gpu, cells, dtype, capacity=None, align=None):
    """engine.ParticleStore.from_cells, with the alignment of the caller's choice."""
    from ccmpc import engine
    T = cells[0].shape[1]
    origin = None
    if dtype == torch.float32:
        origin = np.array([c[:, 0].mean(0) if len(c) else np.zeros(2) for c in cells])
    store = engine.ParticleStore(T, [len(c) for c in cells], dtype=dtype, device=gpu, origin=origin,
                                 capacity=capacity, align=align)
    host = np.zeros((2 * T, store.ld), np.float64 if dtype == torch.float64 else np.float32)
    for j, c in enumerate(cells):
        x = c if origin is None else c - origin[j]
        o = store.offsets[j]
        host[:, o:o + len(c)] = x.transpose(1, 2, 0).reshape(2 * T, len(c))
    store.pos.copy_(torch.from_numpy(host))
    return store


def _same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in zip(a, b))


def _check(gpu, T, counts, dtype, seed, capacity=None, align=None):
    from ccmpc import cycle
    cells, ref = _cells(T, counts, seed)
    store = _store(gpu, cells, dtype, capacity=capacity, align=align)
    assert store.n_bound <= 2 ** 15          # the plain launch, whole-cell items up to 1024
    cyc = cycle.MinkowskiCycle(store, [len(cells)], ref)
    first = _run_all(cyc)
    # a second launch on the same workspace: every arrival counter was left at zero
    assert _same_bits(first, _run_all(cyc))
    # the two-call path: the moments-only instances, then the rows kernel
    cyc.rec.zero_()
    cyc.run_unfused()
    torch.cuda.synchronize(gpu)
    assert _same_bits(first, (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))
    seen = [store.cell_positions(j) if dtype == torch.float32 else cells[j]
            for j in range(len(cells))]
    with warnings.catch_warnings():          # np.cov of no or one sample: 0 / 0, as the kernel's
        warnings.simplefilter("ignore", RuntimeWarning)
        _moments_match_numpy(first, seen, T)
    return store


@pytest.mark.parametrize("T,dtype", STORES, ids=STORE_IDS)
def test_clamp_and_masks_with_an_empty_cell(gpu, T, dtype):
    store = _check(gpu, T, CLAMP_COUNTS, dtype, seed=2400 + T)
    assert store.counts[4] == 0 and store.counts[3] > 0 and store.counts[5] > 0


def _ragged(n_cells):
    # 5 .. 75 particles: under, on and over a wave's group, different from cell to cell
    return [5 + (37 * (i + 1)) % 71 for i in range(n_cells)]


@pytest.mark.parametrize("n_cells", [1, 9, 64, 65])
@pytest.mark.parametrize("T,dtype", STORES, ids=STORE_IDS)
def test_cell_counts_around_the_straight_locate(gpu, T, dtype, n_cells):
    _check(gpu, T, _ragged(n_cells), dtype, seed=2500 + T)


@pytest.mark.parametrize("T,dtype", STORES, ids=STORE_IDS)
def test_capacity_above_the_count(gpu, T, dtype):
    """700 particles in a store sized for 8000: the grid has ~40 workgroups, the cells 7 items."""
    counts = [300, 1, 257, 142]
    store = _check(gpu, T, counts, dtype, seed=2600 + T, capacity=8000)
    assert store.n_bound == 8000 and sum(counts) < store.n_bound // 8


@pytest.mark.parametrize("last", [61, 1, 321])
@pytest.mark.parametrize("T,dtype", STORES, ids=STORE_IDS)
def test_last_cell_ends_with_the_store(gpu, T, dtype, last):
    """Alignment 4: the last cell's last aligned run is the last four columns of the store (61
    and 321: a ragged last quad in a ragged last group of one item and of a second item; 1: the
    cell IS the last run)."""
    counts = [37, last]
    store = _check(gpu, T, counts, dtype, seed=2700 + T, align=4)
    assert store.ld == store.offsets[-1] + (last + 3) // 4 * 4
    assert store.pos.shape == (2 * T, store.ld)
