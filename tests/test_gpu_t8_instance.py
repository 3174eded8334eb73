"""The cycle kernel's T = 8 instance (moments.hip: moments_kernel's compile-time horizon TC and
the helpers it is handed to), which the plain launch picks at T = 8 on either store.

  prefix property    A store at T = 8 against the same particles cut to their first 7 steps at
                     T = 7, which takes the generic instance with the same item cut (the same
                     capacity, so the same n_bound).  Per entry, the Gram sums, the gather order,
                     the finaliser and the records of pairs with t < 7 do not depend on rows 14
                     and 15, so the means of steps 0 .. 6, the leading 14 x 14 covariance, the
                     first 21 records of each cell (p = t (t - 1) / 2 + tau order) and
                     prob_lower[:7] are the same bits.
  group boundaries   Cells ending exactly on a load group (multiples of 64) and on an item
                     (multiples of 256), one particle under and one over each: whole and ragged
                     groups on both sides of every boundary, for whole-cell items (up to 1024
                     particles) and cut ones.  (The instance keeps the generic particle mask and
                     address clamp; a form without them for whole groups was built with this
                     round and removed, profiles/r15.)
  neighbour          A cell of whole groups followed at once by a cell of NaN: a load or a
                     product that reached past the cell's end would carry NaN in.
  T = 7 and T = 2    still the generic instance, on the same counts and checks.

Checks of the boundary tests are test_gpu_block_const.py's, with its tolerances: moments against
NumPy (ddof = 1) at rtol 1e-10 / atol 1e-12, means at rtol 1e-13; status, (t, tau) order, `which`
and `side` against the oracle's generator; the fused launch, a second launch, the two-call path
(whose rows kernel is generic, so the tail is compared too) and a graph replay bit for bit.
"""
import numpy as np
import pytest
import torch

from test_gpu_block_const import _check_one_ov, _clouds, _counts, _run_all

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])

# one lane, one group less / exactly / more than one lane's worth, one item, the item's and the
# whole-cell cap's two sides, then ragged cells of 2, 17 and 33 items of 256: one gather group, two
# groups in a wave's halves, groups through LDS
PREFIX_COUNTS = [3, 63, 64, 65, 200, 255, 256, 257, 1000, 1024, 1025] + _counts((2, 17, 33))
CAPACITY = 2 ** 15  # the plain launch with whole-cell items; the same item cut at T = 8 and 7

# ends on a group / an item, one under, one over: inside one item, at the whole-cell cap, and in
# cells cut into items (1088 = 17 groups, 1280 = 5 items, 4352 = 17 items: a two-group root)
BOUNDARY_COUNTS = [63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 1087, 1088, 1089,
                   1279, 1280, 1281, 4352]


def _store(cells, gpu, dtype, origin=None, capacity=None):
    from ccmpc import engine
    if dtype == torch.float32 and origin is None:
        origin = np.array([c[:, 0].mean(0) for c in cells])
    return engine.ParticleStore.from_cells(cells, device=gpu, dtype=dtype,
                                           origin=origin if dtype == torch.float32 else None,
                                           capacity=capacity)


@DTYPES
def test_t8_prefix_equals_generic_t7(gpu, dtype):
    from ccmpc import cycle
    cells, _, ref = _clouds(8, PREFIX_COUNTS, 9508)
    C = len(cells)
    s8 = _store(cells, gpu, dtype, capacity=CAPACITY)
    s7 = _store([c[:, :7] for c in cells], gpu, dtype, capacity=CAPACITY)
    assert s8.n_bound == s7.n_bound <= 2 ** 15 and s8.offsets == s7.offsets
    if dtype == torch.float32:
        assert torch.equal(s8.origin, s7.origin)
    m8, c8, r8, p8 = _run_all(cycle.MinkowskiCycle(s8, [C], ref, ph=8))
    m7, c7, r7, p7 = _run_all(cycle.MinkowskiCycle(s7, [C], ref[:7], ph=8))
    assert r8.shape == (C, 28, 128) and r7.shape == (C, 21, 128)
    assert torch.equal(m8[:, :7], m7)
    assert torch.equal(c8[:, :14, :14], c7)
    assert torch.equal(p8[:, :7], p7)
    assert torch.equal(r8[:, :21], r7)
    assert bool(torch.isfinite(c8).all()) and bool(torch.isfinite(p8).all())


@DTYPES
def test_t8_group_and_item_boundaries(gpu, dtype):
    store = _check_one_ov(gpu, 8, BOUNDARY_COUNTS, dtype, seed=9518)
    assert store.n_bound <= 2 ** 15


@DTYPES
def test_t8_whole_groups_beside_a_nan_cell(gpu, dtype):
    """Cells of whole groups -- 256 (one whole-cell item, a full group in every wave) and 1280
    (five full items) -- each followed at once by a cell of NaN (offsets are multiples of 32, so
    the neighbour starts where the cell ends): the cell's outputs are finite and the same bits as
    with a benign neighbour."""
    from ccmpc import cycle
    cells, _, ref = _clouds(8, [256, 96, 1280, 96], 9528)
    bad = [c.copy() for c in cells]
    bad[1][:] = np.nan
    bad[3][:] = np.nan
    origin = np.array([c[:, 0].mean(0) for c in cells])
    outs = []
    for cs in (cells, bad):
        store = _store(cs, gpu, dtype, origin=origin)
        assert store.offsets[1] == 256 and store.offsets[3] == store.offsets[2] + 1280
        outs.append(_run_all(cycle.MinkowskiCycle(store, [4], ref)))
    for good, nan in zip(*outs):
        for j in (0, 2):
            assert torch.equal(good[j], nan[j])
    mean, cov, _, prob = outs[1]
    for j in (0, 2):
        assert bool(torch.isfinite(mean[j]).all()) and bool(torch.isfinite(cov[j]).all())
        assert bool(torch.isfinite(prob[j]).all())
    assert bool(torch.isnan(cov[1]).all()) and bool(torch.isnan(cov[3]).all())
    from ccmpc import engine
    h = engine.halfspaces(outs[1][2])
    for j in (0, 2):
        assert np.all(h[j]["status"] == 0)
        for f in ("d", "q00", "q11", "r00", "r11", "lower_bound"):
            assert np.all(np.isfinite(h[j][f])), (j, f)


@pytest.mark.parametrize("T", [7, 2])
def test_other_horizons_keep_the_generic_instance(gpu, T):
    store = _check_one_ov(gpu, T, BOUNDARY_COUNTS, torch.float64, seed=9538)
    assert store.n_bound <= 2 ** 15
