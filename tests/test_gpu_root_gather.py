"""The last arriver's root gather (gram.hpp gather_root) at every width it has a path for.

Below 2^18 particles a work item is 256 particles at every horizon used here (T <= 8: 16-row
tiles, 4 waves; T = 12: 4-row blocks; T = 16: two row blocks), and a cell of more than 1024
particles is cut into items, so a cell of k items meets in a root of k slabs:

  k <= 16        one group, summed in each thread
  17 .. 64       groups of 16 on different threads, added through LDS in index order
  65             two tree levels: the root then holds 5 level-1 slabs

One store holds all of them in mixed order, each with a ragged last item, so a cell's slab
numbering depends on its neighbours.  At T = 5 and T = 2 most of the 16 x 16 tile is dead rows,
which the gather must neither need nor leave for the finaliser to read.

For every shape: moments against NumPy (ddof = 1) at test_gpu_c3_sweep.py's tolerance; the
fused launch against the two-call path, a second launch and a graph replay, bit for bit; every
record's status, (t, tau) order, `which` and `side` against the oracle's generator; and every
cell of the mixed store against the same cell run alone, bit for bit.

Every bitwise comparison here is between two runs of the same gather at the same slab count, so
none of them pins the order in which the groups are added; NumPy at rtol 1e-10 is the only
independent reference.  The order is pinned by tools/bits_compare.py against the parent build
(profiles/r08/).
"""
import numpy as np
import pytest
import torch

from oracle import ccmpc_oracle as orc

pytestmark = pytest.mark.gpu

ITEM = 256
# items per cell, mixed so that no cell sits at a slab index that is a multiple of 16
ITEMS_T8 = (33, 5, 64, 17, 65, 16, 48, 20, 49, 32)
ITEMS_WIDE = (33, 17)          # the 4-row-block and two-row-block geometries


def _counts(items):
    # a ragged last item: 1 .. 255 particles, different for every cell
    return [(k - 1) * ITEM + 1 + (37 * (i + 1)) % (ITEM - 1) for i, k in enumerate(items)]


_CLOUDS = {}


def _clouds(T, items):
    """(cells, past, ref) for one OV whose modes are the cells; built once per shape."""
    key = (T, items)
    if key not in _CLOUDS:
        from ccmpc import synthetic
        rng = np.random.default_rng(np.random.Philox(7000 + T))
        p0 = np.array([190.0, -80.0])
        cells = [synthetic.mode_cloud(rng, n, T, p0) for n in _counts(items)]
        for c in cells:
            c.setflags(write=False)
        _CLOUDS[key] = (cells, p0 - np.array([2.0, 0.5]), synthetic.ego_ref(7000 + T, T))
    return _CLOUDS[key]


def _run_all(cyc):
    cyc.rec.zero_()
    cyc.run()
    return cyc.mean.clone(), cyc.cov.clone(), cyc.rec.clone(), cyc.prob_lower.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _check(gpu, T, items, dtype=torch.float64):
    from ccmpc import cycle, engine
    cells, past, ref = _clouds(T, items)
    C = len(cells)
    assert [-(-c.shape[0] // ITEM) for c in cells] == list(items)
    origin = np.array([c[:, 0].mean(0) for c in cells]) if dtype == torch.float32 else None
    store = engine.ParticleStore.from_cells(cells, device=gpu, dtype=dtype, origin=origin)
    assert store.n_bound <= 2 ** 18          # the plain launch: 256-particle items
    cyc = cycle.MinkowskiCycle(store, [C], ref)
    first = _run_all(cyc)

    # a second launch, the two-call path and a graph replay leave the same bits
    assert _same(first, _run_all(cyc))
    cyc.rec.zero_()
    cyc.run_unfused()
    assert _same(first, (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))
    cyc.rec.zero_()
    cyc.capture()
    cyc.replay()
    torch.cuda.synchronize(gpu)
    assert _same(first, (cyc.mean, cyc.cov, cyc.rec, cyc.prob_lower))

    # moments against NumPy on the positions the store holds
    mean, cov = first[0].cpu().numpy(), first[1].cpu().numpy()
    seen = [store.cell_positions(j) if dtype == torch.float32 else cells[j] for j in range(C)]
    for j, traj in enumerate(seen):
        X = traj.reshape(len(traj), 2 * T)
        np.testing.assert_allclose(cov[j], np.cov(X, rowvar=False), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(mean[j].reshape(-1), X.mean(0), rtol=1e-13)

    # records against the oracle's generator on the same clouds
    p = np.asarray(past, float).reshape(1, 2)
    oov = orc.OVehicle(T, p, np.ones(C) / C, seen, [orc._step_yaws(c, p[-1], T) for c in seen],
                       np.zeros((C, 2)), np.array([4.5, 2.5]))
    want = orc.minkowski_generator([oov], T, T, ref, with_l4=False)["records"]
    h = cyc.records().reshape(-1)
    assert len(h) == len(want) == C * T * (T - 1) // 2
    assert np.all(h["status"] == 0)
    np.testing.assert_array_equal(np.stack((h["t_tau"] >> 16, h["t_tau"] & 0xFFFF), 1),
                                  [(r["t"], r["tau"]) for r in want])
    np.testing.assert_array_equal(h["which"], [r["which"] for r in want])
    np.testing.assert_array_equal(h["side"], [r["side"] for r in want])

    # every cell alone (its own store, slabs numbered from 0, the mixed cycle's risk row)
    for j in range(C):
        alone = engine.ParticleStore.from_cells(
            [cells[j]], device=gpu, dtype=dtype, origin=None if origin is None else origin[j:j + 1])
        one = cycle.MinkowskiCycle(alone, [1], ref)
        one.risk = cyc.risk[j:j + 1].clone()
        got = _run_all(one)
        assert _same(got, tuple(x[j:j + 1] for x in first)), (j, items[j])


@pytest.mark.parametrize("T", [8, 5, 2])
def test_root_widths_mixed_store(gpu, T):
    _check(gpu, T, ITEMS_T8)


def test_root_widths_mixed_store_f32_origin(gpu):
    _check(gpu, 8, ITEMS_T8, torch.float32)


@pytest.mark.parametrize("T", [12, 16])     # 4-row blocks (Scheme4) | two row blocks (RB = 2)
def test_root_widths_other_geometries(gpu, T):
    _check(gpu, T, ITEMS_WIDE)


# Small cells through the shared tangent_frame / block_inverse (constraints.hpp) of the fused tail
# and the two-call kernel, at one 16 x 16 tile (T = 3) and at five and six 4-row blocks
# (T = 10, 11): a one-item cell finalises from the slab its own workgroup combined, the others
# from a gathered root of 5 and 6 slabs.
@pytest.mark.parametrize("T", [3, 10, 11])
def test_small_cells_short_horizons(gpu, T):
    _check(gpu, T, (1, 5, 6))
