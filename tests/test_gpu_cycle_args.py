"""Every launch path of moments.hip whose argument list was reordered (the first 14 dwords of
moments_kernel / moments4_kernel are what locate and the particle addresses need, so that the
build can ask for them in SGPRs at wave start): a swapped or truncated argument must not pass.

Every argument that moved carries a value its neighbours do not: two cells of different counts and
offsets, `cell_ref = [1, 0]` onto two different reference rows, a per-cell origin on the f32 store,
and the four neighbouring integers n_cells (2 or 3), lg_wq (6; 9 in balanced mode), the whole-cell
cap (1024; 0 in balanced mode) and T (2, 7, 8, 10), which differ from one another in every case;
ld is the store's bound, far from all of them.

  T = 8, f64 and f32   moments_kernel<P, 1, true, false, 8>: cells of 300 and 40 particles under
                       n_bound <= 2^15, so `whole` (an int32 argument) is live: both cells are at
                       most the cap of 1024 and are whole-cell items, the 300-particle one longer
                       than a 256-particle chunk.  The f32 store has a non-zero origin per cell.
  T = 8, a cut cell    the same two cells behind one of 1300 particles, which is past the cap and
                       is cut into six items: slabs, arrival counters and the root gather, so the
                       `tree` argument is live (at the built cap the 300-particle cell is one item).
  T = 7                the generic RB = 1 instance (T is read from its argument).
  T = 10               moments4_kernel.
  ccmpc_moments        T = 8, the MINK = false instance (means and covariances only).
  balanced             the smallest store bound past 2^18 particles, the three cells, T = 2
                       (moments_kernel<P, 1, true, true>) and T = 10 (moments4_kernel<P, 5, true,
                       true>).

Checks, at tests/test_gpu_core.py's tolerances: means (rtol 1e-13) and covariances (relative
Frobenius 1e-11) against float64 NumPy on the same particles; records against
oracle.ccmpc_oracle.minkowski_cell -- (t, tau), `which`, `side` exact, status 0, Q and QR at 1e-9
relative Frobenius, the centre at 1e-13, d at 1e-11, lower_bound at rel 1e-8 / abs 1e-12 -- and
prob_lower at rtol 1e-8.  Nothing here is new behaviour: the file passes on the parent's library.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ccmpc_oracle as orc

pytestmark = pytest.mark.gpu

COUNTS = (300, 40)
CUT_COUNTS = (1300, 300, 40)
BALANCED_CAPACITY = 2 ** 18 + 32       # one alignment unit past the balanced-mode threshold


def fro_rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@functools.lru_cache(maxsize=None)
def _inputs(T, counts, f32):
    """Clouds, per-cell origins, the reference rows and their selector, and the particles as the
    store holds them (through float32 for the f32 store).  Built once per shape, never changed."""
    rng = np.random.default_rng(1700 + 10 * T + len(counts) + (5 if f32 else 0))
    cells = [190 + 6 * j + np.cumsum(rng.normal(0, 0.5, size=(n, T, 2)), axis=1)
             for j, n in enumerate(counts)]
    origin = np.array([[120.5 + 3 * j, -40.25 - 2 * j] for j in range(len(counts))])
    if f32:
        seen = [(c - origin[j]).astype(np.float32).astype(np.float64) + origin[j]
                for j, c in enumerate(cells)]
    else:
        seen = cells
    ref = np.array([[[170.0 + 4.0 * (t + 1), 10.0 + 0.5 * (t + 1)] for t in range(T)],
                    [[150.0 + 3.0 * (t + 1), 35.0 - 0.25 * (t + 1)] for t in range(T)]])
    cell_ref = [(j + 1) % 2 for j in range(len(counts))]          # [1, 0(, 1)]
    for a in cells + seen + [origin, ref]:
        a.setflags(write=False)
    return cells, origin, seen, ref, cell_ref


@functools.lru_cache(maxsize=None)
def _expected(T, counts, f32):
    """float64 NumPy moments and the oracle's records of every cell (one OV holding the cells)."""
    from ccmpc import risk
    _, _, seen, ref, cell_ref = _inputs(T, counts, f32)
    K = [len(counts)]
    cr = risk.cell_risk(risk.eps_ura(K), K, T)
    eps = orc.eps_ura_matrix(K)
    out = []
    for j, c in enumerate(seen):
        X = c.transpose(1, 2, 0).reshape(2 * T, -1)
        recs, pl = orc.minkowski_cell(c.reshape(-1, 2), T, T, ref[cell_ref[j]],
                                      eps[0, j] / T, cr[j, 0], cr[j, 1])
        out.append((X.mean(axis=1), np.cov(X), recs, pl))
    return out


def _store(gpu, T, counts, f32, capacity=None):
    from ccmpc import engine
    cells, origin, _, _, _ = _inputs(T, counts, f32)
    return engine.ParticleStore.from_cells(
        list(cells), device=gpu, dtype=torch.float32 if f32 else torch.float64,
        origin=origin.copy() if f32 else None, capacity=capacity)


def _check_moments(mean, cov, T, counts, f32):
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    for j, (m_ref, c_ref, _, _) in enumerate(_expected(T, counts, f32)):
        np.testing.assert_allclose(mean[j].reshape(-1), m_ref, rtol=1e-13)
        assert fro_rel(cov[j], c_ref) < 1e-11, (j, fro_rel(cov[j], c_ref))
        np.testing.assert_array_equal(cov[j], cov[j].T)


def _check_cycle(gpu, T, counts, f32, capacity=None):
    from ccmpc import cycle
    _, _, _, ref, cell_ref = _inputs(T, counts, f32)
    store = _store(gpu, T, counts, f32, capacity)
    cyc = cycle.MinkowskiCycle(store, [len(counts)], ref.copy(), cell_ref=cell_ref)
    cyc.run()
    torch.cuda.synchronize()
    _check_moments(cyc.mean, cyc.cov, T, counts, f32)
    h = cyc.records()
    prob = cyc.prob_lower.cpu().numpy()
    P = T * (T - 1) // 2
    assert h.shape == (len(counts), P)
    assert np.all(h["status"] == 0)
    for j, (_, _, recs, pl) in enumerate(_expected(T, counts, f32)):
        assert len(recs) == P
        hj = h[j]
        np.testing.assert_array_equal(hj["t_tau"] >> 16, [r["t"] for r in recs])
        np.testing.assert_array_equal(hj["t_tau"] & 0xFFFF, [r["tau"] for r in recs])
        np.testing.assert_array_equal(hj["which"], [r["which"] for r in recs])
        np.testing.assert_array_equal(hj["side"], [r["side"] for r in recs])
        for i, r in enumerate(recs):
            Q = np.array([[hj["q00"][i], hj["q01"][i]], [hj["q01"][i], hj["q11"][i]]])
            QR = np.array([[hj["r00"][i], hj["r01"][i]], [hj["r01"][i], hj["r11"][i]]])
            assert fro_rel(Q, r["Q"]) < 1e-9, (j, i)
            assert fro_rel(QR, r["QR"]) < 1e-9, (j, i)
            assert fro_rel([hj["mean0"][i], hj["mean1"][i]], r["mean"]) < 1e-13, (j, i)
            assert hj["d"][i] == pytest.approx(r["d"], rel=1e-11), (j, i)
            assert hj["lower_bound"][i] == pytest.approx(r["lb"], rel=1e-8, abs=1e-12), (j, i)
        np.testing.assert_allclose(prob[j], pl, rtol=1e-8)
    return store


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_t8_whole_cell_items(gpu, f32):
    store = _check_cycle(gpu, 8, COUNTS, f32)
    assert store.n_bound <= 2 ** 15 and store.offsets == [0, 320]
    if f32:
        o = store.origin.cpu().numpy()
        assert np.all(o != 0) and np.all(o[0] != o[1])


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_t8_cut_cell_uses_the_tree(gpu, f32):
    store = _check_cycle(gpu, 8, CUT_COUNTS, f32)
    assert store.n_bound <= 2 ** 15 and max(store.counts) > 1024


def test_t7_generic_instance(gpu):
    _check_cycle(gpu, 7, COUNTS, False)


def test_t10_scheme4(gpu):
    _check_cycle(gpu, 10, COUNTS, False)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_t8_moments_alone(gpu, f32):
    from ccmpc import engine
    mean, cov = engine.moments(_store(gpu, 8, COUNTS, f32))
    torch.cuda.synchronize()
    _check_moments(mean, cov, 8, COUNTS, f32)


@pytest.mark.parametrize("T", [2, 10])
def test_balanced_launch(gpu, T):
    store = _check_cycle(gpu, T, CUT_COUNTS, False, capacity=BALANCED_CAPACITY)
    assert store.n_bound == BALANCED_CAPACITY > 2 ** 18
