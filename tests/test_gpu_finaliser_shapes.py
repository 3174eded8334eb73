"""The moments finaliser (gram.hpp finalize_cell) at the smallest shapes where it can go wrong,
through ccmpc_moments and, from T = 2, through ccmpc_minkowski_cycle:

  T = 1            two live rows: nearly every entry of the 16 x 16 tile unused
  T = 2            the same through the cycle (one half-space per cell)
  T = 8            the Gram is as large as the workgroup: every thread one entry
  T = 9, T = 12    4-row blocks (Scheme4): 240 entries, one per thread, and 336, the entry loop
  T = 13           two row blocks, 768 entries: the entry loop

each on cells of 0, 1, 2, 3 particles (n - 1 <= 0: NaN, as before), 257 (one 256-particle item
plus one particle: a gathered root of two slabs),
700 (one item where cells up to 1024 are whole-cell items) and 5 000 (a root of 20 slabs: the
gather with two groups per wave), in a store below 2^15 particles (whole-cell items at T <= 8)
and in one whose capacity is above it (256-particle items).  Then a cell with an infinite and one
with a NaN coordinate, and the float32 store with an origin.

Reference: finalize_cell's expressions restated in NumPy float64 on the positions the store
holds -- shift by the cell's first particle, S = sum, G = Y^T Y, mean = (shift + S / n) + origin,
cov = (G - S S^T / n) / (n - 1) -- so a non-finite input and a count below two give NaN and
infinity where the kernel's arithmetic does.  Bounds: NaN pattern and infinities equal; the mean
at rtol 1e-13 (the suite's bound for means); every covariance entry within 1e-12 of the cell's
largest |entry| (the suite's 1e-12 for moments, taken relative to the cell's scale: the two sides
differ by the order of sums of n <= 5 000 products, n 2^-53 = 6e-13 of the sum of their
magnitudes at worst, and the shift keeps those sums at the covariance's scale).

Each case also runs after ccmpc_poison_lds(NaN) and ccmpc_poison_lds(0) and must leave the same
bytes (tests/test_gpu_lds_poison.py), and the cycle's moments must be ccmpc_moments' bits.
"""
import numpy as np
import pytest
import torch

from ccmpc import _lib, cycle, engine, synthetic

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 257, 700, 5000)
ITEMS_256 = 2 ** 15 + 32          # a capacity past the whole-cell items' bound

CASES = [("T1", 1, "f64", None, None)]
for _T in (2, 8, 9, 12, 13):
    CASES += [(f"T{_T}-tiny", _T, "f64", None, None), (f"T{_T}-items", _T, "f64", ITEMS_256, None)]
CASES += [("T8-nonfinite", 8, "f64", ITEMS_256, "nonfinite"),
          ("T8-nonfinite-tiny", 8, "f64", None, "nonfinite"),
          ("T8-f32", 8, "f32", ITEMS_256, None), ("T9-f32", 9, "f32", None, None)]

_BUILT = {}


def _case(name, T, dt, capacity, tweak):
    """(cells, origin, ref) of a case, built once and left unchanged."""
    if name not in _BUILT:
        rng = np.random.default_rng(np.random.Philox(9100 + T))
        p0 = np.array([188.0, -77.0])
        cells = [synthetic.mode_cloud(rng, n, T, p0) for n in COUNTS]
        if tweak == "nonfinite":
            cells[5][350, 3, 1] = np.inf        # the one-item cell (or its middle slab)
            cells[6][2600, 5, 0] = np.nan       # slab 10 of the 20-slab root
        origin = None
        if dt == "f32":
            origin = np.array([c[:, 0].mean(0) if len(c) else p0 for c in cells])
        for c in cells:
            c.setflags(write=False)
        _BUILT[name] = (cells, origin, synthetic.ego_ref(9100 + T, T))
    return _BUILT[name]


def _restated(store, j):
    """finalize_cell's expressions in NumPy float64 on cell j as the store holds it."""
    n, o, rows = store.counts[j], store.offsets[j], 2 * store.T
    X = store.pos[:, o:o + n].double().cpu().numpy().T            # (n, 2T), the store's frame
    shift = X[0] if n else np.zeros(rows)
    Y = X - shift
    S, G = Y.sum(0), Y.T @ Y
    org = np.zeros(2) if store.origin is None else store.origin[j].cpu().numpy()
    with np.errstate(all="ignore"):
        mean = (shift + S / np.float64(n)) + np.tile(org, store.T)
        cov = (G - np.outer(S, S) / np.float64(n)) / (np.float64(n) - 1.0)
    return mean, cov


def _check_against_restatement(store, mean, cov, refs):
    for j in range(store.n_cells):
        m_ref, c_ref = refs[j]
        m, c = mean[j].reshape(-1), cov[j]
        fin_m, fin_c = np.isfinite(m_ref), np.isfinite(c_ref)
        assert np.array_equal(np.isnan(m), np.isnan(m_ref)), (j, "mean NaN pattern")
        assert np.array_equal(np.isnan(c), np.isnan(c_ref)), (j, "cov NaN pattern")
        assert np.array_equal(m[~fin_m & ~np.isnan(m_ref)], m_ref[~fin_m & ~np.isnan(m_ref)])
        assert np.array_equal(c[~fin_c & ~np.isnan(c_ref)], c_ref[~fin_c & ~np.isnan(c_ref)])
        np.testing.assert_allclose(m[fin_m], m_ref[fin_m], rtol=1e-13, atol=0)
        if fin_c.any():
            scale = np.abs(c_ref[fin_c]).max()
            err = np.abs(c[fin_c] - c_ref[fin_c]).max()
            assert err <= 1e-12 * scale, (j, store.counts[j], err / max(scale, 1e-300))
        assert np.array_equal(c, c.T, equal_nan=True)


def _poison(v):
    _lib.check(_lib.load().ccmpc_poison_lds(v, engine._stream()), "ccmpc_poison_lds")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,T,dt,capacity,tweak", CASES, ids=[c[0] for c in CASES])
def test_finaliser_shapes(gpu, name, T, dt, capacity, tweak):
    cells, origin, ref = _case(name, T, dt, capacity, tweak)
    store = engine.ParticleStore.from_cells(
        cells, device=gpu, dtype=torch.float64 if dt == "f64" else torch.float32, origin=origin,
        capacity=capacity)
    assert (store.n_bound > 2 ** 15) == (capacity is not None)
    refs = [_restated(store, j) for j in range(store.n_cells)]

    mean, cov = engine.moments(store)
    torch.cuda.synchronize()
    first = (mean.cpu().numpy(), cov.cpu().numpy())
    _check_against_restatement(store, *first, refs)
    for fill in (float("nan"), 0.0):
        _poison(fill)
        m, c = engine.moments(store)
        torch.cuda.synchronize()
        assert m.cpu().numpy().tobytes() == first[0].tobytes(), fill
        assert c.cpu().numpy().tobytes() == first[1].tobytes(), fill
    if T < 2:
        return                      # no (t, tau) pair: the cycle has no half-space to build

    cyc = cycle.MinkowskiCycle(store, [store.n_cells], ref)
    cyc.rec.zero_()
    cyc.run()
    torch.cuda.synchronize()
    got = (cyc.mean.cpu().numpy(), cyc.cov.cpu().numpy())
    _check_against_restatement(store, *got, refs)
    assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes()
    rec, low = cyc.rec.cpu().numpy().copy(), cyc.prob_lower.cpu().numpy().copy()
    for fill in (float("nan"), 0.0):
        _poison(fill)
        cyc.rec.zero_()
        cyc.run()
        torch.cuda.synchronize()
        assert cyc.mean.cpu().numpy().tobytes() == got[0].tobytes(), fill
        assert cyc.cov.cpu().numpy().tobytes() == got[1].tobytes(), fill
        assert cyc.rec.cpu().numpy().tobytes() == rec.tobytes(), fill
        assert cyc.prob_lower.cpu().numpy().tobytes() == low.tobytes(), fill
