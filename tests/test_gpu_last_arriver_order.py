"""The last arriver's path of the non-balanced RB = 1 cycle kernels, from the arrival ticket to the
last record store (gram.hpp gather_root / sum_group2 with the loads in summing order,
CCMPC_GATHER_ORDERED; moments.hip's wait in front of the finaliser, CCMPC_TAIL_LANDED;
constraints.hpp's pair table, CCMPC_PAIR_TABLE), at the cell sizes where the root gather takes
another path.  None of the three changes a value, so every check here holds on the library without
them too.

  whole cell        1 and 1 024 particles: one item, combined in LDS, no gather.
  <= 16 slabs       1 025 (5 items of 256), 1 792 (7) and 4 096 (16): one group in every thread,
                    ragged, odd and full.
  17 .. 32 slabs    4 097 and 8 192: two groups in the halves of a wave.
  two passes        8 193 (33 slabs): three groups through LDS.
  empty cell        between a full whole-cell item (1 024) and a full 16-slab cell (4 096).

Every case at T = 8 (the instances that know their horizon: the pair table) and T = 7
(run-time T: the closed-form pair_of), f64 and f32 store; every launch holds at most 2^15 bound
particles (the plain launch, whole-cell items up to 1 024).

Checks.  mean and cov against NumPy (ddof = 1) at tests/test_gpu_front_order.py's tolerances:
means rtol 1e-13, covariances rtol 1e-10 / atol 1e-12.  Every record and prob_lower against the
float64 oracle's minkowski_cell on the particles the store holds, at the tolerances
tests/test_gpu_cycle_args.py holds the same fields to: t_tau, which, side, status exact; Q and QR
1e-9 relative Frobenius; the centre 1e-13; d rel 1e-11; lower_bound rel 1e-8 / abs 1e-12;
prob_lower rtol 1e-8.  The fields no test compared so far: n1 is 1 exactly; n0 = (a0 - m0) /
(a1 - m1) is held to the first-order bound that the means' own tolerance e = 1e-13 allows,
2 e (|m0| + |n0| |m1|) / |a1 - m1| (the factor 2: the division's and the differences' rounding and
the second-order term); beta1 and beta2 to rel 1e-7, ten times the stop tolerance 1e-8 of the
fixed point, which the kernel and the oracle both iterate until a step is below it.
A cell of one particle or none has no covariance (np.cov: 0 / 0): its moments are NumPy's NaN,
its records keep their (t, tau) order and carry a non-zero status, and the oracle is not run on it.
"""
import warnings

import numpy as np
import pytest
import scipy.stats
import torch

from oracle import ccmpc_oracle as orc
from test_gpu_block_const import _moments_match_numpy, _run_all
from test_gpu_front_order import _cells, _same_bits, _store

pytestmark = pytest.mark.gpu

STORES = [(8, torch.float64), (8, torch.float32), (7, torch.float64), (7, torch.float32)]
STORE_IDS = ["T8-f64", "T8-f32", "T7-f64", "T7-f32"]

CASES = {
    "whole-cell": [1, 1024],
    "le16-slabs": [1025, 1792, 4096],
    "17to32-slabs": [4097, 8192],
    "two-pass": [8193],
    "empty-beside-full": [1024, 0, 4096],
}


def _fro_rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _oracle_cell(x, T, ref, n_cells, k):
    """orc.minkowski_cell with the risk allocation minkowski_generator gives cell k of one OV."""
    eps = orc.eps_ura_matrix([n_cells])[0, k] / T
    chi_r = scipy.stats.chi2.ppf(1 - eps, df=2)
    chi_p = scipy.stats.chi2.ppf(orc.TARGET_P, df=2)
    return orc.minkowski_cell(x.reshape(-1, 2), T, T, ref, eps, chi_r, chi_p)


def _check_records(hj, prob_j, recs, pl, ref, tag):
    np.testing.assert_array_equal(hj["status"], 0)
    np.testing.assert_array_equal(hj["t_tau"], [(r["t"] << 16) | r["tau"] for r in recs])
    np.testing.assert_array_equal(hj["which"], [r["which"] for r in recs])
    np.testing.assert_array_equal(hj["side"], [r["side"] for r in recs])
    worst = dict(Q=0.0, QR=0.0, centre=0.0, d=0.0, n0=0.0, beta=0.0, lb=0.0)
    for i, r in enumerate(recs):
        Q = np.array([[hj["q00"][i], hj["q01"][i]], [hj["q01"][i], hj["q11"][i]]])
        QR = np.array([[hj["r00"][i], hj["r01"][i]], [hj["r01"][i], hj["r11"][i]]])
        m0, m1 = r["mean"]
        a0, a1 = ref[r["t"]]
        n0 = r["n"][0]
        n0_tol = 2 * 1e-13 * (abs(m0) + abs(n0) * abs(m1)) / abs(a1 - m1)
        worst["Q"] = max(worst["Q"], _fro_rel(Q, r["Q"]))
        worst["QR"] = max(worst["QR"], _fro_rel(QR, r["QR"]))
        worst["centre"] = max(worst["centre"],
                              _fro_rel([hj["mean0"][i], hj["mean1"][i]], r["mean"]))
        worst["d"] = max(worst["d"], abs(hj["d"][i] - r["d"]) / abs(r["d"]))
        worst["n0"] = max(worst["n0"], abs(hj["n0"][i] - n0) / n0_tol)
        worst["beta"] = max(worst["beta"], abs(hj["beta1"][i] - r["beta1"]) / abs(r["beta1"]),
                            abs(hj["beta2"][i] - r["beta2"]) / abs(r["beta2"]))
        worst["lb"] = max(worst["lb"], abs(hj["lower_bound"][i] - r["lb"]) / max(abs(r["lb"]), 1e-4))
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in worst.items()),
          "(n0: in units of its bound)")
    for i, r in enumerate(recs):
        Q = np.array([[hj["q00"][i], hj["q01"][i]], [hj["q01"][i], hj["q11"][i]]])
        QR = np.array([[hj["r00"][i], hj["r01"][i]], [hj["r01"][i], hj["r11"][i]]])
        m0, m1 = r["mean"]
        a0, a1 = ref[r["t"]]
        n0 = r["n"][0]
        assert _fro_rel(Q, r["Q"]) < 1e-9, (tag, i)
        assert _fro_rel(QR, r["QR"]) < 1e-9, (tag, i)
        assert _fro_rel([hj["mean0"][i], hj["mean1"][i]], r["mean"]) < 1e-13, (tag, i)
        assert hj["d"][i] == pytest.approx(r["d"], rel=1e-11), (tag, i)
        assert hj["n1"][i] == 1.0 and r["n"][1] == 1.0, (tag, i)
        assert abs(hj["n0"][i] - n0) <= 2 * 1e-13 * (abs(m0) + abs(n0) * abs(m1)) / abs(a1 - m1), \
            (tag, i)
        assert hj["beta1"][i] == pytest.approx(r["beta1"], rel=1e-7), (tag, i)
        assert hj["beta2"][i] == pytest.approx(r["beta2"], rel=1e-7), (tag, i)
        assert hj["lower_bound"][i] == pytest.approx(r["lb"], rel=1e-8, abs=1e-12), (tag, i)
    np.testing.assert_allclose(prob_j, pl, rtol=1e-8)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("T,dtype", STORES, ids=STORE_IDS)
def test_gather_paths_against_the_oracle(gpu, T, dtype, case):
    from ccmpc import cycle
    counts = CASES[case]
    cells, ref = _cells(T, counts, 2500 + 10 * T + len(counts))
    store = _store(gpu, cells, dtype)
    assert store.n_bound <= 2 ** 15 and list(store.counts) == counts
    cyc = cycle.MinkowskiCycle(store, [len(cells)], ref)
    first = _run_all(cyc)
    assert _same_bits(first, _run_all(cyc))   # the arrival counters are back at zero
    torch.cuda.synchronize(gpu)
    seen = [store.cell_positions(j) if dtype == torch.float32 else cells[j]
            for j in range(len(cells))]
    with warnings.catch_warnings():          # np.cov of no or one sample: 0 / 0, as the kernel's
        warnings.simplefilter("ignore", RuntimeWarning)
        _moments_match_numpy(first, seen, T)
    P = T * (T - 1) // 2
    h = cyc.records()
    prob = cyc.prob_lower.cpu().numpy()
    assert h.shape == (len(cells), P) and prob.shape == (len(cells), T)
    order = [(t << 16) | tau for t in range(T) for tau in range(t)]
    for j, x in enumerate(seen):
        tag = f"{case} T{T} {str(dtype)[6:]} cell {j} (n = {counts[j]})"
        if counts[j] < 2:
            np.testing.assert_array_equal(h[j]["t_tau"], order)
            assert np.all(h[j]["status"] != 0), tag
            continue
        recs, pl = _oracle_cell(np.asarray(x, np.float64), T, ref, len(cells), j)
        assert len(recs) == P
        _check_records(h[j], prob[j], recs, pl, ref, tag)
