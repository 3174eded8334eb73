"""compute_mvoe's set-up from trace and determinant (constraints.hpp) on the device: the columns
of the MVOE grid that tests/test_gpu_tail_precision.py had to narrow, the set-up's values and the
loop's last update through the CHAIN selftest kind, and the bytes of failed records.

Bounds.  Un-narrowed columns (aspect 1e6, S2 / S1 = 1e8; the float64 oracle is 1e-6 .. 2e-6 off
the exact Q there, so it cannot be the yardstick): e_f is the error of the host model of the
device's own operation order (tests/_tail_algebra.py) against the exact reference, worst over a
scale's cases, computed at test time; the device must be within max(8 e_f, 1e-12), the rule of
tests/test_gpu_tail_precision.py.  The last update: <= 8 ulp of the exact sqrt(N / D) of its own
float64 (N, D), the bound of test_mvoe_step_within_eight_ulp and for its reason (the hardware
estimate's accuracy is not documented; the roundings alone are <= 2 ulp).  No bound is read off
a GPU run.

The stop iterate is observed, not inferred: the CHAIN kind returns beta and the beta before the
last update, so run with maxiter = the exact iteration's count it must show a step under tol,
and with one fewer a step not under tol.

Measured on the MI355X (printed by the tests):
  un-narrowed columns, 24 clear stops   host model e_f beta 1.6e-11 Q 9.5e-13 (worst scale)
                                        device         beta 1.6e-11 Q 9.5e-13, 0 iterates off
  last update, 4303 (s, p2) pairs and the 644 grid cases   beta worst 1.57 ulp (bound: 8)
"""
import numpy as np
import pytest
import torch

import _tail_algebra as alg
import _tail_ref as ref

pytestmark = pytest.mark.gpu


def _selftest(kind, rows, out_width, tol=ref.TOL, maxiter=ref.MAXITER):
    from ccmpc import _lib, engine
    x = torch.as_tensor(np.ascontiguousarray(rows, np.float64), device="cuda")
    n = x.shape[0]
    y = torch.full((n, out_width), np.nan, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().ccmpc_selftest(kind, n, engine._p(x), engine._p(y), tol, maxiter,
                                          engine._stream()), "ccmpc_selftest")
    return y.cpu().numpy()


def _rows(cases):
    return np.array([[*np.reshape(c["S1"], 4), *np.reshape(c["S2"], 4)] for c in cases])


# ---- 1. the columns the grid runs at aspect 1e5 -------------------------------------------------
def test_unnarrowed_columns(gpu):
    """Aspect 1e6 with S2 / S1 = 1e8 at three scales, 8 clear stops each."""
    from ccmpc import _lib
    cases = alg.wide_cases()
    assert [sum(c["scale"] == sc for c in cases) for sc in alg.WIDE_SCALES] == [alg.WIDE_CLEAR] * 3
    rows = _rows(cases)
    y = _selftest(_lib.SELFTEST_MVOE, rows, 6)
    assert np.all(y[:, 5] == 1.0) and np.all(np.isfinite(y))
    e_f = {sc: [0.0, 0.0] for sc in alg.WIDE_SCALES}
    for c in cases:
        m, ex = alg.mvoe(c["S1"], c["S2"]), c["ref"]
        assert m["iters"] == ex["iters"]
        e = e_f[c["scale"]]
        e[0] = max(e[0], ref.rel(m["beta"], ex["beta"]))
        e[1] = max(e[1], ref.rel_fro(m["Q"], ex["Q"]))
    worst, bad = [0.0, 0.0], []
    for c, out in zip(cases, y):
        ex = c["ref"]
        eb, eq = ref.rel(out[0], ex["beta"]), ref.rel_fro(out[1:5], ex["Q"])
        worst = [max(worst[0], eb), max(worst[1], eq)]
        ab, aq = (ref.bound(v) for v in e_f[c["scale"]])
        if not (eb <= ab and eq <= aq and eq < ref.BAR_Q):
            bad.append((c["scale"], eb, ab, eq, aq))
    # the stop iterate: at maxiter = k (the exact count) the last step is under tol, at k - 1 not
    off = []
    for k in sorted({c["ref"]["iters"] for c in cases}):
        idx = [i for i, c in enumerate(cases) if c["ref"]["iters"] == k]
        at = _selftest(_lib.SELFTEST_CHAIN, rows[idx], 5, maxiter=k)
        off += [(idx[j], k, "no stop") for j in range(len(idx))
                if not abs(at[j, 2] - at[j, 4]) < ref.TOL]
        if k > 1:
            before = _selftest(_lib.SELFTEST_CHAIN, rows[idx], 5, maxiter=k - 1)
            off += [(idx[j], k, "early stop") for j in range(len(idx))
                    if not abs(before[j, 2] - before[j, 4]) >= ref.TOL]
    print(f"\nun-narrowed columns: host model e_f (beta, Q) per scale {e_f}; device worst beta "
          f"{worst[0]:.1e} Q {worst[1]:.1e}; {len(off)} stop iterates off")
    assert not bad, bad
    assert not off, off


# ---- 2. the set-up's values and the last update ---------------------------------------------------
def _last_update(s, p2, prev):
    """The exact sqrt(N / D) for the float64 N = fma(s, prev, 2) and D = fma(p2, prev, s)."""
    from fractions import Fraction as Q
    s, p2, prev = (Q(float(v)) for v in (s, p2, prev))
    N = ref.F(ref._rn(s * prev + 2))                      # an fma: one rounding of the exact value
    D = ref.F(ref._rn(p2 * prev + s))
    return ref.mp.sqrt(N / D)


def test_chain_setup_and_last_update(gpu):
    """The CHAIN kind over (s, p2) pairs in [2^-200, 2^200]^2 -- S1 = I and S2 = [[s, -p2 / 2],
    [1, 0]] must give the set-up exactly those s and p2 -- and over the MVOE grid's cases: beta
    is one update from the beta before it, <= 8 ulp from the exact sqrt(N / D) of that update's
    own (N, D), which is what makes the (beta, previous beta) pair of test 1 a witness of the
    stop."""
    from ccmpc import _lib
    ab = ref.prim_inputs()
    n = len(ab)
    prim = np.zeros((n, 8))
    prim[:, 0] = prim[:, 3] = 1.0
    prim[:, 4], prim[:, 5], prim[:, 6] = ab[:, 0], -0.5 * ab[:, 1], 1.0
    y = _selftest(_lib.SELFTEST_CHAIN, np.concatenate([prim, _rows(ref.mvoe_cases())]), 5)
    assert np.all(np.isfinite(y)) and np.all(y[:, 3] == 1.0)
    assert np.array_equal(y[:n, 0], ab[:, 0]) and np.array_equal(y[:n, 1], ab[:, 1])
    worst = max(ref.ulp_err(beta, _last_update(s, p2, prev)) for s, p2, beta, _, prev in y)
    print(f"\nlast update over {len(y)} rows: beta worst {worst:.3f} ulp")
    assert worst <= 8, worst


# ---- 3. failed records ----------------------------------------------------------------------------
SING_S1 = ([1.0, 2.0, 2.0, 4.0], [0.0, 0.0, 0.0, 0.0])       # test_mvoe_singular_first_matrix's
SING_C = np.array([[1.0, 2.0, 0.5, 0.1], [2.0, 4.0, 0.2, 0.3], [0.5, 0.2, 3.0, 0.4],
                   [0.1, 0.3, 0.4, 2.0]])                    # ..._singular_tau_block's


def test_failed_flags_through_the_selftest(gpu):
    from ccmpc import _lib
    rows = np.array([[*s1, 1.0, 0.0, 0.0, 1.0] for s1 in SING_S1])
    y = _selftest(_lib.SELFTEST_MVOE, rows, 6)
    assert np.all(y[:, 5] == 0.0) and np.all(np.isnan(y[:, 0:5]))
    assert np.all(_selftest(_lib.SELFTEST_CHAIN, rows, 5)[:, 3] == 0.0)
    p = _selftest(_lib.SELFTEST_PAIR, np.array([[*SING_C.reshape(16), 2.7, 18.4]]), 14)
    assert not np.any(np.isfinite(p[0, 0:8])) and np.all(np.isfinite(p[0, 8:12]))
    z = _selftest(_lib.SELFTEST_MVOE, np.hstack((p[:, 0:4], p[:, 4:8])), 6)
    assert np.all(np.isnan(z[0, 0:5]))


def _walsh(n, k):
    return 1.0 - 2.0 * ((np.arange(n) >> k) & 1)


def test_failed_records_through_a_two_step_cycle(gpu):
    """Four cells at T = 2 (one record each) of 64 particles on +-1 Walsh patterns, so every
    moment is exact: (0) the tau block a multiple of [[1, 2], [2, 4]]; (1) step t uncorrelated
    with step tau and its own block that multiple, so S1 = chi_r cov_infer is it too; (2) step
    t's particles all equal, S1 = 0; (3) a healthy neighbour.  The failed records carry
    CCMPC_REC_SINGULAR and NaN beta1, beta2, Q and QR; the neighbour's status stays 0."""
    from ccmpc import _lib, cycle, engine
    n = 64
    w = [_walsh(n, k) for k in range(5)]
    one = np.ones(n)

    def cell(x0, y0, x1, y1):
        return np.stack([np.stack([64.0 + x0, -32.0 + y0], -1),
                         np.stack([66.0 + x1, -31.5 + y1], -1)], 1)
    cells = [cell(w[0], 2 * w[0], w[0] + w[1], 0.5 * w[2]),
             cell(w[0], 0.5 * w[1], w[2], 2 * w[2]),
             cell(w[0], 0.5 * w[1], 0 * one, 0 * one),
             cell(w[0] + 0.5 * w[1], w[1], 0.5 * w[0] + w[2], w[3] + 0.25 * w[1])]
    ref_traj = np.array([[55.0, -28.0], [57.0, -27.5]])
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    cyc = cycle.MinkowskiCycle(store, [len(cells)], ref_traj)
    cyc.run()
    h = cyc.records().reshape(-1)
    cov = cyc.cov.cpu().numpy()
    # the premises, on the device's own covariance
    a = cov[0, 0, 0]
    assert a > 0 and np.array_equal(cov[0, 0:2, 0:2], a * np.array([[1.0, 2.0], [2.0, 4.0]]))
    b = cov[1, 2, 2]
    assert b > 0 and np.array_equal(cov[1, 2:4, 2:4], b * np.array([[1.0, 2.0], [2.0, 4.0]]))
    assert np.all(cov[1, 2:4, 0:2] == 0.0) and np.all(cov[2, 2:4, :] == 0.0)
    assert np.all(h["status"][:3] == _lib.REC_SINGULAR), h["status"]
    for f in ("beta1", "beta2", "q00", "q01", "q11", "r00", "r01", "r11"):
        assert np.all(np.isnan(h[f][:3])), (f, h[f])
    assert h["status"][3] == 0 and np.isfinite(h["beta1"][3]) and np.isfinite(h["r00"][3])
    assert np.array_equal(h["t_tau"], [1 << 16] * 4)
