"""Host tests of the Monte-Carlo offset calibration: the NumPy restatement
(tests/_quantile_ref.py) against a brute-force definition, its two round-trip consequences
through the audit's restatement, the report arithmetic, and ccmpc_risk_quantile's argument
checks through the loaded library (host-only calls: nothing is launched)."""
import ctypes
import types

import numpy as np
import pytest

import _audit_ref as ar
import _quantile_ref as qr

R = 3.4


def _records(rng, C, T, kind, plan_like):
    from ccmpc import _lib
    half = kind in (ar.HALFSPACE, ar.HALFSPACE_COMPACT)
    P = ar.rows(kind, T)
    h = np.zeros((C, P), _lib.HALFSPACE_DTYPE if half else _lib.AFFINE_DTYPE)
    t_of = (np.array([t for t in range(T) for _ in range(t)], np.int64) if half
            else np.arange(T))
    n = rng.uniform(-2, 2, (C, P, 2))
    h["n0"], h["n1"] = n[..., 0], n[..., 1]
    h["side"] = rng.choice([-1, 1], (C, P))
    h["d" if half else "rhs"] = (n * plan_like).sum(-1) + rng.uniform(-5, 5, (C, P))
    if half:
        h["t_tau"] = t_of[None] << 16
    else:
        h["t"] = t_of[None]
    return h


def _brute_offset(n0, n1, side, px, py):
    """Walk over adjacent doubles from the square-root estimate to the predicate's threshold."""
    w = side * (n0 * px + n1 * py) + 0.0
    u = w + np.sqrt(R * R * (n0 * n0 + n1 * n1))
    ok = lambda v: bool(ar.protects(n0, n1, side * v, side, px, py, R))   # noqa: E731
    for _ in range(100000):
        if not ok(u):
            u = np.nextafter(u, np.inf)
        elif ok(np.nextafter(u, -np.inf)):
            u = np.nextafter(u, -np.inf)
        else:
            return u
    raise AssertionError("no threshold near the estimate")


def test_keys_order_doubles():
    x = np.array([-np.inf, -1e300, -1.0, -5e-324, 0.0, 5e-324, 1.0, 2.0, 1e300, np.inf])
    k = qr.key(x)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(qr.unkey(k).view(np.int64), x.view(np.int64))
    assert int(k[0]) == qr.KEY_NEG_INF and int(k[-1]) == qr.KEY_POS_INF


@pytest.mark.parametrize("kind", [ar.HALFSPACE, ar.AFFINE])
def test_reference_equals_brute_force(kind):
    rng = np.random.default_rng(11 + kind)
    T, counts = 4, [0, 1, 2, 7, 7, 7, 7, 7]
    cells = [rng.uniform(-30, 30, (1, 1, 2)) + rng.uniform(-6, 6, (n, T, 2)) for n in counts]
    N = 7
    allow = [0, 0, 1, 0, 1, N - 1, N, N + 1]
    h = _records(rng, len(counts), T, kind, rng.uniform(-30, 30, 2))
    got = qr.quantile(cells, T, R, h, kind, allow)
    n0, n1, rhs, side, status, t = ar.rec_fields(h, kind)
    n_cal = 0
    for c, x in enumerate(cells):
        for p in range(ar.rows(kind, T)):
            if allow[c] >= x.shape[0]:
                assert got["status"][c, p] == qr.CAL_VACUOUS and got["q"][c, p] == -np.inf
                assert got["rhs"][c, p] == rhs[c, p]
                continue
            tp = int(t[c, p])
            w = side[c, p] * (n0[c, p] * x[:, tp, 0] + n1[c, p] * x[:, tp, 1]) + 0.0
            want_q = sorted(w.tolist(), reverse=True)[allow[c]]
            assert got["status"][c, p] == 0 and got["q"][c, p] == want_q
            i = int(np.flatnonzero(w == want_q)[0])
            u = _brute_offset(n0[c, p], n1[c, p], side[c, p], x[i, tp, 0], x[i, tp, 1])
            assert got["rhs"][c, p] == side[c, p] * u
            n_cal += 1
    assert n_cal >= 20


def test_ties_straddling_the_rank_and_negative_zero():
    from ccmpc import _lib
    T = 1
    # projections along n = (1, 0), side +1: 5, 5, 5, 2, 2, -1  (ties straddle ranks 1..2 and 4)
    x = np.zeros((6, T, 2))
    x[:, 0, 0] = [5.0, 2.0, 5.0, -1.0, 2.0, 5.0]
    h = np.zeros((1, 1), _lib.AFFINE_DTYPE)
    h["n0"], h["side"], h["rhs"] = 1.0, 1, 100.0
    for m, want, gt, ge in ((0, 5.0, 0, 3), (1, 5.0, 0, 3), (2, 5.0, 0, 3), (3, 2.0, 3, 5),
                            (4, 2.0, 3, 5), (5, -1.0, 5, 6)):
        got = qr.quantile([x], T, R, h, ar.AFFINE, [m])
        assert got["q"][0, 0] == want and got["n_gt"][0, 0] == gt and got["n_ge"][0, 0] == ge
        assert gt <= m < ge
        assert got["rhs"][0, 0] == _brute_offset(1.0, 0.0, 1.0, want, 0.0)
        assert abs(got["rhs"][0, 0] - (want + R)) < 1e-14
    assert qr.quantile([x], T, R, h, ar.AFFINE, [6])["status"][0, 0] == qr.CAL_VACUOUS
    assert qr.quantile([x], T, R, h, ar.AFFINE, [-1])["status"][0, 0] == qr.CAL_SKIPPED
    # a normal orthogonal to every particle with side -1: every s is +0, side*s is -0, w is +0
    x = np.zeros((4, T, 2))
    x[:, 0, 1] = [1.0, 2.0, 3.0, 4.0]
    h["side"] = -1
    got = qr.quantile([x], T, R, h, ar.AFFINE, [1])
    assert got["q"].view(np.int64)[0, 0] == 0        # +0.0, not -0.0
    assert got["n_gt"][0, 0] == 0 and got["n_ge"][0, 0] == 4
    assert got["rhs"][0, 0] == -_brute_offset(1.0, 0.0, -1.0, 0.0, 1.0)
    assert abs(got["rhs"][0, 0] + R) < 1e-14


def test_skipped_records_keep_their_rhs():
    from ccmpc import _lib
    rng = np.random.default_rng(3)
    T = 3
    x = rng.uniform(-5, 5, (9, T, 2))
    h = _records(rng, 1, T, ar.AFFINE, np.zeros(2))
    h["status"][0, 0] = _lib.REC_NONFINITE
    h["t"][0, 1] = T
    h["n0"][0, 2] = np.nan
    got = qr.quantile([x], T, R, h, ar.AFFINE, [2])
    assert got["status"].tolist() == [[qr.CAL_SKIPPED] * 3]
    assert np.all(np.isnan(got["q"])) and np.array_equal(got["rhs"], h["rhs"])
    h["n0"][0, 2] = np.inf
    assert qr.quantile([x], T, R, h, ar.AFFINE, [2])["status"][0, 2] == qr.CAL_SKIPPED


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("kind", [ar.HALFSPACE, ar.AFFINE])
def test_round_trip_through_the_audit(kind, ties):
    """rhs <- out_rhs: rec_open == #{w > q} <= m; u* one ulp towards the particles:
    rec_open >= #{w >= q} > m."""
    rng = np.random.default_rng(40 + 2 * kind + ties)
    T, counts = 5, [1, 2, 33, 200]
    cells = [rng.uniform(-30, 30, (1, 1, 2)) + rng.uniform(-6, 6, (n, T, 2)) for n in counts]
    h = _records(rng, len(counts), T, kind, rng.uniform(-30, 30, 2))
    if ties:
        cells = [np.round(x * 4) / 4 for x in cells]
        h["n0"], h["n1"] = np.round(h["n0"] * 4) / 4, np.round(h["n1"] * 4) / 4
        h["n0"][(h["n0"] == 0) & (h["n1"] == 0)] = 1.0
    allow = np.array([0, 1, 3, 17])
    got = qr.quantile(cells, T, R, h, kind, allow)
    assert np.all(got["status"] == 0)
    name = "d" if kind == ar.HALFSPACE else "rhs"
    side = h["side"].astype(np.float64)
    cal = h.copy()
    cal[name] = got["rhs"]
    a = ar.audit(cells, T, R, rec=cal, kind=kind)["rec_open"]
    assert np.array_equal(a, got["n_gt"]) and np.all(a <= allow[:, None])
    cal[name] = side * np.nextafter(side * got["rhs"], -np.inf)
    b = ar.audit(cells, T, R, rec=cal, kind=kind)["rec_open"]
    assert np.all(b >= got["n_ge"]) and np.all(b > allow[:, None])
    if ties:
        assert np.any(got["n_ge"] - got["n_gt"] > 1)


def test_allow_counts_and_report_arithmetic():
    from ccmpc import risk
    K, ph = [2, 1], 8
    counts = [400, 0, 1000]
    allow = risk.allow_counts(counts, K, ph)
    assert allow.dtype == np.int64
    assert allow.tolist() == [int(np.floor(0.025 / 8 * 400)), 0, int(np.floor(0.025 / 8 * 1000))]
    assert risk.allow_counts(counts, K, ph, eps=0.8).tolist() == [20, 0, 50]
    with pytest.raises(ValueError):
        risk.allow_counts([1, 2], K, ph)
    quant = types.SimpleNamespace(
        q=np.array([[1.0, 2.0], [-np.inf, -np.inf], [0.5, np.nan]]),
        rhs=np.array([[4.0, -7.0], [9.0, 9.0], [2.0, 5.0]]),
        status=np.array([[0, 0], [1, 1], [0, 2]], np.int32))
    n0 = np.array([[3.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    n1 = np.array([[4.0, 2.0], [0.0, 0.0], [0.5, 0.0]])
    rhs = np.array([[14.0, -6.0], [9.0, 9.0], [1.0, 5.0]])
    side = np.array([[1.0, -1.0], [1.0, 1.0], [1.0, 1.0]])
    rep = risk.calibration_report(quant, (n0, n1, rhs, side), counts, K, ph)
    assert np.array_equal(rep["slack"][0], [10.0, -1.0])       # side*rhs - side*rhs_cal
    assert np.array_equal(rep["slack_m"][0], [2.0, -0.5])      # / |n| = 5, 2
    assert np.all(np.isnan(rep["slack"][1])) and np.isnan(rep["slack"][2, 1])
    assert rep["slack"][2, 0] == -1.0 and rep["slack_m"][2, 0] == -2.0
    assert rep["worst_rec"].tolist() == [1, -1, 0]
    assert rep["worst_slack_m"][0] == -0.5 and np.isnan(rep["worst_slack_m"][1])
    assert rep["worst_slack_m"][2] == -2.0
    assert np.array_equal(rep["status"], quant.status) and rep["counts"].tolist() == counts
    assert np.array_equal(rep["budget_step"], np.full(3, 0.025 / 8))
    assert np.array_equal(rep["allow"], allow)
    assert np.array_equal(rep["rhs_cal"], quant.rhs) and np.array_equal(rep["rhs"], rhs)


def test_binding_has_the_calibration():
    from ccmpc import _lib, cycle, engine, planner, risk
    for name in ("ccmpc_risk_quantile", "ccmpc_risk_quantile_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert engine.RiskQuantile._fields == ("q", "rhs", "status", "workspace")
    assert callable(engine.risk_quantile) and callable(engine.calibrated_records)
    assert callable(cycle.MinkowskiCycle.calibrate) and callable(cycle.AffineCycle.calibrate)
    assert callable(risk.allow_counts) and callable(risk.calibration_report)
    assert callable(planner.MidlevelAgent.calibrate_constraints)
    assert (_lib.CAL_VACUOUS, _lib.CAL_SKIPPED) == (qr.CAL_VACUOUS, qr.CAL_SKIPPED)
    assert _lib.GATHER_DTYPE == ar.GATHER_DTYPE
    assert engine._rec_layout(_lib.REC_KIND_HALFSPACE) == (128, 16, 116, 4)
    assert engine._rec_layout(_lib.REC_KIND_AFFINE) == (128, 32, 116, 4)
    assert engine._rec_layout(_lib.REC_KIND_AFFINE_COMPACT) == (32, 16, 24, 2)


def _call(lib, T=8, R=3.4, kind=0, ld=64, outs=True, n_cells=0, ws_bytes=None, bound=0):
    """ccmpc_risk_quantile with n_cells = 0 (nothing would be launched even if accepted) and
    dummy non-null addresses that are never dereferenced."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    o = p if outs else null
    if ws_bytes is None:
        ws_bytes = lib.ccmpc_risk_quantile_workspace_bytes(min(max(T, 1), 40), kind % 4, n_cells)
    return lib.ccmpc_risk_quantile(p, 0, ld, T, null, p, p, n_cells, bound, p, kind, R, null, p,
                                   ws_bytes, o, o, o, null)


def test_argument_rejection_needs_no_device():
    from ccmpc import _lib
    lib = _lib.load()
    ERR_ARG = -1
    assert _call(lib) == 0                                # accepted: no cells, nothing launched
    assert _call(lib, kind=3) == 0
    assert _call(lib, T=1, kind=0, outs=False) == 0       # P = 0: no rows, no outputs needed
    assert _call(lib, T=41) == ERR_ARG
    assert b"T must be" in lib.ccmpc_last_error()
    assert _call(lib, T=0) == ERR_ARG
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(lib, R=bad) == ERR_ARG
    assert _call(lib, kind=4) == ERR_ARG
    assert _call(lib, kind=-1) == ERR_ARG
    assert _call(lib, ld=66) == ERR_ARG
    assert _call(lib, outs=False) == ERR_ARG
    assert b"null output" in lib.ccmpc_last_error()
    assert _call(lib, T=1, kind=1, outs=False) == ERR_ARG
    assert _call(lib, ws_bytes=0) == ERR_ARG
    assert b"workspace too small" in lib.ccmpc_last_error()
    # a workspace one byte short, with cells (rejected before anything is launched)
    need = lib.ccmpc_risk_quantile_workspace_bytes(8, 0, 5)
    assert _call(lib, n_cells=5, ws_bytes=need - 1) == ERR_ARG
    assert _call(lib, bound=1 << 32) == ERR_ARG
    assert lib.ccmpc_abi_version() == 2


def test_workspace_size_query():
    from ccmpc import _lib
    lib = _lib.load()
    q = lib.ccmpc_risk_quantile_workspace_bytes
    assert q(8, 0, 4) >= 4 * 28 * (1024 + 32 + 8) and q(8, 1, 4) >= 4 * 8 * (1024 + 32 + 8)
    assert q(8, 0, 4) == q(8, 2, 4) and q(8, 1, 4) == q(8, 3, 4)
    assert q(40, 0, 8) >= 8 * 780 * 1024
    assert q(1, 0, 4) > 0 and q(8, 0, 0) > 0              # no rows / no cells: still accepted
    assert q(0, 0, 4) == 0 and q(41, 0, 4) == 0           # rejected arguments
    assert q(8, 4, 4) == 0 and q(8, -1, 4) == 0 and q(8, 0, -1) == 0
