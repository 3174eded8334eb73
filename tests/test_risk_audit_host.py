"""Monte-Carlo risk audit, host side: the NumPy restatement of the contract on hand-made
cases, risk.audit_report's arithmetic, the binding's presence and ccmpc_risk_audit's argument
rejection (which happens before any device work)."""
import ctypes
import types

import numpy as np

import _audit_ref as ar


def _affine_rec(C, T):
    from ccmpc import _lib
    h = np.zeros((C, T), _lib.AFFINE_DTYPE)
    h["t"] = np.arange(T)[None, :]
    h["side"] = 1
    return h


def test_345_tie_is_not_a_hit():
    # particle exactly R = 5 away (3-4-5) is not hit; one a hair closer is
    cells = [np.array([[[3.0, 4.0]], [[3.0, 3.9375]], [[30.0, 40.0]]])]
    out = ar.audit(cells, 1, 5.0, plan=np.zeros((1, 2)))
    assert out["hit"].tolist() == [[1]] and out["hit_any"].tolist() == [1]
    assert out["min_d2"][0, 0] == 9.0 + 3.9375 * 3.9375
    tie_only = ar.audit([cells[0][:1]], 1, 5.0, plan=np.zeros((1, 2)))
    assert tie_only["hit"].tolist() == [[0]] and tie_only["min_d2"][0, 0] == 25.0


def test_tangent_record_protects():
    # x >= 5 (n = (1, 0), side +1, rhs 5): a particle at the origin is exactly R = 5 from the
    # feasible side: protected.  rhs a little smaller: open.  Wrong side of the particle: open.
    cells = [np.zeros((1, 1, 2))]
    h = _affine_rec(1, 1)
    h["n0"], h["rhs"] = 1.0, 5.0
    out = ar.audit(cells, 1, 5.0, rec=h, kind=ar.AFFINE)
    assert out["rec_open"].tolist() == [[0]] and out["open"].tolist() == [[0]]
    h["rhs"] = 4.9375
    out = ar.audit(cells, 1, 5.0, rec=h, kind=ar.AFFINE)
    assert out["rec_open"].tolist() == [[1]] and out["open"].tolist() == [[1]]
    h["rhs"], h["side"] = 5.0, -1                       # x <= 5 contains the particle
    out = ar.audit(cells, 1, 5.0, rec=h, kind=ar.AFFINE)
    assert out["rec_open"].tolist() == [[1]]
    h["rhs"] = -5.0                                     # x <= -5: tangent from the other side
    out = ar.audit(cells, 1, 5.0, rec=h, kind=ar.AFFINE)
    assert out["rec_open"].tolist() == [[0]]
    # scaling the normal changes nothing (no square root, |n|^2 on the right-hand side)
    h["n0"], h["rhs"] = 4.0, -20.0
    assert ar.audit(cells, 1, 5.0, rec=h, kind=ar.AFFINE)["rec_open"].tolist() == [[0]]


def test_failed_and_out_of_range_records_are_not_audited():
    cells = [np.zeros((3, 2, 2))]
    h = _affine_rec(1, 2)
    h["n0"], h["rhs"] = 1.0, 50.0                       # protects everything where audited
    h["status"][0, 0] = -11
    out = ar.audit(cells, 2, 5.0, rec=h, kind=ar.AFFINE)
    assert out["rec_open"].tolist() == [[-1, 0]]
    assert out["open"].tolist() == [[3, 0]]             # no status-0 record at t = 0: all open
    h["status"][0, 0] = 0
    h["t"][0, 1] = 2                                    # t outside [0, T)
    out = ar.audit(cells, 2, 5.0, rec=h, kind=ar.AFFINE)
    assert out["rec_open"].tolist() == [[0, -1]] and out["open"].tolist() == [[0, 3]]
    h["t"][0, 1] = -1
    assert ar.audit(cells, 2, 5.0, rec=h, kind=ar.AFFINE)["rec_open"].tolist() == [[0, -1]]


def test_halfspace_kinds_use_t_of_t_tau_and_compact_agrees():
    from ccmpc import _lib
    T = 3
    cells = [np.zeros((2, T, 2))]
    h = np.zeros((1, 3), _lib.HALFSPACE_DTYPE)
    h["t_tau"] = [[(1 << 16) | 0, (2 << 16) | 0, (2 << 16) | 1]]
    h["side"], h["n1"], h["d"] = 1, 1.0, [[5.0, 4.0, 6.0]]
    out = ar.audit(cells, T, 5.0, rec=h, kind=ar.HALFSPACE)
    assert out["rec_open"].tolist() == [[0, 2, 0]]
    assert out["open"].tolist() == [[2, 0, 0]]          # t = 0 has no record
    g = ar.compact(h, ar.HALFSPACE)
    out2 = ar.audit(cells, T, 5.0, rec=g, kind=ar.HALFSPACE_COMPACT)
    assert out2["rec_open"].tolist() == out["rec_open"].tolist()
    assert out2["open"].tolist() == out["open"].tolist()


def test_empty_cell():
    cells = [np.zeros((0, 2, 2)), np.ones((1, 2, 2))]
    h = _affine_rec(2, 2)
    h["n0"], h["rhs"] = 1.0, 50.0
    out = ar.audit(cells, 2, 5.0, plan=np.zeros((2, 2)), rec=h, kind=ar.AFFINE)
    assert out["hit"][0].tolist() == [0, 0] and out["hit_any"][0] == 0
    assert np.all(np.isinf(out["min_d2"][0])) and np.all(out["min_d2"][1] == 2.0)
    assert out["rec_open"][0].tolist() == [0, 0] and out["open"][0].tolist() == [0, 0]


def test_cell_plan_selects_the_row():
    cells = [np.zeros((1, 1, 2)), np.zeros((1, 1, 2))]
    plan = np.array([[[0.0, 0.0]], [[100.0, 0.0]]])
    out = ar.audit(cells, 1, 5.0, plan=plan, cell_plan=[1, 0])
    assert out["hit"].tolist() == [[0], [1]]


def test_audit_report_arithmetic_nan_and_budgets():
    from ccmpc import risk
    K, ph = [2, 1], 8
    audit = types.SimpleNamespace(
        hit=np.array([[0, 1], [0, 0], [5, 50]]), hit_any=np.array([1, 0, 50]),
        min_d2=np.array([[16.0, 4.0], [np.inf, np.inf], [1.0, 0.25]]),
        rec_open=np.array([[3], [0], [-1]]), open=np.array([[3, 1], [0, 0], [1000, 60]]))
    rep = risk.audit_report(audit, [400, 0, 1000], K, ph)
    assert np.array_equal(rep["budget_traj"], [0.025, 0.025, 0.025])
    assert np.array_equal(rep["budget_step"], np.array([0.025, 0.025, 0.025]) / 8)
    assert np.array_equal(rep["p_hit"][0], [0.0, 1 / 400])
    assert np.all(np.isnan(rep["p_hit"][1])) and np.isnan(rep["p_hit_any"][1])
    assert np.all(np.isnan(rep["p_open"][1]))
    assert np.array_equal(rep["p_hit"][2], [0.005, 0.05])
    assert np.array_equal(rep["p_hit_any"][[0, 2]], [1 / 400, 0.05])
    assert np.array_equal(rep["p_open"][2], [1.0, 0.06])
    assert np.array_equal(rep["min_dist"][0], [4.0, 2.0]) and np.isinf(rep["min_dist"][1, 0])
    assert rep["traj_within_budget"].tolist() == [True, False, False]
    assert rep["step_within_budget"].tolist() == [[True, True], [False, False], [False, False]]
    assert rep["worst"] == (2, 1) and rep["worst_p_hit"] == 0.05
    assert np.array_equal(rep["rec_open"], audit.rec_open)
    # other eps: eps / O
    assert np.array_equal(risk.audit_report(audit, [400, 0, 1000], K, ph, eps=0.1)["budget_traj"],
                          [0.05] * 3)
    # record-only audit: the plan half reports None and nothing raises
    only = types.SimpleNamespace(hit=None, hit_any=None, min_d2=None, rec_open=audit.rec_open,
                                 open=audit.open)
    rep = risk.audit_report(only, [400, 0, 1000], K, ph)
    assert rep["p_hit"] is None and rep["worst"] is None and rep["traj_within_budget"] is None
    assert np.array_equal(rep["p_open"][0], [3 / 400, 1 / 400])


def test_binding_has_the_audit():
    from ccmpc import _lib, cycle, engine, planner, risk
    assert "ccmpc_risk_audit" in _lib.SIGNATURES
    assert hasattr(_lib.load(), "ccmpc_risk_audit")
    assert callable(engine.risk_audit)
    assert engine.RiskAudit._fields == ("hit", "hit_any", "min_d2", "rec_open", "open")
    assert callable(cycle.MinkowskiCycle.audit) and callable(cycle.AffineCycle.audit)
    assert callable(risk.audit_report) and callable(planner.MidlevelAgent.audit_plan)


def _call(lib, T=8, R=3.4, plan=True, rec=False, kind=0, ld=64, outs=True, n_cells=0):
    """ccmpc_risk_audit with n_cells = 0 (nothing would be launched even if accepted) and dummy
    non-null addresses that are never dereferenced."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    o = p if outs else null
    return lib.ccmpc_risk_audit(p, 0, ld, T, null, p, p, n_cells, 0, p if plan else null, null,
                                p if rec else null, kind, R, o, o, o, o, o, null)


def test_argument_rejection_needs_no_device():
    from ccmpc import _lib
    lib = _lib.load()
    ERR_ARG = -1
    assert _call(lib) == 0                                # accepted: no cells, nothing launched
    assert _call(lib, rec=True, kind=3) == 0
    assert _call(lib, T=41) == ERR_ARG
    assert b"T must be" in lib.ccmpc_last_error()
    assert _call(lib, T=0) == ERR_ARG
    assert _call(lib, R=0.0) == ERR_ARG
    assert _call(lib, R=-1.0) == ERR_ARG
    assert _call(lib, R=float("inf")) == ERR_ARG
    assert _call(lib, R=float("nan")) == ERR_ARG
    assert _call(lib, plan=False, rec=False) == ERR_ARG
    assert b"both null" in lib.ccmpc_last_error()
    assert _call(lib, rec=True, kind=4) == ERR_ARG
    assert _call(lib, rec=True, kind=-1) == ERR_ARG
    assert _call(lib, ld=66) == ERR_ARG
    assert _call(lib, outs=False) == ERR_ARG              # missing outputs of an enabled half
    assert _call(lib, plan=False, rec=True, outs=False) == ERR_ARG
    assert lib.ccmpc_abi_version() == 2
