"""planner.MidlevelAgent.calibrate_face_rows and tighten_face_plan: a synthetic scene whose
particles share one heading per step, where the sample cuts are exact and the tightened plan must
meet the particle budget; and the golden scene faces_o2_t8 with its reference shifted 10 m (the
instance of tests/test_gpu_face_audit_planner.py), where the calibration must agree with the
audit and the tightening's outcome is recorded, not asserted."""
import functools

import numpy as np
import pytest

import _face_audit_ref as ar
import _socp_ref as sr
from _faces_ref import CAR_R, LAT, LON, scene_cells

pytestmark = pytest.mark.gpu

TOL_G = 1e-6
SYN_T, SYN_N, SYN_OUT = 8, 640, 12


class Params:
    def __init__(self, O, K, frame):
        self.O, self.K, self.frame = O, np.asarray(K), frame


@functools.lru_cache(maxsize=None)
def common_heading_scene():
    """One OV, one mode, 640 particles: p_i(t) = p_i(0) + D(t) with one displacement D for all of
    them, so every particle has the heading of D(t) - D(t - 1) at t >= 1 (up to the rounding of
    its own differences): v_f has one gradient per (t, f), q is affine in the plan and the sample
    cut is exact.  Step 0's heading is measured from past_last and differs between particles;
    there the cloud is 5.7 m to the ego's left, far from any active row.  The cloud drives along
    the straight reference at 5 m/s, 3.8 m to its left at t = 4 and 0.12 (t - 4)^2 further at the
    other steps; 12 of the 640 particles stand 0.6 m nearer to the ego than the rest (spread
    0.05 m).  The Gaussian row moves the plan by Gamma sigma ~ 0.25 m, which leaves those 12 open;
    the per-step budget 0.05 / 8 allows 4.  Returns (ref, cell (n, T, 2), past_last)."""
    rng = np.random.default_rng(7)
    T, n = SYN_T, SYN_N
    ref = np.stack([150.0 + 3.0 * np.arange(1, T + 1), np.full(T, -60.0)], -1)
    lat = rng.normal(0, 0.05, size=n)
    lat[:SYN_OUT] = -0.6 + rng.normal(0, 0.01, size=SYN_OUT)
    x0 = 155.0 + rng.normal(0, 0.3, size=n)
    off = 3.8 + 0.12 * (np.arange(T) - 4.0) ** 2
    cell = np.stack((x0[:, None] + 2.5 * np.arange(T)[None, :],
                     -60.0 + off[None, :] + lat[:, None]), -1)
    past = cell[:, 0].mean(0) - np.array([2.5, off[0] - (3.8 + 0.12 * 25.0)])
    return ref, cell, past


@pytest.fixture(scope="module")
def synthetic(gpu):
    from ccmpc import ovehicle, planner
    ref, cell, past = common_heading_scene()
    ovs = ovehicle.scene_from_positions([[cell]], [past[None]], device=gpu)
    agent = planner.MidlevelAgent(prediction_horizon=SYN_T, device=gpu)
    prob = sr.model(ref, SYN_T)
    agent.compute_obstacle_constraints_GMM_approx(
        Params(1, [1], 100), ovs, None, None, None, np.array([[0.05]]), None, SYN_T, ref)
    return dict(agent=agent, prob=prob, ref=ref, cell=cell, past=past)


def test_synthetic_scene_is_tightened_to_the_budget(synthetic):
    from ccmpc import risk
    agent, prob, ref = synthetic["agent"], synthetic["prob"], synthetic["ref"]
    T = SYN_T
    src, last, aud_src = agent._face_src, agent._last_rec, agent._audit_src
    allow = risk.allow_counts([SYN_N], [1], T, 0.05)
    assert allow.tolist() == [4]
    sel = agent._face_selection(src[5], 1, T, None)
    assert np.all(sel >= 0)                                    # the OV is gated: every step has a row

    # the premise: the SOCP plan leaves more than `allow` particles open under a selected row
    socp = agent.solve_planning_socp(prob["x_init"], prob["goal"], ref, T, tol_g=TOL_G)
    v, _, _ = ar.values(synthetic["cell"], synthetic["past"], socp["X_star"], (LON, LAT), CAR_R)
    open_socp = ar.tally(v, sel[0])["sel_open"]
    print("SOCP plan: sel_open", open_socp.tolist(), "allow", allow.tolist())
    assert np.any(open_socp > allow[0])
    cal = agent.calibrate_face_rows(socp["X_star"])
    assert np.array_equal(cal["step_meets_budget"][0], open_socp <= allow[0])
    assert np.array_equal(cal["allow"], allow)

    out = agent.tighten_face_plan(prob["x_init"], prob["goal"], ref, T, tol_g=TOL_G)
    print("tighten_rounds", out["tighten_rounds"], "margins per round",
          np.round(out["margins"][:, 0], 7).tolist())
    print("cost", socp["cost"], "->", out["cost"])
    assert 1 <= out["tighten_rounds"] <= 2
    assert out["margins"].shape == (out["tighten_rounds"] + 1, 1, T)
    assert np.all(out["margins"][-1] <= 0.0)                   # every selected q <= 0, exactly
    assert out["socp"]["X_star"].tobytes() == socp["X_star"].tobytes()
    assert out["cost"] >= socp["cost"]                         # its pool is a superset of rows
    rep = agent.audit_face_rows(out["X_star"])
    print("tightened plan: sel_open", rep["sel_open"][0].tolist())
    assert np.all(rep["has_row"])
    assert np.all(rep["sel_open"] <= allow[:, None])           # integers
    after = agent.calibrate_face_rows(out["X_star"])
    assert np.all(after["step_meets_budget"])
    assert np.array_equal(after["margin_sel"], out["margins"][-1])
    assert agent._face_src is src and agent._last_rec is last and agent._audit_src is aud_src


@pytest.fixture(scope="module")
def world(gpu, golden):
    from ccmpc import ovehicle, planner
    g = golden(sr.SCENE)
    T, K, cells, _ = scene_cells(g)
    ovs = ovehicle.scene_from_positions(cells, g["past"], device=gpu)
    agent = planner.MidlevelAgent(prediction_horizon=T, device=gpu)
    prob = sr.instance(10.0)
    agent.compute_obstacle_constraints_GMM_approx(
        Params(len(K), K, 100), ovs, None, None, None, g["eps_ura"], None, T, prob["ref"])
    return dict(T=T, K=K, agent=agent, prob=prob)


def test_golden_scene_calibration_agrees_with_the_audit(world):
    from ccmpc import risk
    agent, prob, T = world["agent"], world["prob"], world["T"]
    src, last, aud_src = agent._face_src, agent._last_rec, agent._audit_src
    ctrl = agent.solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"], T, tol_g=TOL_G)
    aud = agent.audit_face_rows(ctrl["X_star"])
    cal = agent.calibrate_face_rows(ctrl["X_star"])
    allow = risk.allow_counts(src[0].store.counts, src[1], T)
    assert np.array_equal(cal["allow"], allow)
    has = aud["has_row"]
    assert has.any()
    within = has & (aud["sel_open"] <= allow[:, None])         # the audit's verdict through allow
    assert np.array_equal(within, aud["step_within_budget"])
    assert np.array_equal(cal["step_meets_budget"], within)
    assert np.all(np.isnan(cal["margin_sel"][~has]))
    assert not within[has].all()                               # DESIGN 4.13's finding stands
    print("margin_sel [m] at the rows over budget:",
          [(int(c), int(t), float(cal["margin_sel"][c, t]), int(aud["sel_open"][c, t]),
            int(allow[c])) for c, t in zip(*np.nonzero(has & ~within))])
    print("worst row", cal["worst_row"], "worst margin", cal["worst_margin"])
    assert cal["worst_margin"] > 0
    assert agent._face_src is src and agent._last_rec is last and agent._audit_src is aud_src


def test_golden_scene_tightening_outcome_is_recorded(world):
    """Headings differ between the particles here, so the loop is a heuristic: whatever it ends
    in is printed (DESIGN 4.14 quotes it); only what must hold in any case is asserted."""
    from ccmpc import mpc, risk
    from ccmpc.planner import InSimulationException
    agent, prob, T = world["agent"], world["prob"], world["T"]
    src, last, aud_src = agent._face_src, agent._last_rec, agent._audit_src
    allow = risk.allow_counts(src[0].store.counts, src[1], T)
    try:
        out = agent.tighten_face_plan(prob["x_init"], prob["goal"], prob["ref"], T, tol_g=TOL_G)
        status, rounds, margins = mpc.TIGHTEN_OK, out["tighten_rounds"], out["margins"]
    except InSimulationException as e:
        out, status, rounds, margins = None, e.status, e.tighten_rounds, e.margins
    print("status", status, "tighten_rounds", rounds)
    for i, m in enumerate(margins):
        print(f"round {i}: largest selected q per cell [m]",
              np.round(np.nanmax(np.where(np.isnan(m), -np.inf, m), axis=1), 6).tolist())
    assert status in (mpc.TIGHTEN_OK, mpc.TIGHTEN_INFEASIBLE, mpc.TIGHTEN_NUMERIC,
                      mpc.TIGHTEN_MAXROUNDS)
    if out is not None:
        rep = agent.audit_face_rows(out["X_star"])
        has = rep["has_row"]
        print("cost", out["socp"]["cost"], "->", out["cost"], "final open fractions of the rows:",
              np.round(rep["p_sel_open"][has], 5).tolist())
        assert np.all(rep["sel_open"][has] <= np.broadcast_to(allow[:, None], has.shape)[has])
    assert agent._face_src is src and agent._last_rec is last and agent._audit_src is aud_src
