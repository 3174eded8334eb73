"""planner.MidlevelAgent.solve_planning_socp / audit_face_plan on the golden scene faces_o2_t8,
the agent built as tests/test_gpu_faces_planner.py builds it: the plan under the approx rows,
the same plan from the nominal rows with approx's faces given, the refusals, and the audit."""
import numpy as np
import pytest
import torch

import _socp_ref as sr
from _faces_ref import scene_cells

pytestmark = pytest.mark.gpu

TOL_G = 1e-6


class Params:
    def __init__(self, O, K, frame):
        self.O, self.K, self.frame = O, np.asarray(K), frame


@pytest.fixture(scope="module")
def world(gpu, golden):
    from ccmpc import ovehicle, planner
    g = golden(sr.SCENE)
    T, K, cells, _ = scene_cells(g)
    ovs = ovehicle.scene_from_positions(cells, g["past"], device=gpu)
    agent = planner.MidlevelAgent(prediction_horizon=T, device=gpu)

    def generate(variant, ref):
        args = [Params(len(K), K, 100), ovs, None, None, None, g["eps_ura"], None, T]
        if variant == "approx":
            return agent.compute_obstacle_constraints_GMM_approx(*args, ref)
        return agent.compute_obstacle_constraints_GMM(*args)
    return dict(g=g, T=T, K=K, agent=agent, generate=generate)


@pytest.fixture(scope="module")
def approx_plan(world):
    prob = sr.instance(6.0)
    cons = world["generate"]("approx", prob["ref"])[0]
    ctrl = world["agent"].solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"],
                                              world["T"], tol_g=TOL_G)
    return prob, cons, ctrl


def test_approx_rows_give_a_plan_that_holds(world, approx_plan):
    prob, cons, ctrl = approx_plan
    T = world["T"]
    assert ctrl["X_star"].shape == (T, 4) and ctrl["U_star"].shape == (T, 2)
    assert 1 <= ctrl["rounds"] <= 12 and ctrl["max_violation"] <= TOL_G
    rows, ok = cons.check(ctrl["X_star"], tol=TOL_G)
    assert ok and len(rows) == len(cons)
    want = sr.kelley(prob, TOL_G)
    assert ctrl["rounds"] == want["rounds"]
    assert np.max(np.abs(ctrl["u"] - want["u"])) <= 1e-2       # the same plan, coarsely
    agent = world["agent"]
    assert agent._last_rec is None and agent._audit_src is None
    assert agent._face_src is not None
    with pytest.raises(RuntimeError, match="no constraint records"):
        agent.solve_planning_qp(prob["x_init"], prob["goal"], prob["ref"], T)


def test_nominal_rows_with_the_same_faces_give_the_same_bits(world, approx_plan):
    prob, cons, ctrl = approx_plan
    T, agent = world["T"], world["agent"]
    faces = np.array([r.face for r in cons]).reshape(-1, T)
    world["generate"]("nominal", None)
    with pytest.raises(ValueError, match="faces"):
        agent.solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"], T)
    got = agent.solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"], T, faces=faces,
                                    tol_g=TOL_G)
    as_map = {(r.ov, r.k, r.t): r.face for r in cons}
    got2 = agent.solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"], T, faces=as_map,
                                     tol_g=TOL_G)
    for res in (got, got2):
        for key in ("u", "X_star", "U_star"):
            assert res[key].tobytes() == ctrl[key].tobytes(), key
        assert res["cost"] == ctrl["cost"] and res["rounds"] == ctrl["rounds"]
    with pytest.raises(ValueError):
        agent.solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"], T,
                                  faces=np.full_like(faces, 4))


def test_unshifted_reference_has_no_plan(world):
    from ccmpc import planner
    prob = sr.instance(0.0)
    world["generate"]("approx", prob["ref"])
    with pytest.raises(planner.InSimulationException):
        world["agent"].solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"], world["T"])


def test_audit_face_plan_is_the_plan_half_of_the_audit(world, approx_plan, gpu):
    from ccmpc import engine
    prob, _, ctrl = approx_plan
    agent, T = world["agent"], world["T"]
    world["generate"]("approx", prob["ref"])
    rep = agent.audit_face_plan(ctrl["X_star"])
    store = agent._face_src[0].store
    plan = torch.as_tensor(np.ascontiguousarray(ctrl["X_star"][None, :, :2]), device=gpu)
    a = engine.risk_audit(store, plan=plan, R=agent.R, T=T)
    assert np.array_equal(rep["hit"], a.hit.cpu().numpy())
    assert np.array_equal(rep["hit_any"], a.hit_any.cpu().numpy())
    assert np.array_equal(rep["min_d2"], a.min_d2.cpu().numpy())
    assert rep["rec_open"] is None and rep["open"] is None
    assert rep["counts"].sum() == sum(store.counts)
    with pytest.raises(ValueError):
        agent.audit_face_plan(ctrl["X_star"][:-1])


def test_no_face_step_is_refused(gpu):
    from ccmpc import planner
    agent = planner.MidlevelAgent(prediction_horizon=8, device=gpu)
    with pytest.raises(RuntimeError, match="no face records"):
        agent.solve_planning_socp(np.zeros(4), np.zeros(2), np.zeros((8, 2)), 8)
    with pytest.raises(RuntimeError, match="no face records"):
        agent.audit_face_plan(np.zeros((8, 2)))
