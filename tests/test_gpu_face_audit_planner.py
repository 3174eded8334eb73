"""planner.MidlevelAgent.audit_face_rows on the golden scene faces_o2_t8 with its reference
shifted 10 m (the instance of tests/test_gpu_socp_planner.py): the report's counts against the
host restatement on the scene's own particles, the selection solve_planning_socp uses, and the
refusals.  No claim is made on the risk itself."""
import numpy as np
import pytest

import _face_audit_ref as ar
import _socp_ref as sr
from _faces_ref import CAR_R, LAT, LON, scene_cells

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
    prob = sr.instance(10.0)
    cons = world["generate"]("approx", prob["ref"])[0]
    ctrl = world["agent"].solve_planning_socp(prob["x_init"], prob["goal"], prob["ref"],
                                              world["T"], tol_g=TOL_G)
    return prob, cons, ctrl


def _restated(agent, X, sel):
    scene, K, T = agent._face_src[:3]
    past = scene.cell_past_last()
    out = []
    for j in range(scene.store.n_cells):
        w = scene.store.cell_positions(j)[:, :T]
        v, _, _ = ar.values(w, past[j], X, (LON, LAT), CAR_R)
        vld, ex, ey = ar.values(w, past[j], X, (LON, LAT), CAR_R, ld=True)
        # the premise of exact counts: no v_f near enough to zero for rounding to decide it
        scale = 1 + np.abs(ex) + np.abs(ey)
        print(f"cell {j}: smallest |v_f| / scale {float((np.abs(vld) / scale[..., None]).min()):.3g}")
        assert np.all(np.abs(vld) > ar.BAND * scale[..., None])
        assert np.array_equal(v > 0, vld > 0)
        out.append(ar.tally(v, sel[j]))
    return out


def test_approx_rows_are_audited_on_their_own_particles(world, approx_plan):
    prob, cons, ctrl = approx_plan
    agent, T = world["agent"], world["T"]
    world["generate"]("approx", prob["ref"])
    before = agent.audit_face_plan(ctrl["X_star"])
    src = agent._face_src
    rep = agent.audit_face_rows(ctrl["X_star"])
    assert agent._face_src is src                       # no planner state changed
    C = src[0].store.n_cells
    sel = agent._face_selection(src[5], C, T, None)
    gated = set(src[5]._cells)
    assert gated
    for c in range(C):
        if c in gated:
            assert np.all((sel[c] >= 0) & (sel[c] <= 3))
            assert np.all(rep["sel_open"][c] >= 0) and np.all(rep["has_row"][c])
        else:
            assert np.all(sel[c] == -1) and np.all(rep["sel_open"][c] == -1)
            assert rep["sel_open_any"][c] == 0
    want = _restated(agent, ctrl["X_star"], sel)
    for name in ("face_open", "in_box", "in_box_any", "sel_open", "sel_open_any"):
        assert np.array_equal(rep[name], np.stack([w[name] for w in want])), name
    n = np.asarray(src[0].store.counts, np.float64)
    assert np.array_equal(rep["counts"], n.astype(np.int64))
    assert np.array_equal(rep["p_face_open"], rep["face_open"] / n[:, None, None])
    assert np.array_equal(rep["p_in_box"], rep["in_box"] / n[:, None])
    assert np.array_equal(rep["p_in_box_any"], rep["in_box_any"] / n)
    assert np.array_equal(rep["p_sel_open_any"], rep["sel_open_any"] / n)
    has = rep["has_row"]
    assert np.array_equal(rep["p_sel_open"][has], (rep["sel_open"] / n[:, None])[has])
    assert np.all(np.isnan(rep["p_sel_open"][~has]))
    assert rep["budget_step"].shape == (C,) and np.all(rep["budget_step"] * T == rep["budget_traj"])
    print("p_sel_open per gated (cell, t):", np.round(rep["p_sel_open"][sorted(gated)], 4).tolist())
    print("budget_step:", rep["budget_step"].tolist(), "p_sel_open_any:",
          rep["p_sel_open_any"].tolist(), "budget_traj:", rep["budget_traj"].tolist())
    print("worst of the selected rows:",
          [[float(rep["worst"][c, t, sel[c, t]]) for t in range(T)] for c in sorted(gated)])
    after = agent.audit_face_plan(ctrl["X_star"])
    for key in ("hit", "hit_any", "min_d2", "counts"):
        assert np.array_equal(before[key], after[key]), key
    with pytest.raises(ValueError):
        agent.audit_face_rows(ctrl["X_star"][:-1])


def test_nominal_rows_need_faces(world, approx_plan):
    prob, cons, ctrl = approx_plan
    agent, T = world["agent"], world["T"]
    faces = np.array([r.face for r in cons]).reshape(-1, T)
    world["generate"]("approx", prob["ref"])
    want = agent.audit_face_rows(ctrl["X_star"])
    world["generate"]("nominal", None)
    with pytest.raises(ValueError, match="faces"):
        agent.audit_face_rows(ctrl["X_star"])
    got = agent.audit_face_rows(ctrl["X_star"], faces=faces)
    for name in ("face_open", "in_box", "in_box_any", "sel_open", "sel_open_any", "worst"):
        assert got[name].tobytes() == want[name].tobytes(), name


def test_no_face_step_is_refused(gpu):
    from ccmpc import planner
    agent = planner.MidlevelAgent(prediction_horizon=8, device=gpu)
    with pytest.raises(RuntimeError, match="no face records"):
        agent.audit_face_rows(np.zeros((8, 2)))
