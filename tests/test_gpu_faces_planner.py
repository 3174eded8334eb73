"""The three box-face ("TCST") generators of planner.MidlevelAgent on the golden scenes
(tests/golden/faces_*.npz: the reference's own method bodies, recorded by
tests/golden/make_golden_faces.py): tuple shape, row sequence, gating, the approx choice, row
values at probe points, and FaceConstraintList.check."""
import numpy as np
import pytest

import _faces_ref as fr
from _faces_ref import scene_cells

pytestmark = pytest.mark.gpu

SCENES = ("faces_o2_t8", "faces_o3_t12")
VARIANTS = ("nominal", "robust", "approx")
METHOD = {"nominal": "compute_obstacle_constraints_GMM",
          "robust": "compute_robust_constraints_GMM",
          "approx": "compute_obstacle_constraints_GMM_approx"}


class Params:
    def __init__(self, O, K, frame):
        self.O, self.K, self.frame = O, np.asarray(K), frame


@pytest.fixture(scope="module")
def scenes(gpu, golden):
    """name -> dict(golden, T, K, cells, yaws, out[variant] = the generator's 8-tuple), every
    generator run once."""
    from ccmpc import ovehicle, planner
    out = {}
    for name in SCENES:
        g = golden(name)
        T, K, cells, yaws = scene_cells(g)
        ovs = ovehicle.scene_from_positions(cells, g["past"], device=gpu)
        agent = planner.MidlevelAgent(prediction_horizon=T, device=gpu)
        res = {}
        for v in VARIANTS:
            args = [Params(len(K), K, 100), ovs, None, None, None, g["eps_ura"], None, T]
            if v == "approx":
                args.append(g["ref_traj"])
            res[v] = getattr(agent, METHOD[v])(*args)
            assert agent._last_rec is None and agent._audit_src is None
        out[name] = dict(g=g, T=T, K=K, cells=cells, yaws=yaws, out=res, agent=agent)
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SCENES)
def test_tuple_rows_and_gating(scenes, name, variant):
    from ccmpc import planner
    sc = scenes[name]
    g, T, K = sc["g"], sc["T"], sc["K"]
    res = sc["out"][variant]
    assert len(res) == 8
    cons, vertices, A_union, b_union, ovc, direct, smean, scov = res
    assert isinstance(cons, planner.FaceConstraintList)
    assert ovc == bool(g[f"{variant}_ovconstraint"]) and direct == [None] * len(K)
    rows = list(cons)
    seq = g[f"{variant}_seq"]
    assert len(rows) == len(cons) == len(seq)
    assert [0 if isinstance(r, planner.SocConstraint) else 1 for r in rows] == list(seq)
    assert all(isinstance(r, planner.FaceDeltaSum) for r, s in zip(rows, seq) if s == 1)
    okt = g[f"{variant}_okt"]
    want_rows, _ = fr.generator_rows(sc["cells"], sc["yaws"], g["eps_ura"], T, T, variant,
                                     g["ref_traj"])
    assert [(r.ov, r.k, r.t) for r in rows] == [(w["ov"], w["k"], w["t"]) for w in want_rows]
    if variant != "approx":
        assert [(r.ov, r.k, r.t) for r in rows] == [tuple(x) for x in okt]
    else:
        assert [r.t for r in rows] == list(okt[:, 2])
    soc = [r for r in rows if isinstance(r, planner.SocConstraint)]
    assert [r.face for r in soc] == list(g[f"{variant}_face"])        # the approx choice too
    assert all(r.status == 0 and r.offset == 0.5 * fr.CAR_R for r in soc)
    for r in soc:
        assert r.gamma == pytest.approx(g["gamma"][r.ov, r.k], rel=1e-12)
    i = 0
    for o in range(len(K)):
        for k in range(K[o]):
            for j in range(3):
                assert smean[j][o][k] == pytest.approx(g[f"{variant}_state_mean"][i][j], rel=1e-12)
                assert scov[j][o][k] == pytest.approx(g[f"{variant}_state_cov"][i][j], rel=1e-9)
            i += 1
    assert len(A_union) == T and len(b_union) == T


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SCENES)
def test_row_values_at_probe_points(scenes, name, variant):
    """SocConstraint.value against the value recomputed from the golden mean / root:
    |d| <= |dmean| |xi| + Gamma |dR|_2 |xi| (+ the evaluation's own rounding).  xi is about
    200 m long, so a plain rtol on the value would be wrong.  Both sides carry an error against
    the exact row, so each delta is twice its bar: |dmean| <= 2e-12 |mean| (the means' rtol),
    |dR| <= twice the root bound of tests/test_gpu_faces.py (nominal, approx) or 2e-12 s
    (robust)."""
    from ccmpc import planner
    sc = scenes[name]
    g, T = sc["g"], sc["T"]
    kind = "robust" if variant == "robust" else "nominal"
    soc = [r for r in sc["out"][variant][0] if isinstance(r, planner.SocConstraint)]
    ld, err64 = {}, 0.0
    for r in soc:
        key = (r.ov, r.k)
        if key not in ld:
            c, y = sc["cells"][r.ov][r.k], sc["yaws"][r.ov][r.k]
            ld[key] = fr.cell_ld(c, g["past"][r.ov], r.gamma, kind)
            f = fr.cell_f64(c, y, r.gamma, kind, roots=False)
            err64 = max(err64, fr.scaled_cov_error(f["C"], fr.cell_ld_yaw(c, y)))
    tol_c = fr.allowed_cov_error(err64)
    worst = 0.0
    for i, r in enumerate(soc):
        want = ld[(r.ov, r.k)]
        gm = g[f"{variant}_mean"][i]
        M, coef, const = g[f"{variant}_root"][i], g[f"{variant}_coef"][i], g[f"{variant}_const"][i]
        if kind == "robust":
            dR = 2e-12 * float(want["s"][r.t, r.face])
            normR = float(want["s"][r.t, r.face])
        else:
            dR = 2 * fr.root_bound(want["C"][r.t, r.face], want["lam_min"][r.t, r.face],
                                   want["root"][r.t, r.face], tol_c)
            normR = np.linalg.norm(r.root, 2)
        centre = sc["cells"][r.ov][r.k][:, r.t].mean(0)
        for xy in (g["ref_traj"][r.t], g["ref_traj"][r.t] + np.array([5.0, -3.0]),
                   centre + np.array([1.0, 1.0])):
            xi = np.array([xy[0], xy[1], 1.0])
            val_g = gm[:2] @ xy + const + coef * np.linalg.norm(M @ xi)
            nx = np.linalg.norm(xi)
            size = np.linalg.norm(r.mean) * nx + r.gamma * normR * nx + abs(const)
            bound = 2e-12 * np.linalg.norm(r.mean) * nx + r.gamma * dR * nx + 64 * fr.EPS * size
            d = abs(r.value(xy) - val_g)
            worst = max(worst, d / bound)
            assert d <= bound, (i, r, d, bound)
    print(f"{name} {variant}: worst |dvalue| / bound {worst:.2e}")


def test_check_on_a_plan_through_an_ov_and_on_one_clear_of_it(scenes):
    """faces_o2_t8, nominal.  A plan along the gated OV's mean path stands inside the box at
    every step: every face value is positive there and the disjunction fails.  A plan 30 m to
    the side (towards -45 degrees, where the float64 restatement leaves a margin of 15 m at the
    worst step) holds everywhere.  (The longer three-OV scene admits no plan 30 m from its first
    gated OV under these rows, and the robust rows, sqrt(|C|_F) |xi| with |xi| ~ 200 m, hold
    nowhere near the scene: both are the reference's arithmetic, not checked here.)"""
    sc = scenes["faces_o2_t8"]
    cons = sc["out"]["nominal"][0]
    path = sc["cells"][0][0].mean(0)
    rows, ok = cons.check(path)
    assert not ok
    hit = [r for r in rows if (r.ov, r.k) == (0, 0)]
    assert len(hit) == sc["T"] and all(not r.holds and np.all(r.values > 0) for r in hit)
    away = path + 30.0 * np.array([np.cos(np.radians(-45.0)), np.sin(np.radians(-45.0))])
    rows, ok = cons.check(away)
    assert ok and all(r.holds and r.values[r.best] <= 0 for r in rows)
    assert len(rows) == 2 * sc["T"] and {r.ov for r in rows} == {0}


@pytest.mark.parametrize("name", SCENES)
def test_check_of_the_approx_rows_judges_the_chosen_row(scenes, name):
    sc = scenes[name]
    cons = sc["out"]["approx"][0]
    rows, ok = cons.check(sc["g"]["ref_traj"])
    soc = list(cons)
    assert len(rows) == len(soc)
    for r, c in zip(rows, soc):
        assert r.best == c.face
        assert r.holds == (c.value(sc["g"]["ref_traj"][c.t]) <= 0)
    assert ok == all(r.holds for r in rows)


def test_half_space_consumers_refuse_the_face_rows(scenes):
    """The records are not half-spaces: the QP has nothing to read after such a step."""
    agent = scenes["faces_o2_t8"]["agent"]
    assert agent._last_rec is None
    with pytest.raises(RuntimeError, match="no constraint records"):
        agent.solve_planning_qp(np.zeros(4), np.zeros(2), scenes["faces_o2_t8"]["g"]["ref_traj"],
                                8)
