"""mpc.PlanningSOCP (outer approximation over the GPU planning QP) against the NumPy restatement
of the loop (tests/_socp_ref.py) and its KKT certificate, on the shifted golden scene and the
seeded synthetic scene.

Two bars come from a CPU measurement, never from the GPU result: u_ref is the restatement run at
tol_g / 1000; the restatement at tol_g differs from it by du_cpu and has the stationarity residual
stat_cpu; the GPU answer, from another exact QP solver reaching the same minimisers by different
pivoting, gets 10 x each -- with du_cpu floored at tol_g (two plans that both meet max g <= tol_g
may differ by the shift a tol_g move of the active row causes, |grad g| ~ 1) and stat_cpu floored
at 1e-6 (a tenth of the suite's bar on the plain QP's own stationarity, tests/test_gpu_mpc.py)."""
import functools

import numpy as np
import pytest
import torch

import _socp_ref as sr

pytestmark = pytest.mark.gpu

TOL_G = 1e-6
CASES = sr.M_ACTIVE + (sr.M_FREE, "syn")


def problem(case):
    return sr.synthetic() if case == "syn" else sr.instance(case)


@functools.lru_cache(maxsize=None)
def cpu(case):
    """(restatement at tol_g, at tol_g / 1000, du bar, stat bar) -- computed once per case."""
    prob = problem(case)
    loose, tight = sr.kelley(prob, TOL_G), sr.kelley(prob, TOL_G / 1000)
    assert loose["status"] == sr.OK and tight["status"] == sr.OK
    du = float(np.max(np.abs(loose["u"] - tight["u"])))
    stat = sr.kkt(prob, loose["u"])["stat"]
    return loose, tight, 10 * max(du, TOL_G), 10 * max(stat, 1e-6), du, stat


def solve(gpu, cases, max_rounds=12, tol_g=TOL_G):
    """One PlanningSOCP batch over the instances; returns (SocpResult, host u, X, cost)."""
    from ccmpc import mpc
    probs = [problem(c) for c in cases]
    T = probs[0]["T"]
    f64 = dict(dtype=torch.float64, device=gpu)
    rec = np.concatenate([sr.pack_face_records(p["cells_out"], T) for p in probs])
    cells = [len(p["cells_out"]) for p in probs]
    run = mpc.PlanningSOCP(cells, T, max_rounds=max_rounds, tol_g=tol_g, device=gpu)
    xbar, gamma = mpc.ltv(np.array([p["x_init"] for p in probs]), T, Ts=sr.TS, lon=sr.LON)
    ref = torch.as_tensor(np.array([p["ref"] for p in probs]), **f64)
    goal = torch.as_tensor(np.array([p["goal"] for p in probs]), **f64)
    res = run.solve(
        gamma, xbar, goal, ref,
        torch.as_tensor(np.ascontiguousarray(rec).view(np.uint8).reshape(-1), device=gpu),
        torch.as_tensor(np.concatenate([p["cell_gamma"] for p in probs]), **f64), ref)
    return res, res.u.cpu().numpy(), res.X.cpu().numpy(), res.cost.cpu().numpy()


@functools.lru_cache(maxsize=None)
def alone(case):
    return solve(torch.device("cuda:0"), (case,))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_plan_against_the_restatement_and_its_certificate(gpu, case):
    from ccmpc import mpc
    prob = problem(case)
    loose, tight, du_bar, stat_bar, du_cpu, stat_cpu = cpu(case)
    res, u, X, cost = alone(case)
    assert res.status[0] == mpc.SOCP_OK and 1 <= res.rounds[0] <= 12
    assert res.viol[0] <= TOL_G
    costs = res.costs[:res.rounds[0], 0]
    assert np.all(np.diff(costs) >= -1e-9 * (1 + np.abs(costs[:-1]))), costs
    assert costs[-1] == cost[0]
    k = sr.kkt(prob, u[0])
    du = float(np.max(np.abs(u[0] - tight["u"])))
    print(f"{case}: rounds {res.rounds[0]} (cpu {loose['rounds']}), viol {res.viol[0]:.3e}, "
          f"cost {cost[0]:.12g} (cpu {loose['cost']:.12g}, tight {tight['cost']:.12g}); "
          f"|u - u_ref| {du:.3e} (cpu at tol_g {du_cpu:.3e}, bar {du_bar:.3e}); "
          f"stat {k['stat']:.3e} (cpu {stat_cpu:.3e}, bar {stat_bar:.3e}); prim {k['prim']:.3e}")
    # the QP over the cuts relaxes the cone programme, whose optimum the tight run has to 1e-9
    assert cost[0] <= tight["cost"] + 1e-8 * (1 + abs(tight["cost"]))
    assert k["prim"] <= TOL_G + 1e-9 and k["lin"] <= 1e-8
    assert du <= du_bar
    assert k["stat"] <= stat_bar
    assert np.allclose(X[0], (prob["Gf"] @ u[0] + prob["c"]).reshape(-1, 4), rtol=0, atol=1e-6)
    if case == sr.M_FREE:
        assert res.rounds[0] == 1
    if case == "syn":
        assert {ov for ov, _, _ in k["strong_cone"]} == {0, 1}


def test_unshifted_reference_is_infeasible(gpu):
    from ccmpc import mpc
    res, _, _, _ = alone(sr.M_INFEASIBLE)
    assert res.status[0] == mpc.SOCP_INFEASIBLE and res.rounds[0] == 2


def test_one_round_is_not_enough_for_the_six_metre_shift(gpu):
    from ccmpc import mpc
    res, _, _, _ = solve(gpu, (6.0,), max_rounds=1)
    assert res.status[0] == mpc.SOCP_MAXROUNDS and res.rounds[0] == 1
    assert res.viol[0] > TOL_G


def test_batch_returns_each_scene_s_own_bits(gpu):
    cases = (10.0, sr.M_INFEASIBLE, sr.M_FREE)
    res, u, X, cost = solve(gpu, cases)
    for s, case in enumerate(cases):
        r1, u1, X1, c1 = alone(case)
        assert res.status[s] == r1.status[0] and res.rounds[s] == r1.rounds[0], case
        assert u[s].tobytes() == u1[0].tobytes(), case
        assert X[s].tobytes() == X1[0].tobytes(), case
        assert cost[s].tobytes() == c1[0].tobytes(), case
        assert np.array_equal(res.viol[s:s + 1], r1.viol, equal_nan=True), case
