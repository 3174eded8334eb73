"""The oracle of the plan under the box-face cone rows (ccmpc_face_cuts, mpc.PlanningSOCP): a
NumPy restatement of the outer-approximation loop on oracle.mpc_oracle's QP and
_faces_ref.generator_rows' rows, the KKT certificate that judges a returned plan, and the
instances the CPU and GPU tests share.  Not a test.

The loop: linearise every cone row g(x_t) = mean . xi + Gamma |root xi|_2 + 0.5 car_r at the
current plan (round 0: at the reference trajectory, where approx chose its faces), solve the QP
over all cuts so far, stop when max g <= tol_g.  An infeasible QP certifies an infeasible cone
programme (the cuts are an outer approximation).
"""
import functools
import os

import numpy as np

import _faces_ref as fr
from oracle import mpc_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENE = "faces_o2_t8"
LON, TS = 3.7, 0.5
# MPCParams.reference_defaults() (v8ideal/__init__.py:86-109, max_steer 70 degrees)
PARAMS = dict(w_final=6.0, w_ref=3.0, w_accel=0.5, w_joint=0.2, w_turning=1.0, w_ch_accel=0.5,
              w_ch_joint=0.1, w_ch_turning=2.0, min_a=-7.0, max_a=4.0,
              max_delta=0.5 * np.radians(70.0), max_v=10.0)
OK, INFEASIBLE, MAXROUNDS = "ok", "infeasible", "maxrounds"
# shifts of the golden reference trajectory along (cos 45, sin 45): one active cone row (6, 10,
# 15), none (25), infeasible after one round (0)
M_ACTIVE, M_FREE, M_INFEASIBLE = (6.0, 10.0, 15.0), 25.0, 0.0


def row_g(row, p):
    """g of one row at p = (x, y), the kernel's operation order."""
    m, R, x, y = row["mean"], row["root"], p[0], p[1]
    w0 = R[0, 0] * x + R[0, 1] * y + R[0, 2]
    w1 = R[0, 1] * x + R[1, 1] * y + R[1, 2]
    w2 = R[0, 2] * x + R[1, 2] * y + R[2, 2]
    nw = np.sqrt(w0 * w0 + w1 * w1 + w2 * w2)
    return m[0] * x + m[1] * y + m[2] + row["gamma"] * nw + 0.5 * row.get("car_r", fr.CAR_R)


def row_cut(row, p):
    """(g, a, b) of the row's cut at p: a . x <= b, a a subgradient of g at p, b = a . p - g."""
    m, R, x, y, gm = row["mean"], row["root"], p[0], p[1], row["gamma"]
    w0 = R[0, 0] * x + R[0, 1] * y + R[0, 2]
    w1 = R[0, 1] * x + R[1, 1] * y + R[1, 2]
    w2 = R[0, 2] * x + R[1, 2] * y + R[2, 2]
    nw = np.sqrt(w0 * w0 + w1 * w1 + w2 * w2)
    g = m[0] * x + m[1] * y + m[2] + gm * nw + 0.5 * row.get("car_r", fr.CAR_R)
    a0, a1 = m[0], m[1]
    if nw != 0:
        v0 = R[0, 0] * w0 + R[0, 1] * w1 + R[0, 2] * w2
        v1 = R[0, 1] * w0 + R[1, 1] * w1 + R[1, 2] * w2
        a0, a1 = m[0] + gm * v0 / nw, m[1] + gm * v1 / nw
    return g, np.array([a0, a1]), a0 * x + a1 * y - g


def model(ref, T):
    """x_init one reference step behind ref[0], heading along that step, 6 m/s; goal = ref[-1];
    the LTV model about u = 0 (l_r = lon / 2, L = lon)."""
    step = ref[1] - ref[0]
    x_init = np.array([*(ref[0] - step), np.arctan2(step[1], step[0]), 6.0])
    xbar, _, Gamma, _, _ = mo.VehicleModel(T, TS, 0.5 * LON, LON).get_optimization_ltv(
        x_init, np.zeros(2))
    Gf, c = mo.state_map(Gamma, xbar, T, T)
    return dict(T=T, ref=np.ascontiguousarray(ref), x_init=x_init, goal=ref[-1].copy(),
                Gamma=Gamma, xbar=xbar, Gf=Gf, c=c)


@functools.lru_cache(maxsize=None)
def golden_scene():
    g = np.load(os.path.join(GOLDEN, SCENE + ".npz"), allow_pickle=False)
    T, K, cells, yaws = fr.scene_cells(g)
    return g, T, K, cells, yaws


@functools.lru_cache(maxsize=None)
def instance(m):
    """The golden scene with its reference trajectory shifted by m metres along 45 degrees:
    dict(model fields, rows = the approx generator's rows with faces chosen at that ref)."""
    g, T, K, cells, yaws = golden_scene()
    ref = g["ref_traj"][:T] + float(m) * np.array([np.cos(np.radians(45.0)),
                                                   np.sin(np.radians(45.0))])
    prob = model(ref, T)
    rows, per_cell = fr.generator_rows(cells, yaws, g["eps_ura"], T, T, "approx", ref)
    keys = sorted(per_cell)                       # the gated cells, (ov, k) order
    gam = {(r["ov"], r["k"]): r["gamma"] for r in rows}
    prob.update(rows=rows, cells_out=[per_cell[k] for k in keys],
                cell_gamma=np.array([gam[k] for k in keys]))
    return prob


SYN_SEED, SYN_T = 20261021, 8


@functools.lru_cache(maxsize=None)
def synthetic():
    """A seeded scene whose optimum has active cone rows from two cells at several steps: a
    straight reference along +x at 6 m/s and two clouds of 400 particles driving the same way
    at 5 m/s on its left, 3.8 m away at their closest step (2 and 6) and 0.12 (t - t_closest)^2
    further at the others, each with the face chosen at the reference point (the approx rule):
    the ego has to give way to the right twice.  Returns the instance dict plus cells
    (2 x (n, T, 2)), past (2, 2), gamma (2,)."""
    rng = np.random.default_rng(SYN_SEED)
    T = SYN_T
    ref = np.stack([200.0 + 3.0 * np.arange(1, T + 1), np.full(T, -60.0)], -1)
    cells, past = [], []
    for t_at in (2, 6):
        n = 400
        v = 5.0 + rng.normal(0, 0.3, size=(n, 1))
        steps = np.arange(1, T + 1)[None, :] * TS
        x = ref[t_at, 0] - 5.0 * TS * (t_at + 1) + v * steps + rng.normal(0, 0.15, size=(n, T))
        y = (ref[t_at, 1] + 3.8 + 0.12 * (np.arange(T)[None, :] - t_at) ** 2
             + rng.normal(0, 0.05, size=(n, 1)) + rng.normal(0, 0.02, size=(n, T)))
        c = np.stack((x, y), -1)
        cells.append(c)
        past.append(c[:, 0].mean(0) - np.array([5.0 * TS, 0.0]))
    past = np.array(past)
    gamma = fr.gamma_of(np.full(2, 0.05), T)
    rows, outs = [], []
    for j, c in enumerate(cells):
        d = fr.step_deltas(c, past[j])
        yw = np.arctan2(d[..., 1], d[..., 0])
        r = fr.cell_f64(c, yw, float(gamma[j]), "nominal", ref)
        outs.append(r)
        for t in range(T):
            f = int(r["chosen"][t])
            rows.append(dict(ov=j, k=0, t=t, face=f, mean=r["mean"][t, f], root=r["root"][t, f],
                             gamma=float(gamma[j])))
    prob = model(ref, T)
    prob.update(rows=rows, cells=cells, past=past, gamma=gamma, cells_out=outs,
                cell_gamma=np.asarray(gamma, np.float64))
    return prob


def pack_face_records(cells_out, T):
    """ccmpc_face_rec [C, T, 4] (the library's FACE_DTYPE) from cell_f64 outputs: status 0, the
    chosen flag from out["chosen"] (CCMPC_FACE_NO_CHOICE everywhere at a step with chosen < 0)."""
    from ccmpc import _lib
    rec = np.zeros((len(cells_out), T, 4), _lib.FACE_DTYPE)
    for c, o in enumerate(cells_out):
        for t in range(T):
            for f in range(4):
                rec["mean"][c, t, f] = o["mean"][t, f]
                rec["root"][c, t, f] = fr.sym6(o["root"][t, f])
                rec["C"][c, t, f] = fr.sym6(o["C"][t, f])
                ch = o["chosen"][t]
                flag = _lib.FACE_NO_CHOICE if ch < 0 else int(ch == f)
                rec["t_face_chosen"][c, t, f] = (t << 16) | (f << 8) | flag
    return rec


def row_cut_ld(mean, root6, gamma, car_r, p):
    """(g, a, b) of the cut from the record's float64 fields, in longdouble, plus the sizes the
    rounding of each is measured against (the sums of the magnitudes of its terms)."""
    LD = np.longdouble
    m = [LD(v) for v in mean]
    r00, r01, r02, r11, r12, r22 = (LD(v) for v in root6)
    x, y, gm = LD(p[0]), LD(p[1]), LD(gamma)
    w0 = r00 * x + r01 * y + r02
    w1 = r01 * x + r11 * y + r12
    w2 = r02 * x + r12 * y + r22
    nw = np.sqrt(w0 * w0 + w1 * w1 + w2 * w2)
    g = m[0] * x + m[1] * y + m[2] + gm * nw + LD(0.5) * LD(car_r)
    a0, a1 = m[0], m[1]
    sa = max(abs(m[0]), abs(m[1]))
    if nw != 0:
        v0 = r00 * w0 + r01 * w1 + r02 * w2
        v1 = r01 * w0 + r11 * w1 + r12 * w2
        a0, a1 = m[0] + gm * v0 / nw, m[1] + gm * v1 / nw
        # |v| / nw <= |root|_2; the terms of v cancel like those of w
        sa += gm * (abs(r00) + abs(r01) + abs(r02) + abs(r11) + abs(r12)) * (
            abs(r00 * x) + abs(r01 * y) + abs(r02) + abs(r11 * y) + abs(r12)
            + abs(r22) + abs(r02 * x) + abs(r12 * y)) / nw
    b = a0 * x + a1 * y - g
    sg = abs(m[0] * x) + abs(m[1] * y) + abs(m[2]) + gm * (
        abs(r00 * x) + abs(r01 * y) + abs(r02) + abs(r11 * y) + abs(r12) + abs(r22)
        + abs(r02 * x) + abs(r12 * y)) + abs(LD(0.5) * LD(car_r))
    sb = sa * (abs(x) + abs(y)) + sg
    return g, (a0, a1), b, (float(sg), float(sa), float(sb))


def solve_qp_tight(H, f, G, h):
    """mo.solve_qp's answer, then its own active-set iteration again with a primal threshold of
    64 eps (1 + max |h|) instead of 1e-9 (1 + max |h|): solve_qp accepts a point that violates a
    row by up to ~1e-7 here (|h| reaches hundreds), which stalls the loop near max g = 1e-8 --
    a new cut within that slack moves nothing."""
    import scipy.linalg
    u, lam, active = mo.solve_qp(H, f, G, h)
    n = len(f)
    thr = 64 * fr.EPS * (1.0 + np.max(np.abs(h)))
    active = list(active)
    for _ in range(4 * len(h)):
        viol = G @ u - h
        if viol.max() <= thr:
            break
        active = sorted(set(active) | {int(np.argmax(viol))})
        while True:
            Ga = G[active]
            _, _, piv = scipy.linalg.qr(Ga.T, pivoting=True, mode="economic")
            keep = sorted(int(i) for i in piv[:np.linalg.matrix_rank(Ga)])
            idx = [active[i] for i in keep]
            K = np.block([[H, G[idx].T], [G[idx], np.zeros((len(idx), len(idx)))]])
            sol = np.linalg.solve(K, np.concatenate((-f, h[idx])))
            if sol[n:].min() >= -1e-12:
                break
            active = [i for i, lv in zip(idx, sol[n:]) if lv >= -1e-12]
        u, active = sol[:n], idx
    return u


def kelley(prob, tol_g=1e-6, max_rounds=12):
    """The loop.  Returns dict(status, rounds, u, X, cost, viol, viols [per round, round 0 = at
    the reference], costs [per QP])."""
    T, Gf, c, ref, goal, rows = (prob[k] for k in ("T", "Gf", "c", "ref", "goal", "rows"))
    plan = ref
    cuts, viols, costs = [], [], []
    out = dict(status=MAXROUNDS, rounds=0, u=None, X=None, cost=None)
    for rnd in range(max_rounds + 1):
        gs = []
        for r in rows:
            g, a, b = row_cut(r, plan[r["t"]])
            gs.append(g)
            cuts.append((r["t"], a, b))
        viol = max(gs) if gs else -np.inf
        viols.append(viol)
        if rnd > 0 and viol <= tol_g:
            out["status"] = OK
            break
        if rnd == max_rounds:
            break
        H, f, k, G, h = mo.assemble_qp(Gf, c, T, goal, ref, cuts, PARAMS, order="F")
        out["rounds"] = rnd + 1
        if not mo.is_feasible(G, h):
            out["status"] = INFEASIBLE
            break
        u = solve_qp_tight(H, f, G, h)
        X = (Gf @ u + c).reshape(T, 4)
        out.update(u=u, X=X, cost=mo.objective_value(u, Gf, c, T, goal, ref, PARAMS, order="F"))
        costs.append(out["cost"])
        plan = X[:, :2]
    out.update(viol=viols[-1], viols=viols, costs=costs)
    return out


def kkt(prob, u, act_tol=1e-5):
    """The certificate at u: dict(prim = max g over the cone rows, lin = the largest violation of
    the linear rows (control and speed limits), stat = the relative stationarity residual with
    non-negative least-squares multipliers over the active rows -- cone rows with their
    gradients at u --, n_active_cone, active_cone [(ov, k, t)])."""
    T, Gf, c, ref, goal, rows = (prob[k] for k in ("T", "Gf", "c", "ref", "goal", "rows"))
    H, f, k, G, h = mo.assemble_qp(Gf, c, T, goal, ref, [], PARAMS, order="F")
    X = (Gf @ u + c).reshape(T, 4)
    lin = G @ u - h
    grad = H @ u + f
    J, act = [], []
    for i in np.nonzero(lin > -act_tol * (1.0 + np.max(np.abs(h))))[0]:
        J.append(G[i])
    gs = []
    for r in rows:
        g, a, _ = row_cut(r, X[r["t"], :2])
        gs.append(g)
        if g > -act_tol:
            J.append(a @ Gf[4 * r["t"]:4 * r["t"] + 2])
            act.append((r["ov"], r["k"], r["t"]))
    lam = np.zeros(0)
    res = grad
    if J:
        import scipy.optimize
        Jm = np.array(J)
        lam = scipy.optimize.nnls(Jm.T, -grad)[0]
        res = grad + Jm.T @ lam
    n_lin = len(J) - len(act)
    strong = [a for a, lv in zip(act, lam[n_lin:]) if lv > 1e-6]
    return dict(prim=max(gs) if gs else -np.inf, lin=float(lin.max()),
                stat=float(np.max(np.abs(res))) / (1.0 + np.max(np.abs(f))),
                active_cone=act, strong_cone=strong, lam=lam)
