"""GPU tests of the Monte-Carlo risk audit (ccmpc_risk_audit behind engine.risk_audit, the
cycles' .audit and MidlevelAgent.audit_plan) against the NumPy restatement of its contract
(tests/_audit_ref.py).

Exact cases: every input is quantised so that every product and sum of the contract is exact
in float64 -- positions and plans multiples of 2^-6 within +-256, normals multiples of 2^-4
within +-4, rhs a multiple of 2^-10, R = 3.5 -- so integer outputs must be equal and min_d2
bit-equal whatever the evaluation order, and the constructed ties (a particle exactly R from
the plan, a record exactly tangent) test the strict / non-strict comparisons."""
import numpy as np
import pytest
import torch

import _audit_ref as ar

pytestmark = pytest.mark.gpu

R_EXACT = 3.5
COUNTS = [0, 1, 3, 63, 64, 65, 257]


def _q(x, bits):
    return np.round(np.asarray(x) * (1 << bits)) / (1 << bits)


def _exact_case(seed, T, counts, f32, kind, t_store=None, two_plans=True):
    """(cells world f64 [N_c, t_store, 2], plan [n_plans, T, 2], cell_plan, records [C, P] of
    `kind`, origin or None)."""
    from ccmpc import _lib
    rng = np.random.default_rng(seed)
    t_store = T if t_store is None else t_store
    C = len(counts)
    n_plans = 2 if two_plans else 1
    plan = _q(rng.uniform(-150, 150, (n_plans, 1, 2)) + np.cumsum(
        rng.uniform(-1.5, 1.5, (n_plans, t_store, 2)), 1), 6)
    cell_plan = (np.arange(C) % n_plans).astype(np.int32)
    origin = _q(rng.uniform(-40, 40, (C, 2)), 6) if f32 else None
    cells = []
    for c, n in enumerate(counts):
        x = plan[cell_plan[c]][None] + _q(rng.uniform(-8, 8, (n, t_store, 2)), 6)
        if n > 0:
            x[0] = plan[cell_plan[c]] + [R_EXACT, 0.0]          # exactly R away: not a hit
        if n > 1:
            x[1] = plan[cell_plan[c]] + [0.0, -R_EXACT + 2.0 ** -6]   # one quantum inside
        cells.append(x)
    assert all(np.abs(x).max(initial=0) <= 256 for x in cells)
    # records: most at their canonical step, a quarter at a random step of the horizon
    half = kind in (ar.HALFSPACE, ar.HALFSPACE_COMPACT)
    P = ar.rows(kind, T)
    h = np.zeros((C, P), _lib.HALFSPACE_DTYPE if half else _lib.AFFINE_DTYPE)
    if half:
        t_of = np.array([t for t in range(T) for _ in range(t)], np.int64)
        tau_of = np.array([tau for t in range(T) for tau in range(t)], np.int64)
    else:
        t_of, tau_of = np.arange(T), np.zeros(T, np.int64)
    for c in range(C):
        t = t_of.copy()
        move = rng.uniform(size=P) < 0.25
        t[move] = rng.integers(0, T, int(move.sum()))
        n = _q(rng.uniform(-4, 4, (P, 2)), 4)
        n[(n == 0).all(1)] = [1.0, 0.0]
        side = rng.choice([-1, 1], P)
        pl = plan[cell_plan[c]]
        rhs = _q((n * pl[t]).sum(1) + rng.uniform(-20, 20, P), 10)
        status = np.where(rng.uniform(size=P) < 0.15, rng.choice([-10, -11, -12, -13], P), 0)
        bad_t = rng.uniform(size=P) < 0.1
        t_field = np.where(bad_t, rng.choice([-1, T, T + 3], P), t)
        if P and counts[c] > 0:
            # record 0: exactly tangent to particle 0 at its step, from the feasible side
            t0 = int(t[0])
            n[0], side[0], status[0], t_field[0] = [0.0, 1.0], 1, 0, t0
            rhs[0] = cells[c][0, t0, 1] + R_EXACT
        if P > 1 and counts[c] > 0:
            # record 1: one rhs quantum short of tangent to particle 0: open for it
            t1 = int(t[1])
            n[1], side[1], status[1], t_field[1] = [1.0, 0.0], -1, 0, t1
            rhs[1] = cells[c][0, t1, 0] - R_EXACT + 2.0 ** -10
        h["n0"][c], h["n1"][c], h["side"][c], h["status"][c] = n[:, 0], n[:, 1], side, status
        h["d" if half else "rhs"][c] = rhs
        if half:
            h["t_tau"][c] = (t_field.astype(np.int64) << 16) | tau_of
            h["t_tau"][c][t_field < 0] = -1 - tau_of[t_field < 0]      # negative: t = -1
        else:
            h["t"][c] = t_field
    if kind >= ar.HALFSPACE_COMPACT:
        h = ar.compact(h, ar.HALFSPACE if half else ar.AFFINE)
    return cells, plan[:, :T].copy(), cell_plan, h, origin


def _store(cells, origin, gpu, plan, cell_plan, capacity_extra=1000):
    """ParticleStore of the cells with every padding column (between a cell's count and the
    next cell's offset, and the unused capacity behind the last cell) holding a particle that
    sits ON the cell's plan: an unmasked tail lane shows up as extra hits."""
    from ccmpc import engine
    f32 = origin is not None
    total = sum(c.shape[0] for c in cells)
    st = engine.ParticleStore.from_cells(
        cells, device=gpu, dtype=torch.float32 if f32 else torch.float64, origin=origin,
        capacity=total + capacity_extra)
    assert st.n_bound > total
    host = st.pos.cpu().numpy()
    t_store = cells[0].shape[1]
    ends = st.offsets[1:] + [st.ld]
    for c, x in enumerate(cells):
        a, b = st.offsets[c] + x.shape[0], ends[c]
        pl = np.zeros((t_store, 2))
        pl[:plan.shape[1]] = plan[cell_plan[c]]
        if f32:
            pl = pl - origin[c]
        host[:, a:b] = pl.reshape(2 * t_store)[:, None]
    st.pos.copy_(torch.from_numpy(host))
    return st


def _dev(h, gpu):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).reshape(
        h.shape[0], h.shape[1], h.dtype.itemsize)).to(gpu)


def _check(got, want):
    torch.cuda.synchronize()
    for name in ("hit", "hit_any", "rec_open", "open"):
        g, w = getattr(got, name), want[name]
        assert (g is None) == (w is None), name
        if w is not None:
            g = g.cpu().numpy()
            assert g.dtype == np.int64 and g.shape == w.shape, name
            assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5], g[g != w][:5],
                                          w[g != w][:5])
    if want["min_d2"] is not None:
        g = got.min_d2.cpu().numpy()
        assert np.array_equal(g.view(np.int64), want["min_d2"].view(np.int64))
    else:
        assert got.min_d2 is None


def _run_exact(gpu, seed, T, counts, f32, kind, t_store=None):
    from ccmpc import engine
    cells, plan, cell_plan, h, origin = _exact_case(seed, T, counts, f32, kind, t_store)
    st = _store(cells, origin, gpu, plan, cell_plan)
    want = ar.audit(cells, T, R_EXACT, plan=plan, cell_plan=cell_plan, rec=h, kind=kind)
    got = engine.risk_audit(st, plan=torch.from_numpy(plan).to(gpu), rec=_dev(h, gpu),
                            rec_kind=kind, R=R_EXACT, T=T,
                            cell_plan=torch.from_numpy(cell_plan).to(gpu))
    _check(got, want)
    return cells, st, plan, cell_plan, h, want


@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["halfspace", "affine", "halfspace_compact",
                                                    "affine_compact"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("T", [1, 3, 8, 12, 40])
def test_exact_cases(gpu, T, f32, kind):
    cells, st, plan, cell_plan, h, want = _run_exact(gpu, 1000 + 10 * T + kind, T, COUNTS, f32,
                                                     kind)
    # the constructed ties decided as the contract says
    n_plans = plan.shape[0]
    for c, x in enumerate(cells):
        if x.shape[0] == 0:
            assert np.all(np.isinf(want["min_d2"][c])) and want["hit_any"][c] == 0
            continue
        pl = plan[cell_plan[c]]
        assert ((x[0, :T] - pl) ** 2).sum(1).tolist() == [R_EXACT ** 2] * T   # the tie exists
        if x.shape[0] > 1:
            assert want["hit"][c].min() >= 1 and want["hit_any"][c] >= 1     # particle 1
    assert n_plans == 2 and want["rec_open"].shape[1] == ar.rows(kind, T)
    if ar.rows(kind, T) >= 8:
        assert (want["rec_open"] == -1).any() and (want["rec_open"] >= 0).any()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_exact_several_workgroups_per_cell(gpu, f32):
    _run_exact(gpu, 77, 8, [20000, 31], f32, ar.HALFSPACE)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_exact_horizon_shorter_than_the_store(gpu, f32):
    _run_exact(gpu, 78, 5, COUNTS, f32, ar.AFFINE, t_store=8)
    _run_exact(gpu, 79, 5, COUNTS, f32, ar.HALFSPACE, t_store=7)


def test_tangent_and_near_tangent_records(gpu):
    """Record 0 of every non-empty cell is exactly tangent to particle 0 (protected), record 1
    one rhs quantum short of it (open): the restatement sees the difference, and so does the
    kernel (test_exact_cases compares them; this pins that the constructed cases are what
    they claim)."""
    T = 8
    cells, plan, cell_plan, h, _ = _exact_case(5, T, [3, 64], False, ar.AFFINE)
    n0, n1, rhs, side, status, t = ar.rec_fields(h, ar.AFFINE)
    for c, x in enumerate(cells):
        for p, expect in ((0, True), (1, False)):
            tp = int(t[c, p])
            assert status[c, p] == 0
            ok = ar.protects(n0[c, p], n1[c, p], rhs[c, p], side[c, p], x[0, tp, 0],
                             x[0, tp, 1], R_EXACT)
            assert bool(ok) is expect
    _run_exact(gpu, 5, T, [3, 64], False, ar.AFFINE)


def test_either_half_switched_off(gpu):
    from ccmpc import engine
    T = 8
    cells, plan, cell_plan, h, origin = _exact_case(6, T, COUNTS, True, ar.HALFSPACE)
    st = _store(cells, origin, gpu, plan, cell_plan)
    tp, tc = torch.from_numpy(plan).to(gpu), torch.from_numpy(cell_plan).to(gpu)
    _check(engine.risk_audit(st, plan=tp, cell_plan=tc, R=R_EXACT, T=T),
           ar.audit(cells, T, R_EXACT, plan=plan, cell_plan=cell_plan))
    _check(engine.risk_audit(st, rec=_dev(h, gpu), rec_kind=ar.HALFSPACE, R=R_EXACT, T=T),
           ar.audit(cells, T, R_EXACT, rec=h, kind=ar.HALFSPACE))
    with pytest.raises(ValueError):
        engine.risk_audit(st, R=R_EXACT)
    with pytest.raises(ValueError):
        engine.risk_audit(st, plan=tp, R=R_EXACT, T=T)          # two plans, no cell_plan


# ---- product case -------------------------------------------------------------------------
SEED = 1


def _margin_ok(cells, T, R, plans, h, kind, rel=1e-9):
    """No decision quantity within `rel` of its threshold (so equality with the restatement does
    not hang on the last bit of anything)."""
    for x in cells:
        for pl in plans:
            d2 = ((x[:, :T] - pl[None, :T]) ** 2).sum(2)
            if np.any(np.abs(d2 - R * R) <= rel * R * R):
                return False
    n0, n1, rhs, side, status, t = ar.rec_fields(h, kind)
    for c, x in enumerate(cells):
        for p in range(ar.rows(kind, T)):
            if status[c, p] != 0 or not 0 <= t[c, p] < T:
                continue
            px, py = x[:, t[c, p], 0], x[:, t[c, p], 1]
            s = n0[c, p] * px + n1[c, p] * py
            v = side[c, p] * (rhs[c, p] - s)
            r2n = R * R * (n0[c, p] ** 2 + n1[c, p] ** 2)
            if np.any(np.abs(v) <= rel * (abs(rhs[c, p]) + np.abs(s))):
                return False
            if np.any(np.abs(v * v - r2n) <= rel * r2n):
                return False
    return True


@pytest.fixture(scope="module")
def product(gpu):
    from ccmpc import cycle, engine, synthetic
    T = 8
    ovs, ref, _ = synthetic.scene(SEED, O=2, N=600, T=T, K=2)
    K = [len(o) for o in ovs]
    cells = [np.asarray(c, np.float64) for o in ovs for c in o]
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    track = cells[0].mean(0)                        # the first OV's mean track
    line = track[0][None] + np.linspace(0.0, 1.0, T)[:, None] * (track[-1] - track[0])[None]
    mink = cycle.MinkowskiCycle(store, K, ref)
    mink.run()
    aff = cycle.AffineCycle(store, K, ref)
    aff.run()
    torch.cuda.synchronize()
    return dict(T=T, K=K, cells=cells, store=store, plans=[np.asarray(ref, np.float64), line],
                mink=mink, aff=aff)


@pytest.mark.parametrize("which", ["mink", "aff"])
def test_product_cycles_audit_equals_restatement(gpu, product, which):
    from ccmpc import risk
    cyc = product[which]
    kind = ar.HALFSPACE if which == "mink" else ar.AFFINE
    T, cells, R = product["T"], product["cells"], risk.R_COLLISION
    assert cyc.R == R == 3.4
    h = cyc.records()
    assert _margin_ok(cells, T, R, product["plans"], h, kind), "pick another SEED"
    n0, n1, rhs, side, status, t = ar.rec_fields(h, kind)
    n_checked = 0
    for plan in product["plans"]:
        got = cyc.audit(torch.from_numpy(plan).to(gpu))
        want = ar.audit(cells, T, R, plan=plan, rec=h, kind=kind)
        _check(got, want)
        assert want["hit"].sum() <= sum(c.shape[0] for c in cells) * T
        # where the plan satisfies every status-0 record of (c, t): every hit particle is open
        for c in range(len(cells)):
            for tt in range(T):
                m = (status[c] == 0) & (t[c] == tt)
                g = side[c, m] * ((n0[c, m] * plan[tt, 0] + n1[c, m] * plan[tt, 1]) - rhs[c, m])
                scale = np.abs(rhs[c, m]) + np.abs(n0[c, m] * plan[tt, 0]) + np.abs(
                    n1[c, m] * plan[tt, 1])
                if np.all(g >= 1e-9 * scale):
                    assert want["hit"][c, tt] <= want["open"][c, tt]
                    n_checked += 1
    assert n_checked > 0
    # the line through the first OV's mean track runs into its particles
    line = ar.audit(cells, T, R, plan=product["plans"][1])
    assert line["hit_any"][0] > 0
    rep = risk.audit_report(cyc.audit(torch.from_numpy(product["plans"][1]).to(gpu)),
                            [c.shape[0] for c in cells], product["K"], T)
    assert np.array_equal(rep["hit_any"], line["hit_any"])
    assert rep["traj_within_budget"].shape == (len(cells),) and not rep["traj_within_budget"][0]


# ---- graph and planner --------------------------------------------------------------------
def test_audit_captured_in_a_graph_follows_the_plan(gpu):
    from ccmpc import engine
    T = 8
    cells, plan, cell_plan, h, origin = _exact_case(9, T, [65, 700, 3], False, ar.HALFSPACE,
                                                    two_plans=False)
    planB = plan + _q([[1.25, -0.5]], 6)
    st = _store(cells, origin, gpu, plan, cell_plan)
    rec = _dev(h, gpu)
    tp = torch.from_numpy(plan).to(gpu)
    out = engine.risk_audit(st, plan=tp, rec=rec, rec_kind=ar.HALFSPACE, R=R_EXACT, T=T)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        engine.risk_audit(st, plan=tp, rec=rec, rec_kind=ar.HALFSPACE, R=R_EXACT, T=T, out=out)
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        again = engine.risk_audit(st, plan=tp, rec=rec, rec_kind=ar.HALFSPACE, R=R_EXACT, T=T,
                                  out=out)
    assert all(a is b for a, b in zip(again, out))
    for t in out:
        t.fill_(-7)                                  # the call initialises its own outputs
    wantA = ar.audit(cells, T, R_EXACT, plan=plan, rec=h, kind=ar.HALFSPACE)
    wantB = ar.audit(cells, T, R_EXACT, plan=planB, rec=h, kind=ar.HALFSPACE)
    assert not np.array_equal(wantA["hit"], wantB["hit"])
    graph.replay()
    _check(out, wantA)
    first = [t.clone() for t in out]
    tp.copy_(torch.from_numpy(planB).to(gpu))
    graph.replay()
    _check(out, wantB)
    tp.copy_(torch.from_numpy(plan).to(gpu))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, first):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_planner_audit_plan(gpu):
    from ccmpc import episode, risk
    rep = episode.EpisodeReplay(O=2, N=3000, ph=8, n_ideal=20_000, receding_steps=1, seed=5,
                                device=gpu)
    agent, ph = rep.agent, 8
    K = [int(np.count_nonzero(rep.pmf[o] > 0.1)) for o in range(rep.O)]
    eps = np.full((rep.O, max(K)), 0.05 / rep.O)
    with pytest.raises(RuntimeError):
        agent.audit_plan(np.zeros((ph, 4)))

    def restate(T, plan, h):
        st = agent._audit_src[0].store
        cells = [st.cell_positions(j) for j in range(st.n_cells)]
        return cells, ar.audit(cells, T, agent.R, plan=plan, rec=h,
                               kind=ar.HALFSPACE if h is not None else None)

    # Tsh == ph: one frame, one QP, the audit of its X_star and of the frame's records
    ref = rep.ref_traj(0)
    sampler = dict(init_state=rep.init, latent_pmf=rep.pmf, gmm=rep.gmm, N=rep.N,
                   seed=rep.seed * 7919)
    agent.predict_and_constrain(episode.Params(rep.O, K, 0), sampler, eps, ph, ref, rep.minpos,
                                rep.pasts)
    ctrl = agent.solve_planning_qp(rep.x_init(0), ref[-1] + [4.0, 0.5], ref, ph,
                                   lon=agent.ego_lon)
    X = ctrl["X_star"]
    report = agent.audit_plan(X)
    cells, want = restate(ph, X[:, :2], agent.last_records)
    for name in ("hit", "hit_any", "rec_open", "open"):
        assert np.array_equal(report[name], want[name]), name
    assert np.array_equal(report["min_d2"], want["min_d2"])
    assert np.array_equal(report["counts"], [c.shape[0] for c in cells])
    assert np.array_equal(report["budget_traj"], np.full(sum(K), risk.EPS_TOTAL / rep.O))
    assert np.array_equal(report["budget_step"], report["budget_traj"] / ph)
    wider = agent.audit_plan(X, R=2 * agent.R)
    assert np.all(wider["hit"] >= report["hit"]) and np.all(wider["open"] >= report["open"])

    # Tsh < ph: the records come from the ideal rollout, so only the plan is audited
    T = ph - 1
    ref = rep.ref_traj(10)
    sampler["seed"] = rep.seed * 7919 + 10
    agent.predict_and_constrain(episode.Params(rep.O, K, 10), sampler, eps, T, ref[:T],
                                rep.minpos, rep.pasts)
    report = agent.audit_plan(ref[:T])
    cells, want = restate(T, ref[:T], None)
    assert report["rec_open"] is None and report["open"] is None and report["p_open"] is None
    assert np.array_equal(report["hit"], want["hit"])
    assert np.array_equal(report["hit_any"], want["hit_any"])
    assert report["p_hit"].shape == (sum(K), T)
    with pytest.raises(ValueError):
        agent.audit_plan(np.zeros((ph, 2)))          # the last frame's horizon is T
