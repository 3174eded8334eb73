"""GPU tests of the Monte-Carlo offset calibration (ccmpc_risk_quantile behind
engine.risk_quantile, engine.calibrated_records, the cycles' .calibrate and
MidlevelAgent.calibrate_constraints) against the NumPy restatement of its contract
(tests/_quantile_ref.py).

Every comparison is bit for bit -- q and rhs as int64 views, status equal: the contract has no
order-dependent sum, so the inputs need no quantising (the record builder shared with the audit
tests quantises anyway; the ties test needs it).  Every store carries, in each padding column
between the cells and in the capacity behind the last one, a particle a million metres out in
one of the four quadrants: a tail lane that is not masked changes q."""
import numpy as np
import pytest
import torch

import _audit_ref as ar
import _quantile_ref as qr
import test_gpu_risk_audit as tga

pytestmark = pytest.mark.gpu

R_EXACT = tga.R_EXACT
COUNTS = [0, 1, 3, 63, 64, 65, 257, 513, 1025, 1500]
BIG = 1.0e6
KIND_IDS = ["halfspace", "affine", "halfspace_compact", "affine_compact"]


def _pad_columns(st, c, n):
    ends = st.offsets[1:] + [st.ld]
    return st.offsets[c] + n, ends[c]


def _store(cells, origin, gpu, capacity_extra=1000):
    """ParticleStore of the cells whose padding columns hold far-away particles."""
    from ccmpc import engine
    f32 = origin is not None
    total = sum(c.shape[0] for c in cells)
    st = engine.ParticleStore.from_cells(
        cells, device=gpu, dtype=torch.float32 if f32 else torch.float64, origin=origin,
        capacity=total + capacity_extra)
    assert st.n_bound > total
    host = st.pos.cpu().numpy()
    for c, x in enumerate(cells):
        a, b = _pad_columns(st, c, x.shape[0])
        col = np.arange(a, b)
        host[0::2, a:b] = np.where(col % 2 == 0, BIG, -BIG)[None]
        host[1::2, a:b] = np.where((col // 2) % 2 == 0, BIG, -BIG)[None]
    st.pos.copy_(torch.from_numpy(host))
    return st


def _world(cells, origin):
    """The positions the kernel sees: (double)(float)rel + origin for an f32 store."""
    if origin is None:
        return [np.asarray(x, np.float64) for x in cells]
    return [(np.asarray(x, np.float64) - origin[c]).astype(np.float32).astype(np.float64)
            + origin[c] for c, x in enumerate(cells)]


def _check(got, want):
    torch.cuda.synchronize()
    st = got.status.cpu().numpy()
    assert st.dtype == np.int32 and st.shape == want["status"].shape
    assert np.array_equal(st, want["status"]), np.argwhere(st != want["status"])[:5]
    for name in ("q", "rhs"):
        g, w = getattr(got, name).cpu().numpy(), want[name]
        assert g.dtype == np.float64 and g.shape == w.shape, name
        bad = g.view(np.int64) != w.view(np.int64)
        assert not bad.any(), (name, np.argwhere(bad)[:5], g[bad][:5], w[bad][:5])


def _allow_options(n):
    return [0, 1, int(np.floor(0.0016 * n)), n - 1, n, n + 5]


def _run(gpu, cells, origin, h, kind, T, allow, R=R_EXACT):
    from ccmpc import engine
    st = _store(cells, origin, gpu)
    want = qr.quantile(_world(cells, origin), T, R, h, kind, allow)
    got = engine.risk_quantile(st, tga._dev(h, gpu), kind, R=R, T=T,
                               allow=torch.as_tensor(np.asarray(allow, np.int64), device=gpu))
    _check(got, want)
    return st, want, got


# ---- 1: item and wave edges ---------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=KIND_IDS)
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_item_and_wave_edges(gpu, f32, kind):
    T = 8
    cells, _, _, h, origin = tga._exact_case(2000 + 10 * kind + f32, T, COUNTS, f32, kind)
    rng = np.random.default_rng(kind + 4 * f32)
    P = ar.rows(kind, T)
    for c in range(len(COUNTS)):            # a few non-finite normals: SKIPPED, never read as data
        p = rng.integers(0, P, 2)
        h["n0"][c, p[0]] = np.nan
        h["n1"][c, p[1]] = np.inf if c % 2 else -np.inf
    allow = [_allow_options(n)[(c + kind + 4 * f32) % 6] for c, n in enumerate(COUNTS)]
    _, want, _ = _run(gpu, cells, origin, h, kind, T, allow)
    for s in (qr.CAL_OK, qr.CAL_VACUOUS, qr.CAL_SKIPPED):
        assert (want["status"] == s).any()
    assert (want["status"][7:] == 0).any()  # cells that span several workgroups are selected in


def test_every_allow_option_on_every_cell(gpu):
    """Each cell of the edge counts with each of its allow options (one call per option)."""
    T, kind = 8, ar.AFFINE
    cells, _, _, h, origin = tga._exact_case(2100, T, COUNTS, False, kind)
    for k in range(6):
        allow = [_allow_options(n)[k] for n in COUNTS]
        _, want, _ = _run(gpu, cells, origin, h, kind, T, allow)
        if k == 3:      # the empty cell's N - 1 is negative: SKIPPED, decided on the device
            assert allow[0] == -1 and np.all(want["status"][0] == qr.CAL_SKIPPED)


# ---- 2: ties and signed zeros -------------------------------------------------------------
def test_ties_and_signed_zeros(gpu):
    from ccmpc import _lib
    rng = np.random.default_rng(31)
    T, kind = 4, ar.AFFINE
    counts = [200, 513, 64, 300]
    q2 = lambda x: np.round(np.asarray(x) * 4) / 4          # noqa: E731
    cells = [q2(rng.uniform(-20, 20, (1, 1, 2)) + rng.uniform(-3, 3, (n, T, 2))) for n in counts]
    cells[2][:] = cells[2][0]                      # N identical particles
    cells[3][:, :, 0] = 0.0                        # on the line x = 0
    C = len(counts)
    h = np.zeros((C, T), _lib.AFFINE_DTYPE)
    n = q2(rng.uniform(-2, 2, (C, T, 2)))
    n[(n == 0).all(-1)] = [1.0, 0.0]
    h["n0"], h["n1"] = n[..., 0], n[..., 1]
    h["side"] = rng.choice([-1, 1], (C, T))
    h["rhs"] = q2(rng.uniform(-50, 50, (C, T)))
    h["t"] = np.arange(T)[None]
    # orthogonal to every particle of cell 3, side -1: every s is +0, side*s is -0, w is +0
    h["n0"][3, 1], h["n1"][3, 1], h["side"][3, 1] = 1.0, 0.0, -1
    allow = [37, 100, 5, 11]
    _, want, _ = _run(gpu, cells, None, h, kind, T, allow)
    assert np.all(want["status"] == 0)
    width = want["n_ge"] - want["n_gt"]
    inside = (width > 1) & (want["n_gt"] < np.array(allow)[:, None])
    assert inside[:2].sum() >= 4                   # the rank falls inside a tie group
    assert np.all(width[2] == 64)                  # identical particles: one group
    assert want["q"].view(np.int64)[3, 1] == 0 and width[3, 1] == 300   # +0.0, not -0.0


# ---- 3: padding ---------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_padding_is_never_selected(gpu, f32):
    T, kind, counts = 3, ar.AFFINE, [1, 3, 65, 257, 513]
    cells, _, _, h, origin = tga._exact_case(2200 + f32, T, counts, f32, kind)
    h["status"][:] = 0
    h["t" if kind == ar.AFFINE else "t_tau"][:] = np.arange(T)[None]
    allow = [0, 1, 2, 0, 3]
    st, want, _ = _run(gpu, cells, origin, h, kind, T, allow)
    # the padding exists and would change q: the restatement on the cells with their padding
    host = st.pos.double().cpu().numpy()
    padded = []
    for c, x in enumerate(_world(cells, origin)):
        a, b = _pad_columns(st, c, x.shape[0])
        assert b > a
        pad = host[:, a:b].reshape(T, 2, b - a).transpose(2, 0, 1)
        padded.append(np.concatenate([x, pad + (origin[c] if f32 else 0.0)], 0))
    wrong = qr.quantile(padded, T, R_EXACT, h, kind, allow)
    assert np.all((wrong["q"] != want["q"]).any(1))


# ---- 4: record chunking and short horizons ------------------------------------------------
@pytest.mark.parametrize("T,kind", [(12, ar.HALFSPACE), (40, ar.HALFSPACE), (40, ar.AFFINE),
                                    (12, ar.HALFSPACE_COMPACT), (40, ar.AFFINE_COMPACT)])
def test_record_chunks(gpu, T, kind):
    counts = [65, 513]
    cells, _, _, h, origin = tga._exact_case(2300 + T + kind, T, counts, False, kind)
    assert ar.rows(kind, T) > 32                  # more than one chunk of records
    _, want, _ = _run(gpu, cells, origin, h, kind, T, [1, 7])
    assert (want["status"] == 0).sum() > 32


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_horizon_shorter_than_the_store(gpu, f32):
    for kind in (ar.AFFINE, ar.HALFSPACE):
        cells, _, _, h, origin = tga._exact_case(2400 + kind, 5, [3, 65, 513], f32, kind,
                                                 t_store=12)
        _run(gpu, cells, origin, h, kind, 5, [0, 2, 9])


def test_one_step_horizon(gpu):
    from ccmpc import engine
    for kind in (ar.AFFINE, ar.AFFINE_COMPACT):
        cells, _, _, h, origin = tga._exact_case(2500 + kind, 1, [3, 65, 513], False, kind)
        h["status"][:], h["t" if kind == ar.AFFINE else "t_tau"][:] = 0, 0
        _run(gpu, cells, origin, h, kind, 1, [0, 2, 9])
    # the half-space kinds have no rows at T = 1: the call succeeds and writes nothing
    for kind in (ar.HALFSPACE, ar.HALFSPACE_COMPACT):
        cells, _, _, h, origin = tga._exact_case(2600 + kind, 1, [3, 65], False, kind)
        st = _store(cells, origin, gpu)
        width = 32 if kind >= ar.HALFSPACE_COMPACT else 128
        got = engine.risk_quantile(st, torch.zeros((2, 0, width), dtype=torch.uint8, device=gpu),
                                   kind, R=R_EXACT, T=1)
        torch.cuda.synchronize()
        assert got.q.shape == got.rhs.shape == got.status.shape == (2, 0)


# ---- 5: round trip through the audit on the cycles' own records ---------------------------
SEED = 1


@pytest.fixture(scope="module")
def product(gpu):
    from ccmpc import cycle, engine, synthetic
    T = 8
    ovs, ref, _ = synthetic.scene(SEED, O=4, N=600, T=T)
    K = [len(o) for o in ovs]
    cells = [np.asarray(c, np.float64) for o in ovs for c in o]
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    mink = cycle.MinkowskiCycle(store, K, ref)
    mink.run()
    aff = cycle.AffineCycle(store, K, ref)
    aff.run()
    torch.cuda.synchronize()
    return dict(T=T, K=K, cells=cells, store=store, mink=mink, aff=aff)


@pytest.mark.parametrize("eps", [None, 0.8], ids=["eps_total", "eps_0.8"])
@pytest.mark.parametrize("which", ["mink", "aff"])
def test_round_trip_on_cycle_records(gpu, product, which, eps):
    from ccmpc import _lib, engine, risk
    cyc, T, cells, K = product[which], product["T"], product["cells"], product["K"]
    kind = ar.HALFSPACE if which == "mink" else ar.AFFINE
    counts = [c.shape[0] for c in cells]
    allow = risk.allow_counts(counts, K, T, **({} if eps is None else dict(eps=eps)))
    if eps is not None:
        assert allow.max() > 0
    h = cyc.records()
    want = qr.quantile(cells, T, cyc.R, h, kind, allow)
    quant = cyc.calibrate(allow)
    _check(quant, want)
    cal = want["status"] == 0
    assert cal.sum() > cal.size // 2
    before = cyc.rec.clone()

    def rec_open(rec):
        a = engine.risk_audit(product["store"], rec=rec, rec_kind=kind, R=cyc.R)
        torch.cuda.synchronize()
        return a.rec_open.cpu().numpy()

    # rhs <- rhs*: exactly the particles strictly beyond q stay open, at most allow
    replaced = engine.calibrated_records(cyc.rec, kind, quant, "replace")
    ro = rec_open(replaced)
    assert np.array_equal(ro[cal], want["n_gt"][cal])
    assert np.all(ro[cal] <= np.broadcast_to(allow[:, None], ro.shape)[cal])
    # u* one ulp towards the particles: more than allow stay open
    n0, n1, rhs, side, status, t = engine.record_fields(replaced, kind)
    assert np.array_equal(rhs.view(np.int64)[cal], want["rhs"].view(np.int64)[cal])
    assert np.array_equal(rhs[~cal], engine.record_fields(before, kind)[2][~cal])
    inward = np.where(cal, side * np.nextafter(side * rhs, -np.inf), rhs)
    h2 = h.copy()
    h2["d" if kind == ar.HALFSPACE else "rhs"] = inward
    ro2 = rec_open(tga._dev(h2, gpu))
    assert np.all(ro2[cal] >= want["n_ge"][cal])
    assert np.all(ro2[cal] > np.broadcast_to(allow[:, None], ro2.shape)[cal])
    # tighten / relax against their definitions, elementwise; everything else byte-identical
    old = engine.record_fields(before, kind)[2]
    name = "d" if kind == ar.HALFSPACE else "rhs"
    for mode, pick in (("tighten", np.maximum), ("relax", np.minimum)):
        out = engine.calibrated_records(cyc.rec, kind, quant, mode)
        new = engine.record_fields(out, kind)[2]
        expect = np.where(cal, side * pick(side * old, side * want["rhs"]), old)
        assert np.array_equal(new.view(np.int64), expect.view(np.int64)), mode
        a = out.cpu().numpy().view(_lib.HALFSPACE_DTYPE if kind == ar.HALFSPACE
                                   else _lib.AFFINE_DTYPE)[..., 0].copy()
        a[name] = old
        assert a.tobytes() == before.cpu().numpy().tobytes(), mode
    assert torch.equal(cyc.rec, before)             # the cycle's own tensor is never written
    with pytest.raises(ValueError):
        engine.calibrated_records(cyc.rec, kind, quant, "loosen")
    # the compact packing carries the same calibration
    from ccmpc import dist
    comp = dist.compact_records(cyc.rec, kind)
    torch.cuda.synchronize()
    ckind = kind + 2
    _check(engine.risk_quantile(product["store"], comp, ckind, allow=allow, R=cyc.R), want)
    cout = engine.calibrated_records(comp, ckind, quant, "replace")
    assert np.array_equal(engine.record_fields(cout, ckind)[2].view(np.int64),
                          rhs.view(np.int64))


# ---- 6: determinism, capture, workspace reuse ---------------------------------------------
def test_capture_and_reuse(gpu):
    from ccmpc import engine
    T, kind, counts = 8, ar.HALFSPACE, [65, 700, 3]
    cellsA, _, _, h, origin = tga._exact_case(2700, T, counts, False, kind)
    cellsB, _, _, hB, _ = tga._exact_case(2701, T, counts, False, kind)
    allow = [1, 4, 0]
    wantA = qr.quantile(cellsA, T, R_EXACT, h, kind, allow)
    wantB = qr.quantile(cellsB, T, R_EXACT, hB, kind, allow)
    assert not np.array_equal(wantA["q"], wantB["q"])
    st = _store(cellsA, origin, gpu)
    posA = st.pos.clone()
    posB = _store(cellsB, origin, gpu).pos.clone()
    assert posA.shape == posB.shape
    rec, recB = tga._dev(h, gpu), tga._dev(hB, gpu)
    al = torch.as_tensor(np.asarray(allow, np.int64), device=gpu)
    # two different inputs back to back on one RiskQuantile
    out = engine.risk_quantile(st, rec, kind, allow=al, R=R_EXACT, T=T)
    _check(out, wantA)
    st.pos.copy_(posB)
    again = engine.risk_quantile(st, recB, kind, allow=al, R=R_EXACT, T=T, out=out)
    assert all(a is b for a, b in zip(again, out))
    _check(out, wantB)
    st.pos.copy_(posA)
    _check(engine.risk_quantile(st, rec, kind, allow=al, R=R_EXACT, T=T, out=out), wantA)
    # captured (a linear graph), replayed twice, then on the store changed in place
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        engine.risk_quantile(st, rec, kind, allow=al, R=R_EXACT, T=T, out=out)
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        engine.risk_quantile(st, rec, kind, allow=al, R=R_EXACT, T=T, out=out)
    for t in out:
        t.fill_(0xA5 if t.dtype == torch.uint8 else -7)   # needs no initialised buffers
    graph.replay()
    _check(out, wantA)
    first = [t.clone() for t in out[:3]]
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out[:3], first):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    st.pos.copy_(posB)
    rec.copy_(recB)
    graph.replay()
    _check(out, wantB)


# ---- 7: planner surface -------------------------------------------------------------------
def test_planner_calibrate_constraints(gpu):
    from ccmpc import engine, episode, risk
    rep = episode.EpisodeReplay(O=2, N=3000, ph=8, n_ideal=20_000, receding_steps=1, seed=5,
                                device=gpu)
    agent, ph = rep.agent, 8
    K = [int(np.count_nonzero(rep.pmf[o] > 0.1)) for o in range(rep.O)]
    eps = np.full((rep.O, max(K)), 0.05 / rep.O)
    with pytest.raises(RuntimeError):
        agent.calibrate_constraints()
    ref = rep.ref_traj(0)
    sampler = dict(init_state=rep.init, latent_pmf=rep.pmf, gmm=rep.gmm, N=rep.N,
                   seed=rep.seed * 7919)
    agent.predict_and_constrain(episode.Params(rep.O, K, 0), sampler, eps, ph, ref, rep.minpos,
                                rep.pasts)
    scene, _, T, (rec, kind, _) = agent._audit_src
    assert T == ph and kind == ar.HALFSPACE
    before = rec.clone()
    report, cal_rec = agent.calibrate_constraints(mode="tighten")
    store = scene.store
    C = store.n_cells
    allow = risk.allow_counts(store.counts, K, ph)
    rec3 = rec.reshape(C, -1, 128)
    quant = engine.risk_quantile(store, rec3, kind, allow=allow, R=agent.R, T=ph)
    torch.cuda.synchronize()
    assert np.array_equal(report["status"], quant.status.cpu().numpy())
    assert np.array_equal(report["allow"], allow) and report["allow"].max() > 0
    n0, n1, rhs, side, status, t = engine.record_fields(rec3, kind)
    P = ph * (ph - 1) // 2
    cal = report["status"] == 0
    assert cal.any()
    slack = side[:, :P] * rhs[:, :P] - side[:, :P] * quant.rhs.cpu().numpy()
    assert np.array_equal(report["slack"][cal], slack[cal]) and np.all(np.isnan(
        report["slack"][~cal]))
    assert torch.equal(cal_rec, engine.calibrated_records(rec3, kind, quant, "tighten"))
    assert cal_rec.shape == rec3.shape and torch.equal(rec, before)
    # the restatement agrees with what the planner reported
    cells = [store.cell_positions(j) for j in range(C)]
    want = qr.quantile(cells, ph, agent.R, agent.last_records, kind, allow)
    assert np.array_equal(report["rhs_cal"].view(np.int64), want["rhs"].view(np.int64))
    assert isinstance(agent.calibrate_constraints(), dict)       # no mode: the report alone
    # a later step of the same shape overwrites the store: stale
    sampler["seed"] = rep.seed * 7919 + 1
    agent.predict_and_constrain(episode.Params(rep.O, K, 1), sampler, eps, ph, rep.ref_traj(1),
                                rep.minpos, rep.pasts)
    stale = agent._audit_src
    agent._audit_src = (scene,) + tuple(stale[1:])
    with pytest.raises(RuntimeError, match="stale"):
        agent.calibrate_constraints()
    agent._audit_src = stale
    # Tsh < ph: the frame's records were never materialised
    T = ph - 1
    ref = rep.ref_traj(10)
    sampler["seed"] = rep.seed * 7919 + 10
    agent.predict_and_constrain(episode.Params(rep.O, K, 10), sampler, eps, T, ref[:T],
                                rep.minpos, rep.pasts)
    with pytest.raises(RuntimeError, match="no materialised records"):
        agent.calibrate_constraints()
