"""GPU tests of the Monte-Carlo audit on the ideal rollout's samples
(ccmpc_ideal_risk_audit behind engine.ideal_risk_audit).

The oracle is the contract's own sentence: engine.ideal_rollout (Philox) followed by
engine.risk_audit on its store, device against device.  All five outputs and the status must be
EQUAL -- integers exactly, min_d2 as int64 bit patterns; there is no tolerance anywhere.  On the
small cases tests/_audit_ref.audit on the rollout read back to the host is compared too, so the
tests do not rest on ccmpc_risk_audit alone.

Source moments: engine.moments of a store the test builds, 3 cells x 500 particles of a random
walk with independent increments (every conditional covariance is positive definite).

Not vacuous: every plan row is a cell's mean path displaced by R along x, so the disc's edge
passes through the cloud; the "shifted" record sets have rhs = n.mean_t + side R |n|, which puts
the predicate's boundary through the centre of the cloud.  The conditions on the oracle's
output (0 < sum hit < sum N T, hit_any != max_t hit somewhere, some rec_open strictly between 0
and N) are asserted where they can hold at all: a cell of one sample has hit_any == max_t hit,
and one step has hit_any == hit, so they are asserted from 257 samples and 2 steps on."""
import functools

import numpy as np
import pytest
import torch

import _audit_ref as ar

pytestmark = pytest.mark.gpu

R = 3.4
C = 3
SEED = 11


@functools.lru_cache(maxsize=None)
def _source(T_src):
    """(mean [C, T_src, 2], cov [C, 2 T_src, 2 T_src]) device moments of the test's own store."""
    from ccmpc import engine
    rng = np.random.default_rng(100 + T_src)
    cells = [np.array([190.0 + 3 * c, 5.0 - 2 * c]) + np.cumsum(
        rng.normal([1.5, 0.2 * c], 0.6, size=(500, T_src, 2)), axis=1) for c in range(C)]
    store = engine.ParticleStore.from_cells(cells, device="cuda:0")
    mean, cov = engine.moments(store)
    torch.cuda.synchronize()
    return mean, cov


def _i32(x, gpu):
    return None if x is None else torch.tensor(list(x), dtype=torch.int32, device=gpu)


def _dev(h, gpu):
    if h.shape[1] == 0:                      # T = 1 of the half-space kinds: no rows
        return torch.empty((h.shape[0], 0, h.dtype.itemsize), dtype=torch.uint8, device=gpu)
    return torch.from_numpy(np.ascontiguousarray(h).view(np.uint8).reshape(
        h.shape[0], h.shape[1], h.dtype.itemsize)).to(gpu)


@functools.lru_cache(maxsize=None)
def _frame(T_src, T, n, src=None, x0=False, rng_cell=None, seed=SEED):
    """What a frame at these rollout arguments holds, computed once: the cycle's mean path and
    its own half-space records, the affine records of the ideal moments, the plan rows (each
    cell's mean path displaced by R along x) -- all on the host."""
    from ccmpc import engine, risk
    gpu = torch.device("cuda:0")
    pm, pc = _source(T_src)
    nc = len(src) if src is not None else C
    s = _i32(src if src is not None else range(C), gpu)
    x0_t = _x0(T_src, nc, gpu) if x0 else None
    n_cyc = max(n, 64)                       # the fused moments need a sample covariance
    cr = torch.as_tensor(risk.cell_risk(risk.eps_ura([nc]), [nc], T_src), device=gpu)
    ref = torch.as_tensor((np.array([170.0, 5.0]) + np.arange(1, T + 1)[:, None] * [4.0, 0.5])
                          [None], device=gpu)
    mean, cov, st, rec, _ = engine.ideal_minkowski_cycle(
        pm, pc, s, T, n_cyc, ref, cr, x0=x0_t, seed=seed, rng_cell=_i32(rng_cell, gpu), R=R)
    m2, c2, _ = engine.ideal_moments(pm, pc, s, T, n_cyc, x0=x0_t, seed=seed,
                                     rng_cell=_i32(rng_cell, gpu))
    aff = engine.affine(m2, c2, ref, cr[:, 2].contiguous(), R=R)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * nc
    mean_h = mean.cpu().numpy()
    plan = mean_h + np.array([R, 0.0])
    return dict(mean=mean_h, plan=plan, half=engine.halfspaces(rec)[:, :T * (T - 1) // 2].copy(),
                aff=engine.affine_records(aff).copy())


def _x0(T_src, nc, gpu):
    pm, _ = _source(T_src)
    m0 = pm[:, 0, :].cpu().numpy()
    return torch.as_tensor((m0[np.arange(nc) % C] + [0.25, -0.5]).copy(), device=gpu)


def _records(fr, kind, T, shifted=False, edits=False):
    """Host records of `kind` (a 128-byte kind) from a frame: the generator's own, or shifted so
    that the predicate's boundary passes through the cloud's centre; with `edits` some rows get
    status -11 and some a step outside [0, T)."""
    half = kind == ar.HALFSPACE
    h = fr["half" if half else "aff"].copy()
    n0, n1, _, side, _, t = ar.rec_fields(h, kind)
    if shifted and h.size:
        mt = np.take_along_axis(fr["mean"], np.clip(t, 0, T - 1)[:, :, None], axis=1)
        h["d" if half else "rhs"] = (n0 * mt[:, :, 0] + n1 * mt[:, :, 1]
                                     + side * R * np.sqrt(n0 * n0 + n1 * n1))
    if edits and h.shape[1] >= 3:
        P = h.shape[1]
        h["status"][:, 1 % P] = -11
        if half:
            tau = h["t_tau"] & 0xffff
            h["t_tau"][0, P - 1] = (T << 16) | tau[0, P - 1]        # t = T
            h["t_tau"][1, P - 2] = -1 - tau[1, P - 2]               # negative: t = -1
        else:
            h["t"][0, P - 1] = T
            h["t"][1, P - 2] = -1
    return h


def _rec_dev(h, kind, gpu):
    """Device bytes of the host records h (of kind & 1) as `kind`, compact kinds through
    ccmpc_compact_records."""
    from ccmpc import dist
    d = _dev(h, gpu)
    if kind >= ar.HALFSPACE_COMPACT:
        if d.shape[1] == 0:
            return torch.empty((d.shape[0], 0, 32), dtype=torch.uint8, device=gpu)
        return dist.compact_records(d, kind - 2)
    return d


def _both(gpu, T_src, T, n, plan=None, cell_plan=None, rec=None, kind=None, src=None, x0=None,
          rng_cell=None, seed=SEED, pc=None, out=None, seed_dev=None):
    """(new call's (RiskAudit, status), oracle's (RiskAudit, status, store))."""
    from ccmpc import engine
    pm, pc0 = _source(T_src)
    pc = pc0 if pc is None else pc
    s = _i32(src if src is not None else range(C), gpu)
    r = _i32(rng_cell, gpu)
    store, wst = engine.ideal_rollout(pm, pc, s, T, n, x0=x0, seed=seed, rng_cell=r)
    assert store.counts == [n] * len(s)
    want = engine.risk_audit(store, plan=plan, rec=rec, rec_kind=kind, R=R, cell_plan=cell_plan,
                             T=T)
    got, gst = engine.ideal_risk_audit(pm, pc, s, T, n, plan=plan, rec=rec, rec_kind=kind, R=R,
                                       cell_plan=cell_plan, x0=x0, seed=seed, seed_dev=seed_dev,
                                       rng_cell=r, out=out)
    torch.cuda.synchronize()
    return (got, gst), (want, wst, store)


def _host(a):
    return {k: (None if getattr(a, k) is None else getattr(a, k).cpu().numpy())
            for k in ("hit", "hit_any", "min_d2", "rec_open", "open")}


def _assert_equal(got, want, what=""):
    """got / want: RiskAudit or the dict _host makes.  Integers exactly, min_d2 bit for bit."""
    g = got if isinstance(got, dict) else _host(got)
    w = want if isinstance(want, dict) else _host(want)
    for name in ("hit", "hit_any", "rec_open", "open"):
        assert (g[name] is None) == (w[name] is None), (what, name)
        if w[name] is not None:
            assert g[name].dtype == np.int64 and g[name].shape == w[name].shape, (what, name)
            bad = g[name] != w[name]
            assert not bad.any(), (what, name, np.argwhere(bad)[:5], g[name][bad][:5],
                                   w[name][bad][:5])
    assert (g["min_d2"] is None) == (w["min_d2"] is None), what
    if w["min_d2"] is not None:
        assert np.array_equal(g["min_d2"].view(np.int64), w["min_d2"].view(np.int64)), (
            what, g["min_d2"], w["min_d2"])


def _check(new, oracle, what=""):
    (got, gst), (want, wst, _) = new, oracle
    _assert_equal(got, want, what)
    assert gst.dtype == torch.int32 and gst.cpu().tolist() == wst.cpu().tolist(), what


def _check_ref(oracle, T, plan, cell_plan, h, kind, what=""):
    """The oracle's output against the NumPy restatement on the rollout read back."""
    want, _, store = oracle
    cells = [store.cell_positions(j) for j in range(store.n_cells)]
    ref = ar.audit(cells, T, R, plan=plan, cell_plan=cell_plan, rec=h, kind=kind)
    _assert_equal(_host(want), ref, what + " (NumPy restatement)")


def _plan_not_vacuous(want, n, T):
    w = _host(want)
    assert 0 < w["hit"].sum() < w["hit"].shape[0] * n * T
    assert (w["hit_any"] != w["hit"].max(1)).any()


def _rec_not_vacuous(want, n):
    ro = _host(want)["rec_open"]
    assert ((ro > 0) & (ro < n)).any()


# ---- horizons ----------------------------------------------------------------------------------
@pytest.mark.parametrize("T_src, T", [(2, 1), (3, 2), (8, 7), (9, 8), (12, 11), (40, 39),
                                      (12, 7)])
def test_horizons(gpu, T_src, T):
    n = 777
    fr = _frame(T_src, T, n)
    plan = torch.as_tensor(fr["plan"][:1].copy(), device=gpu)
    h = _records(fr, ar.HALFSPACE, T, shifted=True, edits=True)
    rec = _rec_dev(h, ar.HALFSPACE, gpu)
    new, oracle = _both(gpu, T_src, T, n, plan=plan, rec=rec, kind=ar.HALFSPACE)
    _check(new, oracle)
    _check_ref(oracle, T, fr["plan"][:1], None, h, ar.HALFSPACE)
    if T >= 2:
        _plan_not_vacuous(oracle[0], n, T)
    if T >= 3:
        _rec_not_vacuous(oracle[0], n)
        assert (_host(oracle[0])["rec_open"] == -1).any()


# ---- sample counts: one sample, ragged waves, a ragged last item, many items per cell ----------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 777, 4099, 70001])
def test_sample_counts(gpu, n):
    T_src, T = 8, 7
    fr = _frame(T_src, T, n)
    plan = torch.as_tensor(fr["plan"][:1].copy(), device=gpu)
    h = _records(fr, ar.AFFINE, T, shifted=True)
    rec = _rec_dev(h, ar.AFFINE, gpu)
    new, oracle = _both(gpu, T_src, T, n, plan=plan, rec=rec, kind=ar.AFFINE)
    _check(new, oracle)
    if n <= 4099:
        _check_ref(oracle, T, fr["plan"][:1], None, h, ar.AFFINE)
    if n >= 257:
        _plan_not_vacuous(oracle[0], n, T)
        _rec_not_vacuous(oracle[0], n)


def test_planner_sample_count(gpu):
    """2 cells x 1 000 000 at T = 7, the planner's n_ideal (the materialised store is 224 MB)."""
    T_src, T, n = 8, 7, 1_000_000
    fr = _frame(T_src, T, n, src=(0, 1))
    plan = torch.as_tensor(fr["plan"].copy(), device=gpu)
    h = _records(fr, ar.HALFSPACE, T)
    new, oracle = _both(gpu, T_src, T, n, plan=plan, cell_plan=[0, 1],
                        rec=_rec_dev(h, ar.HALFSPACE, gpu), kind=ar.HALFSPACE, src=(0, 1))
    _check(new, oracle)
    _plan_not_vacuous(oracle[0], n, T)


# ---- rollout arguments -------------------------------------------------------------------------
@pytest.mark.parametrize("x0", [False, True], ids=["x0_drawn", "x0_given"])
@pytest.mark.parametrize("src, rng_cell", [((1, 0, 1), None), (None, (5, 2, 9)),
                                           ((1, 0, 1), (5, 2, 9))],
                         ids=["src", "rng", "src_rng"])
def test_rollout_arguments(gpu, src, rng_cell, x0):
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T, n, src=src, x0=x0, rng_cell=rng_cell)
    plan = torch.as_tensor(fr["plan"][:1].copy(), device=gpu)
    h = _records(fr, ar.HALFSPACE, T, shifted=True)
    new, oracle = _both(gpu, T_src, T, n, plan=plan, rec=_rec_dev(h, ar.HALFSPACE, gpu),
                        kind=ar.HALFSPACE, src=src, x0=_x0(T_src, C, gpu) if x0 else None,
                        rng_cell=rng_cell)
    _check(new, oracle)
    _plan_not_vacuous(oracle[0], n, T)
    _rec_not_vacuous(oracle[0], n)
    if src is not None and rng_cell is None and not x0:
        # a repeated source with different streams: the same moments, different samples
        w = _host(oracle[0])
        assert not np.array_equal(w["hit"][0], w["hit"][2])


def test_sharding_invariance(gpu):
    """Three cells in one call == the same cells in two calls with the matching slices."""
    from ccmpc import engine
    T_src, T, n = 9, 8, 4099
    src, rng_cell = (1, 0, 1), (5, 2, 9)
    fr = _frame(T_src, T, n, src=src, rng_cell=rng_cell)
    pm, pc = _source(T_src)
    plan = torch.as_tensor(fr["plan"].copy(), device=gpu)
    h = _records(fr, ar.AFFINE, T, shifted=True, edits=True)
    rec = _rec_dev(h, ar.AFFINE, gpu)
    x0 = _x0(T_src, C, gpu)
    whole, st = engine.ideal_risk_audit(pm, pc, _i32(src, gpu), T, n, plan=plan, rec=rec,
                                        rec_kind=ar.AFFINE, R=R, cell_plan=[0, 1, 2], x0=x0,
                                        seed=SEED, rng_cell=_i32(rng_cell, gpu))
    parts = []
    for sl in (slice(0, 1), slice(1, 3)):
        nc = sl.stop - sl.start
        parts.append(engine.ideal_risk_audit(
            pm, pc, _i32(src[sl], gpu), T, n, plan=plan, rec=rec[sl].contiguous(),
            rec_kind=ar.AFFINE, R=R, cell_plan=list(range(sl.start, sl.stop)),
            x0=x0[sl].contiguous(), seed=SEED, rng_cell=_i32(rng_cell[sl], gpu)))
        assert parts[-1][1].shape == (nc,)
    torch.cuda.synchronize()
    w = _host(whole)
    joined = {k: np.concatenate([_host(p[0])[k] for p in parts]) for k in w}
    _assert_equal(joined, w)
    assert torch.cat([p[1] for p in parts]).cpu().tolist() == st.cpu().tolist() == [0, 0, 0]
    _plan_not_vacuous(whole, n, T)


# ---- halves, plan rows, record kinds -----------------------------------------------------------
@pytest.mark.parametrize("halves", ["plan", "rec", "both"])
def test_halves(gpu, halves):
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T, n)
    plan = torch.as_tensor(fr["plan"][:1].copy(), device=gpu) if halves != "rec" else None
    h = _records(fr, ar.HALFSPACE, T, shifted=True, edits=True) if halves != "plan" else None
    rec = _rec_dev(h, ar.HALFSPACE, gpu) if h is not None else None
    new, oracle = _both(gpu, T_src, T, n, plan=plan, rec=rec,
                        kind=ar.HALFSPACE if h is not None else None)
    _check(new, oracle)
    got = new[0]
    assert (got.hit is None) == (halves == "rec") and (got.min_d2 is None) == (halves == "rec")
    assert (got.rec_open is None) == (halves == "plan") and (got.open is None) == (halves == "plan")
    _check_ref(oracle, T, None if plan is None else fr["plan"][:1], None, h,
               ar.HALFSPACE if h is not None else None)


def test_two_plan_rows_with_cell_plan(gpu):
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T, n)
    rows = fr["plan"][[2, 0]].copy()                  # row 0: cell 2's path, row 1: cell 0's
    cell_plan = [1, 1, 0]
    plan = torch.as_tensor(rows, device=gpu)
    for cp in (cell_plan, _i32(cell_plan, gpu)):      # host sequence and device tensor
        new, oracle = _both(gpu, T_src, T, n, plan=plan, cell_plan=cp)
        _check(new, oracle)
    _check_ref(oracle, T, rows, cell_plan, None, None)
    _plan_not_vacuous(oracle[0], n, T)
    w = _host(oracle[0])
    assert w["hit_any"][0] > 0 and w["hit_any"][2] > 0      # each against its own path


@pytest.mark.parametrize("shifted", [False, True], ids=["own", "shifted"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["halfspace", "affine", "halfspace_compact",
                                                    "affine_compact"])
def test_record_kinds(gpu, kind, shifted):
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T, n)
    h = _records(fr, kind & 1, T, shifted=shifted, edits=True)
    rec = _rec_dev(h, kind, gpu)
    plan = torch.as_tensor(fr["plan"][:1].copy(), device=gpu)
    new, oracle = _both(gpu, T_src, T, n, plan=plan, rec=rec, kind=kind)
    _check(new, oracle)
    h_ref = ar.compact(h, kind & 1) if kind >= ar.HALFSPACE_COMPACT else h
    _check_ref(oracle, T, fr["plan"][:1], None, h_ref, kind)
    w = _host(oracle[0])
    assert (w["rec_open"] == -1).sum() >= C + 2            # the edited rows: status, then t
    if shifted:
        _rec_not_vacuous(oracle[0], n)


# ---- a failed cell: a status code, not a device fault ------------------------------------------
def test_failed_cell(gpu):
    """tests/test_gpu_selftest.py::test_not_pd_conditional_covariance_in_predict_ideal's
    construction on cell 1: its step-2 conditional covariance is not positive definite.  Its
    slots are NaN from that step on: hit by nothing, protected by nothing."""
    from ccmpc import _lib
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T, n)
    _, pc = _source(T_src)
    bad = pc.clone()
    c = bad[1]
    c[4:6, 2:4] = 2.0 * torch.linalg.cholesky(c[4:6, 4:6]) @ torch.linalg.cholesky(c[2:4, 2:4]).T
    c[2:4, 4:6] = c[4:6, 2:4].T
    plan = torch.as_tensor(fr["plan"].copy(), device=gpu)
    h = _records(fr, ar.AFFINE, T, shifted=True)
    rec = _rec_dev(h, ar.AFFINE, gpu)
    new, oracle = _both(gpu, T_src, T, n, plan=plan, cell_plan=[0, 1, 2], rec=rec,
                        kind=ar.AFFINE, pc=bad)
    _check(new, oracle)
    assert new[1].cpu().tolist() == [0, _lib.REC_NOT_PD, 0]
    g = _host(new[0])
    assert g["hit"][1, 1:].tolist() == [0] * (T - 1) and np.isinf(g["min_d2"][1, 1:]).all()
    assert g["open"][1, 1:].tolist() == [n] * (T - 1)
    assert g["rec_open"][1, 1:].tolist() == [n] * (T - 1)
    assert np.isfinite(g["min_d2"][1, 0]) and g["open"][1, 0] < n      # the step before it
    # the other cells are those of the good covariance
    good, _ = _both(gpu, T_src, T, n, plan=plan, cell_plan=[0, 1, 2], rec=rec, kind=ar.AFFINE)
    gg = _host(good[0])
    for k in g:
        assert np.array_equal(g[k][[0, 2]].view(np.int64), gg[k][[0, 2]].view(np.int64)), k


# ---- reproducibility ---------------------------------------------------------------------------
def _filled(like, status, fill):
    from ccmpc import engine
    out = engine.RiskAudit(*[torch.full_like(t, float("nan") if t.is_floating_point() and
                                             fill != 0 else fill) for t in like])
    return out, torch.full_like(status, fill)


def test_prefilled_outputs_and_repeated_call(gpu):
    T_src, T, n = 9, 8, 4099
    fr = _frame(T_src, T, n)
    plan = torch.as_tensor(fr["plan"][:1].copy(), device=gpu)
    rec = _rec_dev(_records(fr, ar.HALFSPACE, T, shifted=True, edits=True), ar.HALFSPACE, gpu)
    new, oracle = _both(gpu, T_src, T, n, plan=plan, rec=rec, kind=ar.HALFSPACE)
    _check(new, oracle)
    for fill in (-7, 0):
        out = _filled(new[0], new[1], fill)
        again, _ = _both(gpu, T_src, T, n, plan=plan, rec=rec, kind=ar.HALFSPACE, out=out)
        assert all(a is b for a, b in zip(again[0], out[0])) and again[1] is out[1]
        _check(again, oracle, f"prefilled with {fill}")
        again, _ = _both(gpu, T_src, T, n, plan=plan, rec=rec, kind=ar.HALFSPACE, out=out)
        _check(again, oracle, "repeated")
    # a bare RiskAudit: the status is not written and nothing is allocated for it
    bare, _ = _both(gpu, T_src, T, n, plan=plan, rec=rec, kind=ar.HALFSPACE, out=out[0])
    assert bare[1] is None
    _assert_equal(bare[0], oracle[0])


def test_captured_graph_follows_seed_and_plan(gpu):
    """A captured call replayed after seed_dev and the plan were overwritten in place gives the
    bits of fresh calls with those values."""
    from ccmpc import engine
    T_src, T, n = 9, 8, 4099
    fr = _frame(T_src, T, n)
    pm, pc = _source(T_src)
    src = _i32(range(C), gpu)
    planA = fr["plan"][:1].copy()
    planB = fr["plan"][1:2].copy() + [0.5, -0.25]
    seedA, seedB = SEED, 2**40 + 12345
    rec = _rec_dev(_records(fr, ar.HALFSPACE, T, shifted=True), ar.HALFSPACE, gpu)
    tp = torch.as_tensor(planA.copy(), device=gpu)
    sd = torch.tensor([seedA], dtype=torch.int64, device=gpu)
    out = engine.ideal_risk_audit(pm, pc, src, T, n, plan=tp, rec=rec, rec_kind=ar.HALFSPACE,
                                  R=R, seed=999, seed_dev=sd)           # warm-up, allocates
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        again = engine.ideal_risk_audit(pm, pc, src, T, n, plan=tp, rec=rec,
                                        rec_kind=ar.HALFSPACE, R=R, seed=999, seed_dev=sd,
                                        out=out)
    assert all(a is b for a, b in zip(again[0], out[0])) and again[1] is out[1]
    fresh = {}
    for name, (pl, sv) in dict(A=(planA, seedA), B=(planB, seedB)).items():
        new, oracle = _both(gpu, T_src, T, n, plan=torch.as_tensor(pl.copy(), device=gpu),
                            rec=rec, kind=ar.HALFSPACE, seed=sv)
        _check(new, oracle, name)
        fresh[name] = _host(new[0])
    assert not np.array_equal(fresh["A"]["hit"], fresh["B"]["hit"])
    for t in list(out[0]) + [out[1]]:
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(out[0], fresh["A"], "replay A")
    tp.copy_(torch.from_numpy(planB).to(gpu))
    sd.fill_(seedB)
    graph.replay()
    torch.cuda.synchronize()
    _assert_equal(out[0], fresh["B"], "replay B")
    assert out[1].cpu().tolist() == [0] * C
