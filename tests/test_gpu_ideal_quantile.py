"""GPU tests of the Monte-Carlo calibration on the ideal rollout's samples
(ccmpc_ideal_risk_quantile behind engine.ideal_risk_quantile).

The oracle is the contract's own sentence: engine.ideal_rollout (Philox) followed by
engine.risk_quantile on its store, device against device.  q and rhs are compared as int64 bit
patterns and the statuses exactly; there is no tolerance anywhere.  Up to 4099 samples
tests/_quantile_ref.quantile on the rollout read back to the host is compared too, so the tests
do not rest on ccmpc_risk_quantile alone.

Source moments, frames and records are built as tests/test_gpu_ideal_audit.py builds them (the
helpers are copied): 3 cells x 500 particles of a random walk with independent increments, the
cycle's own half-space records and the affine records of the ideal moments, and the "shifted"
sets whose offsets put the predicate's boundary through the centre of the cloud."""
import functools

import numpy as np
import pytest
import torch

import _audit_ref as ar
import _quantile_ref as qr

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


def _x0(T_src, nc, gpu):
    pm, _ = _source(T_src)
    m0 = pm[:, 0, :].cpu().numpy()
    return torch.as_tensor((m0[np.arange(nc) % C] + [0.25, -0.5]).copy(), device=gpu)


@functools.lru_cache(maxsize=None)
def _frame(T_src, T, src=None, x0=False, rng_cell=None, seed=SEED):
    """What a frame at these rollout arguments holds, computed once: the cycle's mean path, its
    own half-space records and the affine records of the ideal moments -- all on the host."""
    from ccmpc import engine, risk
    gpu = torch.device("cuda:0")
    pm, pc = _source(T_src)
    nc = len(src) if src is not None else C
    s = _i32(src if src is not None else range(C), gpu)
    x0_t = _x0(T_src, nc, gpu) if x0 else None
    n_cyc = 777
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
    return dict(mean=mean.cpu().numpy(),
                half=engine.halfspaces(rec)[:, :T * (T - 1) // 2].copy(),
                aff=engine.affine_records(aff).copy())


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


def _both(gpu, T_src, T, n, rec, kind, allow=None, src=None, x0=None, rng_cell=None, seed=SEED,
          pc=None, out=None, seed_dev=None):
    """(new call's (RiskQuantile, cell_status), oracle's (RiskQuantile, status, store))."""
    from ccmpc import engine
    pm, pc0 = _source(T_src)
    pc = pc0 if pc is None else pc
    s = _i32(src if src is not None else range(C), gpu)
    r = _i32(rng_cell, gpu)
    store, wst = engine.ideal_rollout(pm, pc, s, T, n, x0=x0, seed=seed, rng_cell=r)
    assert store.counts == [n] * len(s)
    want = engine.risk_quantile(store, rec, kind, allow=allow, R=R, T=T)
    got, gst = engine.ideal_risk_quantile(pm, pc, s, T, n, rec, kind, allow=allow, R=R, x0=x0,
                                          seed=seed, seed_dev=seed_dev, rng_cell=r, out=out)
    torch.cuda.synchronize()
    return (got, gst), (want, wst, store)


def _host(a):
    if isinstance(a, dict):
        return a
    return dict(q=a.q.cpu().numpy(), rhs=a.rhs.cpu().numpy(), status=a.status.cpu().numpy())


def _assert_equal(got, want, what="", rows=None):
    """Statuses exactly, q and rhs bit for bit; rows: a boolean [C, P] mask of what to compare."""
    g, w = _host(got), _host(want)
    for name in ("status", "q", "rhs"):
        a, b = g[name], w[name]
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert a.dtype == (np.int32 if name == "status" else np.float64), (what, name)
        if name != "status":
            a, b = a.view(np.int64), b.view(np.int64)
        bad = a != b
        if rows is not None:
            bad &= rows
        assert not bad.any(), (what, name, np.argwhere(bad)[:5], g[name][bad][:5],
                               w[name][bad][:5])


def _check(new, oracle, what=""):
    (got, gst), (want, wst, _) = new, oracle
    _assert_equal(got, want, what)
    assert gst.dtype == torch.int32 and gst.cpu().tolist() == wst.cpu().tolist(), what


def _ref(oracle, T, h, kind, allow):
    """The NumPy restatement on the rollout read back; compared with the oracle's output."""
    want, _, store = oracle
    cells = [store.cell_positions(j) for j in range(store.n_cells)]
    ref = qr.quantile(cells, T, R, h, kind, allow)
    w = _host(want)
    assert np.array_equal(w["status"], ref["status"])
    assert np.array_equal(w["q"], ref["q"], equal_nan=True)
    assert np.array_equal(w["rhs"].view(np.int64), ref["rhs"].view(np.int64))
    return ref


def _statuses(a):
    return set(np.unique(_host(a)["status"]).tolist())


# ---- sample counts: one sample, ragged waves, a ragged last item, two trips per item ------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4099, 100_003])
def test_sample_counts(gpu, n):
    T_src, T = 8, 7
    fr = _frame(T_src, T)
    allow = [n // 2, 0, 1]
    for kind, shifted in ((ar.HALFSPACE, False), (ar.AFFINE, True)):
        h = _records(fr, kind, T, shifted=shifted)
        new, oracle = _both(gpu, T_src, T, n, _rec_dev(h, kind, gpu), kind, allow=allow)
        _check(new, oracle, kind)
        if n <= 4099:
            _ref(oracle, T, h, kind, allow)
        want = _host(oracle[0])
        assert (want["status"][:2] == 0).any()
        if n == 1:                                   # allow[2] = 1 >= N
            assert np.all(want["status"][2] == qr.CAL_VACUOUS)
    if n == 100_003:
        from ccmpc import _lib
        # the workspace the fused call needs instead of the 16 T n bytes per cell of the store
        need = _lib.load().ccmpc_ideal_risk_quantile_workspace_bytes(T, kind, C)
        assert 0 < need < 16 * T * n * C


# ---- horizons and record kinds -------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["halfspace", "affine", "halfspace_compact",
                                                    "affine_compact"])
@pytest.mark.parametrize("T_src, T", [(2, 1), (3, 2), (8, 7), (13, 12), (40, 39)])
def test_horizons_and_kinds(gpu, T_src, T, kind):
    n = 257 if T == 39 else 777
    fr = _frame(T_src, T)
    h = _records(fr, kind & 1, T, shifted=bool(T & 1), edits=True)
    allow = [3, n // 2, 0]
    new, oracle = _both(gpu, T_src, T, n, _rec_dev(h, kind, gpu), kind, allow=allow)
    _check(new, oracle)
    P = ar.rows(kind, T)
    assert tuple(new[0].q.shape) == (C, P)
    if P == 0:
        assert new[1].cpu().tolist() == [0] * C        # only the status is written
        return
    h_ref = ar.compact(h, kind & 1) if kind >= ar.HALFSPACE_COMPACT else h
    ref = _ref(oracle, T, h_ref, kind, allow)
    assert (ref["status"] == 0).any()
    if P >= 3:
        assert (ref["status"] == qr.CAL_SKIPPED).sum() >= C + 2    # the edited rows
    if T == 39 and not kind & 1:
        assert P == 741                                 # 24 record chunks


# ---- allow ---------------------------------------------------------------------------------------
def test_allow_options(gpu):
    T_src, T, n = 8, 7, 4099
    fr = _frame(T_src, T)
    kind = ar.HALFSPACE
    h = _records(fr, kind, T, shifted=True)
    rec = _rec_dev(h, kind, gpu)
    seen = set()
    for allow in ([0, 1, n // 2], [n - 1, n, n + 5]):
        for a in (allow, torch.tensor(allow, dtype=torch.int64, device=gpu)):
            new, oracle = _both(gpu, T_src, T, n, rec, kind, allow=a)
            _check(new, oracle, allow)
        _ref(oracle, T, h, kind, allow)
        seen |= _statuses(new[0])
    allow = [-1, n // 2, n]                          # a negative count: found on the device
    new, oracle = _both(gpu, T_src, T, n, rec, kind,
                        allow=torch.tensor(allow, dtype=torch.int64, device=gpu))
    _check(new, oracle, allow)
    _ref(oracle, T, h, kind, allow)
    g = _host(new[0])
    assert np.all(g["status"][0] == qr.CAL_SKIPPED) and np.all(g["status"][1] == 0)
    assert np.all(g["status"][2] == qr.CAL_VACUOUS)
    assert seen | _statuses(new[0]) == {0, qr.CAL_VACUOUS, qr.CAL_SKIPPED}
    none, oracle = _both(gpu, T_src, T, n, rec, kind)            # allow = None: zeros
    _check(none, oracle, "allow None")
    with pytest.raises(ValueError):
        from ccmpc import engine
        pm, pc = _source(T_src)
        engine.ideal_risk_quantile(pm, pc, _i32(range(C), gpu), T, n, rec, kind, allow=[0, -1, 0])


# ---- edited records and non-finite normals --------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["halfspace", "affine", "halfspace_compact",
                                                    "affine_compact"])
def test_edited_records_and_non_finite_normals(gpu, kind):
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T)
    h = _records(fr, kind & 1, T, shifted=True, edits=True)
    h["n0"][0, 0] = np.nan
    h["n1"][1, 2] = np.inf
    h["n0"][2, 3], h["n1"][2, 3] = -np.inf, np.nan
    allow = [5, 0, n // 3]
    new, oracle = _both(gpu, T_src, T, n, _rec_dev(h, kind, gpu), kind, allow=allow)
    _check(new, oracle)
    h_ref = ar.compact(h, kind & 1) if kind >= ar.HALFSPACE_COMPACT else h
    ref = _ref(oracle, T, h_ref, kind, allow)
    g = _host(new[0])
    for c, p in ((0, 0), (1, 2), (2, 3), (0, 1), (1, 1)):
        assert g["status"][c, p] == qr.CAL_SKIPPED and np.isnan(g["q"][c, p])
    own = ar.rec_fields(h_ref, kind)[2]
    skipped = ref["status"] == qr.CAL_SKIPPED
    assert np.array_equal(g["rhs"].view(np.int64)[skipped], own.view(np.int64)[skipped])


# ---- ties ----------------------------------------------------------------------------------------
def test_all_samples_tied_at_plus_zero(gpu):
    """n = (0, 0) with side -1: every s is +0, side*s is -0, w is +0 -- 4099 equal keys, more
    than any candidate list holds, so the selection runs all eight digits."""
    T_src, T, n = 8, 7, 4099
    fr = _frame(T_src, T)
    kind = ar.AFFINE
    h = _records(fr, kind, T)
    h["n0"], h["n1"], h["side"] = 0.0, 0.0, -1
    allow = [0, n // 2, n - 1]
    new, oracle = _both(gpu, T_src, T, n, _rec_dev(h, kind, gpu), kind, allow=allow)
    _check(new, oracle)
    ref = _ref(oracle, T, h, kind, allow)
    g = _host(new[0])
    assert np.all(g["status"] == 0) and np.all(g["q"].view(np.int64) == 0)
    assert np.all(ref["n_ge"] == n) and np.all(ref["n_gt"] == 0)


@pytest.mark.parametrize("n", [257, 4099])
def test_rank_inside_a_tie_group(gpu, n):
    """n = (k 5e-324, 0): s is a small multiple of the smallest subnormal, so the samples fall
    into a handful of tie groups of hundreds (at 257 samples every record is inside a candidate
    list from the first pass on)."""
    T_src, T = 8, 7
    fr = _frame(T_src, T)
    kind = ar.AFFINE
    h = _records(fr, kind, T)
    k = np.array([1, 2, 3])[:, None] * np.ones((1, T), np.int64)
    h["n0"], h["n1"] = k * 5e-324, 0.0
    allow = [n // 2, n // 3, n // 5]
    new, oracle = _both(gpu, T_src, T, n, _rec_dev(h, kind, gpu), kind, allow=allow)
    _check(new, oracle)
    ref = _ref(oracle, T, h, kind, allow)
    assert np.all(ref["status"] == 0)
    width = ref["n_ge"] - ref["n_gt"]
    inside = (width > 1) & (ref["n_gt"] < np.array(allow)[:, None])
    assert inside.sum() >= 4, (width, ref["n_gt"])      # the rank falls inside a tie group
    assert width.max() >= 100 if n == 4099 else width.max() >= 10


# ---- failed cells --------------------------------------------------------------------------------
def test_failed_step(gpu):
    """Cell 1's covariance block of step 3's samples is zero: steps 3 (no Cholesky factor of its
    conditional covariance) and 4 (a singular source block) cannot be built, so f(1) = 3.
    Records of steps 0..2 are the oracle's, records from step 3 on are SKIPPED with their own
    rhs, and the cell status is the rollout's."""
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T)
    _, pc = _source(T_src)
    bad = pc.clone()
    bad[1, 8:10, 8:10] = 0.0
    allow = [7, 7, 7]
    for kind in (ar.HALFSPACE, ar.AFFINE):
        h = _records(fr, kind, T, shifted=True)
        new, oracle = _both(gpu, T_src, T, n, _rec_dev(h, kind, gpu), kind, allow=allow, pc=bad)
        st = new[1].cpu().tolist()
        assert st == oracle[1].cpu().tolist() and st[0] == 0 and st[1] < 0 and st[2] == 0
        t = ar.rec_fields(h, kind)[5]
        before = np.ones(t.shape, bool)
        before[1] = t[1] < 3
        assert before[1].any() and (~before[1]).any()
        _assert_equal(new[0], oracle[0], kind, rows=before)
        g = _host(new[0])
        assert np.all(g["status"][before] == 0) and np.all(np.isfinite(g["q"][before]))
        assert np.all(g["status"][~before] == qr.CAL_SKIPPED) and np.all(np.isnan(g["q"][~before]))
        own = ar.rec_fields(h, kind)[2]
        assert np.array_equal(g["rhs"].view(np.int64)[~before], own.view(np.int64)[~before])
        # the host restatement on the finite steps of the rollout read back
        cells = [oracle[2].cell_positions(j) for j in range(C)]
        assert np.isfinite(cells[1][:, :3]).all() and np.isnan(cells[1][:, 3:]).all()
        ref = qr.quantile([np.nan_to_num(x) for x in cells], T, R, h, kind, allow)
        _assert_equal(g, dict(q=ref["q"], rhs=ref["rhs"], status=ref["status"]), kind,
                      rows=before)


def test_failed_initial_draw(gpu):
    """Cell 1's cov_0 is not positive definite: without x0 the draw fails, f(1) = 0 and every
    record of the cell is SKIPPED; with x0 given nothing is drawn and the cell is calibrated."""
    from ccmpc import _lib
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T)
    _, pc = _source(T_src)
    bad = pc.clone()
    bad[1, 0:2, 0:2] = -torch.eye(2, dtype=pc.dtype, device=pc.device)
    kind = ar.HALFSPACE
    h = _records(fr, kind, T, shifted=True)
    rec = _rec_dev(h, kind, gpu)
    allow = [7, 7, 7]
    new, oracle = _both(gpu, T_src, T, n, rec, kind, allow=allow, pc=bad)
    assert new[1].cpu().tolist() == oracle[1].cpu().tolist() == [0, _lib.REC_NOT_PD, 0]
    others = np.ones((C, h.shape[1]), bool)
    others[1] = False
    _assert_equal(new[0], oracle[0], rows=others)
    g = _host(new[0])
    assert np.all(g["status"][1] == qr.CAL_SKIPPED) and np.all(np.isnan(g["q"][1]))
    assert np.array_equal(g["rhs"][1].view(np.int64), h["d"][1].view(np.int64))
    assert np.all(g["status"][others] == 0)
    given, oracle = _both(gpu, T_src, T, n, rec, kind, allow=allow, pc=bad,
                          x0=_x0(T_src, C, gpu))
    _check(given, oracle, "x0 given")
    assert given[1].cpu().tolist() == [0] * C and np.all(_host(given[0])["status"] == 0)
    _ref(oracle, T, h, kind, allow)


# ---- rollout arguments ---------------------------------------------------------------------------
@pytest.mark.parametrize("x0", [False, True], ids=["x0_drawn", "x0_given"])
@pytest.mark.parametrize("src, rng_cell", [((1, 0, 1), None), (None, (5, 2, 9)),
                                           ((1, 0, 1), (5, 2, 9))],
                         ids=["src", "rng", "src_rng"])
def test_rollout_arguments(gpu, src, rng_cell, x0):
    T_src, T, n = 9, 8, 777
    fr = _frame(T_src, T, src=src, x0=x0, rng_cell=rng_cell)
    kind = ar.HALFSPACE
    h = _records(fr, kind, T, shifted=True)
    allow = [n // 4, 2, 0]
    new, oracle = _both(gpu, T_src, T, n, _rec_dev(h, kind, gpu), kind, allow=allow, src=src,
                        x0=_x0(T_src, C, gpu) if x0 else None, rng_cell=rng_cell)
    _check(new, oracle)
    _ref(oracle, T, h, kind, allow)
    assert np.all(_host(new[0])["status"] == 0)


def test_sharding_invariance(gpu):
    """Three cells in one call == three one-cell calls with the matching slices."""
    from ccmpc import engine
    T_src, T, n = 9, 8, 4099
    src, rng_cell = (1, 0, 1), (5, 2, 9)
    fr = _frame(T_src, T, src=src, rng_cell=rng_cell)
    pm, pc = _source(T_src)
    kind = ar.AFFINE
    h = _records(fr, kind, T, shifted=True, edits=True)
    rec = _rec_dev(h, kind, gpu)
    x0 = _x0(T_src, C, gpu)
    allow = torch.tensor([n // 2, 3, 0], dtype=torch.int64, device=gpu)
    whole, oracle = _both(gpu, T_src, T, n, rec, kind, allow=allow, src=src, x0=x0,
                          rng_cell=rng_cell)
    _check(whole, oracle)
    parts = [engine.ideal_risk_quantile(
        pm, pc, _i32(src[c:c + 1], gpu), T, n, rec[c:c + 1].contiguous(), kind,
        allow=allow[c:c + 1].contiguous(), R=R, x0=x0[c:c + 1].contiguous(), seed=SEED,
        rng_cell=_i32(rng_cell[c:c + 1], gpu)) for c in range(C)]
    torch.cuda.synchronize()
    joined = {k: np.concatenate([_host(p[0])[k] for p in parts]) for k in ("q", "rhs", "status")}
    _assert_equal(joined, whole[0])
    assert torch.cat([p[1] for p in parts]).cpu().tolist() == whole[1].cpu().tolist()
    assert (joined["status"] == 0).sum() > joined["status"].size // 2


# ---- initialisation, reuse, capture ---------------------------------------------------------------
def test_prefilled_workspace_and_repeated_call(gpu):
    from ccmpc import engine
    T_src, T, n = 9, 8, 4099
    fr = _frame(T_src, T)
    kind = ar.HALFSPACE
    rec = _rec_dev(_records(fr, kind, T, shifted=True, edits=True), kind, gpu)
    allow = [n // 2, 1, n + 5]
    new, oracle = _both(gpu, T_src, T, n, rec, kind, allow=allow)
    _check(new, oracle)
    assert _statuses(new[0]) == {0, qr.CAL_VACUOUS, qr.CAL_SKIPPED}
    out = (engine.RiskQuantile(*[torch.empty_like(t) for t in new[0]]), torch.empty_like(new[1]))
    for t in list(out[0]) + [out[1]]:
        t.view(torch.uint8).fill_(0xFF)
    again, _ = _both(gpu, T_src, T, n, rec, kind, allow=allow, out=out)
    assert all(a is b for a, b in zip(again[0], out[0])) and again[1] is out[1]
    _check(again, oracle, "prefilled with 0xFF")
    out[0].q.fill_(7.0)
    again, _ = _both(gpu, T_src, T, n, rec, kind, allow=allow, out=out)     # the used workspace
    _check(again, oracle, "repeated")
    bare, _ = _both(gpu, T_src, T, n, rec, kind, allow=allow, out=out[0])
    assert bare[1] is None
    _assert_equal(bare[0], oracle[0])


def test_captured_graph_follows_seed(gpu):
    """One captured call, replayed after seed_dev was overwritten in place, gives the bits of
    eager calls with those seeds."""
    from ccmpc import engine
    T_src, T, n = 9, 8, 4099
    fr = _frame(T_src, T)
    pm, pc = _source(T_src)
    src = _i32(range(C), gpu)
    kind = ar.HALFSPACE
    rec = _rec_dev(_records(fr, kind, T, shifted=True), kind, gpu)
    allow = torch.tensor([n // 2, 6, 0], dtype=torch.int64, device=gpu)
    seedA, seedB = SEED, 2**40 + 12345
    sd = torch.tensor([seedA], dtype=torch.int64, device=gpu)
    out = engine.ideal_risk_quantile(pm, pc, src, T, n, rec, kind, allow=allow, R=R, seed=999,
                                     seed_dev=sd)                       # warm-up, allocates
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        again = engine.ideal_risk_quantile(pm, pc, src, T, n, rec, kind, allow=allow, R=R,
                                           seed=999, seed_dev=sd, out=out)
    assert all(a is b for a, b in zip(again[0], out[0])) and again[1] is out[1]
    fresh = {}
    for name, sv in dict(A=seedA, B=seedB).items():
        new, oracle = _both(gpu, T_src, T, n, rec, kind, allow=allow, seed=sv)
        _check(new, oracle, name)
        fresh[name] = _host(new[0])
    assert not np.array_equal(fresh["A"]["q"], fresh["B"]["q"])
    for name, sv in dict(A=seedA, B=seedB).items():
        for t in list(out[0]) + [out[1]]:
            t.view(torch.uint8).fill_(0xFF)
        sd.fill_(sv)
        graph.replay()
        torch.cuda.synchronize()
        _assert_equal(out[0], fresh[name], "replay " + name)
        assert out[1].cpu().tolist() == [0] * C


# ---- the round trip with the audit on the same samples ---------------------------------------------
@pytest.mark.parametrize("kind", [ar.HALFSPACE, ar.AFFINE], ids=["halfspace", "affine"])
def test_round_trip_with_the_ideal_audit(gpu, kind):
    """Records carrying the calibrated offsets, audited on the same samples, leave at most
    allow[c] of them open: exactly the samples strictly beyond q wherever the host restatement
    shows that no sample lies within the rounding of u*."""
    from ccmpc import engine
    T_src, T, n = 9, 8, 4099
    fr = _frame(T_src, T)
    pm, pc = _source(T_src)
    src = _i32(range(C), gpu)
    h = _records(fr, kind, T)
    rec = _rec_dev(h, kind, gpu)
    allow = np.array([n // 2, 6, 0])
    new, oracle = _both(gpu, T_src, T, n, rec, kind, allow=allow.tolist())
    _check(new, oracle)
    ref = _ref(oracle, T, h, kind, allow)
    cal = ref["status"] == 0
    assert cal.sum() > cal.size // 2
    replaced = engine.calibrated_records(rec, kind, new[0], "replace")
    a, _ = engine.ideal_risk_audit(pm, pc, src, T, n, rec=replaced, rec_kind=kind, R=R, seed=SEED)
    torch.cuda.synchronize()
    ro = a.rec_open.cpu().numpy()
    assert np.all(ro[cal] <= np.broadcast_to(allow[:, None], ro.shape)[cal])
    # the host's own count of the samples the calibrated record leaves open
    n0, n1, _, side, _, t = ar.rec_fields(h, kind)
    cells = [oracle[2].cell_positions(j) for j in range(C)]
    host_open = np.full(ro.shape, -1, np.int64)
    for c, p in np.argwhere(cal):
        x = cells[c][:, t[c, p]]
        host_open[c, p] = int((~ar.protects(n0[c, p], n1[c, p], ref["rhs"][c, p], side[c, p],
                                            x[:, 0], x[:, 1], R)).sum())
    assert np.array_equal(ro[cal], host_open[cal])
    clear = cal & (host_open == ref["n_gt"])
    assert clear.sum() > cal.sum() // 2
    assert np.array_equal(ro[clear], ref["n_gt"][clear])
    assert ((ro[0] > 0) & (ro[0] < n)).any()                  # allow = n // 2: not vacuous
