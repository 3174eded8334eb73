"""The predict_ideal kernels (cc-mpc_amd/csrc/rollout.hip: ccmpc_ideal_rollout,
ccmpc_ideal_moments, ccmpc_ideal_minkowski_cycle) against the exact reference of
tests/_rollout_ref.py: step plans read out bit for bit, whole trajectories, fused moments,
every status by an exact margin, the x0 draw, sharding by rng_cell, and what a failed cell
leaves behind.

Allowances: _tail_ref.bound(e_oracle) = max(8 e_oracle, 1e-12) with e_oracle the float64
oracle's own worst error on the same inputs by the same measure (tests/_rollout_ref.py); the
kernel's error never enters its own allowance.  Every figure is printed before it is judged
(run with -s); profiles/r13/README.md holds a run's figures.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ccmpc_oracle as orc

import _rollout_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77                 # pad slots of the position store must keep it


def _dev(a, dt=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dt, device="cuda")      # (a writable copy)


def _i32(a):
    return None if a is None else _dev(np.asarray(a, np.int32), torch.int32)


def _rollout(mean, cov, src, T, n, x0=None, Z=None, seed=0, rng_cell=None):
    """ccmpc_ideal_rollout on a store pre-filled with SENTINEL, eight spare columns behind the
    last cell.  Returns X (C, n, T, 2), status (C,), and whether every pad slot (between cells
    and behind the last) still holds the sentinel."""
    from ccmpc import _lib, engine
    mean, cov = np.asarray(mean), np.asarray(cov)
    Cn, T_src, stride = len(src), mean.shape[1], (n + 3) // 4 * 4
    assert cov.shape == (mean.shape[0], 2 * T_src, 2 * T_src) and max(src) < mean.shape[0]
    assert 1 <= T <= T_src - 1
    assert x0 is None or np.shape(x0) == (Cn, 2)
    assert Z is None or np.shape(Z) == (Cn, T, 2, n)
    assert rng_cell is None or len(rng_cell) == Cn
    ld = Cn * stride + 8
    pos = torch.full((2 * T, ld), SENTINEL, dtype=torch.float64, device="cuda")
    status = torch.full((Cn,), 99, dtype=torch.int32, device="cuda")
    args = [_dev(mean), _dev(cov), _i32(src), None if x0 is None else _dev(x0),
            None if Z is None else _dev(Z), _i32(rng_cell)]
    _lib.check(_lib.load().ccmpc_ideal_rollout(
        engine._p(args[0]), engine._p(args[1]), T_src, engine._p(args[2]), Cn, T, n,
        engine._p(args[3]), engine._p(args[4]), int(seed), engine._p(args[5]), engine._p(pos), ld,
        engine._p(status), engine._stream()), "ccmpc_ideal_rollout")
    raw = pos.cpu().numpy()
    cells = raw[:, :Cn * stride].reshape(2 * T, Cn, stride)
    X = cells[:, :, :n].reshape(T, 2, Cn, n).transpose(2, 3, 0, 1).copy()
    pads_kept = bool(np.all(cells[:, :, n:] == SENTINEL) and np.all(raw[:, Cn * stride:] == SENTINEL))
    return X, status.cpu().numpy(), pads_kept


def _refs_and_risk(T, Cn):
    from ccmpc import risk
    ref_traj = _dev((np.array([170.0, 5.0]) + np.arange(1, T + 1)[:, None] * [4.0, 0.5])[None])
    return ref_traj, _dev(risk.cell_risk(risk.eps_ura([Cn]), [Cn], T + 1))


def _moments(mean, cov, src, T, n, x0=None, seed=0, rng_cell=None):
    from ccmpc import engine
    m, c, st = engine.ideal_moments(_dev(mean), _dev(cov), _i32(src), T, n,
                                    x0=None if x0 is None else _dev(x0), seed=seed,
                                    rng_cell=_i32(rng_cell))
    return m.cpu().numpy(), c.cpu().numpy(), st.cpu().numpy()


def _cycle(mean, cov, src, T, n, x0=None, seed=0, rng_cell=None):
    from ccmpc import engine
    rt, cr = _refs_and_risk(T, len(src))
    m, c, st, rec, pl = engine.ideal_minkowski_cycle(
        _dev(mean), _dev(cov), _i32(src), T, n, rt, cr, x0=None if x0 is None else _dev(x0),
        seed=seed, rng_cell=_i32(rng_cell))
    return m.cpu().numpy(), c.cpu().numpy(), st.cpu().numpy(), engine.halfspaces(rec), \
        pl.cpu().numpy()


# ---- a. plan read-out ---------------------------------------------------------------------------
@pytest.mark.parametrize("kappa,q,asym", [(k, q, False) for k, q in ref.GRID]
                         + [(1.0, q, True) for q in ref.QS])
def test_step_plans_read_out_bit_for_bit(gpu, kappa, q, asym):
    """Every step plan of a family (624) as its own source cell, T_src = 2, T = 1, zero means,
    x0 in {0, e1, e2} and three injected samples Z in {0, e1, e2} (n = 3: a ragged 4-particle
    stride with injected Z): the outputs are the entries of A_t and L_t themselves.  One launch
    of 1872 cells; status 0 on every instance (the zero cap of the host test, on the device).
    asym: Sigma_{t+1}'s upper off-diagonal entry is offset and must be ignored."""
    r = ref.plan_reference(kappa, q, asym)
    inp = ref.readout_inputs(kappa, q, asym)
    X, status, pads = _rollout(inp["mean"], inp["cov"], inp["src"], 1, 3, x0=inp["x0"], Z=inp["Z"])
    A, L = ref.readout_plan(X)
    eA, eL = ref.plan_errors(A, L, r)
    print(f"\nplans kappa={kappa:g} q={q:g} asym={asym}: oracle e_A={r['e_A']:.2e} "
          f"e_L={r['e_L']:.2e}  kernel e_A={eA.max():.2e} e_L={eL.max():.2e}  ratio "
          f"{eA.max() / r['e_A']:.2f} {eL.max() / r['e_L']:.2f}  bad status "
          f"{int(np.count_nonzero(status))}")
    assert r["oracle_fail"] == [] and np.all(r["lam"] > 0)
    assert np.all(status == 0)
    assert pads
    np.testing.assert_array_equal(X[0::3, 0], 0.0)                  # x0 = 0, z = 0: nothing
    assert eA.max() <= ref.bound(r["e_A"])
    assert eL.max() <= ref.bound(r["e_L"])
    # the model of build_step is the kernel, bit for bit (IEEE division and square root, no
    # contraction): a difference here is a change of the formulas, not of their accuracy
    mA, mL = ref.kernel_plan_f64(*ref.plan_instances(kappa, q, asym))
    np.testing.assert_array_equal(A, mA)
    np.testing.assert_array_equal(L, mL)


# ---- b. whole trajectories ------------------------------------------------------------------------
@pytest.mark.parametrize("T_src,T,n", [(2, 1, 1), (9, 3, 5), (9, 8, 257), (40, 39, 257)])
@pytest.mark.parametrize("offset", ref.OFFSETS)
@pytest.mark.parametrize("kappa,q", ref.TRAJ_FAMILIES)
def test_trajectories_against_the_exact_rollout(gpu, kappa, q, offset, T_src, T, n):
    """Injected x0 (three standard deviations off mean_0) and Z, three cells on two sources
    (src = [1, 0, 1]); (9, 3, 5) is T < T_src - 1 with a ragged stride, 257 one lane past a
    block.  Per step |X_t - X_t*|_F / |X_t* - mean(X_t*)|_F, worst over t, against the oracle's
    same measure; the pad slots between the cells keep their sentinel."""
    sc = ref.traj_scene(kappa, q, offset, T_src, n)
    Z = np.ascontiguousarray(sc["Z"][:, :T])
    ex = ref.exact_rollout(sc["mean"], sc["cov"], sc["src"], T, sc["x0"], Z)
    e_o = ref.traj_error(ref.oracle_rollout(dict(sc, Z=Z), T), ex)
    X, status, pads = _rollout(sc["mean"], sc["cov"], sc["src"], T, n, x0=sc["x0"], Z=Z)
    e_k = ref.traj_error(X, ex)
    print(f"\ntrajectories kappa={kappa:g} q={q:g} offset={offset:g} (T_src, T, n)="
          f"({T_src}, {T}, {n}): oracle {e_o:.2e} kernel {e_k:.2e} ratio {e_k / e_o:.2f}")
    assert np.all(status == 0)
    assert pads
    assert e_k <= ref.bound(e_o)


# ---- c. fused moments ---------------------------------------------------------------------------
@pytest.mark.parametrize("T_src,n", [(2, 2), (9, 321), (9, 777), (10, 321), (17, 321), (18, 321),
                                     (40, 321)])
@pytest.mark.parametrize("offset", ref.OFFSETS)
@pytest.mark.parametrize("kappa,q", ref.TRAJ_FAMILIES)
def test_fused_moments_against_the_exact_sample_moments(gpu, kappa, q, offset, T_src, n):
    """ccmpc_ideal_moments and the out_mean / out_cov of ccmpc_ideal_minkowski_cycle against
    exact_sample_moments(exact_rollout(...)) driven by oracle.philox's normals.  The device's
    normals may differ from those in the last place (log, sin and cos come from another libm):
    1e-16 of a step's spread, far inside the 1e-12 floor.  T_src = 9 | 10, 17 | 18, 40 are the
    row-block instances' edges; at n = 321 the second work item holds one full wave and one
    lane.  Means in units of the exact marginal standard deviation, covariances by relative
    Frobenius error, both against the oracle route's error (orc.predict_ideal + np.cov)."""
    seed, T = 1000 + T_src, T_src - 1
    sc = ref.traj_scene(kappa, q, offset, T_src, n, philox_seed=seed)
    ex = ref.exact_rollout(sc["mean"], sc["cov"], sc["src"], T, sc["x0"], sc["Z"])
    mom = ref.exact_sample_moments(ex)
    om, oc = ref.oracle_moments(ref.oracle_rollout(sc, T))
    o_m, o_c = ref.moment_errors(om, oc, ex, mom)
    m1, c1, st1 = _moments(sc["mean"], sc["cov"], sc["src"], T, n, x0=sc["x0"], seed=seed)
    m2, c2, st2, rec, _ = _cycle(sc["mean"], sc["cov"], sc["src"], T, n, x0=sc["x0"], seed=seed)
    k_m, k_c = ref.moment_errors(m1, c1, ex, mom)
    print(f"\nmoments kappa={kappa:g} q={q:g} offset={offset:g} (T_src, n)=({T_src}, {n}): "
          f"oracle mean {o_m:.2e} cov {o_c:.2e}  kernel mean {k_m:.2e} cov {k_c:.2e}")
    assert np.all(st1 == 0) and np.all(st2 == 0)
    assert m1.tobytes() == m2.tobytes() and c1.tobytes() == c2.tobytes()
    assert k_m <= ref.bound(o_m)
    assert k_c <= ref.bound(o_c)


# ---- d. statuses by an exact margin ---------------------------------------------------------------
N_ROLL, N_MOM, ST_T = 257, 321, 4


def _status_scene():
    sc = ref.traj_scene(1.0, 0.5, 190.0, ST_T + 1, 4)
    return np.array(sc["mean"]), np.array(sc["cov"]), np.array(sc["x0"])


def _launches(mean, cov, src, x0, rng):
    """The three kernels on one set of cells: dict of host arrays."""
    X, s0, pads = _rollout(mean, cov, src, ST_T, N_ROLL, x0=x0, seed=7, rng_cell=rng)
    m1, c1, s1 = _moments(mean, cov, src, ST_T, N_MOM, x0=x0, seed=7, rng_cell=rng)
    m2, c2, s2, rec, pl = _cycle(mean, cov, src, ST_T, N_MOM, x0=x0, seed=7, rng_cell=rng)
    assert pads
    return dict(X=X, s0=s0, m1=m1, c1=c1, s1=s1, m2=m2, c2=c2, s2=s2, rec=rec, pl=pl)


def _with_bad_cell(bad_mean, bad_cov, give_x0):
    """Cells (good on source 0, BAD, good on source 1) with rng_cell = [0, 1, 2] against the
    two good cells alone with rng_cell = [0, 2]: the neighbours must keep status 0 and exactly
    their bits.  Returns the bad launch's outputs."""
    mean, cov, x0 = _status_scene()
    mean3, cov3 = np.concatenate([mean, bad_mean[None]]), np.concatenate([cov, bad_cov[None]])
    x3 = np.stack([x0[0], bad_mean[0] + [0.5, -0.25], x0[1]])
    bad = _launches(mean3, cov3, [0, 2, 1], x3 if give_x0 else None, [0, 1, 2])
    good = _launches(mean, cov, [0, 1], x3[[0, 2]] if give_x0 else None, [0, 2])
    for k in ("s0", "s1", "s2"):
        assert good[k].tolist() == [0, 0] and bad[k][[0, 2]].tolist() == [0, 0], k
    for k in ("X", "m1", "c1", "m2", "c2", "rec", "pl"):
        assert bad[k][[0, 2]].tobytes() == good[k].tobytes(), k
    assert np.all(good["rec"]["status"] == 0)
    assert np.all(bad["rec"][1]["status"] != 0)
    return bad


def _oracle_raises(mean, cov, x0, nan_ok=False):
    T_src = mean.shape[0]
    mom = dict(mean_p0p1=[[list(mean)]],
               cov_p0p1=[[[cov[2 * t:2 * t + 2, 2 * t:2 * t + 2] for t in range(T_src)]]],
               cross_cov=[[[[cov[2 * t:2 * t + 2, 2 * u:2 * u + 2] for u in range(T_src)]
                            for t in range(T_src)]]])
    if nan_ok:
        # np.linalg.inv and, in NumPy builds whose potrf wrapper does not test for it,
        # np.linalg.cholesky let NaN through: the oracle then raises or returns no finite value
        try:
            got = orc.predict_ideal(mom, [1], ST_T, 4, x0s=None if x0 is None else [[x0]], seed=7)
        except np.linalg.LinAlgError:
            return
        assert not np.any(np.isfinite(got[0][0]))
        return
    with pytest.raises(np.linalg.LinAlgError):
        orc.predict_ideal(mom, [1], ST_T, 4, x0s=None if x0 is None else [[x0]], seed=7)


@pytest.mark.parametrize("block", [[[4.0, 2.0], [2.0, 1.0]], [[1.0, 0.0], [0.0, 0.0]],
                                   [[0.0, 0.0], [0.0, 0.0]]])
def test_exactly_singular_source_is_singular(gpu, block):
    """A dyadic Sigma_0 whose float64 determinant is exactly 0 (x0 given, so that the draw does
    not read it): CCMPC_REC_SINGULAR from build_step, np.linalg.inv raises in the oracle."""
    from ccmpc import _lib
    mean, cov, _ = _status_scene()
    bm, bc = mean[0].copy(), cov[0].copy()
    bc[0:2, 0:2] = block
    assert ref.exact_plan(bc[0:2, 0:2], bc[2:4, 2:4], bc[2:4, 0:2])["singular"]
    out = _with_bad_cell(bm, bc, give_x0=True)
    assert [out[k][1] for k in ("s0", "s1", "s2")] == [_lib.REC_SINGULAR] * 3
    assert np.all(np.isnan(out["X"][1])) and np.all(np.isnan(out["m1"][1]))
    _oracle_raises(bm, bc, bm[0] + [0.5, -0.25])
    assert isinstance(_lib.record_error(_lib.REC_SINGULAR, "predict_ideal"), np.linalg.LinAlgError)


def _scaled_cross(t):
    mean, cov, _ = _status_scene()
    bm, bc = mean[1].copy(), cov[1].copy()
    bc[2 * t + 2:2 * t + 4, 2 * t:2 * t + 2] *= 2.0
    bc[2 * t:2 * t + 2, 2 * t + 2:2 * t + 4] *= 2.0
    p = ref.exact_plan(bc[2 * t:2 * t + 2, 2 * t:2 * t + 2], bc[2 * t + 2:2 * t + 4, 2 * t + 2:2 * t + 4],
                       bc[2 * t + 2:2 * t + 4, 2 * t:2 * t + 2])
    assert p["lam"] <= -1e-3 and p["L"] is None          # the exact margin
    return bm, bc


def test_scaled_cross_block_is_not_pd(gpu):
    """C(t+1, t) doubled at t = 1: the exact lambda_min(K) is below -1e-3 |N|_F."""
    from ccmpc import _lib
    bm, bc = _scaled_cross(1)
    for x0 in (True, False):
        out = _with_bad_cell(bm, bc, give_x0=x0)
        assert [out[k][1] for k in ("s0", "s1", "s2")] == [_lib.REC_NOT_PD] * 3
        assert np.all(np.isfinite(out["X"][1][:, :1])) and np.all(np.isnan(out["X"][1][:, 1:]))
    _oracle_raises(bm, bc, None)


def test_nan_source_covariance_of_a_one_particle_cell(gpu):
    """The saved moments of a mode that kept one particle: ccmpc_moments leaves a NaN
    covariance.  Both kernels report a non-zero status, which record_error maps to
    LinAlgError; orc.predict_ideal raises it too where NumPy's cholesky rejects NaN, and
    returns nothing finite where it does not."""
    from ccmpc import _lib, engine
    mean, _, _ = _status_scene()
    one = mean[0][None] + 0.125                                  # (1, T_src, 2): one particle
    store = engine.ParticleStore.from_cells([one], device=gpu)
    bm, bc = (a.cpu().numpy()[0] for a in engine.moments(store))
    assert np.all(np.isfinite(bm)) and not np.any(np.isfinite(bc))
    for x0 in (True, False):
        out = _with_bad_cell(bm, bc, give_x0=x0)
        for k in ("s0", "s1", "s2"):
            assert out[k][1] in (_lib.REC_SINGULAR, _lib.REC_NOT_PD), (k, out[k])
            assert isinstance(_lib.record_error(out[k][1], "predict_ideal"), np.linalg.LinAlgError)
        assert np.all(np.isnan(out["X"][1]))
    _oracle_raises(bm, bc, None, nan_ok=True)
    _oracle_raises(bm, bc, bm[0], nan_ok=True)


def test_x0_draw_from_a_covariance_that_is_not_pd(gpu):
    """x0 == NULL and cov_0 = [[1, 2], [2, 1]] (det -3: no Cholesky factor, not singular)."""
    from ccmpc import _lib
    mean, cov, _ = _status_scene()
    bm, bc = mean[0].copy(), cov[0].copy()
    bc[0:2, 0:2] = [[1.0, 2.0], [2.0, 1.0]]
    out = _with_bad_cell(bm, bc, give_x0=False)
    assert [out[k][1] for k in ("s0", "s1", "s2")] == [_lib.REC_NOT_PD] * 3
    assert np.all(np.isnan(out["X"][1])) and np.all(np.isnan(out["m1"][1]))
    _oracle_raises(bm, bc, None)


# ---- e. the x0 = NULL draw ------------------------------------------------------------------------
def test_x0_draw_follows_rng_cell(gpu):
    """Sigma_0 = C = [[4, 2], [2, 2]], Sigma_1 = Sigma_0 + I, zero means, Z = 0: A = I and
    L = I exactly, so slot 0 is x0 = chol(Sigma_0) z itself, chol = [[2, 0], [1, 1]] exactly.
    The draw is keyed by rng_cell[c], not by the cell's place in the call."""
    S0 = np.array([[4.0, 2.0], [2.0, 2.0]])
    cov = np.zeros((1, 4, 4))
    cov[0, 0:2, 0:2], cov[0, 2:4, 2:4], cov[0, 2:4, 0:2], cov[0, 0:2, 2:4] = S0, S0 + np.eye(2), S0, S0
    mean = np.zeros((1, 2, 2))
    rng = [5, 0, 5]
    X, status, _ = _rollout(mean, cov, [0, 0, 0], 1, 2, Z=np.zeros((3, 1, 2, 2)), seed=11,
                            rng_cell=rng)
    assert status.tolist() == [0, 0, 0]
    for c, r in enumerate(rng):
        want = orc.ideal_x0(mean[0, 0], S0, r, 11)
        np.testing.assert_allclose(X[c, 0, 0], want, rtol=1e-14)
        np.testing.assert_array_equal(X[c, 1, 0], X[c, 0, 0])
    np.testing.assert_array_equal(X[0], X[2])
    assert not np.array_equal(X[0], X[1])


# ---- f. sharding invariance ---------------------------------------------------------------------
def test_results_do_not_depend_on_how_cells_are_sharded(gpu):
    """Three cells in one call against the same cells in two calls with rng_cell = [0, 1] and
    [2]; rng_cell = NULL equals rng_cell = arange.  Positions bit-identical; at n = 777 the
    fused moments, covariances and statuses too: ideal_chunk is 256 samples for every
    n_cells n <= 131 072, so a cell's items, and with them the order of its sums, are the
    same in a 1-, 2- and 3-cell launch."""
    sc = ref.traj_scene(1e2, 1e-2, 190.0, 9, 4)
    mean, cov, src, T = sc["mean"], sc["cov"], list(sc["src"]), 8
    whole = _rollout(mean, cov, src, T, 257, seed=3)
    named = _rollout(mean, cov, src, T, 257, seed=3, rng_cell=[0, 1, 2])
    a = _rollout(mean, cov, src[:2], T, 257, seed=3, rng_cell=[0, 1])
    b = _rollout(mean, cov, src[2:], T, 257, seed=3, rng_cell=[2])
    assert whole[1].tolist() == [0, 0, 0]
    assert whole[0].tobytes() == named[0].tobytes()
    assert whole[0].tobytes() == np.concatenate([a[0], b[0]]).tobytes()
    assert not np.array_equal(whole[0][0], whole[0][2])           # same source, other stream
    for run in (_moments, lambda *a, **k: _cycle(*a, **k)[:3]):
        w = run(mean, cov, src, T, 777, seed=3)
        nm = run(mean, cov, src, T, 777, seed=3, rng_cell=[0, 1, 2])
        p = run(mean, cov, src[:2], T, 777, seed=3, rng_cell=[0, 1])
        r = run(mean, cov, src[2:], T, 777, seed=3, rng_cell=[2])
        for k in range(3):
            assert w[k].tobytes() == nm[k].tobytes()
            assert w[k].tobytes() == np.concatenate([p[k], r[k]]).tobytes()
        assert w[2].tolist() == [0, 0, 0]


# ---- g. failed cells are reproducible -------------------------------------------------------------
def test_failed_cell_outputs_do_not_depend_on_stale_lds(gpu):
    """One NOT_PD cell (its step t = 2 of 4 fails) and one good cell, after NaN, zero and huge
    fills of every CU's LDS (ccmpc_poison_lds, as tests/test_gpu_lds_poison.py): every output of
    all three kernels is the same bytes, the failed cell's positions and moments are NaN from
    its first failed step on and as a good cell's before it, and every half-space record of
    the failed cell carries a non-zero status."""
    from ccmpc import _lib, engine
    mean, cov, x0 = _status_scene()
    bm, bc = _scaled_cross(2)
    mean3, cov3 = np.concatenate([mean, bm[None]]), np.concatenate([cov, bc[None]])
    runs = []
    for v in (float("nan"), 0.0, 1e300):
        _lib.check(_lib.load().ccmpc_poison_lds(ctypes.c_double(v), engine._stream()),
                   "ccmpc_poison_lds")
        torch.cuda.synchronize()
        runs.append(_launches(mean3, cov3, [2, 0], x0[:2], [0, 1]))
    first = runs[0]
    same = {k: all(r[k].tobytes() == first[k].tobytes() for r in runs[1:]) for k in first}
    print("\nfailed cell, same bytes under the three fills:", same)
    status = {k: first[k].tolist() for k in ("s0", "s1", "s2")}
    X, m, c, rec = first["X"], first["m2"], first["c2"], first["rec"]
    checks = dict(
        status=all(v == [_lib.REC_NOT_PD, 0] for v in status.values()),
        positions_before=bool(np.all(np.isfinite(X[0][:, :2]))),
        positions_from=bool(np.all(np.isnan(X[0][:, 2:]))),
        moments_before=bool(np.all(np.isfinite(m[0][:2])) and np.all(np.isfinite(c[0][:4, :4]))),
        moments_from=bool(np.all(np.isnan(m[0][2:])) and np.all(np.isnan(c[0][4:, :]))
                          and np.all(np.isnan(c[0][:, 4:]))),
        records_flagged=bool(np.all(rec[0]["status"] != 0)),
        good_cell=bool(np.all(np.isfinite(X[1])) and np.all(np.isfinite(c[1]))
                       and np.all(rec[1]["status"] == 0)),
        fused_pair=first["m1"].tobytes() == first["m2"].tobytes()
        and first["c1"].tobytes() == first["c2"].tobytes())
    print("failed cell:", status, checks)
    assert all(same.values()), same
    assert all(checks.values()), checks
    # the steps before the failure are the steps of the same cell without it
    ok = _launches(mean, cov, [1, 0], x0[:2], [0, 1])
    assert X[0][:, :2].tobytes() == ok["X"][0][:, :2].tobytes()
