"""Accuracy of the half-space tail (constraints.hpp / constraints.hip) and of the moment
reduction against an exact (50-digit) reference, off the beaten scale.

How results are judged.  For each input family, e_f is the worst error of the float64 oracle
(oracle/ccmpc_oracle.py; for moments the NumPy model of the kernel's own shifted one-pass
formula) against the exact reference on the family's cases, computed at test time
(tests/_tail_ref.py; tests/test_tail_ref_host.py prints and checks them on the host).  The
kernel must be within max(8 e_f, 1e-12): 8 = the kernel's <= 2 ulp divisions and roots against
IEEE's 0.5 (4x), doubled for its different operation order; 1e-12 is the level the suite calls
typical.  Q also meets the project's 1e-5 bar everywhere.  No bound is read off a GPU run.

Integer decisions (which, side, the MVOE stop iterate) are compared wherever the exact margin
allows: which / side above an exact relative margin of 1e-9; the stop iterate on *clear stops*
(last step < tol / 2, the one before > 2 tol).  On the other stops beta may be one iterate off:
|beta - beta_ref| <= tol plus the rounding allowance, Q judged through that.

What was narrowed: at aspect 1e6 and S2 / S1 >= 1e4 the float64 oracle alone is 1e-6 .. 3e-6
off the exact Q, so those two columns of the MVOE grid run at aspect 1e5.  Grid cells whose
fixed point contracts by less than 4x per step have no clear stops at all (aspect >= 1e3 near
ratio 1); they are thinned to 2 cases so that <= 25 % of the MVOE cases are judged loosely.

e_f per family (host, float64 oracle against exact) and the kernel's measured worst (MI355X):

  family                        e_f                             kernel
  rcp_nr / div_nr / sqrt_gs     0.5 ulp (IEEE)                  0.500 ulp each (bound: 2)
  one MVOE step                 --                              1.63 ulp (bound: 8)
  MVOE aspect 1                 beta 1.8e-16  Q 2.6e-16         beta 2.8e-16  Q 2.6e-16
  MVOE aspect 1e3               beta 5.0e-11  Q 6.7e-12         beta 4.8e-11  Q 6.5e-12
  MVOE aspect 1e6 (1e5)         beta 6.2e-07  Q 4.7e-08         beta 4.8e-07  Q 4.3e-08
  MVOE second call (Q, R^2 I)   beta 2.1e-14  Q 2.4e-15         beta 2.9e-14  Q 2.6e-15
  MVOE S1 / S2 = 1e-12, 1e12    beta 4.1e-12  Q 1.6e-16         beta 1.4e-11  Q 2.2e-16
  pair rho 1e-3   aspect 1e6    blocks 8.6e-17 lb 1.0e-09 scale 2.1e-14   8.6e-17 5.8e-10 5.2e-14
  pair rho 0.5    aspect 1e6    blocks 7.3e-12 lb 2.9e-11 scale 8.8e-12   5.5e-12 2.2e-11 6.6e-12
  pair rho 1-1e-3 aspect 1e6    blocks 3.4e-11 lb 8.9e-11 scale 4.4e-10   3.4e-11 8.9e-11 4.4e-10
  pair rho 1-1e-6 aspect 1e6    blocks 2.6e-11 lb 1.7e-09 scale 1.2e-08   2.3e-11 1.5e-09 1.0e-08
  pair rho 1-1e-9 aspect 1e6    blocks 2.5e-11 lb 4.4e-08 scale 3.1e-07   1.6e-11 3.4e-08 2.3e-07
  pair rho 1-1e-9 aspect 1      blocks 1.4e-16 lb 2.6e-13 scale 1.8e-12   1.9e-16 3.8e-13 2.6e-12
  (18 pair families, rho x aspect; rho = 0 is exact on both sides)
  tangent                       d 2.1e-16                       d 2.1e-16, 0 of 480 skipped
  near-singular affine          margin 2.3e-12 rhs 8.4e-13      margin 4.1e-13 rhs 4.3e-14
  moments, cov (one-pass model) 8e-17 .. 1e-14; outlier cell 2.8e-13   <= 1.6e-15; outlier 8.9e-14
  records, plain stores (worst) m, d, margin, rhs 4.4e-08; Q 1.6e-13; beta1 3.7e-13
                                                         kernel 1.7e-08; Q 7.8e-16; beta1 1.8e-15
  records, squeezed (worst)     m, d, margin, rhs 2.0e-07; Q 1.6e-09; QR 6.1e-09; beta1 6.6e-08
                                                 kernel 1.8e-07; Q 1.8e-10; QR 8.8e-11; beta1 5.6e-09
  (record families are per store; m and d lose digits only at 1e6 m translation with 2^-10 scale,
  where ref - mean is 1e-2 against coordinates of 1e6)
"""
import numpy as np
import pytest
import torch

import _tail_ref as ref

pytestmark = pytest.mark.gpu


def _selftest(kind, rows, out_width, tol=ref.TOL, maxiter=ref.MAXITER):
    from ccmpc import _lib, engine
    x = torch.as_tensor(np.ascontiguousarray(rows, np.float64), device="cuda")
    n = x.shape[0]
    y = torch.full((n, out_width), np.nan, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().ccmpc_selftest(kind, n, engine._p(x), engine._p(y), tol, maxiter,
                                          engine._stream()), "ccmpc_selftest")
    return y.cpu().numpy()


def _dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ---- a. primitives ----------------------------------------------------------------------------
def _primitive_ulps():
    """Worst ulp error of (rcp_nr, div_nr, sqrt_gs, mvoe_step) over prim_inputs()."""
    from ccmpc import _lib
    ab = ref.prim_inputs()
    y = _selftest(_lib.SELFTEST_PRIM, ab, 4)
    assert np.all(np.isfinite(y))
    F, mp = ref.F, ref.mp
    worst = np.zeros(4)
    for (a, b), out in zip(ab, y):
        a, b = F(float(a)), F(float(b))
        want = (1 / b, a / b, mp.sqrt(b), mp.sqrt((b * a + 2) / (a + b)))
        worst = np.maximum(worst, [ref.ulp_err(o, w) for o, w in zip(out, want)])
    print(f"\nprimitives, worst ulp: rcp_nr {worst[0]:.3f} div_nr {worst[1]:.3f} "
          f"sqrt_gs {worst[2]:.3f} mvoe_step {worst[3]:.3f}")
    return worst


def test_primitives_within_two_ulp(gpu):
    """rcp_nr, div_nr and sqrt_gs over [2^-200, 2^200], powers of two and their neighbours:
    <= 2 ulp of the exact value, the bound constraints.hpp claims.  Measured on the MI355X:
    0.500 ulp each, i.e. correctly rounded on all 4303 inputs."""
    worst = _primitive_ulps()
    assert worst[0] <= 2 and worst[1] <= 2 and worst[2] <= 2, worst


def test_mvoe_step_within_eight_ulp(gpu):
    """One update N rsqrt(N D) of the MVOE fixed point against the exact sqrt(N / D).

    With y = rsqrt(x) (1 + e) the step forms r = 1 - x y^2 = -(2 e + e^2) and returns
    N y (1 + r / 2 + 3/8 r^2) = N / sqrt(x) (1 + O(e^3)) before rounding; its roundings (N, D,
    x = N D, g = x y, A = N y, the final fma) add at most (1/2 + 1/2 + 1/2 + 1/2 + 1 + 1) 2^-53 =
    2 ulp.  The accuracy e of the hardware's f64 reciprocal-square-root estimate is not
    documented in anything this project can cite (neither the ROCm headers nor the programming
    guides state it), so the analytic bound cannot be closed; what is asserted is the code
    comment's "a few ulp per step", taken as <= 8 ulp.

    This test found the step wrong as first written: with the first-order correction
    N y (1 + r / 2) it measured 17.02 ulp on the MI355X, i.e. 3/2 e^2 with e ~ 2^-24.2 (the
    estimate is a single-precision-grade seed).  The second-order term costs no operation and no
    depth of chain (constraints.hpp, mvoe_step) and measures 1.63 ulp (worst of 4303 inputs)."""
    worst = _primitive_ulps()
    assert worst[3] <= 8, worst


def test_primitives_edge_values(gpu):
    """sqrt_gs(0) = 0 and sqrt_gs(x < 0) = NaN, as compute_mvoe's discriminant relies on."""
    from ccmpc import _lib
    y = _selftest(_lib.SELFTEST_PRIM, np.array([[1.0, 0.0], [1.0, -1.0], [1.0, -0.0]]), 4)
    assert y[0, 2] == 0.0 and np.isnan(y[1, 2]) and y[2, 2] == 0.0


# ---- b. MVOE grid -----------------------------------------------------------------------------
def test_mvoe_grid(gpu):
    """The scale x ratio x aspect grid, the tail's second call shape and the two extreme
    ratios through compute_mvoe on the device."""
    from ccmpc import _lib
    cases, refs = ref.mvoe_cases(), ref.mvoe_reference()
    errs = ref.family_errors(cases, refs, ("e_beta", "e_q"), only=lambda c, r: r["same_iters"])
    rows = np.array([[*c["S1"].reshape(4), *c["S2"].reshape(4)] for c in cases])
    y = _selftest(_lib.SELFTEST_MVOE, rows, 6)
    assert np.all(y[:, 5] == 1.0) and np.all(np.isfinite(y))
    worst, bad = {}, []
    for c, r, out in zip(cases, refs, y):
        ex = r["ref"]
        eb, eq = ref.rel(out[0], ex["beta"]), ref.rel_fro(out[1:5], ex["Q"])
        ab, aq = ref.mvoe_allowance(ex, errs[c["family"]])
        w = worst.setdefault((c["family"], ex["clear"]), [0.0, 0.0])
        w[0], w[1] = max(w[0], eb), max(w[1], eq)
        if not (eb <= ab and eq <= aq and eq < ref.BAR_Q):
            bad.append((c["tag"], ex["clear"], eb, ab, eq, aq))
    msg = (f"e_f {errs}; kernel worst (family, clear stop) -> (beta, Q): "
           + "; ".join(f"{k}: {v[0]:.1e}, {v[1]:.1e}" for k, v in sorted(worst.items())))
    print("\nMVOE " + msg)
    assert not bad, (bad[:5], len(bad), msg)


def test_mvoe_singular_first_matrix(gpu):
    from ccmpc import _lib
    y = _selftest(_lib.SELFTEST_MVOE, np.array([[1.0, 2.0, 2.0, 4.0, 1.0, 0.0, 0.0, 1.0],
                                                [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0]]), 6)
    assert np.all(y[:, 5] == 0.0)
    assert ref.compute_mvoe([[1.0, 2.0], [2.0, 4.0]], np.eye(2)) is None


# ---- c. pair moments --------------------------------------------------------------------------
def test_pair_moments_weak_and_strong_correlation(gpu):
    """predict_moments, the lower bound and the scale from 4x4 covariances whose t / tau
    blocks are correlated by 0 .. 1 - 1e-9: the 1 - alpha cancellation at weak correlation and
    the Schur-complement cancellation at strong correlation.  The blocks' errors are measured
    against |c_t|_F (cov_infer + cov_mu = c_t)."""
    from ccmpc import _lib
    cases, refs = ref.pair_cases(), ref.pair_reference()
    errs = ref.family_errors(cases, refs, ref.PAIR_KEYS)
    rows = np.array([[*c["C"].reshape(16), ref.PAIR_GAMMA, ref.PAIR_CHI_P] for c in cases])
    y = _selftest(_lib.SELFTEST_PAIR, rows, 14)
    worst, bad = {}, []
    for c, r, out in zip(cases, refs, y):
        e = ref.pair_errors(out[0:4], out[4:8], out[8:12], out[12], out[13], r["ex"])
        w = worst.setdefault(c["family"], {k: 0.0 for k in ref.PAIR_KEYS})
        for k in ref.PAIR_KEYS:
            w[k] = max(w[k], e[k])
            if not e[k] <= ref.bound(errs[c["family"]][k]):
                bad.append((c["tag"], k, e[k], ref.bound(errs[c["family"]][k])))
        if c["rho"] == 0.0:
            assert np.all(out[4:8] == 0.0) and np.array_equal(out[0:4], out[8:12])
            assert np.isnan(out[12]) and out[13] == 1.0
    msg = "; ".join(f"{f}: e_f {errs[f]} kernel {w}" for f, w in sorted(worst.items()))
    print("\npair " + msg)
    assert not bad, (bad[:5], len(bad), msg)


def test_pair_moments_singular_tau_block(gpu):
    """An exactly singular tau block: NaN cov_mu / cov_infer, bound and scale, as today (the
    record status this becomes, CCMPC_REC_SINGULAR, is test_gpu_selftest's through the cycle),
    and a NaN beta from compute_mvoe on them."""
    from ccmpc import _lib
    C = np.array([[1.0, 2.0, 0.5, 0.1], [2.0, 4.0, 0.2, 0.3], [0.5, 0.2, 3.0, 0.4],
                  [0.1, 0.3, 0.4, 2.0]])
    assert ref.predict_moments(C, 1, 0) is None
    y = _selftest(_lib.SELFTEST_PAIR, np.array([[*C.reshape(16), 2.7, 18.4]]), 14)
    assert not np.any(np.isfinite(y[0, 0:8])) and np.all(np.isfinite(y[0, 8:12]))
    assert np.isnan(y[0, 12]) and np.isnan(y[0, 13])
    z = _selftest(_lib.SELFTEST_MVOE, np.hstack((y[:, 0:4], y[:, 4:8])), 6)
    assert not np.isfinite(z[0, 0])


# ---- d. tangent -------------------------------------------------------------------------------
def test_tangent_slopes_aspects_and_distances(gpu):
    """which and the side test n.mu <= d equal the exact decision wherever the exact relative
    margin is > 1e-9; d is measured against |n.mu| + |c sqrt(n^T Sigma n)|."""
    from ccmpc import _lib
    cases, refs = ref.tangent_cases(), ref.tangent_reference()
    e_f = max(r["e_d"] for r in refs)
    rows = ref.tangent_rows(cases)
    y = _selftest(_lib.SELFTEST_TANGENT, rows, 5)
    assert np.all(y[:, 4] == 0)
    worst, skipped = 0.0, 0
    for c, r, out in zip(cases, refs, y):
        ex = r["ex"]
        which = int(out[3])
        assert out[0] == -c["m"] and out[1] == 1.0
        if ex["margin"] > ref.MARGIN:
            assert which == ex["which"], (c["tag"], ex["margin"])
        else:
            skipped += 1
        proj = -c["m"] * c["mu"][0] + 1.0 * c["mu"][1]       # the device's n0 mu0 + n1 mu1
        side = 1 if proj <= out[2] else -1
        if ex["margin"] > ref.MARGIN and ex["side_margin"] > ref.MARGIN:
            assert side == ex["side"], (c["tag"], ex["side_margin"])
        e = ref.rel(out[2], ex["cands"][which], ex["scale"])
        worst = max(worst, e)
        assert e <= ref.bound(e_f), (c["tag"], e, e_f)
    print(f"\ntangent e_f {e_f:.1e} kernel worst {worst:.1e}, skipped {skipped}")
    assert skipped <= 0.05 * len(cases)


# ---- f. moments conditioning ------------------------------------------------------------------
@pytest.mark.parametrize("ci,f32", ref.MOM_STORES)
def test_moments_conditioning(gpu, ci, f32):
    """Cells of 2 .. 4100 particles (the last through the combine tree) at offset / spread up
    to 1e6 / 1e-3, one cell led by an outlier 1e3 spreads away, one f32 store with origin 1e6.
    The mean: 1e-14 of |mean| plus 1e-14 of the spread.  The covariance: max(8 e_f, 1e-12) in
    units of the coordinates' spreads, e_f from the NumPy model of the shifted one-pass formula
    -- so the documented cost of an outlying first particle is allowed and an absent shift is
    not: on the f64 stores the unshifted form is >= 100x worse than the shifted one and
    outside the bound (premise, asserted)."""
    from ccmpc import engine
    sc, rs = ref.moments_scene(ci, f32), ref.moments_reference(ci, f32)
    store = engine.ParticleStore.from_cells(
        sc["cells"], device=gpu, dtype=torch.float32 if f32 else torch.float64,
        origin=sc["origin"])
    for j, r in enumerate(rs):          # the store holds what the reference was computed from
        o, n = store.offsets[j], store.counts[j]
        assert np.array_equal(store.pos[:, o:o + n].double().cpu().numpy().T, r["X"])
    mean, cov = engine.moments(store)
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    out = []
    for j, r in enumerate(rs):
        if not f32 and j != ref.MOM_OUTLIER_CELL:
            assert r["e_unshifted"] >= 100 * max(r["e_model"], 2.0 ** -53)
            assert r["e_unshifted"] > ref.bound(r["e_model"])
        em, ec = ref.mean_err(mean[j], r["mean"], r["cov"]), ref.cov_err(cov[j], r["cov"])
        out.append((ref.MOM_COUNTS[j], r["e_model"], ec, em))
        assert np.array_equal(cov[j], cov[j].T)
    msg = "; ".join(f"n={n}: e_f {e:.1e} kernel {k:.1e} mean {m:.2f}" for n, e, k, m in out)
    print(f"\nmoments {ref.MOM_CONDS[ci]} f32={f32}: {msg}")
    for n, e, k, m in out:
        assert k <= ref.bound(e) and m <= 1.0, msg


# ---- g. near-singular covariances in ccmpc_affine ---------------------------------------------
def _affine_injected(mean, cov, ref_traj, gamma):
    from ccmpc import engine
    rec = engine.affine(_dev(mean), _dev(cov), _dev(ref_traj), _dev(gamma), R=ref.R_COLLISION)
    return engine.affine_records(rec)


def test_affine_near_singular_covariances(gpu):
    """Rank-1 covariances v v^T at 12 rotation angles and three scales, the same plus
    1e-12 I, and aspect 1e8, injected into ccmpc_affine.  Wherever the float64 entries, taken
    exactly, form a PSD matrix the status is 0 and margin / rhs are within the yardstick of the
    exact principal root.  Where rounding left v v^T exactly indefinite (det < 0 by ~1e-16),
    the kernel's plain a d - b c says so or rounds to 0; which of the two is decided by IEEE
    arithmetic alone and is asserted bit for bit.

    The plain determinant was expected to fail the PSD clause and does not: a d >= b c exactly
    implies fl(a d) >= fl(b c), so no case can (tests/test_tail_ref_host.py checks the same on
    the host, with the compensated product for comparison).  The kernel keeps the plain form."""
    from ccmpc import _lib
    sc, refs = ref.singular_scene(), ref.singular_reference()
    psd = [r for r in refs if r["psd"]]
    e_m, e_r = max(r["e_margin"] for r in psd), max(r["e_rhs"] for r in psd)
    h = _affine_injected(sc["mean"], sc["cov"], sc["ref"], sc["gamma"])
    worst = [0.0, 0.0]
    for r in refs:
        g = h[r["cell"], r["t"]]
        if r["psd"]:
            assert g["status"] == 0, (r["cell"], r["t"], r["plain"])
            ex = r["ex"]
            em = ref.rel(g["margin"], ex["margin"])
            er = ref.rel(g["rhs"], ex["rhs"], ex["tangent"]["scale"] + ex["margin"])
            worst = [max(worst[0], em), max(worst[1], er)]
            assert g["which"] == ex["which"] and g["side"] == ex["side"]
            assert em <= ref.bound(e_m) and er <= ref.bound(e_r), (r["cell"], r["t"], em, er)
        else:
            want = _lib.REC_NOT_PSD if r["plain"] < 0 else 0
            assert g["status"] == want, (r["cell"], r["t"], r["plain"])
            if want:
                assert np.isnan(g["s00"]) and np.isnan(g["s01"]) and np.isnan(g["s11"])
    print(f"\nnear-singular affine: e_f margin {e_m:.1e} rhs {e_r:.1e}; kernel worst margin "
          f"{worst[0]:.1e} rhs {worst[1]:.1e}")


def test_affine_not_psd_and_infinite_slope(gpu):
    """A genuinely indefinite covariance: CCMPC_REC_NOT_PSD, NaN s**, and the planner's
    exception for that status.  ref_y == mean_y: CCMPC_REC_NONFINITE here too."""
    from ccmpc import _lib
    T = 3
    mean = np.tile([190.0, -80.0], (1, T, 1))
    cov = np.zeros((1, 2 * T, 2 * T))
    cov[0, 0:2, 0:2] = [[1.0, 2.0], [2.0, 1.0]]             # eigenvalues 3, -1
    cov[0, 2:4, 2:4] = [[2.0, 0.5], [0.5, 1.0]]
    cov[0, 4:6, 4:6] = [[2.0, 0.5], [0.5, 1.0]]
    ref_traj = mean[0] + np.array([-9.0, 4.0])
    ref_traj[2, 1] = mean[0, 2, 1]                           # infinite slope at t = 2
    h = _affine_injected(mean, cov, ref_traj, np.array([2.5]))[0]
    assert h["status"].tolist() == [_lib.REC_NOT_PSD, 0, _lib.REC_NONFINITE]
    assert np.isnan(h["s00"][0]) and np.isnan(h["s01"][0]) and np.isnan(h["s11"][0])
    assert np.isnan(h["margin"][0]) and np.isfinite(h["margin"][1])
    assert ref.sqrtm2(ref.m2(cov[0, 0:2, 0:2])) is None
    e = _lib.record_error(_lib.REC_NOT_PSD, "affine")
    assert isinstance(e, _lib.NonFiniteRecordError) and "not PSD" in str(e)
    with pytest.raises(_lib.NonFiniteRecordError):
        raise e


# ---- e. whole records -------------------------------------------------------------------------
def _judge(errors, e_f, worst):
    ok = True
    for k, v in errors.items():
        worst[k] = max(worst.get(k, 0.0), v)
        ok = ok and v <= ref.bound(e_f[k])
    return ok


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("squeeze", [False, True])
def test_whole_records_under_similarity_transforms(gpu, f32, squeeze):
    """One base cloud (T = 4, cells of 64, 65 and 300 particles) translated by 0 / 1e3 / 1e6 m,
    scaled by 2^-10 / 1 / 2^10 (ref_traj and R along) and optionally squeezed along a 30 degree
    axis, in an f64 store or an f32 store whose origin is the translation, through
    ccmpc_moments + ccmpc_minkowski, ccmpc_minkowski_cycle (bit-equal to the former),
    ccmpc_affine and ccmpc_affine_scale (scaled and unscaled).  Every record field is judged
    against the exact pipeline on the store's actual values, e_f per store.

    Narrowed: the squeeze is to aspect 1e3, not 1e4 (there 8 e_f of beta1 is 3e-5: too
    ill-conditioned to judge).  MVOE stops that are not clear (half of the plain stores', 8 of 9
    of the squeezed ones': the 25 % cap cannot be met on these records) are judged against the
    exact pipeline stopped one iterate earlier, on, and one later, at the full allowance."""
    from ccmpc import engine
    worst = {}
    for tr in ref.REC_TRANSLATIONS:
        for s in ref.REC_SCALES:
            sc, rr = ref.record_scene(tr, s, squeeze, f32), ref.record_reference(tr, s, squeeze, f32)
            store = engine.ParticleStore.from_cells(
                sc["cells"], device=gpu, dtype=torch.float32 if f32 else torch.float64,
                origin=sc["origin"])
            rt, risk = _dev(sc["ref"]), _dev(sc["risk"])
            mean, cov = engine.moments(store)
            rec_u, pl_u = engine.minkowski(mean, cov, rt, risk, R=sc["R"])
            mean_f, cov_f, rec_f, pl_f = engine.minkowski_cycle(store, rt, risk, R=sc["R"])
            assert torch.equal(mean, mean_f) and torch.equal(cov, cov_f)
            assert torch.equal(rec_u, rec_f) and torch.equal(pl_u, pl_f)
            h = engine.halfspaces(rec_f)
            aff = engine.affine_records(engine.affine(mean, cov, rt, _dev(sc["risk"][:, 2]),
                                                      R=sc["R"]))
            scl = engine.affine_records(engine.affine_scale(mean, cov, rt, risk, R=sc["R"]))
            uns = engine.affine_records(engine.affine_scale(mean, cov, rt, risk, R=sc["R"],
                                                            scaled=False))
            pl = pl_f.cpu().numpy()
            tag = (tr, s)
            for j in range(len(sc["cells"])):
                k = 0
                for t in range(ref.REC_T):
                    assert ref.rel(pl[j, t], rr["prob_lower"][j][t]) <= ref.bound(
                        rr["e_mink"]["lb"]), (tag, j, t)
                    for tau in range(t):
                        g, cands = h[j, k], rr["mink"][j][k]
                        k += 1
                        assert g["status"] == 0 and g["t_tau"] == (t << 16) | tau
                        assert g["n1"] == 1.0
                        hit, tried = False, []
                        for cd in cands:
                            w = {}
                            e = ref.record_errors(g, cd)
                            good = _judge(e, rr["e_mink"], w) and e["q"] < ref.BAR_Q
                            good = good and g["which"] == cd["tg"]["which"] \
                                and g["side"] == cd["tg"]["side"]
                            tried.append(e)
                            if good:
                                hit = True
                                for f, v in w.items():
                                    worst["mink." + f] = max(worst.get("mink." + f, 0.0), v)
                                break
                        assert hit, (tag, j, t, tau, tried, rr["e_mink"])
                    ex = rr["affine"][j][t]
                    a = aff[j, t]
                    w = {}
                    assert a["status"] == 0 and a["t"] == t
                    assert a["which"] == ex["which"] and a["side"] == ex["side"]
                    assert _judge(ref.affine_errors(a, ex), rr["e_affine"], w), \
                        (tag, j, t, w, rr["e_affine"])
                    for f, v in w.items():
                        worst["affine." + f] = max(worst.get("affine." + f, 0.0), v)
                    for name, got, want in (("scaled", scl, rr["scaled"]),
                                            ("unscaled", uns, rr["unscaled"])):
                        b, ex = got[j, t], want[j][t]
                        w = {}
                        assert b["status"] == 0 and b["which"] == ex["which"] \
                            and b["side"] == ex["side"]
                        assert _judge(ref.scaled_errors(b, ex), rr["e_scaled"], w), \
                            (tag, name, j, t, w, rr["e_scaled"])
                        for f, v in w.items():
                            worst[name + "." + f] = max(worst.get(name + "." + f, 0.0), v)
                    assert uns[j, t]["s00"] == 1.0
    print(f"\nrecords f32={f32} squeeze={squeeze}: kernel worst "
          + ", ".join(f"{k}={v:.1e}" for k, v in sorted(worst.items())))
