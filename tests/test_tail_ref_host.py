"""The exact reference of the tail-precision tests (tests/_tail_ref.py) against the reference
project's component goldens, the float64 oracle's own error on every input family of
tests/test_gpu_tail_precision.py (the yardstick e_f of those tests), and the caps on skipped
and loosely judged cases.  Host only.

Where the goldens are not reproduced to 1e-13 relative:
  * mvoe.npz: beta of cases 24 and 142 (1.2e-13, 1.7e-13).  The eigenvalues of S1^-1 S2 are
    2.7e3 and 1.4e4 apart there and beta inherits that spread; the bound used is
    max(1e-13, 2^-52 lambda_1 / lambda_2).  Q agrees to 1e-13 on all 160.
  * predict_moments.npz: cov_infer is a Schur complement 3e-4 .. 8e-2 the size of cov_t, so
    measured against itself the fixture's float64 np.cov / inv chain is up to 4.7e-12 off (case
    12: N = 5, cond(c_tau) = 81); measured against |cov_t|_F, the scale of the subtraction, all
    18 cases agree to 1e-13.
  * tangent.npz: `which` matches on the 180 cases with a margin; the first 20 are exact ties
    (a == mu, margin < 1e-40 at 50 digits), which the fixture's rounding resolves both ways.
"""
import numpy as np
import pytest

from oracle import ccmpc_oracle as orc

import _tail_ref as ref


def _table(errs):
    return "; ".join(f"{f}: " + ", ".join(f"{k}={v:.1e}" for k, v in e.items())
                     for f, e in sorted(errs.items()))


# ---- the reference against the goldens --------------------------------------------------------
def test_mvoe_golden(golden):
    g = golden("mvoe")
    loose = []
    for i in range(len(g["beta"])):
        r = ref.compute_mvoe(g["S1"][i], g["S2"][i])
        _, _, it = orc.compute_mvoe(g["S1"][i], g["S2"][i])
        assert it == r["iters"], (i, it, r["iters"])           # the iteration, step for step
        assert ref.rel_fro(g["Q"][i], r["Q"]) < 1e-13, i
        spread = float(r["lam"][0] / r["lam"][1])
        eb = ref.rel(g["beta"][i], r["beta"])
        assert eb < max(1e-13, 2.0 ** -52 * spread), (i, eb, spread)
        if eb >= 1e-13:
            loose.append(i)
    assert loose == [24, 142], loose


def test_tangent_golden(golden):
    g = golden("tangent")
    ties = []
    for i in range(len(g["m"])):
        ex = ref.closest_tangent(g["mu"][i], g["Sigma"][i], g["c"][i], g["m"][i], g["a"][i])
        w = int(g["which"][i])
        if ex["margin"] > ref.MARGIN:
            assert ex["which"] == w, i
        else:
            ties.append(i)
            assert ex["margin"] < 1e-40                         # a tie to the working precision
        assert ref.rel(g["d"][i], ex["cands"][w], ex["scale"]) < 1e-13, i
        assert float(ex["n0"]) == g["n"][i][0] and g["n"][i][1] == 1.0
    assert ties == list(range(20))


def test_lower_bound_golden(golden):
    g = golden("lower_bound")
    chi_p = orc.scipy.stats.chi2.ppf(orc.TARGET_P, df=2)
    for i in range(len(g["eps"])):
        a, b, c = (ref.m2(g[k][i]) for k in ("cov_infer", "cov_mu", "cov_t"))
        assert ref.rel(g["lower_bound"][i],
                       ref.compute_lower_bound(a, b, c, g["gamma"][i])) < 1e-13, i
        assert ref.rel(g["scale"][i], ref.compute_scale(a, b, c, g["gamma"][i], chi_p)) < 1e-13


def test_predict_moments_golden(golden):
    """The exact ddof = 1 covariance of the fixture's points, split exactly, against the
    reference's np.cov-based outputs."""
    g = golden("predict_moments")
    offs = g["offsets"]
    worst_self = 0.0
    for i in range(len(offs) - 1):
        p = g["points"][:, offs[i]:offs[i + 1]]
        _, cov = ref.exact_moments(np.stack([p[2], p[3], p[0], p[1]], 1))   # tau rows first

        def blk(a, b):
            return (cov[2 * a][2 * b], cov[2 * a][2 * b + 1], cov[2 * a + 1][2 * b],
                    cov[2 * a + 1][2 * b + 1])
        ct = blk(1, 1)
        cm = ref.mul(ref.mul(blk(1, 0), ref.inv(blk(0, 0))), blk(0, 1))
        ci = tuple(x - y for x, y in zip(ct, cm))
        assert ref.rel_fro(g["cov_t"][i], ct) < 1e-13 and ref.rel_fro(g["cov_mu"][i], cm) < 1e-13
        e_self = ref.rel_fro(g["cov_infer"][i], ci)
        worst_self = max(worst_self, e_self)
        assert e_self * float(ref.fro(ci) / ref.fro(ct)) < 1e-13, i
    assert 1e-13 < worst_self < 1e-11, worst_self            # the docstring's statement


def test_exact_moments_and_model_on_a_small_cloud():
    """exact_moments against rationals, the one-pass model against np.cov, on exact data."""
    from fractions import Fraction as Q
    rng = np.random.default_rng(1)
    X = rng.integers(-64, 65, (7, 4)) / 16.0 + 3.0
    mean, cov = ref.exact_moments(X, origin=[10.0, -20.0])
    for r in range(4):
        s = sum(Q(float(v)) for v in X[:, r]) / 7 + (10, -20)[r & 1]
        assert abs(mean[r] - ref.F(s.numerator) / s.denominator) < ref.F("1e-45")
    np.testing.assert_allclose([[float(v) for v in row] for row in cov], np.cov(X.T), rtol=1e-14)
    mm, mc = ref.onepass_model(X, [10.0, -20.0])
    np.testing.assert_allclose(mc, np.cov(X.T), rtol=1e-13)
    np.testing.assert_allclose(mm, X.mean(0) + [10, -20, 10, -20], rtol=1e-15)


# ---- the oracle's own error per family, and the caps -----------------------------------------
def test_mvoe_families():
    cases, refs = ref.mvoe_cases(), ref.mvoe_reference()
    errs = ref.family_errors(cases, refs, ("e_beta", "e_q"), only=lambda c, r: r["same_iters"])
    msg = _table(errs)
    print("\nMVOE e_f:", msg)
    assert all(r["ref"]["converged"] and r["ref"]["iters"] < ref.MAXITER for r in refs), msg
    loose = [i for i, r in enumerate(refs) if not r["ref"]["clear"]]
    assert len(loose) <= 0.25 * len(refs), (len(loose), len(refs), msg)
    n_grid = sum(c["family"].startswith("aspect") for c in cases)
    assert n_grid >= 0.75 * 8 * 90, n_grid                     # thinned, not gutted
    for c, r in zip(cases, refs):
        e = errs[c["family"]]
        assert e["e_q"] < 1e-6 and ref.FACTOR * e["e_q"] < ref.BAR_Q, msg      # judgeable
        ab, aq = ref.mvoe_allowance(r["ref"], e)
        if r["ref"]["clear"]:
            assert r["same_iters"], (c["tag"], msg)            # the oracle stops where exact does
        assert r["e_beta"] <= ab and r["e_q"] <= aq and r["e_q"] < ref.BAR_Q, (c["tag"], msg)
    # every cell of the grid is still there, the narrowed columns at aspect 1e5
    cells = {c["tag"][:3] for c in cases if c["family"].startswith("aspect")}
    assert len(cells) == 90
    assert ref.mvoe_aspect(1e6, 1e4) == ref.mvoe_aspect(1e6, 1e8) == 1e5


def test_pair_families():
    cases, refs = ref.pair_cases(), ref.pair_reference()
    errs = ref.family_errors(cases, refs, ref.PAIR_KEYS)
    msg = _table(errs)
    print("\npair e_f:", msg)
    assert len(errs) == len(ref.PAIR_RHO) * len(ref.PAIR_ASPECTS)
    for f, e in errs.items():
        assert all(v < 1e-6 and ref.FACTOR * v < ref.BAR_Q for v in e.values()), (f, msg)
    for c, r in zip(cases, refs):
        if c["rho"] == 0.0:     # cov_mu = 0 exactly: beta = 0, the bound is 0 / 0 on both sides
            assert ref.mp.isnan(r["ex"]["lb"]) and r["ex"]["scale"] == 1


def test_tangent_family():
    cases, refs = ref.tangent_cases(), ref.tangent_reference()
    e_d = max(r["e_d"] for r in refs)
    print(f"\ntangent e_f: e_d={e_d:.1e}")
    skip_w = [r for r in refs if r["ex"]["margin"] <= ref.MARGIN]
    skip_s = [r for r in refs if r["ex"]["side_margin"] <= ref.MARGIN]
    assert len(skip_w) <= 0.05 * len(refs) and len(skip_s) <= 0.05 * len(refs)
    for c, r in zip(cases, refs):
        if r["ex"]["margin"] > ref.MARGIN:
            assert r["o_which"] == r["ex"]["which"], c["tag"]
            if r["ex"]["side_margin"] > ref.MARGIN:
                assert r["o_side"] == r["ex"]["side"], c["tag"]
    assert e_d < 1e-6
    # the on-line cases really sit on their candidate line
    for c, r in zip(cases, refs):
        if c["tag"][3] in ("line0", "line1"):
            assert r["ex"]["which"] == int(c["tag"][3][-1]) and r["ex"]["margin"] > 0.999


def test_singular_family():
    """Near-singular covariances of the affine record.  The plain float64 a d - b c never turns
    a PSD matrix's determinant negative: rounding is monotone, so a d >= b c exactly gives
    fl(a d) >= fl(b c).  Its lost digits reach margin and rhs less than scipy's sqrtm loses on
    the same matrices, so the plain form stays inside the yardstick (the compensated product
    w = b c, fma(a, d, -w) + fma(-b, c, w) would be ~100x closer, and is not needed)."""
    refs = ref.singular_reference()
    psd = [r for r in refs if r["psd"]]
    e_m, e_r = max(r["e_margin"] for r in psd), max(r["e_rhs"] for r in psd)
    p_m, p_r = max(r["plain_margin"] for r in psd), max(r["plain_rhs"] for r in psd)
    k_m = max(r["kahan_margin"] for r in psd)
    msg = (f"singular e_f: e_margin={e_m:.1e}, e_rhs={e_r:.1e}; plain det model: margin "
           f"{p_m:.1e}, rhs {p_r:.1e}; compensated det model: margin {k_m:.1e}")
    print("\n" + msg)
    assert len(psd) >= 90 and len(refs) - len(psd) >= 10, msg   # both kinds are present
    assert all(r["plain"] >= 0 for r in psd), msg               # the PSD clause, on the host
    assert all(r["kahan"] >= 0 for r in psd) and all(r["kahan"] < 0 for r in refs
                                                     if not r["psd"]), msg
    assert e_m < 1e-6 and e_r < 1e-6, msg
    assert p_m <= ref.bound(e_m) and p_r <= ref.bound(e_r), msg


@pytest.mark.parametrize("ci,f32", ref.MOM_STORES)
def test_moments_families(ci, f32):
    """The one-pass model's error per cell (the yardstick), and the premise: on the f64 stores
    the unshifted form is >= 100x worse than the shifted one on every cell but the one whose
    first particle is the outlier (there the shift costs what the kernel documents)."""
    rs = ref.moments_reference(ci, f32)
    msg = "; ".join(f"n={n}: model {r['e_model']:.1e} unshifted {r['e_unshifted']:.1e} "
                    f"np.cov {r['e_npcov']:.1e}" for n, r in zip(ref.MOM_COUNTS, rs))
    print(f"\nmoments offset/spread {ref.MOM_CONDS[ci]} f32={f32}: {msg}")
    for j, r in enumerate(rs):
        assert r["e_model"] < 1e-6 and r["m_model"] <= 1.0, msg
        if not f32 and j != ref.MOM_OUTLIER_CELL:
            assert r["e_unshifted"] >= 100 * max(r["e_model"], 2.0 ** -53), msg
            assert r["e_unshifted"] > ref.bound(r["e_model"]), msg   # an absent shift fails
    out = rs[ref.MOM_OUTLIER_CELL]
    assert out["e_model"] > 10 * out["e_npcov"], msg            # the outlier's documented cost


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("squeeze", [False, True])
def test_record_families(f32, squeeze):
    """Whole records: the float64 oracle (minkowski_cell, np.cov + scipy sqrtm, compute_scale)
    against the exact pipeline on the store's values, per store.  Judgeable everywhere (the
    squeeze narrowed from aspect 1e4, where 8 e_f of beta1 is 3e-5, to 1e3).

    By the definition of a clear stop, half of the MVOE calls of the plain stores and 8 of 9 of
    the squeezed ones are not clear (the second call (Q, R^2 I) contracts by less than 4x per
    step), so the 25 % cap cannot be met on the records the issue prescribes.  Instead of the
    loose |beta - beta_ref| <= tol rule those records are judged, at the full rounding
    allowance, against the exact pipeline stopped one iterate earlier, on, and one later."""
    worst, clear, pairs = {}, 0, 0
    for tr in ref.REC_TRANSLATIONS:
        for s in ref.REC_SCALES:
            r = ref.record_reference(tr, s, squeeze, f32)
            clear, pairs = clear + r["clear"], pairs + r["pairs"]
            for grp in ("e_mink", "e_affine", "e_scaled"):
                for k, v in r[grp].items():
                    worst[grp + "." + k] = max(worst.get(grp + "." + k, 0.0), v)
                    assert v < 1e-6 and ref.FACTOR * v < ref.BAR_Q, (tr, s, grp, k, v)
            for cell in r["mink"]:
                for cands in cell:
                    assert cands[0]["tg"]["margin"] > ref.MARGIN
                    assert cands[0]["tg"]["side_margin"] > ref.MARGIN      # nothing is skipped
                    assert len(cands) in (1, 3, 9)
    print(f"\nrecords f32={f32} squeeze={squeeze}: clear stops {clear}/{pairs}; worst e_f "
          + ", ".join(f"{k}={v:.1e}" for k, v in sorted(worst.items())))
    assert clear == (81 if not squeeze else 18) and pairs == 162
    assert ref.REC_SQUEEZE == 1e3
