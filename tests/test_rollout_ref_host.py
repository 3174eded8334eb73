"""The exact reference of the rollout-precision tests (tests/_rollout_ref.py) against the
golden rollout and the oracle, the float64 oracle's own error on every input family of
tests/test_gpu_rollout_precision.py (the yardstick of those tests), the zero cap on instances
left out, and the proof that the shared comparison functions see a subtly wrong build_step.
Host only; run with -s for the per-family figures."""
import numpy as np
import pytest

import _rollout_ref as ref


def _golden_inputs(g):
    T_src = g["mean"].shape[1]
    cov = np.zeros((2, 2 * T_src, 2 * T_src))
    for k in range(2):
        for t in range(T_src):
            cov[k, 2 * t:2 * t + 2, 2 * t:2 * t + 2] = g["cov"][k][t]
            for tau in range(t):
                cov[k, 2 * t:2 * t + 2, 2 * tau:2 * tau + 2] = g["xcov"][k][t][tau]
                cov[k, 2 * tau:2 * tau + 2, 2 * t:2 * t + 2] = g["xcov"][k][t][tau].T
    Z = np.ascontiguousarray(np.asarray(g["Z"]).transpose(0, 1, 3, 2))        # [c][t][2][n]
    return dict(mean=np.asarray(g["mean"]), cov=cov, src=(0, 1), x0=np.asarray(g["x0"]), Z=Z)


def test_exact_rollout_reproduces_golden_and_oracle(golden):
    """The benign family (random walk, condition number ~1): the golden trajectories, the oracle
    run afresh and the NumPy model of the kernel all sit within 1e-12 of the exact rollout; the
    mpmath and the np.longdouble recursion agree to 1e-17 of the largest deviation."""
    g = golden("ideal_rollout")
    inp = _golden_inputs(g)
    T = g["traj"].shape[2]
    centre, dev = ref.exact_rollout(T=T, arith="mp", **inp)
    exact = (centre[:, None].astype(ref.LD) + dev).astype(float)
    np.testing.assert_allclose(g["traj"], exact, rtol=1e-12)
    again = ref.oracle_rollout(inp, T)
    np.testing.assert_allclose(again, exact, rtol=1e-12)
    np.testing.assert_array_equal(again, g["traj"])
    assert ref.traj_error(g["traj"], (centre, dev)) < 1e-12
    assert ref.traj_error(ref.kernel_rollout_f64(T=T, **inp), (centre, dev)) < 1e-12
    _, dev_ld = ref.exact_rollout(T=T, arith="ld", **inp)
    assert float(np.max(np.abs(dev_ld - dev)) / np.max(np.abs(dev))) < 1e-17


def test_exact_sample_moments_on_exact_data():
    """Dyadic deviations: the sums are exact in float64, so np.mean / np.cov are the answer to
    a few ulp of the largest entry (the division by n = 7 is not exact)."""
    rng = np.random.default_rng(3)
    dev = (rng.integers(-64, 65, (2, 7, 3, 2)) / 16.0).astype(ref.LD)
    centre = np.tile(np.array([190.0, -133.0]), (2, 3, 1))
    dmean, cov = ref.exact_sample_moments((centre, dev))
    X = centre[:, None] + dev.astype(float)
    m, c = ref.oracle_moments(X)
    np.testing.assert_allclose((centre.reshape(2, -1) + dmean).astype(float), m.reshape(2, -1),
                               rtol=1e-15)
    np.testing.assert_allclose(cov.astype(float), c, rtol=1e-13, atol=1e-14)
    em, ec = ref.moment_errors(m, c, (centre, dev), (dmean, cov))
    assert em < 1e-13 and ec < 1e-13


@pytest.mark.parametrize("kappa,q", ref.GRID)
def test_every_instance_of_the_grid_is_judged(kappa, q):
    """Zero cap: on every family the oracle succeeds on every instance and every instance's
    exact lambda_min(K) / |N|_F is positive -- nothing is left out of the GPU test.  The
    family's oracle errors (the yardstick) are printed; the NumPy model of build_step stays
    inside the allowance they give."""
    r = ref.plan_reference(kappa, q)
    S, N, C = ref.plan_instances(kappa, q)
    A, L = ref.kernel_plan_f64(S, N, C)
    mA, mL = ref.plan_errors(A, L, r)
    print(f"\nplans kappa={kappa:g} q={q:g}: n={len(S)} lam_min={r['lam'].min():.2e} "
          f"oracle e_A={r['e_A']:.2e} e_L={r['e_L']:.2e}  f64 model e_A={mA.max():.2e} "
          f"e_L={mL.max():.2e}  ratio {mA.max() / r['e_A']:.2f} {mL.max() / r['e_L']:.2f}")
    assert len(S) >= 600
    assert r["oracle_fail"] == []
    assert np.all(r["lam"] > 0)
    assert np.all(np.isfinite(r["eA"])) and np.all(np.isfinite(r["eL"]))
    assert r["e_A"] < 1e-6 and r["e_L"] < 1e-3          # a yardstick, not a blank cheque
    assert mA.max() <= ref.bound(r["e_A"]) and mL.max() <= ref.bound(r["e_L"])


@pytest.mark.parametrize("kappa,q", ref.TRAJ_FAMILIES)
def test_trajectory_yardstick(kappa, q):
    for off in ref.OFFSETS:
        sc = ref.traj_scene(kappa, q, off, 9, 5)
        ex = ref.exact_rollout(T=3, **sc)
        e_o = ref.traj_error(ref.oracle_rollout(sc, 3), ex)
        e_m = ref.traj_error(ref.kernel_rollout_f64(T=3, **sc), ex)
        print(f"\ntrajectories kappa={kappa:g} q={q:g} offset={off:g}: oracle {e_o:.2e} "
              f"f64 model {e_m:.2e}")
        assert e_o < 1e-6 and e_m <= ref.bound(e_o)


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_mutation_exceeds_the_allowance(mutation):
    """Each subtly wrong build_step / advance, as a mutation of the NumPy model, through the
    comparison functions of the GPU test (the plan read-out and a (9, 3, 5) trajectory run), on
    every kappa = 1 family: it must land outside the allowance in at least one of them.
    K_upper is invisible on symmetric inputs (see _rollout_ref) and runs on the asym variant,
    on which the unmutated model must stay inside."""
    asym = mutation == "K_upper"
    for q in ref.QS:
        r = ref.plan_reference(1.0, q, asym)
        inp = ref.readout_inputs(1.0, q, asym)
        sc = ref.traj_scene(1.0, q, 190.0, 9, 5)
        ex = ref.exact_rollout(T=3, **sc)
        allow_t = ref.bound(ref.traj_error(ref.oracle_rollout(sc, 3), ex))
        seen = {}
        for m in (None, mutation):
            A, L = ref.readout_plan(ref.kernel_rollout_f64(T=1, mutate=m, **inp))
            eA, eL = ref.plan_errors(A, L, r)
            et = ref.traj_error(ref.kernel_rollout_f64(T=3, mutate=m, **sc), ex)
            seen[m] = (eA.max() > ref.bound(r["e_A"]), eL.max() > ref.bound(r["e_L"]),
                       et > allow_t)
            print(f"\n{m} q={q:g}: e_A={eA.max():.2e} e_L={eL.max():.2e} traj={et:.2e}")
        assert not any(seen[None]), (q, seen)
        assert any(seen[mutation]), (q, seen)
        assert r["oracle_fail"] == [] and np.all(r["lam"] > 0)
