"""The NumPy restatement of the outer-approximation loop (tests/_socp_ref.py) on the instances
the GPU tests use: outcomes, rounds, monotone cost, and the KKT certificate of every returned
plan (host only).  SLSQP stalls on these cone programmes, so the certificate is the truth: the
primal max g and linear rows, non-negative least-squares multipliers over the active rows with
the gradients of g at the returned u, and the relative stationarity residual."""
import numpy as np
import pytest

import _socp_ref as sr

TOL_G = 1e-6


@pytest.fixture(scope="module")
def runs():
    out = {m: (sr.instance(m), sr.kelley(sr.instance(m), TOL_G))
           for m in sr.M_ACTIVE + (sr.M_FREE, sr.M_INFEASIBLE)}
    out["syn"] = (sr.synthetic(), sr.kelley(sr.synthetic(), TOL_G))
    return out


@pytest.mark.parametrize("m", sr.M_ACTIVE)
def test_one_active_row_converges_in_three_to_five_rounds(runs, m):
    prob, r = runs[m]
    assert r["status"] == sr.OK and 3 <= r["rounds"] <= 5
    assert r["viol"] <= TOL_G and r["viols"][0] > 1.0           # the reference point is inside
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(r["costs"], r["costs"][1:]))
    k = sr.kkt(prob, r["u"])
    print(f"m = {m}: rounds {r['rounds']}, viols {r['viols']}, kkt stat {k['stat']:.3e}")
    assert k["prim"] <= TOL_G and k["lin"] <= 1e-9
    assert len(k["strong_cone"]) == 1
    # the QP over the cuts is solved exactly, so what is left of stationarity is the multiplier
    # times the turn of the active row's gradient between its last cut and u: it shrinks with
    # the tolerance
    tight = sr.kelley(prob, TOL_G / 1000)
    kt = sr.kkt(prob, tight["u"])
    assert tight["status"] == sr.OK and kt["stat"] <= k["stat"] and kt["stat"] <= 1e-4
    assert np.max(np.abs(tight["u"] - r["u"])) <= 1e-2


def test_violation_sequence_of_the_six_metre_shift(runs):
    """1.0 / 1.3e-2 / 7e-5 / 9e-7 after the QPs of rounds 1..4 (to a factor of two)."""
    _, r = runs[6.0]
    for got, want in zip(r["viols"][1:], (1.0, 1.3e-2, 7e-5, 9e-7)):
        assert want / 2 <= got <= want * 2, r["viols"]


def test_no_active_row_is_the_plain_qp(runs):
    from oracle import mpc_oracle as mo
    prob, r = runs[sr.M_FREE]
    assert r["status"] == sr.OK and r["rounds"] == 1 and r["viol"] < -1.0
    H, f, k, G, h = mo.assemble_qp(prob["Gf"], prob["c"], prob["T"], prob["goal"], prob["ref"],
                                   [], sr.PARAMS)
    u, _, _ = mo.solve_qp(H, f, G, h)
    assert np.max(np.abs(u - r["u"])) <= 1e-9
    assert sr.kkt(prob, r["u"])["strong_cone"] == []


def test_unshifted_reference_is_infeasible_in_the_second_round(runs):
    _, r = runs[sr.M_INFEASIBLE]
    assert r["status"] == sr.INFEASIBLE and r["rounds"] == 2
    assert 4.0 < r["viols"][1] < 5.0                             # 4.38 after the first QP


def test_synthetic_scene_has_active_rows_of_both_cells(runs):
    prob, r = runs["syn"]
    assert r["status"] == sr.OK and r["viol"] <= TOL_G
    k = sr.kkt(prob, r["u"])
    print(f"synthetic: rounds {r['rounds']}, viols {r['viols']}, strong {k['strong_cone']}")
    assert k["prim"] <= TOL_G and k["lin"] <= 1e-9 and k["stat"] <= 1e-3
    assert {ov for ov, _, _ in k["strong_cone"]} == {0, 1}
    assert len({t for _, _, t in k["strong_cone"]}) >= 2


def test_cut_supports_and_underestimates():
    prob = sr.instance(6.0)
    rng = np.random.default_rng(3)
    for r in prob["rows"][:4]:
        p = prob["ref"][r["t"]]
        g, a, b = sr.row_cut(r, p)
        assert g == sr.row_g(r, p)
        assert abs(a @ p - b - g) <= 64 * 2.0 ** -52 * (abs(b) + abs(g))
        for q in p + rng.uniform(-30, 30, size=(50, 2)):
            assert a @ q - b <= sr.row_g(r, q) + 1e-9
