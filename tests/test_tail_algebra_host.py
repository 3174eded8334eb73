"""compute_mvoe's operation order (constraints.hpp: the set-up from trace and determinant, the
loop, Q), restated in float64 NumPy (tests/_tail_algebra.py) and judged against the exact
reference of tests/_tail_ref.py with the allowances of tests/test_gpu_tail_precision.py.  Host
only; the device's own figures are in tests/test_gpu_tail_algebra.py.

Figures of the host model (this file prints them):
  MVOE grid, 644 cases, 536 clear stops: 0 outside mvoe_allowance, 0 stop iterates off.
  worst on clear stops, beta / Q     LU + eigenvalue form      trace / determinant form
    aspect 1e3                       4.8e-11 / 4.9e-12         2.1e-14 / 2.5e-15
    aspect 1e6 (1e5 in two columns)  4.8e-07 / 1.3e-08         1.0e-11 / 9.2e-13
  goldens (mvoe.npz): Q 1.4e-14, beta 1.7e-13.
"""
import numpy as np

import _tail_algebra as alg
import _tail_ref as ref


def _grid(form):
    """Per case of mvoe_cases(): (case, exact, model result, beta error, Q error)."""
    out = []
    for c in ref.mvoe_cases():
        ex = c["ref"]
        m = alg.mvoe(c["S1"], c["S2"], form)
        out.append((c, ex, m, ref.rel(m["beta"], ex["beta"]), ref.rel_fro(m["Q"], ex["Q"])))
    return out


def _worst(rows, family):
    sel = [(eb, eq) for c, ex, m, eb, eq in rows if c["family"] == family and ex["clear"]]
    return max(e[0] for e in sel), max(e[1] for e in sel)


def test_trace_determinant_form_on_the_whole_grid():
    """Every case of mvoe_cases(), none left out: within mvoe_allowance of the exact result,
    and on every clear stop the iterate the exact iteration stops on."""
    cases, refs = ref.mvoe_cases(), ref.mvoe_reference()
    errs = ref.family_errors(cases, refs, ("e_beta", "e_q"), only=lambda c, r: r["same_iters"])
    rows = _grid("trdet")
    assert len(rows) == len(cases)
    bad, off, clear = [], [], 0
    for c, ex, m, eb, eq in rows:
        ab, aq = ref.mvoe_allowance(ex, errs[c["family"]])
        if not (eb <= ab and eq <= aq and eq < ref.BAR_Q):
            bad.append((c["tag"], ex["clear"], eb, ab, eq, aq))
        if ex["clear"]:
            clear += 1
            if m["iters"] != ex["iters"]:
                off.append((c["tag"], m["iters"], ex["iters"]))
    print(f"\n{len(rows)} cases, {clear} clear stops, {len(bad)} outside the allowance, "
          f"{len(off)} stop iterates off; worst beta / Q on clear stops: "
          + "; ".join(f"{f}: {b:.1e} / {q:.1e}" for f in sorted({c['family'] for c in cases})
                      for b, q in [_worst(rows, f)]))
    assert not bad, (bad[:5], len(bad))
    assert not off, off[:5]


def test_lu_form_is_a_hundred_times_further_at_aspect_1e6():
    """The premise of the accuracy claim: on the aspect-1e6 family the LU + eigenvalue order,
    restated the same way, is >= 100x further from the exact Q than the trace / determinant
    order (it forms l2 = tr / 2 - sqrt(disc), which cancels at high aspect)."""
    lu, td = _worst(_grid("lu"), "aspect1e+06"), _worst(_grid("trdet"), "aspect1e+06")
    print(f"\naspect 1e6, worst on clear stops, beta / Q: LU form {lu[0]:.1e} / {lu[1]:.1e}, "
          f"trace / determinant form {td[0]:.1e} / {td[1]:.1e}")
    assert lu[1] >= 100.0 * td[1], (lu, td)


def test_trace_determinant_form_on_the_goldens(golden):
    g = golden("mvoe")
    wq = wb = 0.0
    for i in range(len(g["beta"])):
        m = alg.mvoe(g["S1"][i], g["S2"][i])
        wq = max(wq, float(np.linalg.norm(m["Q"] - g["Q"][i].reshape(4))
                           / np.linalg.norm(g["Q"][i])))
        wb = max(wb, abs(float(m["beta"]) - float(g["beta"][i])) / abs(float(g["beta"][i])))
    print(f"\nmvoe.npz: worst Q {wq:.1e}, worst beta {wb:.1e}")
    assert wq < 1e-9 and wb < 1e-8, (wq, wb)


def test_wide_columns_have_their_clear_stops():
    """The draws of the GPU test's un-narrowed columns: 8 clear stops per scale within 16."""
    cases = alg.wide_cases()
    for sc in alg.WIDE_SCALES:
        assert sum(c["scale"] == sc for c in cases) == alg.WIDE_CLEAR, sc
