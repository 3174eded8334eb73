"""The premises of the face audit's GPU tests, checked on the host: on the tests' inputs no v_f
lies in the band where rounding could change its sign (so the device counts can be demanded
exactly), the relative form equals the records' a_f . (X, Y, 1) + 0.5 car_r, and the tie case
holds exact zeros with neighbours one ulp to either side (host only; no device work)."""
import numpy as np
import pytest

import _face_audit_ref as ar
from _faces_ref import CAR_R, LAT, LON, coefficients
from _l4_ref import LD, step_deltas, store_world, unit

EPS = 2.0 ** -52
CASES = [(T, f32) for T in ar.HORIZONS for f32 in (False, True)]


@pytest.mark.parametrize("T,f32", CASES)
def test_ambiguous_band_is_empty(T, f32):
    ref = ar.reference(T, f32)
    smallest, own = np.inf, 0.0
    hlon = 0.5 * LON + 0.5 * CAR_R
    for r in ref:
        if not r["vld"].shape[0]:
            continue
        scale = 1 + np.abs(r["ex"]) + np.abs(r["ey"])
        assert np.all(np.abs(r["vld"]) > ar.BAND * scale[..., None])
        assert np.array_equal(r["v64"] > 0, r["vld"] > 0)
        smallest = min(smallest, float(np.abs(r["vld"]).min()))
        rel = np.abs(r["v64"].astype(LD) - r["vld"]) / (scale - 1 + hlon)[..., None]
        own = max(own, float(rel.max()))
    print(f"T={T} f32={f32}: smallest |v_f| {smallest:.3g} m, float64 restatement error "
          f"{own:.3g}")
    assert own < 64 * EPS


def test_counts_are_mixed():
    """The plan rows stand near a corner of the inflated box: open and closed particles in most
    (cell, t, face), some in the box and some not."""
    ref = ar.reference(8, False)
    big = ref[-1]["want"]
    n = ref[-1]["v64"].shape[0]
    assert np.sum((big["face_open"] > 0) & (big["face_open"] < n)) >= 8
    assert np.any((big["in_box"] > 0) & (big["in_box"] < n))
    for T in ar.HORIZONS:
        some = [r for r in ar.reference(T, False) if r["v64"].shape[0] > 60]
        assert any(0 < r["want"]["in_box_any"] < r["v64"].shape[0] for r in some), T
        assert any(0 < r["want"]["sel_open_any"] < r["v64"].shape[0] for r in some), T
    inp = ar.inputs(8, False)
    assert np.all(inp["face_sel"][inp["counts"].index(2)] == -1)
    assert {-1, 0, 1, 2, 3} <= set(inp["face_sel"].reshape(-1).tolist())


@pytest.mark.parametrize("T,f32", CASES)
def test_relative_form_is_the_records_definition(T, f32):
    inp = ar.inputs(T, f32)
    ref = ar.reference(T, f32)
    world = store_world(inp["cells"], bool(f32), inp["origin"])
    for j, w in enumerate(world):
        if not w.shape[0]:
            continue
        row = inp["plan"][inp["cell_plan"][j]]
        C_, S_ = unit(step_deltas(w, inp["past"][j]))
        x, y = w[..., 0].astype(LD), w[..., 1].astype(LD)
        for t in range(T):
            X, Y = LD(row[t, 0]), LD(row[t, 1])
            A = coefficients(x[:, t], y[:, t], C_[:, t], S_[:, t], LD(LON), LD(LAT))
            for f, a in enumerate(A):
                val = a[0] * X + a[1] * Y + a[2] + LD(0.5) * LD(CAR_R)
                # the magnitudes of the expression's terms, a[2] split into its own three
                c, s = C_[:, t], S_[:, t]
                own = (np.abs(c * x[:, t]) + np.abs(s * y[:, t]) + LD(LAT) / 2 if f % 2 == 0
                       else np.abs(s * x[:, t]) + np.abs(c * y[:, t]) + LD(LON) / 2)
                mag = np.abs(a[0] * X) + np.abs(a[1] * Y) + own + LD(0.5) * LD(CAR_R)
                assert np.all(np.abs(val - ref[j]["vld"][:, t, f]) <= 64 * EPS * mag), (j, t, f)


def test_tie_case_is_exact_and_strict():
    cells, past, plan, expect = ar.tie_case()
    v, _, _ = ar.values(cells[0], past[0], plan[0], ar.TIE_EXTENT, ar.TIE_CAR_R)
    vld, ex, ey = ar.values(cells[0], past[0], plan[0], ar.TIE_EXTENT, ar.TIE_CAR_R, ld=True)
    assert np.array_equal(v[:, 1].astype(LD), vld[:, 1])          # t = 1: every operation exact
    for f, (neg, zero, pos) in expect.items():
        assert v[zero, 1, f] == 0.0
        assert v[neg, 1, f] < 0.0 and v[pos, 1, f] > 0.0
        assert abs(v[neg, 1, f]) <= 2.0 ** -49 and abs(v[pos, 1, f]) <= 2.0 ** -49
    want = ar.tally(v)
    # of the three particles built for face f only one is open under it; the nine built for the
    # other faces stand at ex = 0 or ey = 0 or on the far side
    for f in range(4):
        others = int(np.sum(np.delete(v[:, 1, f], list(expect[f])) > 0))
        assert want["face_open"][1, f] == others + 1
    # t = 0 (headings from past_last): nothing near a tie
    scale = 1 + np.abs(ex[:, 0]) + np.abs(ey[:, 0])
    assert np.all(np.abs(vld[:, 0]) > ar.BAND * scale[:, None])
    assert np.array_equal(v[:, 0] > 0, vld[:, 0] > 0)
