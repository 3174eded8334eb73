"""The oracle of the box-face constraints (tests/_faces_ref.py) against the reference's own
generator bodies (tests/golden/faces_*.npz, recorded by tests/golden/make_golden_faces.py), and
its two restatements against each other.  Host only."""
import numpy as np
import pytest

import _faces_ref as fr

SCENES = ("faces_o2_t8", "faces_o3_t12")
VARIANTS = ("nominal", "robust", "approx")


scene_cells = fr.scene_cells


@pytest.fixture(scope="module", params=SCENES)
def scene(request, golden):
    g = golden(request.param)
    return (g,) + scene_cells(g)


def test_fixture_has_an_ov_on_each_side_of_the_junction_test(scene):
    g, T, K, cells, yaws = scene
    gate = fr.in_junction(cells)
    assert any(gate) and not all(gate)
    for cs in cells:                      # clear of the thresholds
        for c in cs:
            m = c[:, 0].mean(0)
            assert abs(m[0] - 190) > 5 and abs(m[1] + 80) > 5


@pytest.mark.parametrize("variant", VARIANTS)
def test_float64_restatement_reproduces_the_reference_rows(scene, variant):
    g, T, K, cells, yaws = scene
    rows, _ = fr.generator_rows(cells, yaws, g["eps_ura"], T, T, variant, g["ref_traj"])
    seq = g[f"{variant}_seq"]
    assert [0 if r["face"] >= 0 else 1 for r in rows] == list(seq)
    gate = fr.in_junction(cells)
    assert bool(g[f"{variant}_ovconstraint"]) == any(gate)
    okt = g[f"{variant}_okt"]
    face_rows = [r for r in rows if r["face"] >= 0]
    assert len(face_rows) == len(g[f"{variant}_face"])
    if variant != "approx":
        assert [(r["ov"], r["k"], r["t"]) for r in rows] == [tuple(x) for x in okt]
        assert sorted({int(o) for o in okt[:, 0]}) == [o for o, f in enumerate(gate) if f]
    else:
        assert [r["t"] for r in rows] == list(okt[:, 2])
        assert len(rows) == sum(K[o] for o, f in enumerate(gate) if f) * T
    # (face, the approx choice) exactly; mean, root / scalar, Gamma to rtol 1e-12
    assert [r["face"] for r in face_rows] == list(g[f"{variant}_face"])
    want_gamma = g["gamma"]
    for i, r in enumerate(face_rows):
        np.testing.assert_allclose(r["gamma"], want_gamma[r["ov"], r["k"]], rtol=1e-12)
        np.testing.assert_allclose(r["mean"][:2], g[f"{variant}_mean"][i][:2], rtol=1e-12)
        np.testing.assert_allclose(r["mean"][2] + 0.5 * fr.CAR_R, g[f"{variant}_const"][i],
                                   rtol=1e-12)
        M = g[f"{variant}_root"][i]
        if variant == "robust":
            np.testing.assert_array_equal(M, np.eye(3))
            np.testing.assert_allclose(r["gamma"] * r["s"], g["robust_coef"][i], rtol=1e-12)
        else:
            np.testing.assert_allclose(g[f"{variant}_coef"][i], r["gamma"], rtol=1e-12)
            assert np.linalg.norm(r["root"] - M) <= 1e-12 * np.linalg.norm(M)


def test_state_statistics(scene):
    g, T, K, cells, yaws = scene
    m, v = fr.state_stats(cells, yaws)
    for variant in VARIANTS:
        np.testing.assert_allclose(m, g[f"{variant}_state_mean"], rtol=1e-12)
        np.testing.assert_allclose(v, g[f"{variant}_state_cov"], rtol=1e-12)


def test_longdouble_restatement_agrees_with_float64(scene):
    """Per (cell, t, face): means to rtol 1e-12; the float64 np.cov against the longdouble
    covariance of the same coefficients, max |dC_ij| / sqrt(C_ii C_jj) <= 1e-13 (printed)."""
    g, T, K, cells, yaws = scene
    worst = 0.0
    for o, (cs, ys) in enumerate(zip(cells, yaws)):
        for c, y in zip(cs, ys):
            f = fr.cell_f64(c, y, 2.0, "nominal", g["ref_traj"])
            Cl = fr.cell_ld_yaw(c, y)
            worst = max(worst, fr.scaled_cov_error(f["C"], Cl))
            # the exact unit vector against cos / sin of the float64 yaw: the same constraint
            past = g["past"][o]
            l = fr.cell_ld(c, past, 2.0, "nominal", g["ref_traj"])
            np.testing.assert_allclose(f["mean"], l["mean"].astype(float), rtol=1e-12)
            assert fr.scaled_cov_error(f["C"], l["C"]) <= 1e-12
            for t in range(T):
                for k in range(4):
                    R = l["root"][t, k]
                    assert np.linalg.norm((R @ R - l["C"][t, k]).astype(float)) <= (
                        1e-17 * np.linalg.norm(l["C"][t, k].astype(float)))
                    assert (np.linalg.norm(f["root"][t, k] - R.astype(float))
                            <= 1e-11 * np.linalg.norm(f["root"][t, k]))
            assert np.array_equal(f["chosen"], l["chosen"])
            r64 = fr.cell_f64(c, y, 2.0, "robust")
            rld = fr.cell_ld(c, past, 2.0, "robust")
            np.testing.assert_allclose(r64["s"], rld["s"].astype(float), rtol=1e-12)
    print(f"worst scaled covariance error of float64 np.cov: {worst:.2e}")
    assert worst <= 1e-13


def test_mirror_relations():
    """a3 = -a1 + (0, 0, lat), a4 = -a2 + (0, 0, lon): what lets the kernel reduce two families."""
    rng = np.random.default_rng(5)
    c = fr.cloud(rng, 40, 3)
    past = c[0, 0] - 1.0
    l = fr.cell_ld(c, past, 2.0, "nominal")
    for t in range(3):
        for f, ext in ((0, fr.LAT), (1, fr.LON)):
            np.testing.assert_allclose(
                (l["mean"][t, f + 2] + l["mean"][t, f]).astype(float), [0, 0, ext], atol=1e-15)
            assert fr.scaled_cov_error(l["C"][t, f + 2], l["C"][t, f]) <= 1e-17


def test_test_inputs_are_what_the_gpu_tests_assume():
    for T in (1, 2, 8, 12):
        for f32 in (False, True):
            inp = fr.inputs(T, f32)
            ch = fr.CHUNK[f32]
            assert inp["counts"] == [2, 3, 5, 63, 64, 1, 65, 255, 257, ch + 1, 2 * ch + 3]
            assert np.array_equal(inp["cells"][4][11, 0], inp["past"][4])
            if T > 1:
                tz = min(3, T - 1)
                assert np.array_equal(inp["cells"][3][7, tz], inp["cells"][3][7, tz - 1])
            assert len(set(inp["cell_ref"])) == len(inp["cells"])     # every cell its own row
            assert not np.array_equal(inp["cell_ref"], np.arange(len(inp["cells"])))


def test_constructed_tie_is_exact_in_float64():
    """The approx tie case of the GPU test: the float64 restatement on the kernel's unit-vector
    headings (exact for axis-parallel unit steps) ties too, and picks the lower index."""
    from _l4_ref import step_deltas, unit
    cells, past, ref = fr.tie_case()
    C, S = unit(step_deltas(cells, past))
    f = fr.cell_f64(cells, None, 2.0, "robust", ref, lon=fr.TIE_EXTENT[0], lat=fr.TIE_EXTENT[1],
                    cs=(C.astype(float), S.astype(float)))
    v = f["val"][1]
    assert v[0] == v[1] and v[0] < v[2] and v[0] < v[3]
    assert f["chosen"][1] == 0
    l = fr.cell_ld(cells, past, 2.0, "robust", ref, lon=fr.TIE_EXTENT[0], lat=fr.TIE_EXTENT[1])
    assert l["val"][1, 0] == l["val"][1, 1] and l["chosen"][1] == 0
