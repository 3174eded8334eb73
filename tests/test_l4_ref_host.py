"""The L4 reference of the edge tests (tests/_l4_ref.py) against the golden-pinned oracle, and
the conditioning of the edge tests' inputs.  Host only."""
import numpy as np
import pytest

from oracle import ccmpc_oracle as orc

import _l4_ref as ref


def _scene():
    """2 OVs x 2 modes, 200 particles, T = 4: random walks away from the origin."""
    rng = np.random.default_rng(7)
    T, ovs, cells, pasts = 4, [], [], []
    for o in range(2):
        past = np.array([[40.0 + 30 * o, 25.0 - 60 * o]]) + rng.uniform(-1, 1, (1, 2))
        mine = []
        for k in range(2):
            h = rng.uniform(-np.pi, np.pi) + rng.normal(0, 0.4, (200, T))
            step = rng.uniform(1, 5, (200, T, 1)) * np.stack([np.cos(h), np.sin(h)], -1)
            mine.append(past[-1] + np.cumsum(step, axis=1))
        yaws = [orc._step_yaws(c, past[-1], T) for c in mine]
        ovs.append(orc.OVehicle(T, past, np.full(2, 0.5), mine, yaws,
                                np.array([c[:, T - 1].mean(0) for c in mine]),
                                np.array([4.5 + o, 2.5 - 0.5 * o])))
        cells += mine
        pasts += [past[-1]] * 2
    bbox = np.array([ov.bbox for ov in ovs for _ in range(2)])
    return T, ovs, cells, np.array(pasts), bbox


def test_reference_matches_oracle():
    T, ovs, cells, pasts, bbox = _scene()
    got = ref.reference(cells, pasts, bbox, heading="yaw")
    vert, A_u, b_u = orc.vertices_and_l4(ovs, T)
    (_, _, myaw), (_, _, vyaw) = orc.state_stats(ovs, T)
    j = 0
    for o, ov in enumerate(ovs):
        for k in range(ov.n_states):
            g = got[j]
            np.testing.assert_allclose(g["yaw"], orc._step_yaws(cells[j], pasts[j], T),
                                       rtol=1e-13, atol=0)
            np.testing.assert_allclose(g["yaw_mean"][0], myaw[o][k], rtol=1e-13)
            np.testing.assert_allclose(g["yaw0_var"], vyaw[o][k], rtol=1e-9)
            for t in range(T):
                np.testing.assert_allclose(g["vertices"][:, t], vert[t][k][o], rtol=1e-13)
                theta = np.mean(ov.pred_yaws[k][:, t])
                np.testing.assert_allclose(g["yaw_mean"][t], theta, rtol=1e-13)
                np.testing.assert_allclose(ref.A_of(theta), A_u[t][k][o], rtol=1e-13, atol=0)
                b, _ = ref.b_of(theta, g["vertices"][:, t])
                np.testing.assert_allclose(b, b_u[t][k][o], rtol=1e-13)
            # the exact unit vector is the heading's cos / sin to the rounding of the heading
            Cu, Su = ref.unit(g["d"])
            np.testing.assert_allclose(Cu.astype(float), np.cos(g["yaw"]), rtol=0, atol=4e-16)
            np.testing.assert_allclose(Su.astype(float), np.sin(g["yaw"]), rtol=0, atol=4e-16)
            j += 1


def test_reference_edge_values():
    assert np.isnan(ref.yaw0_var(np.array([0.3])))
    assert ref.yaw0_var(np.full(7, 0.3)) == 0.0
    C, S = ref.unit(np.array([[0.0, 0.0], [3e-160, 4e-160], [0.0, -2.0 ** -1074]]))
    assert (C[0], S[0]) == (1, 0) and (C[2], S[2]) == (0, -1)
    assert abs(float(C[1]) - 0.6) < 1e-16 and abs(float(S[1]) - 0.8) < 1e-16
    v = ref.vertices(np.zeros((1, 2)), np.array([0.6]), np.array([0.8]), 2.0, 0.0)
    np.testing.assert_array_equal(v[0, 0], [0.6, 0.8])       # corner 0 of a (2, 0) box: (C, S)


def test_split_premises_restated():
    """S and the chunk layout the split cases rely on, from the restated build knobs (the GPU
    tests assert the same premises against the library's workspace size)."""
    S = {n: ref.edge_scene(n, False)["S"] for n, sp, *_ in ref.EDGE_CASES if sp}
    assert S == dict(split_tail=2, split_empty=3, split_cap=64, split_4096=3, split_t40=1)
    assert ref.chunks(9000, 2)[0] == (0, 4500)               # > 2048: the tail loop runs
    assert ref.chunks(2, 3) == [(0, 1), (1, 2), (2, 2)]      # an empty chunk


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", [c[0] for c in ref.EDGE_CASES])
def test_edge_inputs_are_well_conditioned(name, f32):
    """float64 np.mean / np.var of the edge cases' headings sit within half the device tests'
    tolerances (rtol 1e-12 + atol 1e-13; rtol 1e-9) of the longdouble values, so a float64
    summation order cannot decide those tests; identical-delta cells have bit-identical t = 0
    headings; and the planted particles are the extremes the tests need."""
    sc, rf = ref.edge_scene(name, f32), ref.edge_reference(name, f32)
    hosted = set()
    for j, r in enumerate(rf):
        y, n = r["yaw"], r["yaw"].shape[0]
        assert np.all(np.abs(np.mean(y, axis=0) - r["yaw_mean"])
                      <= 0.5 * (1e-12 * np.abs(r["yaw_mean"]) + 1e-13))
        if n == 1:
            assert np.isnan(r["yaw0_var"])
        elif sc["family"][j] == "identical":
            assert np.all(y[:, 0] == y[0, 0]) and r["yaw0_var"] == 0.0
        else:
            assert abs(np.var(y[:, 0], ddof=1) - r["yaw0_var"]) <= 0.5e-9 * r["yaw0_var"]
        for t in range(sc["T"]):
            _, arg = ref.b_of(r["yaw_mean"][t], r["vertices"][:, t])
            hosted |= {ref.region_of(int(i), n, sc["S"]) for i in arg}
    want = {ref.region_of(i, n, sc["S"]) for n in sc["counts"]
            for i in ref.plant_candidates(n, sc["S"])}
    assert hosted >= want, (sorted(want - hosted), "regions that host no extreme")
