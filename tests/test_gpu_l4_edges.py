"""The L4 kernels (l4_kernel, l4_pass1_kernel, l4_pass2_kernel) against the longdouble
reference of tests/_l4_ref.py: the heading cos / sin read out bit-exactly at ulp level, and
both forms at the cell sizes where their code paths change, with b's extremes planted on every
path, padding columns and the split form's workspace checked."""
import numpy as np
import pytest
import torch

import _l4_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77          # pre-fill of out_yaw / out_vertices


def _store(cells, gpu, f32, origin=None, capacity=None):
    from ccmpc import engine
    return engine.ParticleStore.from_cells(
        cells, device=gpu, dtype=torch.float32 if f32 else torch.float64, origin=origin,
        capacity=capacity)


def _bits(t):
    return t.contiguous().view(torch.int64)


# ---------------------------------------------------------------------------------------------
# heading accuracy
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_heading_cos_sin_within_4_units(gpu, f32):
    """C, S of heading_cs_rsq, read bit-exactly as corner 0 of a (lon, lat) = (2, 0) box at
    the origin (T = 2, pos_0 = -d, pos_1 = 0: the step-1 delta is d and the corner is (C, S)
    with no rounding), against the exact unit vector d / |d|:
        |got - exact| <= 4 * 2^-52 * |exact| + 2^-1022   for every point.
    The factor is the code's rounding analysis (n2: 1 unit halved by the inverse square root,
    the Newton update's three roundings 1.25, the product 0.5: 2.25), not a device figure.
    Three copies of the points in one cell: each point meets the one-workgroup form's cached
    path (first copy) and its re-reading path (third copy), and the copies spread over the
    split form's preloaded and tail paths; the two forms must agree bit for bit.  Measured figures (units of 2^-52) are printed: DESIGN.md 4.5 quotes them."""
    fam = ref.heading_points(f32)
    names = list(fam)
    d1 = np.concatenate([fam[k] for k in names])
    which1 = np.concatenate([np.full(len(fam[k]), i) for i, k in enumerate(names)])
    d, which = np.tile(d1, (3, 1)), np.tile(which1, 3)
    n = len(d)
    cell = np.zeros((n, 2, 2))
    cell[:, 0] = 0.0 - d
    cells = [cell, np.zeros((1, 2, 2))]           # a 1-particle cell: S from the average cell
    store = _store(cells, gpu, f32, origin=np.zeros((2, 2)) if f32 else None)
    assert len(d1) < ref.ONE_WG_CACHED and n > ref.ONE_WG_CACHED + len(d1)
    S = ref.split_factor(2, store.n_bound)
    i0, i1 = ref.chunks(n, S)[0]
    assert S > 1 and i1 - i0 > ref.SPLIT_PRELOADED + 512, "split form: no tail loop"
    past, bbox = np.zeros((2, 2)), np.tile([2.0, 0.0], (2, 1))
    got = {}
    for form, split in (("one", False), ("split", True)):
        out = ref.run_l4(store, past, bbox, split)
        v = out["vertices"][8:10, :n].cpu().numpy()
        got[form] = (v[0], v[1], out["yaw"][1, :n].cpu().numpy())
    Ce, Se = ref.unit(d)
    tiny = np.longdouble(ref.TINY)
    bad = []
    for form, (C, S_, y) in got.items():
        for nm, g, e in (("C", C, Ce), ("S", S_, Se)):
            err = np.abs(g.astype(np.longdouble) - e)
            over = err > 4 * ref.U * np.abs(e) + tiny
            rel = (np.maximum(err - tiny, 0) / np.where(e == 0, 1, np.abs(e)) / ref.U)
            for i, k in enumerate(names):
                m = which == i
                print(f"L4 heading {'f32' if f32 else 'f64'} {form:5s} {nm} {k:13s} "
                      f"max err {float(rel[m].max()):6.3f} x 2^-52  ({int(over[m].sum())} of "
                      f"{int(m.sum())} over the bound)")
            bad += [(form, nm, tuple(d[i]), float(g[i]), float(e[i]), float(rel[i]))
                    for i in np.flatnonzero(over)[:8]]
    assert not bad, bad
    zero = np.flatnonzero((d[:, 0] == 0) & (d[:, 1] == 0))
    assert len(zero) == 3
    for form, (C, S_, y) in got.items():
        assert np.all(C[zero] == 1.0) and np.all(S_[zero] == 0.0), form
        m = (which == names.index("random")) | (which == names.index("near_axis"))
        np.testing.assert_allclose(y[m], np.arctan2(d[m, 1], d[m, 0]), rtol=1e-13, atol=1e-14)
    for a, b in zip(got["one"], got["split"]):
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))


# ---------------------------------------------------------------------------------------------
# edge shapes
# ---------------------------------------------------------------------------------------------
def _premises(name, sc, store, lib):
    """What the case is there for, asserted: a changed build knob fails here."""
    C, T = store.n_cells, store.T
    if not sc["split"]:
        assert sc["S"] is None
        return
    S = ref.split_factor(C, store.n_bound)
    assert S == sc["S"]
    # the library's own S, through its workspace size: counters, 2 x [C T][S][4], [C T][2]
    head = -(-2 * C * T * 4 // 256) * 256
    body = head + 2 * C * T * S * 32 + C * T * 16
    assert lib.ccmpc_l4_workspace_bytes(T, C, store.n_bound) == -(-body // 256) * 256
    ch = [ref.chunks(n, S) for n in sc["counts"]]
    empty = sum(i1 <= i0 for c in ch for i0, i1 in c)
    if name == "split_tail":
        assert S == 2 and ch[0][0][1] - ch[0][0][0] > ref.SPLIT_PRELOADED
    elif name == "split_empty":
        assert S == 3 and ch[1][2][1] <= ch[1][2][0]
    elif name == "split_cap":
        assert S == ref.SPLIT_MAX == 64 and empty > 0.5 * S * C
    elif name == "split_4096":
        assert S == 3
    elif name == "split_t40":
        assert T == 40


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", [c[0] for c in ref.EDGE_CASES])
def test_l4_edge_shapes(gpu, name, f32):
    """Every t, particle and corner of an edge case against the reference (tolerances: the
    project's own, test_gpu_fused.py / test_gpu_planner.py).  A and b are judged at the
    kernel's own returned mean heading, the mean on its own; b two-sided, so a dropped or
    mis-indexed extreme shows (the extremes sit on the edges of every code-path region,
    _l4_ref.edge_scene).  Padding columns of yaw / vertices keep their pre-fill bit for bit;
    the split form leaves its counters at zero and reads nothing else stale from its
    workspace."""
    from ccmpc import _lib
    lib = _lib.load()
    sc, rf = ref.edge_scene(name, f32), ref.edge_reference(name, f32)
    store = _store(sc["cells"], gpu, f32, origin=sc["origin"], capacity=sc["capacity"])
    T, C, ld = store.T, store.n_cells, store.ld
    _premises(name, sc, store, lib)

    def prefilled():
        return (torch.full((T, ld), SENTINEL, dtype=torch.float64, device=gpu),
                torch.full((8 * T, ld), SENTINEL, dtype=torch.float64, device=gpu))

    ws = None
    if sc["split"]:
        need = lib.ccmpc_l4_workspace_bytes(T, C, store.n_bound)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)
        ws[:2 * C * T * 4] = 0
    oy, ov = prefilled()
    out = ref.run_l4(store, sc["past_last"], sc["bbox"], sc["split"], oy, ov, ws)

    if sc["split"]:
        assert int(ws[:2 * C * T * 4].view(torch.int32).abs().max()) == 0, "counters not zero"
        oy0, ov0 = prefilled()
        clean = ref.run_l4(store, sc["past_last"], sc["bbox"], True, oy0, ov0, None)
        for k in ("A", "b", "yaw_mean", "yaw0_var", "yaw", "vertices"):
            assert torch.equal(_bits(out[k]), _bits(clean[k])), f"{k} depends on the workspace"

    # padding: every column outside the cells keeps the pre-fill
    pad = torch.ones(ld, dtype=torch.bool, device=gpu)
    for o, n in zip(store.offsets, store.counts):
        pad[o:o + n] = False
    fill = _bits(torch.tensor([SENTINEL], dtype=torch.float64, device=gpu))
    assert bool((_bits(out["yaw"][:, pad]) == fill).all()), "yaw padding written"
    assert bool((_bits(out["vertices"][:, pad]) == fill).all()), "vertices padding written"

    used = (~pad).cpu().numpy()
    yaw = out["yaw"].cpu().numpy()[:, used]
    vert = out["vertices"].cpu().numpy()[:, used]
    A, b = out["A"].cpu().numpy(), out["b"].cpu().numpy()
    mean, var = out["yaw_mean"].cpu().numpy(), out["yaw0_var"].cpu().numpy()
    o = 0
    for j, r in enumerate(rf):
        n = r["yaw"].shape[0]
        where = f"cell {j} (n = {n}, {sc['family'][j]})"
        np.testing.assert_allclose(yaw[:, o:o + n].T, r["yaw"], rtol=1e-13, atol=1e-14,
                                   err_msg=where)
        got_v = vert[:, o:o + n].reshape(T, 4, 2, n).transpose(3, 0, 1, 2)
        np.testing.assert_allclose(got_v, r["vertices"], rtol=1e-13, atol=1e-13, err_msg=where)
        np.testing.assert_allclose(mean[j], r["yaw_mean"], rtol=1e-12, atol=1e-13,
                                   err_msg=where)
        if n == 1:
            assert np.isnan(var[j]), where
        elif sc["family"][j] == "identical":
            assert var[j] == 0.0, (where, var[j])
        else:
            np.testing.assert_allclose(var[j], r["yaw0_var"], rtol=1e-9, err_msg=where)
        np.testing.assert_allclose(A[j], ref.A_of(mean[j]), rtol=1e-13, atol=1e-15,
                                   err_msg=where)
        scale = np.abs(r["vertices"]).max()
        for t in range(T):
            want, _ = ref.b_of(mean[j, t], r["vertices"][:, t])
            np.testing.assert_allclose(b[j, t], want, rtol=1e-12, atol=1e-12 * scale,
                                       err_msg=f"{where} t = {t}")
        o += n
