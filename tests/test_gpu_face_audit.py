"""ccmpc_face_audit on the device against tests/_face_audit_ref.py: exact counts on every cell
size, horizon and dtype of its inputs (test_face_audit_ref_host.py shows that no v_f is near
enough to zero for rounding to decide a count), out_worst against the longdouble maxima, exact
ties, a shorter horizon, the plan read in place at ld_plan = 4, reproducibility under prefilled
outputs and a captured graph, the identities between the outputs, and ccmpc_risk_audit's disc
inside the box."""
import numpy as np
import pytest
import torch

import _face_audit_ref as ar

pytestmark = pytest.mark.gpu

CASES = [(T, f32) for T in ar.HORIZONS for f32 in (False, True)]
COUNT_NAMES = ("face_open", "in_box", "in_box_any", "sel_open", "sel_open_any")


def _host(a):
    return {n: (None if getattr(a, n) is None else getattr(a, n).cpu().numpy())
            for n in a._fields}


def _bits(a):
    return {n: (None if v is None else v.tobytes()) for n, v in _host(a).items()}


@pytest.fixture(scope="module")
def runs(gpu):
    """engine.face_audit with everything on, per (T, f32), computed once."""
    from ccmpc import engine
    cache = {}

    def get(T, f32):
        if (T, f32) not in cache:
            inp = ar.inputs(T, f32)
            store = ar.make_store(T, f32, gpu)
            a = engine.face_audit(store, inp["past"], inp["plan"], face_sel=inp["face_sel"],
                                  cell_plan=inp["cell_plan"])
            cache[(T, f32)] = (store, a, _host(a))
        return cache[(T, f32)]
    return get


@pytest.mark.parametrize("T,f32", CASES)
def test_counts_are_exact(runs, T, f32):
    ref = ar.reference(T, f32)
    _, _, got = runs(T, f32)
    for name in COUNT_NAMES:
        want = ar.stack(ref, name)
        print(name, "differing entries:", int(np.sum(got[name] != want)))
        assert np.array_equal(got[name], want), name
    inp = ar.inputs(T, f32)
    norow = inp["counts"].index(2)
    assert got["sel_open_any"][norow] == 0 and np.all(got["sel_open"][norow] == -1)
    assert np.all(got["face_open"][inp["counts"].index(0)] == 0)


@pytest.mark.parametrize("T,f32", CASES)
def test_worst_against_the_longdouble_maximum(runs, T, f32):
    ref = ar.reference(T, f32)
    _, _, got = runs(T, f32)
    e_got, e_own = ar.worst_errors(got["worst"], ref)
    print(f"T={T} f32={f32}: out_worst error {e_got:.3g}, float64 restatement {e_own:.3g}")
    assert e_got <= ar.allowed_worst_error(e_own)
    empty = ar.inputs(T, f32)["counts"].index(0)
    assert np.all(np.isneginf(got["worst"][empty]))
    assert np.all(np.isfinite(np.delete(got["worst"], empty, axis=0)))


@pytest.mark.parametrize("T,f32", [(8, False), (8, True), (1, True)])
def test_without_face_sel_and_without_worst(runs, gpu, T, f32):
    from ccmpc import engine
    inp = ar.inputs(T, f32)
    store, _, full = runs(T, f32)
    a = _host(engine.face_audit(store, inp["past"], inp["plan"], cell_plan=inp["cell_plan"]))
    assert a["sel_open"] is None and a["sel_open_any"] is None
    b = _host(engine.face_audit(store, inp["past"], inp["plan"], cell_plan=inp["cell_plan"],
                                worst=False))
    c = _host(engine.face_audit(store, inp["past"], inp["plan"], face_sel=inp["face_sel"],
                                cell_plan=inp["cell_plan"], worst=False))
    assert b["worst"] is None and c["worst"] is None
    for name in ("face_open", "in_box", "in_box_any"):
        for other in (a, b, c):
            assert np.array_equal(other[name], full[name]), name
    assert a["worst"].tobytes() == full["worst"].tobytes()
    for name in ("sel_open", "sel_open_any"):
        assert np.array_equal(c[name], full[name]), name


def test_device_face_sel_outside_0_3_means_no_row(runs, gpu):
    from ccmpc import engine
    T, f32 = 2, False
    inp = ar.inputs(T, f32)
    store, _, full = runs(T, f32)
    sel = inp["face_sel"].copy()
    sel[sel < 0] = np.array([4, 9, -7, 255])[np.arange(int(np.sum(sel < 0))) % 4]
    with pytest.raises(ValueError, match="face_sel"):
        engine.face_audit(store, inp["past"], inp["plan"], face_sel=sel,
                          cell_plan=inp["cell_plan"])
    got = _host(engine.face_audit(store, inp["past"], inp["plan"],
                                  face_sel=torch.as_tensor(sel, device=gpu),
                                  cell_plan=inp["cell_plan"]))
    for name in COUNT_NAMES:
        assert np.array_equal(got[name], full[name]), name


def test_tie_case_is_exact(gpu):
    from ccmpc import engine
    cells, past, plan, expect = ar.tie_case()
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    sel = np.array([[2, 0]], np.int32)
    got = _host(engine.face_audit(store, past, plan, face_sel=sel, extent=ar.TIE_EXTENT,
                                  car_r=ar.TIE_CAR_R))
    v, _, _ = ar.values(cells[0], past[0], plan[0], ar.TIE_EXTENT, ar.TIE_CAR_R)
    want = ar.tally(v, sel[0])
    for name in COUNT_NAMES:
        assert np.array_equal(got[name][0], want[name]), name
    # t = 1: every operation is exact, so the maxima are the restatement's bits
    assert got["worst"][0, 1].tobytes() == want["worst"][1].tobytes()
    for f, (neg, zero, pos) in expect.items():
        others = int(np.sum(np.delete(v[:, 1, f], [neg, zero, pos]) > 0))
        assert got["face_open"][0, 1, f] == others + 1          # the tie itself is not open


def test_shorter_horizon_reads_the_first_steps(gpu):
    from ccmpc import engine
    inp = ar.inputs(8, False)
    store = ar.make_store(8, False, gpu)
    ref = ar.reference(8, False, 5)
    got = _host(engine.face_audit(store, inp["past"], inp["plan"][:, :5],
                                  face_sel=inp["face_sel"][:, :5], cell_plan=inp["cell_plan"],
                                  T=5))
    assert got["face_open"].shape == (len(ref), 5, 4)
    for name in COUNT_NAMES:
        assert np.array_equal(got[name], ar.stack(ref, name)), name
    e_got, e_own = ar.worst_errors(got["worst"], ref)
    assert e_got <= ar.allowed_worst_error(e_own)
    with pytest.raises(ValueError):
        engine.face_audit(store, inp["past"], inp["plan"], T=9)


@pytest.mark.parametrize("f32", [False, True])
def test_plan_read_in_place_at_ld_plan_4(runs, gpu, f32):
    from ccmpc import engine
    T = 8
    inp = ar.inputs(T, f32)
    store, _, full = runs(T, f32)
    X = np.full(inp["plan"].shape[:2] + (4,), np.nan)
    X[..., :2] = inp["plan"]
    Xd = torch.as_tensor(X, device=gpu)
    got = engine.face_audit(store, inp["past"], Xd, face_sel=inp["face_sel"],
                            cell_plan=inp["cell_plan"])
    for name, b in _bits(got).items():
        assert b == full[name].tobytes(), name
    flat = engine.face_audit(store, inp["past"], Xd.reshape(-1), face_sel=inp["face_sel"],
                             cell_plan=inp["cell_plan"], ld_plan=4)
    for name, b in _bits(flat).items():
        assert b == full[name].tobytes(), name


@pytest.mark.parametrize("T,f32", [(8, False), (12, True)])
def test_reproducible_under_prefill_repeat_and_graph(runs, gpu, T, f32):
    from ccmpc import engine
    inp = ar.inputs(T, f32)
    store, _, full = runs(T, f32)
    want = {n: v.tobytes() for n, v in full.items()}
    C = store.n_cells
    f64 = dict(dtype=torch.float64, device=gpu)
    past = torch.as_tensor(inp["past"], **f64).contiguous()
    extent = torch.as_tensor(np.array([3.7, 1.79]), **f64)
    plan = torch.as_tensor(inp["plan"], **f64).contiguous()
    cell_plan = torch.as_tensor(inp["cell_plan"], device=gpu)
    sel = torch.as_tensor(inp["face_sel"], device=gpu)

    def call(out):
        return engine.face_audit(store, past, plan, face_sel=sel, cell_plan=cell_plan,
                                 extent=extent, out=out)
    for fill in (float("nan"), 0.0):
        i64 = torch.full((C, T, 4), -7 if fill else 0, dtype=torch.int64, device=gpu)
        out = engine.FaceAudit(i64, i64[..., 0].clone(), i64[:, 0, 0].clone(),
                               i64[..., 1].clone(), i64[:, 0, 1].clone(),
                               torch.full((C, T, 4), fill, **f64))
        call(out)
        assert _bits(out) == want, fill
    call(out)                                               # a repeated call on its own outputs
    assert _bits(out) == want
    # a captured graph, replayed after the plan tensor was overwritten in place
    other = ar.inputs(T, f32)["plan"][::-1].copy()
    fresh = _bits(engine.face_audit(store, past, torch.as_tensor(other, **f64), face_sel=sel,
                                    cell_plan=cell_plan, extent=extent))
    assert fresh != want
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        call(out)
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(out)
    plan.copy_(torch.as_tensor(other, **f64))
    for t in out:
        t.fill_(5)
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(out) == fresh


@pytest.mark.parametrize("T,f32", CASES)
def test_identities_between_the_outputs(runs, T, f32):
    _, _, g = runs(T, f32)
    assert np.all(g["in_box"] <= g["face_open"].min(-1))
    rows = np.where(g["sel_open"] >= 0, g["sel_open"], 0)
    assert np.all(g["sel_open_any"] >= rows.max(1))
    assert np.all(g["sel_open_any"] <= rows.sum(1))
    assert np.all(g["in_box_any"] >= g["in_box"].max(1))
    assert np.array_equal(g["worst"] <= 0, g["face_open"] == 0)


@pytest.mark.parametrize("T,f32", [(8, False), (8, True), (12, False)])
def test_risk_audit_disc_lies_inside_the_box(runs, gpu, T, f32):
    """The disc of radius 3.0 lies inside every inflated box (half-widths 3.13 and 4.09 m)."""
    from ccmpc import engine
    inp = ar.inputs(T, f32)
    store, _, g = runs(T, f32)
    plan = torch.as_tensor(inp["plan"], dtype=torch.float64, device=gpu)
    a = engine.risk_audit(store, plan=plan, R=3.0, cell_plan=inp["cell_plan"])
    hit, hit_any = a.hit.cpu().numpy(), a.hit_any.cpu().numpy()
    assert hit.sum() > 0
    assert np.all(hit <= g["in_box"]) and np.all(hit_any <= g["in_box_any"])
