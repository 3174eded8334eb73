"""ccmpc_face_constraints (cc-mpc_amd/csrc/faces.hip) through the C ABI against the longdouble
restatement of tests/_faces_ref.py -- never against the kernel's own output.

Shapes: cells of 2, 3, 5, 63, 64, 65, 255, 257, chunk + 1 and 2 chunk + 3 particles and a
one-particle cell in one store; T in {1, 2, 8, 12}; f64 and f32 (non-zero origins); a zero step
at t = 0 and at a later t; one reference row per cell, in a permuted order.

Measured on an MI355X (worst over all shapes and both dtypes):
    mean                 1.4e-13 relative         (bar 1e-12)
    C, scaled            4.4e-13                  (bar max(1e-12, 32 x float64's own) = 5.8e-12
                                                   in that case; at most 0.08 of the bar anywhere)
    root_f / its bound   2.9e-05
    robust s             2.2e-13 relative         (bar 1e-12)
    |R R - C| / |C|      10.6 eps                 (bar 256 eps)
Cells of 2 and 3 particles have a singular covariance: their root bound is infinite and only
the root's self-consistency judges them.
"""
import numpy as np
import pytest
import torch

import _faces_ref as fr

pytestmark = pytest.mark.gpu

TS = (1, 2, 8, 12)
NONFINITE = -12


def _bits(t):
    return t.cpu().numpy().copy()


@pytest.fixture(scope="module")
def runs(gpu):
    """(T, f32, kind) -> (records [C, T, 4], raw bytes), computed once and left unchanged."""
    cache = {}

    def get(T, f32, kind):
        key = (T, bool(f32), kind)
        if key not in cache:
            inp = fr.inputs(T, f32)
            store = fr.make_store(T, f32, gpu)
            out, _, _ = fr.run_faces(store, inp["past"], inp["gamma"], kind, inp["ref"],
                                     inp["cell_ref"])
            cache[key] = (fr.records(out), _bits(out))
        return cache[key]
    return get


@pytest.mark.parametrize("kind", ["nominal", "robust"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("T", TS)
def test_records_against_the_longdouble_reference(runs, T, f32, kind):
    rec, _ = runs(T, f32, kind)
    inp = fr.inputs(T, f32)
    ref, err64 = fr.reference(T, f32, kind)
    tol_c = fr.allowed_cov_error(err64)
    C = len(inp["cells"])
    assert rec.shape == (C, T, 4)
    assert np.array_equal(rec["t"], np.broadcast_to(np.arange(T)[None, :, None], rec.shape))
    assert np.array_equal(rec["face"], np.broadcast_to(np.arange(4), rec.shape))
    worst = dict(mean=0.0, C=0.0, root=0.0, s=0.0, self=0.0)
    for j in range(C):
        r, want = rec[j], ref[j]
        if j == inp["single"]:
            continue
        assert np.all(r["status"] == 0), (j, r["status"])
        mean = want["mean"].astype(np.float64)
        worst["mean"] = max(worst["mean"], float(np.max(np.abs(r["mean"] - mean) / np.abs(mean))))
        Cg = fr.full3(r["C"])
        Rg = fr.full3(r["root"])
        for t in range(T):
            for f in range(4):
                worst["C"] = max(worst["C"], fr.scaled_cov_error(Cg[t, f], want["C"][t, f]))
                if kind == "robust":
                    s = float(want["s"][t, f])
                    assert np.array_equal(r["root"][t, f][[1, 2, 4]], [0, 0, 0])
                    assert r["root"][t, f][0] == r["root"][t, f][3] == r["root"][t, f][5]
                    worst["s"] = max(worst["s"], abs(r["root"][t, f][0] - s) / s)
                else:
                    b = fr.root_bound(want["C"][t, f], want["lam_min"][t, f], want["root"][t, f],
                                      tol_c)
                    dR = np.linalg.norm(Rg[t, f] - want["root"][t, f].astype(np.float64))
                    if np.isfinite(b):
                        worst["root"] = max(worst["root"], dR / b)
                    sc = np.linalg.norm(Rg[t, f] @ Rg[t, f] - Cg[t, f]) / np.linalg.norm(Cg[t, f])
                    worst["self"] = max(worst["self"], sc / fr.EPS)
        # the approx choice: exact, on the premise (asserted on the reference alone) that the
        # runner-up is clear of the rounding of any of this
        v = np.sort(want["val"].astype(np.float64), axis=1)
        assert np.all(v[:, 1] - v[:, 0] > 1e-6 * (1 + np.abs(v[:, 0]))), j
        assert np.array_equal(np.argmax(r["chosen"] == 1, axis=1), want["chosen"]), j
        assert np.all((r["chosen"] == 1).sum(axis=1) == 1) and np.all(r["chosen"] <= 1)
    print(f"T={T} f32={f32} {kind}: float64's own scaled C error {err64:.2e} -> bar {tol_c:.2e};"
          f" worst mean rel {worst['mean']:.2e}, C scaled {worst['C']:.2e}, root / bound "
          f"{worst['root']:.2e}, s rel {worst['s']:.2e}, |RR - C| / |C| {worst['self']:.1f} eps")
    assert worst["mean"] <= 1e-12
    assert worst["C"] <= tol_c
    assert worst["root"] <= 1.0
    assert worst["s"] <= 1e-12
    assert worst["self"] <= 256


@pytest.mark.parametrize("kind", ["nominal", "robust"])
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("T", TS)
def test_one_particle_cell_fails_alone(runs, T, f32, kind):
    rec, raw = runs(T, f32, kind)
    j = fr.inputs(T, f32)["single"]
    r = rec[j]
    assert np.all(r["status"] == NONFINITE)
    assert np.all(r["chosen"] == 255)
    for name in ("mean", "root", "C"):
        assert np.all(np.isnan(r[name]))
        bits = np.ascontiguousarray(r[name]).view(np.uint64)
        assert np.all(bits == bits.flat[0])                  # one NaN, the same everywhere
    assert np.all(rec[j - 1]["status"] == 0) and np.all(rec[j + 1]["status"] == 0)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_kinds_share_mean_and_covariance_bits(runs, f32):
    a, _ = runs(8, f32, "nominal")
    b, _ = runs(8, f32, "robust")
    for name in ("mean", "C", "status"):
        assert np.array_equal(np.ascontiguousarray(a[name]).view(np.uint8),
                              np.ascontiguousarray(b[name]).view(np.uint8))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_prefill_repeat_and_graph_give_the_same_bits(gpu, runs, f32):
    """NaN-byte and zero pre-filled outputs / workspace, a second call, and a captured graph's
    replay all give the bits of the first run."""
    T, kind = 8, "nominal"
    _, want = runs(T, f32, kind)
    inp = fr.inputs(T, f32)
    store = fr.make_store(T, f32, gpu)
    C = len(inp["cells"])
    from ccmpc import _lib
    need = _lib.load().ccmpc_face_workspace_bytes(T, C, store.n_bound)
    keep = None
    for fill in (0xff, 0x00):
        out = torch.full((C, T, 4, 128), fill, dtype=torch.uint8, device=gpu)
        ws = torch.full((need,), fill, dtype=torch.uint8, device=gpu)
        out, ws, keep = fr.run_faces(store, inp["past"], inp["gamma"], kind, inp["ref"],
                                     inp["cell_ref"], out_rec=out, workspace=ws)
        assert np.array_equal(_bits(out), want), hex(fill)
    out, ws, keep = fr.run_faces(store, None, None, kind, out_rec=out, workspace=ws, keep=keep)
    assert np.array_equal(_bits(out), want)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        fr.run_faces(store, None, None, kind, out_rec=out, workspace=ws, keep=keep)
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fr.run_faces(store, None, None, kind, out_rec=out, workspace=ws, keep=keep, sync=False)
    out.fill_(0x5a)
    ws.fill_(0xff)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), want)


def test_no_reference_means_no_choice(gpu):
    inp = fr.inputs(2, False)
    store = fr.make_store(2, False, gpu)
    out, _, _ = fr.run_faces(store, inp["past"], inp["gamma"], "nominal")
    rec = fr.records(out)
    assert np.all(rec["chosen"] == 255)
    ok = np.arange(len(inp["cells"])) != inp["single"]
    assert np.all(rec["status"][ok] == 0)


def test_equal_faces_pick_the_lower_index(gpu):
    """Two faces with bit-equal device values (tests/_faces_ref.tie_case; the float64
    restatement ties too, tests/test_faces_ref_host.py): the first index is chosen."""
    from ccmpc import engine
    cells, past, ref = fr.tie_case()
    store = engine.ParticleStore.from_cells([cells], device=gpu)
    out, _, _ = fr.run_faces(store, past[None], [2.0], "robust", ref[None], extent=fr.TIE_EXTENT)
    rec = fr.records(out)[0]
    assert np.all(rec["status"] == 0)
    r = rec[1]
    xi = np.array([ref[1, 0], ref[1, 1], 1.0])
    val = [fr.lhs_value(r["mean"][f], fr.full3(r["root"][f]), 2.0, xi[:2]) for f in range(4)]
    assert r["mean"][0][0] == r["mean"][1][0] and r["mean"][0][2] == r["mean"][1][2]
    assert r["root"][0][0] == r["root"][1][0]
    assert val[0] == val[1] and val[0] < min(val[2], val[3])
    assert list(r["chosen"]) == [1, 0, 0, 0]
