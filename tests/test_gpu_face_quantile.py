"""ccmpc_face_quantile on the device against tests/_face_quantile_ref.py and against
ccmpc_face_audit on the same store: the exact identities between the two calls, the rank of
out_q among the longdouble values, exact ties, the cut, the statuses and bit-reproducibility.

Cells: _face_audit_ref.counts_of (0, 1, 2, 63, 64, 65, 255, 257, I - 1, I, I + 1, 2 I + 3, I the
work item); horizons 1, 2, 8, 9, 12 (9: the first past one chunk of 8 steps); both dtypes; per
cell m in {0, 1, floor(0.003125 N), N - 1, N, -1}."""
import numpy as np
import pytest
import torch

import _face_audit_ref as ar
import _face_quantile_ref as qr
from _l4_ref import LD, TINY, U as ULP, store_world

pytestmark = pytest.mark.gpu

CASES = [(T, f32) for T in qr.HORIZONS for f32 in (False, True)]
NM = len(qr.M_NAMES)
HLON = 0.5 * ar.LON + 0.5 * ar.CAR_R
MARGIN = 1e-6


def _host(a):
    return {n: (None if getattr(a, n) is None else getattr(a, n).cpu().numpy())
            for n in a._fields}


def _bits(a):
    return {n: v.tobytes() for n, v in _host(a).items()}


def _allow(T, f32, k):
    return np.array([qr.allows_of(n)[k] for n in ar.inputs(T, f32)["counts"]], np.int64)


@pytest.fixture(scope="module")
def runs(gpu):
    """Per (T, f32), computed once: the store, engine.face_audit's outputs, and
    engine.face_quantile's for each of the six allows (device allow tensors: -1 is not checked on
    the host)."""
    from ccmpc import engine
    cache = {}

    def get(T, f32):
        if (T, f32) not in cache:
            inp = ar.inputs(T, f32)
            store = ar.make_store(T, f32, gpu)
            audit = _host(engine.face_audit(store, inp["past"], inp["plan"],
                                            cell_plan=inp["cell_plan"]))
            quants = []
            for k in range(NM):
                allow = torch.as_tensor(_allow(T, f32, k), device=gpu)
                q = engine.face_quantile(store, inp["past"], inp["plan"], allow=allow,
                                         cell_plan=inp["cell_plan"], margin=MARGIN)
                h = _host(q)
                h["rec"] = engine.face_quantile_cuts(q)
                quants.append(h)
            cache[(T, f32)] = (store, audit, quants)
        return cache[(T, f32)]
    return get


@pytest.mark.parametrize("T,f32", CASES)
def test_exact_against_the_audit(runs, T, f32):
    """m = 0: out_q is out_worst bit for bit.  Every m: face_open <= m  <=>  q <= 0."""
    _, audit, quants = runs(T, f32)
    counts = np.array(ar.inputs(T, f32)["counts"])
    live0 = quants[0]["status"] == 0
    assert np.array_equal(live0, np.broadcast_to((counts > 0)[:, None], live0.shape))
    q0, worst = quants[0]["q"], audit["worst"]
    assert q0[live0].tobytes() == worst[live0].tobytes()
    for k in range(NM):
        g = quants[k]
        live = g["status"] == 0
        m = _allow(T, f32, k)[:, None, None]
        lhs = (audit["face_open"] <= m)[live]
        rhs = (g["q"] <= 0)[live]
        print(f"m = {qr.M_NAMES[k]}: {int(live.sum())} live (cell, t), "
              f"{int(np.sum(lhs != rhs))} disagreements, {int(rhs.sum())} rows within budget")
        assert np.array_equal(lhs, rhs), qr.M_NAMES[k]


@pytest.mark.parametrize("T,f32", CASES)
def test_status_and_the_rows_that_select_nothing(runs, T, f32):
    _, _, quants = runs(T, f32)
    for k in range(NM):
        g = quants[k]
        want = np.array([d["status"] for d in qr.reference(T, f32, k)])
        assert np.array_equal(g["status"], np.broadcast_to(want[:, None], g["status"].shape))
        vac, skip, live = (g["status"] == s for s in (qr.VACUOUS, qr.SKIPPED, 0))
        assert np.all(np.isneginf(g["q"][vac])) and np.all(np.isnan(g["q"][skip]))
        assert np.all(np.isfinite(g["q"][live]))
        assert np.all(g["arg"][~live] == -1) and np.all(g["arg"][live] >= 0)
        rec = g["rec"]
        assert np.all(rec["status"][~live] == qr.EMPTY)
        assert np.all(rec["side"] == -1)
        assert np.array_equal(rec["t_tau"], np.broadcast_to(np.arange(T)[None, :, None], rec.shape))
    assert {s for g in quants for s in np.unique(g["status"])} == {0, qr.VACUOUS, qr.SKIPPED}


@pytest.mark.parametrize("T,f32", CASES)
def test_rank_against_longdouble(runs, T, f32):
    """For every live (c, t, f) and every m, with b = allowed_worst_error(own) (|ex| + |ey| +
    hlon) at the arg particle: #{vld > q + b} <= m, #{vld >= q - b} >= m + 1, |vld[arg] - q| <= b.
    own: the error of the float64 restatement's own order statistic against the longdouble value
    of the particle it selected, over the same rows, in the same units."""
    _, _, quants = runs(T, f32)
    ref = ar.reference(T, f32)
    tt, ff = np.meshgrid(np.arange(T), np.arange(4), indexing="ij")
    own, rows = 0.0, []
    for k in range(NM):
        for j, (r, d) in enumerate(zip(ref, qr.reference(T, f32, k))):
            if d["status"]:
                continue
            a64 = d["arg64"]
            scale = (np.abs(r["ex"][a64, tt]) + np.abs(r["ey"][a64, tt]) + HLON).astype(np.float64)
            e = np.abs(d["q64"].astype(LD) - r["vld"][a64, tt, ff]).astype(np.float64) / scale
            own = max(own, float(e.max()))
            rows.append((k, j, r, d))
    bar = ar.allowed_worst_error(own)
    worst = 0.0
    for k, j, r, d in rows:
        g = quants[k]
        q, arg, m = g["q"][j], g["arg"][j], d["m"]
        assert np.all((arg >= 0) & (arg < d["n"]))
        scale = np.abs(r["ex"][arg, tt]) + np.abs(r["ey"][arg, tt]) + LD(HLON)
        b = LD(bar) * scale
        vld = r["vld"]
        assert np.all((vld > (q.astype(LD) + b)[None]).sum(0) <= m), (k, j)
        assert np.all((vld >= (q.astype(LD) - b)[None]).sum(0) >= m + 1), (k, j)
        err = np.abs(vld[arg, tt, ff] - q.astype(LD)) / scale
        worst = max(worst, float(err.max()))
        assert np.all(err <= LD(bar)), (k, j)
    print(f"T={T} f32={f32}: float64 restatement's own error {own:.3g}, bar {bar:.3g}, "
          f"|vld[arg] - q| / scale worst {worst:.3g} = {worst / bar:.3g} of the bar")


@pytest.mark.parametrize("T,f32", CASES)
def test_cut_of_the_arg_particle(runs, T, f32):
    """n within 4 x 2^-52 |exact| + 2^-1022 of the longdouble unit vector of the arg particle
    (the heading bar of tests/test_gpu_l4_edges.py); n . P - rhs - q - margin within max(1e-13, 32 x the float64
    restatement's own error), relative to the magnitudes of the terms (the rhs bar of
    tests/test_gpu_face_cuts.py); a record is empty exactly where q + margin <= 0."""
    _, _, quants = runs(T, f32)
    inp = ar.inputs(T, f32)
    world = store_world(inp["cells"], bool(f32), inp["origin"])
    tt, ff = np.meshgrid(np.arange(T), np.arange(4), indexing="ij")
    e_n = e_own = e_rhs = 0.0
    n_cut = n_empty = 0
    for k in range(NM):
        g = quants[k]
        for j, d in enumerate(qr.reference(T, f32, k)):
            if d["status"]:
                continue
            q, arg, rec = g["q"][j], g["arg"][j], g["rec"][j]
            empty = q + MARGIN <= 0.0
            assert np.array_equal(rec["status"] == qr.EMPTY, empty)
            assert np.all(rec["status"][~empty] == 0)
            for name in ("n0", "n1", "rhs"):
                assert np.all(rec[name][empty] == 0)
            n_cut += int((~empty).sum())
            n_empty += int(empty.sum())
            if empty.all():
                continue
            plan = inp["plan"][inp["cell_plan"][j]]
            nld, _ = qr.cut(world[j], inp["past"][j], plan, q, arg, MARGIN, ld=True)
            n64, rhs64 = qr.cut(world[j], inp["past"][j], plan, q, arg, MARGIN)
            P = plan[:T, :2].astype(LD)
            terms = (np.abs(nld[..., 0] * P[:, None, 0]) + np.abs(nld[..., 1] * P[:, None, 1])
                     + np.abs(q) + MARGIN).astype(np.float64)
            for nm, comp in (("n0", 0), ("n1", 1)):
                dn = np.abs(rec[nm].astype(LD) - nld[..., comp]).astype(np.float64)
                e_n = max(e_n, float(dn[~empty].max()) / ULP)
                lim = 4 * ULP * np.abs(nld[..., comp]).astype(np.float64) + TINY
                assert np.all(dn[~empty] <= lim[~empty]), (k, j, nm)

            def support(n0, n1, rhs):
                s = n0.astype(LD) * P[:, None, 0] + n1.astype(LD) * P[:, None, 1] - rhs.astype(LD)
                return (np.abs(s - q.astype(LD) - LD(MARGIN)).astype(np.float64) / terms)[~empty]
            e_own = max(e_own, float(support(n64[..., 0], n64[..., 1], rhs64).max()))
            e_rhs = max(e_rhs, float(support(rec["n0"], rec["n1"], rec["rhs"]).max()))
    bar = max(1e-13, 32 * e_own)
    print(f"T={T} f32={f32}: {n_cut} cuts, {n_empty} empty; n error {e_n:.3g} x 2^-52; support "
          f"error {e_rhs:.3g}, float64 restatement {e_own:.3g}, bar {bar:.3g}")
    assert n_cut > 0 and n_empty > 0
    assert e_rhs <= bar


def test_ties_are_exact_and_take_the_lowest_index(gpu):
    """_face_audit_ref.tie_case() with every particle twice: at t = 1 every v_f is exact, so q is
    the float64 sort's bits; every value is held by two particles, arg is the lower."""
    from ccmpc import engine
    cells, past, plan, expect = qr.tie_store_cells()
    store = engine.ParticleStore.from_cells(cells, device=gpu)
    v, _, _ = ar.values(cells[0], past[0], plan[0], ar.TIE_EXTENT, ar.TIE_CAR_R)
    audit = _host(engine.face_audit(store, past, plan, extent=ar.TIE_EXTENT, car_r=ar.TIE_CAR_R))
    for m in (0, 1, 2, 3, 5, 11, 23):
        g = _host(engine.face_quantile(store, past, plan, allow=[m], extent=ar.TIE_EXTENT,
                                       car_r=ar.TIE_CAR_R))
        q, arg = qr.select(v, m)
        assert np.all(g["status"] == 0)
        assert g["q"][0, 1].tobytes() == q[1].tobytes()           # t = 1: exact
        assert np.array_equal(g["arg"][0, 1], arg[1])
        assert np.all(g["arg"][0] < 12)                           # both steps: the lower copy
        assert np.array_equal(audit["face_open"][0] <= m, g["q"][0] <= 0)
    # the planted ties: v_f == 0 exactly for the middle particle of face f's triple and its copy
    for f, (neg, zero, pos) in expect.items():
        above = int(np.sum(v[:, 1, f] > 0))
        g = _host(engine.face_quantile(store, past, plan, allow=[above], extent=ar.TIE_EXTENT,
                                       car_r=ar.TIE_CAR_R))
        assert g["q"][0, 1, f] == 0.0 and not np.signbit(g["q"][0, 1, f])
        assert g["arg"][0, 1, f] == zero


def test_host_allow_is_checked(gpu):
    from ccmpc import engine
    inp = ar.inputs(2, False)
    store = ar.make_store(2, False, gpu)
    with pytest.raises(ValueError, match="allow"):
        engine.face_quantile(store, inp["past"], inp["plan"], allow=_allow(2, False, 5),
                             cell_plan=inp["cell_plan"])
    with pytest.raises(ValueError, match="margin"):
        engine.face_quantile(store, inp["past"], inp["plan"], cell_plan=inp["cell_plan"],
                             margin=-1.0)


@pytest.mark.parametrize("T,f32", [(9, False), (12, True)])
def test_reproducible_under_prefill_repeat_graph_and_ld_plan(runs, gpu, T, f32):
    from ccmpc import engine, _lib
    lib = _lib.load()
    inp = ar.inputs(T, f32)
    store, _, quants = runs(T, f32)
    k = 2
    want = {n: v.tobytes() for n, v in quants[k].items() if n != "rec"}
    C = store.n_cells
    f64 = dict(dtype=torch.float64, device=gpu)
    past = torch.as_tensor(inp["past"], **f64).contiguous()
    extent = torch.as_tensor(np.array([3.7, 1.79]), **f64)
    plan = torch.as_tensor(inp["plan"], **f64).contiguous()
    cell_plan = torch.as_tensor(inp["cell_plan"], device=gpu)
    allow = torch.as_tensor(_allow(T, f32, k), device=gpu)
    need = int(lib.ccmpc_face_quantile_workspace_bytes(T, C))
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)

    def call(out, p=plan):
        return engine.face_quantile(store, past, p, allow=allow, cell_plan=cell_plan,
                                    extent=extent, margin=MARGIN, out=out, workspace=ws)
    for fill in (float("nan"), 0.0):
        out = engine.FaceQuantile(torch.full((C, T, 4), fill, **f64),
                                  torch.full((C, T, 4), -7 if fill else 0, dtype=torch.int64,
                                             device=gpu),
                                  torch.full((C, T, 4, 32), 0xff if fill else 0, dtype=torch.uint8,
                                             device=gpu),
                                  torch.full((C, T), -7 if fill else 0, dtype=torch.int32,
                                             device=gpu))
        ws.fill_(0xff if fill else 0)
        call(out)
        assert _bits(out) == want, fill
    call(out)                                                   # a repeated call, used workspace
    assert _bits(out) == want
    # ld_plan = 4 with NaN in the unused columns
    X = np.full(inp["plan"].shape[:2] + (4,), np.nan)
    X[..., :2] = inp["plan"]
    assert _bits(call(out, torch.as_tensor(X, **f64))) == want
    # a captured graph, replayed after the plan tensor was overwritten in place
    other = inp["plan"][::-1].copy()
    fresh = _bits(engine.face_quantile(store, past, torch.as_tensor(other, **f64), allow=allow,
                                       cell_plan=cell_plan, extent=extent, margin=MARGIN))
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
    ws.fill_(5)
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(out) == fresh
