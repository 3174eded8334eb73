"""ccmpc_face_cuts on records fabricated on the host (tests/_faces_ref.cell_f64, no store): g,
the cut's normal and offset against a longdouble restatement, the support and outer-approximation
properties, the pool's bookkeeping over rounds, and bit-reproducibility.

The bar on g, n and rhs is max(1e-13, 32 x the float64 NumPy restatement's own error against
longdouble on the same inputs), each error relative to the sum of the magnitudes of the terms
it is made of (the rows cancel: |mean . xi| is hundreds, g is metres) -- the convention of
tests/test_gpu_faces.py."""
import functools

import numpy as np
import pytest
import torch

import _faces_ref as fr
import _socp_ref as sr

pytestmark = pytest.mark.gpu

C = 3
TS_ = (1, 2, 8, 12)
MAX_ROUNDS = 3
EMPTY, CUT, OK, BAD = 1, 1, 0, 2          # CCMPC_CUT_EMPTY; CCMPC_SOCP_CUT / _OK / _BAD_ROW


@functools.lru_cache(maxsize=None)
def inputs(T):
    """Three cells of 40 particles, their cell_f64 faces chosen at a reference some metres off
    the clouds, gamma, and plans [2, T, 4] (x, y in the first two columns) near the clouds."""
    rng = np.random.default_rng(977 + T)
    outs, gamma = [], fr.gamma_of(np.full(C, 0.05 / 3), max(T, 1))
    centres = []
    for j in range(C):
        c = fr.cloud(rng, 40, T)
        past = c[0, 0] - np.array([3.0, 0.7])
        d = fr.step_deltas(c, past)
        ref = c.mean(0) + rng.uniform(-12, 12, size=(T, 2))
        outs.append(fr.cell_f64(c, np.arctan2(d[..., 1], d[..., 0]), float(gamma[j]), "nominal",
                                ref))
        centres.append(c.mean(0))
    plan = np.zeros((2, T, 4))
    plan[..., :2] = np.mean(centres, 0)[None] + rng.uniform(-25, 25, size=(2, T, 2))
    plan[..., 2:] = rng.normal(size=(2, T, 2))           # the columns the kernel must not read
    return dict(outs=outs, gamma=gamma, rec=sr.pack_face_records(outs, T), plan=plan)


def run(gpu, T, scene_cells, rec, gamma, plan, rnd=0, face_sel=None, tol_g=1e-6,
        only_violated=False, bufs=None, max_rounds=MAX_ROUNDS, fill=0xff, sync=True):
    """One engine.face_cuts call; bufs = a previous call's dict (its pool and state carried on)."""
    from ccmpc import engine
    S = len(scene_cells)
    off = np.concatenate(([0], np.cumsum(scene_cells))).astype(np.int64)
    n = int(off[-1])
    if bufs is None:
        u8 = dict(dtype=torch.uint8, device=gpu)
        bufs = dict(
            rec=torch.as_tensor(np.ascontiguousarray(rec).view(np.uint8).reshape(-1), device=gpu),
            scene_cell=torch.as_tensor(off, device=gpu),
            pool_cell=torch.as_tensor(off * (max_rounds + 1), device=gpu),
            gamma=torch.as_tensor(np.ascontiguousarray(gamma, np.float64), device=gpu),
            plan=torch.as_tensor(np.ascontiguousarray(plan[:S]), device=gpu),
            sel=None if face_sel is None else torch.as_tensor(
                np.ascontiguousarray(face_sel, np.int32), device=gpu),
            pool=torch.full(((max_rounds + 1) * n * T * 32,), fill, **u8),
            g=torch.full((n * T * 8,), fill, **u8).view(torch.float64),
            viol=torch.full((S * 8,), fill, **u8).view(torch.float64),
            state=torch.full((S * 4,), fill, **u8).view(torch.int32))
    b = bufs
    engine.face_cuts(b["rec"], T, b["scene_cell"], n, b["gamma"], b["plan"], b["pool"],
                     b["pool_cell"], b["g"], b["viol"], b["state"], rnd, max_rounds, tol_g,
                     b["sel"], fr.CAR_R, only_violated)
    if sync:
        torch.cuda.synchronize()
    return bufs


def host(bufs, T, n_cells, max_rounds=MAX_ROUNDS):
    """(pool [S-major as laid out: flat cells, T], g [cells, T], viol, state) on the host."""
    from ccmpc import _lib
    pool = bufs["pool"].cpu().numpy().view(_lib.GATHER_DTYPE).reshape(-1, T)
    return (pool, bufs["g"].cpu().numpy().reshape(n_cells, T), bufs["viol"].cpu().numpy(),
            bufs["state"].cpu().numpy())


def region(pool, scene_cells, s, r, max_rounds=MAX_ROUNDS):
    """Region r of scene s: [cells_s, T] records."""
    base = (max_rounds + 1) * int(np.sum(scene_cells[:s]))
    return pool[base + r * scene_cells[s]: base + (r + 1) * scene_cells[s]]


def selection(inp, T, mode):
    """(face_sel or None, faces [C, T] the rows use, -1 = none)."""
    chosen = np.array([o["chosen"] for o in inp["outs"]], np.int64)
    if mode == "chosen":
        return None, chosen
    sel = (chosen + 1 + np.arange(C)[:, None] + np.arange(T)[None, :]) % 4
    if mode == "minus":
        sel[1, :] = -1
        sel[2, ::2] = -1
    return sel.astype(np.int32), sel


@pytest.mark.parametrize("mode", ["chosen", "explicit", "minus"])
@pytest.mark.parametrize("cells", [(3,), (2, 1)], ids=["S1", "S2"])
@pytest.mark.parametrize("T", TS_)
def test_round_zero_against_longdouble(gpu, T, cells, mode):
    inp = inputs(T)
    sel, faces = selection(inp, T, mode)
    bufs = run(gpu, T, cells, inp["rec"], inp["gamma"], inp["plan"], face_sel=sel)
    pool, g, viol, state = host(bufs, T, C)
    scene_of = np.repeat(np.arange(len(cells)), cells)
    first = np.concatenate(([0], np.cumsum(cells)))
    err64 = dict(g=0.0, a=0.0, b=0.0)
    err = dict(g=0.0, a=0.0, b=0.0, support=0.0)
    rng = np.random.default_rng(5)
    want_viol = np.full(len(cells), -np.inf)
    for c in range(C):
        s = scene_of[c]
        reg0 = region(pool, cells, s, 0)[c - first[s]]
        for t in range(T):
            r = reg0[t]
            assert r["t_tau"] == t and r["side"] == -1
            f = faces[c, t]
            if f < 0:
                assert g[c, t] == -np.inf and r["status"] == EMPTY
                assert r["n0"] == 0 and r["n1"] == 0 and r["rhs"] == 0
                continue
            p = inp["plan"][s, t, :2]
            o = inp["outs"][c]
            row = dict(mean=o["mean"][t, f], root=o["root"][t, f], gamma=float(inp["gamma"][c]))
            gl, al, bl, (sg, sa, sb) = sr.row_cut_ld(o["mean"][t, f], fr.sym6(o["root"][t, f]),
                                                     inp["gamma"][c], fr.CAR_R, p)
            g64, a64, b64 = sr.row_cut(row, p)
            err64["g"] = max(err64["g"], float(abs(g64 - gl)) / sg)
            err64["a"] = max(err64["a"], float(max(abs(a64[0] - al[0]), abs(a64[1] - al[1]))) / sa)
            err64["b"] = max(err64["b"], float(abs(b64 - bl)) / sb)
            assert r["status"] == 0
            err["g"] = max(err["g"], float(abs(g[c, t] - gl)) / sg)
            err["a"] = max(err["a"], float(max(abs(r["n0"] - al[0]), abs(r["n1"] - al[1]))) / sa)
            err["b"] = max(err["b"], float(abs(r["rhs"] - bl)) / sb)
            # support: a . p - b == g
            sup = np.longdouble(r["n0"]) * p[0] + np.longdouble(r["n1"]) * p[1] - r["rhs"]
            err["support"] = max(err["support"], float(abs(sup - g[c, t])) / sb)
            want_viol[s] = max(want_viol[s], g[c, t])
            # outer approximation at 1000 / (C T) random points per row, 1000 per row at T = 1
            q = p + rng.uniform(-40, 40, size=(max(1000 // (C * T), 40), 2))
            for qq in q:
                gq, _, _, (sgq, _, _) = sr.row_cut_ld(o["mean"][t, f], fr.sym6(o["root"][t, f]),
                                                      inp["gamma"][c], fr.CAR_R, qq)
                lin = np.longdouble(r["n0"]) * qq[0] + np.longdouble(r["n1"]) * qq[1] - r["rhs"]
                slack = 1e-13 * (sb + sgq + sa * (abs(qq[0]) + abs(qq[1])))
                assert lin <= gq + slack, (c, t, float(lin - gq))
    bars = {k: max(1e-13, 32 * v) for k, v in err64.items()}
    print(f"T={T} {cells} {mode}: float64's own error {err64} -> bars {bars}; kernel {err}")
    assert err["g"] <= bars["g"] and err["a"] <= bars["a"] and err["b"] <= bars["b"]
    assert err["support"] <= bars["b"]
    assert np.array_equal(viol, want_viol)                      # max is exact
    assert np.all(state == CUT)                                 # round 0 never ends a scene
    for s in range(len(cells)):                                 # the later regions: empty
        for rr in range(1, MAX_ROUNDS + 1):
            reg = region(pool, cells, s, rr)
            assert np.all(reg["status"] == EMPTY) and np.all(reg["n0"] == 0)
            assert np.array_equal(reg["t_tau"], np.broadcast_to(np.arange(T), reg.shape))


def test_zero_root_gives_the_mean_as_the_subgradient(gpu):
    T = 2
    inp = inputs(T)
    rec = inp["rec"].copy()
    rec["root"][0] = 0.0
    bufs = run(gpu, T, (3,), rec, inp["gamma"], inp["plan"])
    pool, g, _, _ = host(bufs, T, C)
    for t in range(T):
        f = int(inp["outs"][0]["chosen"][t])
        m = rec["mean"][0, t, f]
        x, y = inp["plan"][0, t, :2]
        r = region(pool, (3,), 0, 0)[0, t]
        assert r["status"] == 0 and r["n0"] == m[0] and r["n1"] == m[1]
        want = m[0] * x + m[1] * y + m[2] + 0.0 + 0.5 * fr.CAR_R
        assert g[0, t] == want and r["rhs"] == m[0] * x + m[1] * y - want


@pytest.mark.parametrize("what", ["status", "no_choice", "sel_range"])
def test_bad_row_stops_its_scene_only(gpu, what):
    """Scene 0 = cells 0, 1 with a bad selected row; scene 1 = cell 2 stays as it was."""
    T, cells = 8, (2, 1)
    inp = inputs(T)
    rec, sel = inp["rec"].copy(), None
    if what == "status":
        f = int(inp["outs"][1]["chosen"][3])
        rec["status"][1, 3, f] = -14
    elif what == "no_choice":
        rec["t_face_chosen"][1, 5] = (rec["t_face_chosen"][1, 5] & ~np.uint32(0xff)) | 255
    else:
        sel = np.array([o["chosen"] for o in inp["outs"]], np.int32)
        sel[0, 2] = 4
    bufs = run(gpu, T, cells, rec, inp["gamma"], inp["plan"], face_sel=sel)
    good = run(gpu, T, cells, inp["rec"], inp["gamma"], inp["plan"])
    pool, g, viol, state = host(bufs, T, C)
    pool_g, g_g, viol_g, state_g = host(good, T, C)
    assert state[0] == BAD and np.isnan(viol[0]) and state[1] == CUT
    assert np.all(region(pool, cells, 0, 0)["status"] == EMPTY)
    assert np.sum(np.isnan(g)) == 1
    for a, b in zip(region(pool, cells, 1, 0).reshape(-1), region(pool_g, cells, 1, 0).reshape(-1)):
        assert a.tobytes() == b.tobytes()
    assert viol[1] == viol_g[1] and np.array_equal(g[2], g_g[2], equal_nan=True)
    # sticky: a later round on the mended records still writes nothing for scene 0
    bufs["rec"].copy_(good["rec"])
    bufs["sel"] = None
    run(gpu, T, cells, None, None, None, rnd=1, bufs=bufs)
    pool, _, _, state = host(bufs, T, C)
    assert state[0] == BAD and np.all(region(pool, cells, 0, 1)["status"] == EMPTY)


def test_later_rounds_ok_is_sticky_and_only_violated(gpu):
    """Scene 0's tolerance is met in round 1 (a huge tol_g would end both, so the plans differ:
    scene 1's plan stands inside an obstacle)."""
    T, cells = 8, (2, 1)
    inp = inputs(T)
    b0 = run(gpu, T, cells, inp["rec"], inp["gamma"], inp["plan"])
    _, g0, viol0, _ = host(b0, T, C)
    tol = float(0.5 * (viol0[0] + viol0[1]))
    lo, hi = (0, 1) if viol0[0] < viol0[1] else (1, 0)        # scene lo ends, scene hi goes on
    assert viol0[lo] < tol < viol0[hi]
    run(gpu, T, cells, None, None, None, rnd=1, tol_g=tol, bufs=b0, only_violated=True)
    pool, g1, viol1, state = host(b0, T, C)
    assert state[lo] == OK and state[hi] == CUT
    assert np.array_equal(g1, g0) and np.array_equal(viol1, viol0)
    assert np.all(region(pool, cells, lo, 1)["status"] == EMPTY)
    first = np.concatenate(([0], np.cumsum(cells)))
    reg = region(pool, cells, hi, 1)
    gh = g0[first[hi]:first[hi + 1]]
    assert np.array_equal(reg["status"] == 0, gh > 0)            # only the violated rows
    assert np.any(gh > 0) and np.array_equal(reg["status"] == EMPTY, ~(gh > 0))
    # round 0's region is untouched, and rounds 2, 3 are still empty
    for s in (0, 1):
        assert np.all(region(pool, cells, s, 2)["status"] == EMPTY)
        assert np.all(region(pool, cells, s, 0)["status"] == 0)
    # round 2 with a tolerance nothing meets: the scene that was OK stays OK and empty
    run(gpu, T, cells, None, None, None, rnd=2, tol_g=-1e9, bufs=b0)
    pool, _, _, state = host(b0, T, C)
    assert state[lo] == OK and state[hi] == CUT
    assert np.all(region(pool, cells, lo, 2)["status"] == EMPTY)
    assert np.all(region(pool, cells, hi, 2)["status"] == 0)     # every row again


def _bits(bufs):
    return tuple(bufs[k].cpu().numpy().tobytes() for k in ("pool", "g", "viol", "state"))


def test_prefill_repeat_and_graph_give_the_same_bits(gpu):
    T, cells = 8, (2, 1)
    inp = inputs(T)
    sel, _ = selection(inp, T, "minus")
    want = None
    for fill in (0xff, 0x00):
        b = run(gpu, T, cells, inp["rec"], inp["gamma"], inp["plan"], face_sel=sel, fill=fill)
        run(gpu, T, cells, None, None, None, rnd=1, bufs=b)
        got = _bits(b)
        assert want is None or got == want, hex(fill)
        want = got
    run(gpu, T, cells, None, None, None, rnd=0, bufs=b)          # the whole sequence again
    run(gpu, T, cells, None, None, None, rnd=1, bufs=b)
    assert _bits(b) == want
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        run(gpu, T, cells, None, None, None, rnd=0, bufs=b)
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(gpu, T, cells, None, None, None, rnd=0, bufs=b, sync=False)
        run(gpu, T, cells, None, None, None, rnd=1, bufs=b, sync=False)
    for k in ("pool", "g", "viol", "state"):
        b[k].view(torch.uint8).fill_(0x5a)
    graph.replay()
    torch.cuda.synchronize()
    assert _bits(b) == want


def test_binding_refuses_short_buffers(gpu):
    T = 2
    inp = inputs(T)
    b = run(gpu, T, (3,), inp["rec"], inp["gamma"], inp["plan"])
    from ccmpc import engine
    with pytest.raises(ValueError, match="pool"):
        engine.face_cuts(b["rec"], T, b["scene_cell"], C, b["gamma"], b["plan"], b["pool"][:-32],
                         b["pool_cell"], b["g"], b["viol"], b["state"], 0, MAX_ROUNDS)
    with pytest.raises(ValueError, match="plan"):
        engine.face_cuts(b["rec"], T, b["scene_cell"], C, b["gamma"], b["plan"][:, :, :1],
                         b["pool"], b["pool_cell"], b["g"], b["viol"], b["state"], 0, MAX_ROUNDS)
