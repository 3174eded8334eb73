"""The oracle of the box-face Monte-Carlo audit (cc-mpc_amd/csrc/face_audit.hip,
ccmpc_face_audit): a float64 NumPy restatement of the contract in its stated order, an
np.longdouble restatement from the exact unit vector of the float64 step delta, the counts both
imply, and the inputs of the tests.  Not a test.
"""
import functools

import numpy as np

from _faces_ref import CAR_R, LAT, LON, cloud
from _l4_ref import LD, step_deltas, store_world, unit

ITEM = {False: 512, True: 1024}        # particles per work item of face_audit_kernel (f64, f32)
HORIZONS = (1, 2, 8, 12)
BAND = 1e-9                            # no |v_f| may lie within BAND (1 + |ex| + |ey|) of zero


def counts_of(f32):
    i = ITEM[bool(f32)]
    return (0, 1, 2, 63, 64, 65, 255, 257, i - 1, i, i + 1, 2 * i + 3)


# ---------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------
def heading_f64(d):
    """(c, s) of float64 step deltas (n, T, 2): d / |d| in float64, a zero step gives (1, 0)."""
    dx, dy = d[..., 0], d[..., 1]
    n = np.sqrt(dx * dx + dy * dy)
    zero = n == 0
    n = np.where(zero, 1.0, n)
    return np.where(zero, 1.0, dx / n), np.where(zero, 0.0, dy / n)


def values(world, past_last, plan, extent=(LON, LAT), car_r=CAR_R, ld=False):
    """v [n, T, 4], ex, ey [n, T] of one cell: world (n, T, 2) float64 as the kernel reads it,
    plan (T, >= 2) the cell's plan row.  ld=False: float64 in the contract's order; ld=True:
    longdouble from the exact unit vector of the float64 step delta."""
    world = np.asarray(world, np.float64)
    T = world.shape[1]
    d = step_deltas(world, past_last) if world.shape[0] else np.zeros_like(world)
    ft = LD if ld else np.float64
    c, s = unit(d) if ld else heading_f64(d)
    X, Y = np.asarray(plan, np.float64)[:T, 0].astype(ft), np.asarray(plan, np.float64)[:T, 1].astype(ft)
    ex, ey = X[None] - world[..., 0].astype(ft), Y[None] - world[..., 1].astype(ft)
    p, q = c * ex - s * ey, s * ex + c * ey
    half = ft(0.5)
    hlat = half * ft(extent[1]) + half * ft(car_r)
    hlon = half * ft(extent[0]) + half * ft(car_r)
    return np.stack([hlat - p, hlon - q, hlat + p, hlon + q], -1), ex, ey


def tally(v, sel=None):
    """The outputs one cell's v [n, T, 4] implies: dict(face_open [T, 4], in_box [T], in_box_any,
    sel_open [T], sel_open_any, worst [T, 4]); sel [T]: 0..3 or anything else for no row."""
    n, T = v.shape[:2]
    opn = v > 0
    box = opn.all(-1)
    out = dict(face_open=opn.sum(0).astype(np.int64), in_box=box.sum(0).astype(np.int64),
               in_box_any=np.int64(box.any(1).sum()),
               worst=(v.max(0) if n else np.full((T, 4), -np.inf)))
    if sel is not None:
        so = np.full(T, -1, np.int64)
        anyrow = np.zeros(n, bool)
        for t in range(T):
            if 0 <= sel[t] <= 3:
                so[t] = opn[:, t, sel[t]].sum()
                anyrow |= opn[:, t, sel[t]]
        out.update(sel_open=so, sel_open_any=np.int64(anyrow.sum()))
    return out


# ---------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(T, f32):
    """One store's worth of cells for horizon T: counts_of(f32) particles, clouds from
    _faces_ref.cloud, the f32 store quantised as _faces_ref.inputs does it.  One particle of the
    63-particle cell does not move at some t >= 1 (T > 1), one of the 64-particle cell at t = 0.
    Plan: one row per cell, in a permuted cell_plan: the cloud's mean position displaced in the
    mean heading's face frame to p = hlat (0.83 + 0.045 t), q = -hlon (0.91 + 0.021 t), near a
    corner of the inflated box, so that the counts are mixed.  face_sel mixes 0..3 and -1 rows;
    the 2-particle cell has no row at all.  Treat as read-only."""
    rng = np.random.default_rng(20261021 + 100 * T + int(f32))
    counts = list(counts_of(f32))
    cells = [cloud(rng, n, T) for n in counts]
    centre = np.array([205.0, -62.0])
    past = np.array([(c[0, 0] if len(c) else centre) - np.array([3.0, 0.7]) for c in cells])
    origin = None
    if f32:
        origin = np.array([np.round(c[:, 0].mean(0)) if len(c) else centre for c in cells])
        cells = [((c - o).astype(np.float32).astype(np.float64) + o)
                 for c, o in zip(cells, origin)]
    i63, i64 = counts.index(63), counts.index(64)
    if T > 1:
        tz = min(3, T - 1)
        cells[i63][7, tz] = cells[i63][7, tz - 1]          # a zero step at t = tz
    past[i64] = cells[i64][11, 0]                          # a zero step at t = 0
    C = len(cells)
    perm = np.random.default_rng(11).permutation(C)
    hlat, hlon = 0.5 * LAT + 0.5 * CAR_R, 0.5 * LON + 0.5 * CAR_R
    ts = np.arange(T)
    p, q = hlat * (0.83 + 0.045 * ts), -hlon * (0.91 + 0.021 * ts)
    plan = np.empty((C, T, 2))
    for j, c in enumerate(cells):
        if not len(c):
            plan[perm[j]] = centre
            continue
        d = step_deltas(c, past[j])
        h = (d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-300)).mean(0)
        h /= np.linalg.norm(h, axis=-1, keepdims=True)
        cc, ss = h[:, 0], h[:, 1]
        plan[perm[j], :, 0] = c[:, :, 0].mean(0) + cc * p + ss * q
        plan[perm[j], :, 1] = c[:, :, 1].mean(0) - ss * p + cc * q
    sel = rng.integers(-1, 4, size=(C, T)).astype(np.int32)
    # at that corner faces 1 and 2 are open for nearly every particle: every other cell selects
    # among the mixed faces 0 and 3 (and no row), so that its any-step count is mixed too
    sel[1::2] = np.array([-1, 0, 3], np.int32)[rng.integers(0, 3, size=sel[1::2].shape)]
    for j in range(C):
        if not np.any(sel[j] >= 0):
            sel[j, 0] = j % 4
    sel[counts.index(2)] = -1
    return dict(cells=cells, past=past, origin=origin, plan=plan,
                cell_plan=perm.astype(np.int32), face_sel=sel, counts=counts)


@functools.lru_cache(maxsize=None)
def reference(T, f32, T_audit=None):
    """Per cell of inputs(T, f32), audited over the first T_audit steps (default T): list of
    dict(v64, vld [n, Ta, 4], ex, ey (longdouble), want = tally(v64, face_sel), want_nosel).
    Treat as read-only."""
    inp = inputs(T, f32)
    Ta = T if T_audit is None else T_audit
    world = store_world(inp["cells"], bool(f32), inp["origin"])
    out = []
    for j, w in enumerate(world):
        row = inp["plan"][inp["cell_plan"][j]]
        v64, _, _ = values(w[:, :Ta], inp["past"][j], row)
        vld, ex, ey = values(w[:, :Ta], inp["past"][j], row, ld=True)
        out.append(dict(v64=v64, vld=vld, ex=ex, ey=ey,
                        want=tally(v64, inp["face_sel"][j, :Ta]), want_nosel=tally(v64)))
    return out


def stack(ref, name):
    return np.stack([r["want"][name] for r in ref])


def worst_errors(got, ref, hlon=0.5 * LON + 0.5 * CAR_R):
    """(the largest error of `got` [C, T, 4] against the longdouble maxima, relative to
    |ex| + |ey| + hlon at the maximising particle; the float64 restatement's own)."""
    e_got = e_own = 0.0
    for j, r in enumerate(ref):
        vld = r["vld"]
        if not vld.shape[0]:
            continue
        arg = vld.argmax(0)                                   # [T, 4]
        for t in range(vld.shape[1]):
            for f in range(4):
                i = arg[t, f]
                scale = float(abs(r["ex"][i, t]) + abs(r["ey"][i, t]) + hlon)
                e_got = max(e_got, float(abs(LD(got[j, t, f]) - vld[i, t, f])) / scale)
                e_own = max(e_own, float(abs(LD(r["v64"][:, t, f].max()) - vld[i, t, f])) / scale)
    return e_got, e_own


def allowed_worst_error(e_own):
    """The bar on out_worst: max(1e-13, 32 x the float64 restatement's own error)."""
    return max(1e-13, 32.0 * e_own)


# ---------------------------------------------------------------------------------------------
# exact ties
# ---------------------------------------------------------------------------------------------
TIE_EXTENT, TIE_CAR_R = (2.0, 2.0), 1.0       # hlat = hlon = 1.5
TIE_PLAN = np.array([[8.0, 4.0], [8.0, 4.0]])
TIE_PAST = np.array([-100.0, -50.0])


def tie_case():
    """One cell, T = 2, of particles that stand still from t = 0 to t = 1 (c = 1, s = 0 at
    t = 1, so p = ex and q = ey there) at small dyadic coordinates: for every face f one particle
    with v_f == 0 exactly at t = 1 and its neighbours one ulp to either side.  Every difference
    and sum is exact, so strictness alone decides the counts.
    Returns (cells [(12, 2, 2)], past (1, 2), plan (1, 2, 2), expect): expect[f] = (particles
    with v_f < 0, == 0, > 0 among the three built for face f)."""
    X, Y = TIE_PLAN[1]
    pts, expect = [], {}
    # face: (coordinate that ties, other coordinate); v0 = 1.5 - ex, v1 = 1.5 - ey,
    # v2 = 1.5 + ex, v3 = 1.5 + ey with ex = X - x, ey = Y - y
    for f, (axis, at) in enumerate(((0, X - 1.5), (1, Y - 1.5), (0, X + 1.5), (1, Y + 1.5))):
        lo, hi = np.nextafter(at, -np.inf), np.nextafter(at, np.inf)
        ids = []
        for val in (lo, at, hi):
            xy = [X, Y]
            xy[axis] = val
            ids.append(len(pts))
            pts.append(xy)
        # faces 0, 1: v = 1.5 - (X - x) grows with x; faces 2, 3: v = 1.5 + (X - x) falls with x
        expect[f] = (ids[0], ids[1], ids[2]) if f < 2 else (ids[2], ids[1], ids[0])
    pts = np.array(pts)
    cell = np.stack([pts, pts], axis=1)                    # (12, 2, 2): no step at t = 1
    return [cell], TIE_PAST[None].copy(), TIE_PLAN[None].copy(), expect


def make_store(T, f32, device):
    import torch
    from ccmpc import engine
    inp = inputs(T, f32)
    return engine.ParticleStore.from_cells(
        inp["cells"], device=device, dtype=torch.float32 if f32 else torch.float64,
        origin=inp["origin"])
