"""A precise NumPy restatement of what the L4 kernels (cc-mpc_amd/csrc/l4.hip) return, the
inputs of the L4 edge tests, and a thin caller of ccmpc_l4 / ccmpc_l4_split that takes
pre-filled outputs and a pre-filled workspace.  Not a test.

Inside: np.longdouble (64-bit mantissa), float64 where the reference planner rounds (the step
deltas and np.arctan2 of them, ovehicle.py:72-76).  Everything starts from what the store
really holds: for an f32 store the f32-rounded relative coordinates, cast to float64, plus
origin -- the kernels' `world()`.
"""
import ctypes
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the L4 reference needs an extended-precision np.longdouble"

U = 2.0 ** -52            # the unit of the heading bound
TINY = 2.0 ** -1022

# build knobs of l4.hip the tests' premises restate (a changed knob fails the premise asserts)
ONE_WG_THREADS, ONE_WG_CACHED = 1024, 5120      # kL4Threads, kL4Cache * kL4Threads
SPLIT_CHUNK, SPLIT_PRELOADED, SPLIT_MAX = 2048, 2048, 64   # CCMPC_L4_SPLIT_CHUNK, kL4Pre * 512


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
def store_world(cells, f32=False, origin=None):
    """World-frame float64 coordinates as the kernels read them back from a ParticleStore built
    by from_cells(cells, dtype, origin): list of (n, T, 2)."""
    out = []
    for j, c in enumerate(cells):
        c = np.asarray(c, np.float64)
        if origin is not None:
            o = np.asarray(origin, np.float64).reshape(-1, 2)[j]
            c = c - o
        if f32:
            c = c.astype(np.float32).astype(np.float64)
        if origin is not None:
            c = c + o
        out.append(c)
    return out


def step_deltas(world, past_last):
    """(n, T, 2) float64 step deltas, step 0 measured from past_last (oracle._step_yaws)."""
    d = np.empty_like(world)
    d[:, 0] = world[:, 0] - np.asarray(past_last, np.float64)
    d[:, 1:] = world[:, 1:] - world[:, :-1]
    return d


def yaw(d):
    return np.arctan2(d[..., 1], d[..., 0])


def unit(d):
    """The exact unit vector d / |d| in longdouble (C, S); a zero delta gives cos / sin of
    arctan2's answer for it, as the reference planner computes."""
    dx, dy = d[..., 0].astype(LD), d[..., 1].astype(LD)
    n = np.sqrt(dx * dx + dy * dy)
    zero = n == 0
    n = np.where(zero, LD(1), n)
    y0 = yaw(d).astype(LD)
    return np.where(zero, np.cos(y0), dx / n), np.where(zero, np.sin(y0), dy / n)


def cs_of_yaw(y):
    """cos / sin of the float64 heading, in longdouble."""
    y = np.asarray(y).astype(LD)
    return np.cos(y), np.sin(y)


def vertices(xy, C, S, lon, lat):
    """Box corners in the order of write_corners / oracle.vertices_of_bboxes:
    xy (..., 2), C, S (...) -> (..., 4, 2) float64."""
    C, S = np.asarray(C).astype(LD), np.asarray(S).astype(LD)
    lon, lat = LD(lon), LD(lat)
    x, y = xy[..., 0].astype(LD), xy[..., 1].astype(LD)
    h = LD(0.5)
    cx = np.stack([x + h * (C * lon + S * lat), x + h * (C * lon - S * lat),
                   x + h * (-C * lon - S * lat), x + h * (-C * lon + S * lat)], -1)
    cy = np.stack([y + h * (S * lon - C * lat), y + h * (S * lon + C * lat),
                   y + h * (-S * lon + C * lat), y + h * (-S * lon - C * lat)], -1)
    return np.stack([cx, cy], -1).astype(np.float64)


def yaw_mean(y):
    """Mean over particles (axis 0) of float64 headings, accumulated in longdouble."""
    return (np.sum(y.astype(LD), axis=0) / LD(y.shape[0])).astype(np.float64)


def yaw0_var(y0):
    """ddof = 1 variance in longdouble; NaN for one particle, as np.var(ddof=1) gives."""
    n = y0.shape[0]
    if n < 2:
        return np.nan
    y = y0.astype(LD)
    m = np.sum(y) / LD(n)
    return float(np.sum((y - m) ** 2) / LD(n - 1))


def A_of(theta):
    """A = [I; -I] R(theta): (..., 4, 2) float64."""
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([np.stack([c, s], -1), np.stack([-s, c], -1),
                     np.stack([-c, -s], -1), np.stack([s, -c], -1)], -2)


def b_of(theta, vert):
    """max over particles and corners of A(theta) v, vert (n, 4, 2): (b (4,) float64, the
    particle that attains each maximum (4,))."""
    A = A_of(np.float64(theta)).astype(LD)
    p = np.einsum("rk,nck->rnc", A, vert.astype(LD)).max(axis=2)    # (4, n)
    return p.max(axis=1).astype(np.float64), p.argmax(axis=1)


def reference(cells, past_last, bbox, f32=False, origin=None, heading="unit"):
    """Per cell: dict(world, d, yaw (n, T), C, S, vertices (n, T, 4, 2), yaw_mean (T,),
    yaw0_var).  heading = "unit": corners from the exact unit vector; "yaw": from cos / sin of
    the float64 heading (the reference planner's own arithmetic)."""
    out = []
    for j, w in enumerate(store_world(cells, f32, origin)):
        d = step_deltas(w, past_last[j])
        y = yaw(d)
        C, S = unit(d) if heading == "unit" else cs_of_yaw(y)
        out.append(dict(world=w, d=d, yaw=y, C=C, S=S,
                        vertices=vertices(w, C, S, bbox[j][0], bbox[j][1]),
                        yaw_mean=yaw_mean(y), yaw0_var=yaw0_var(y[:, 0])))
    return out


# ---------------------------------------------------------------------------------------------
# the caller
# ---------------------------------------------------------------------------------------------
def split_factor(n_cells, n_bound):
    """S of ccmpc_l4_split, restated: min(64, ceil(ceil(n_bound / C) / 2048)), at least 1."""
    per = -(-int(n_bound) // int(n_cells))
    return max(1, min(SPLIT_MAX, -(-per // SPLIT_CHUNK)))


def chunks(n, S):
    """[i0, i1) of each of the S chunk workgroups of an n-particle cell (l4_cell)."""
    c = -(-n // S)
    return [(k * c, min(n, (k + 1) * c)) for k in range(S)]


def run_l4(store, past_last, bbox, split, out_yaw=None, out_vertices=None, workspace=None):
    """ccmpc_l4 (split=False) or ccmpc_l4_split through ccmpc._lib.load(), as engine.l4 calls
    them, on pre-filled out_yaw [T, ld] / out_vertices [8 T, ld] and, for the split form, a
    pre-filled uint8 workspace tensor.  Synchronises; returns the tensors in a dict."""
    import torch
    from ccmpc import _lib
    lib = _lib.load()
    C, T, dev = store.n_cells, store.T, store.device
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(A=torch.empty((C, T, 4, 2), **f64), b=torch.empty((C, T, 4), **f64),
               yaw_mean=torch.empty((C, T), **f64), yaw0_var=torch.empty((C,), **f64),
               yaw=out_yaw if out_yaw is not None else torch.empty((T, store.ld), **f64),
               vertices=(out_vertices if out_vertices is not None
                         else torch.empty((8 * T, store.ld), **f64)))
    assert out["yaw"].shape == (T, store.ld) and out["vertices"].shape == (8 * T, store.ld)
    assert out["yaw"].is_contiguous() and out["vertices"].is_contiguous()
    pl = torch.as_tensor(np.ascontiguousarray(past_last, np.float64).reshape(C, 2), device=dev)
    bb = torch.as_tensor(np.ascontiguousarray(bbox, np.float64).reshape(C, 2), device=dev)

    def p(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if split:
        need = lib.ccmpc_l4_workspace_bytes(T, C, store.n_bound)
        if workspace is None:
            workspace = torch.zeros(need, dtype=torch.uint8, device=dev)
        assert workspace.dtype == torch.uint8 and workspace.numel() >= need
        _lib.check(lib.ccmpc_l4_split(
            p(store.pos), store.ccmpc_dtype, store.ld, T, p(store.origin), p(store.cell_off),
            p(store.cell_cnt), C, store.n_bound, p(pl), p(bb), p(workspace), workspace.numel(),
            p(out["A"]), p(out["b"]), p(out["yaw_mean"]), p(out["yaw0_var"]), p(out["yaw"]),
            p(out["vertices"]), stream), "ccmpc_l4_split")
        out["workspace"] = workspace
    else:
        _lib.check(lib.ccmpc_l4(
            p(store.pos), store.ccmpc_dtype, store.ld, T, p(store.origin), p(store.cell_off),
            p(store.cell_cnt), C, p(pl), p(bb), p(out["A"]), p(out["b"]), p(out["yaw_mean"]),
            p(out["yaw0_var"]), p(out["yaw"]), p(out["vertices"]), stream), "ccmpc_l4")
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------
# inputs of the heading-accuracy test
# ---------------------------------------------------------------------------------------------
NEAR_AXIS_J_SMALL = list(range(1, 61))
NEAR_AXIS_J_FAR = [100, 300, 520, 540, 600, 1000, 1074]
LADDER_E = sorted(set(range(-545, -504)) | set(range(500, 513)) | set(range(-496, 500, 16)))


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e, np.int64))


@functools.lru_cache(maxsize=None)
def heading_points(f32):
    """The step deltas d of the heading test by family: dict name -> (k, 2) float64.  f32: the
    same families restricted to values float32 holds exactly, |exponent| <= 60."""
    rng = np.random.default_rng(20240607)
    ang = -rng.uniform(-np.pi, np.pi, 4096)             # (-pi, pi]
    mag = 2.0 ** rng.uniform(-40, 40, 4096)
    random = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    if f32:
        random = random.astype(np.float32).astype(np.float64)
    js = NEAR_AXIS_J_SMALL + ([] if f32 else NEAR_AXIS_J_FAR)

    def near(js):
        out = []
        for j in js:
            e = float(_pow2(-j))
            for sa in (1.0, -1.0):
                for sb in (1.0, -1.0):
                    out += [(sa, sb * e), (sb * e, sa)]
        return out
    axis_small = np.array(near(NEAR_AXIS_J_SMALL))
    axis_rest = near([j for j in js if j > 60]) + [(1.0, 0.0), (-1.0, 0.0), (0.0, 1.0),
                                                   (0.0, -1.0), (0.0, 0.0)]
    es = [e for e in LADDER_E if abs(e) <= 60] if f32 else LADDER_E
    ladder = np.concatenate([_pow2(es)[:, None] * np.array(v)[None]
                             for v in ((3.0, 4.0), (1.0, 0.0), (1.0, 1.0))])
    fam = dict(random=random, near_axis=axis_small, near_axis_far=np.array(axis_rest),
               ladder=ladder)
    for v in fam.values():
        assert np.all(np.isfinite(v))
        if f32:
            assert np.all(v.astype(np.float32).astype(np.float64) == v)
    return fam


# ---------------------------------------------------------------------------------------------
# inputs of the edge-shape tests
# ---------------------------------------------------------------------------------------------
FAMILIES = ("narrow", "straddle", "identical", "uniform")

# (name, split, counts, T, capacity)
EDGE_CASES = [
    ("one_t3", False, [1, 2, 63, 64, 65, 1023, 1024, 1025, 5119, 5120, 5121, 6200], 3, None),
    ("one_t1", False, [1, 2, 63, 64, 65, 1023, 1024, 1025, 5119, 5120, 5121, 6200], 1, None),
    ("one_t40", False, [65, 1025], 40, None),
    ("split_tail", True, [9000, 100, 100, 100], 3, None),
    ("split_empty", True, [10000, 2], 3, None),
    ("split_cap", True, [100, 37, 1], 3, 3 * 64 * 2048),
    ("split_4096", True, [4096, 4097, 4095], 3, None),
    ("split_t40", True, [65, 1025], 40, None),
]
EDGE_CASE = {c[0]: c for c in EDGE_CASES}


def store_bound(counts, capacity=None, align=32):
    """n_bound of engine.ParticleStore for these cell counts (cells at multiples of align)."""
    cur = 0
    for c in counts:
        cur = -(-(cur + c) // align) * align
    return cur if capacity is None else max(cur, capacity)


def plant_candidates(n, S):
    """Particle indices that sit at the edges of the kernels' code-path regions.  S = None: the
    one-workgroup form (register-cached below 5120, re-read above); else the split form's
    chunks: first and last particle of each, and the first one past the preloaded 2048."""
    if S is None:
        c = [0, n - 1, ONE_WG_THREADS - 1, ONE_WG_THREADS, ONE_WG_CACHED - 1, ONE_WG_CACHED]
    else:
        c = []
        for i0, i1 in chunks(n, S):
            if i1 > i0:
                c += [i0, i1 - 1, i0 + SPLIT_PRELOADED]
    out = []
    for i in c:
        if 0 <= i < n and i not in out:
            out.append(i)
    return out


def region_of(i, n, S):
    """The code path that handles particle i of an n-particle cell."""
    if S is None:
        return "one:first" if i < ONE_WG_THREADS else ("one:cached" if i < ONE_WG_CACHED
                                                       else "one:tail")
    for k, (i0, i1) in enumerate(chunks(n, S)):
        if i0 <= i < i1:
            where = "preloaded" if i < i0 + SPLIT_PRELOADED else "tail"
            return f"split:{'chunk0' if k == 0 else 'later'}:{where}"
    raise ValueError(i)


@functools.lru_cache(maxsize=None)
def edge_scene(name, f32):
    """One edge case's inputs: dict(cells [(n, T, 2)], past_last (C, 2), bbox (C, 2), origin
    (C, 2) or None, family [str], S (None for the one-workgroup form), planted {(cell, t, face):
    particle}).  Random walks from past_last with steps of 1-5 m whose headings follow the
    cell's family; then one particle is pushed ~50 m out of the cloud along each face direction
    of every (cell, t), at an index on the edge of a code-path region (plant_candidates), so
    that b's maximum is attained on every path.  Identical-delta cells get none at t = 0: their
    t = 0 headings must stay bit-identical (variance exactly 0).  Treat as read-only."""
    _, split, counts, T, capacity = EDGE_CASE[name]
    ci = [c[0] for c in EDGE_CASES].index(name)
    rng = np.random.default_rng(1000 + 2 * ci + int(f32))
    C = len(counts)
    S = split_factor(C, store_bound(counts, capacity)) if split else None
    cells, family, planted = [], [], {}
    past_last = np.zeros((C, 2))
    origin = np.zeros((C, 2)) if f32 else None
    bbox = np.tile([4.5, 2.5], (C, 1)) + rng.uniform(-0.5, 0.5, (C, 2))
    for j, n in enumerate(counts):
        fam = FAMILIES[(j + ci) % 4]
        family.append(fam)
        if f32:
            origin[j] = np.array([1000.0, -2000.0]) + rng.uniform(-50, 50, 2)
            past_last[j] = origin[j] + rng.uniform(-4, 4, 2)
        else:
            past_last[j] = rng.uniform(-100, 100, 2)
        m = 1 if fam == "identical" else n
        length = rng.uniform(1.0, 5.0, (m, T))
        if fam == "narrow":
            h = 0.3 + rng.uniform(-0.1, 0.1, (m, T))
        elif fam == "straddle":
            h = np.pi + rng.uniform(-0.2, 0.2, (m, T))
        elif fam == "identical":
            h = 0.3 + rng.uniform(-0.5, 0.5, (m, T))
        else:
            h = rng.uniform(-np.pi, np.pi, (m, T))
        step = length[..., None] * np.stack([np.cos(h), np.sin(h)], -1)
        pos = past_last[j] + np.cumsum(step, axis=1)
        pos = np.repeat(pos, n // m, axis=0)
        # the extremes, along the faces of the cloud's own mean heading
        d = step_deltas(pos, past_last[j])
        theta = yaw(d).mean(axis=0)
        centre = pos.mean(axis=0)
        cand = plant_candidates(n, S)
        for t in range(T):
            if fam == "identical" and t == 0:
                continue
            used = set()
            for f in range(4):
                k = 4 * t + f + j
                pick = next((cand[(k + r) % len(cand)] for r in range(len(cand))
                             if cand[(k + r) % len(cand)] not in used), None)
                if pick is None:
                    continue
                used.add(pick)
                a = theta[t] + f * np.pi / 2
                pos[pick, t] = centre[t] + rng.uniform(45, 55) * np.array([np.cos(a), np.sin(a)])
                planted[(j, t, f)] = pick
        cells.append(pos)
    return dict(cells=cells, past_last=past_last, bbox=bbox, origin=origin, family=family, S=S,
                planted=planted, T=T, counts=list(counts), capacity=capacity, split=split)


@functools.lru_cache(maxsize=None)
def edge_reference(name, f32):
    """reference() of edge_scene(name, f32), computed once.  Treat as read-only."""
    sc = edge_scene(name, f32)
    return reference(sc["cells"], sc["past_last"], sc["bbox"], f32, sc["origin"])
