"""NumPy restatement of ccmpc_risk_audit's contract (include/ccmpc.h), shared by the host and
GPU audit tests.  Every expression is float64 elementwise NumPy in the order the header states,
so no product is fused with a sum."""
import numpy as np

HALFSPACE, AFFINE, HALFSPACE_COMPACT, AFFINE_COMPACT = 0, 1, 2, 3
GATHER_DTYPE = np.dtype([("n0", "<f8"), ("n1", "<f8"), ("rhs", "<f8"), ("side", "<i2"),
                         ("status", "<i2"), ("t_tau", "<i4")])
assert GATHER_DTYPE.itemsize == 32


def rows(kind, T):
    return T * (T - 1) // 2 if kind in (HALFSPACE, HALFSPACE_COMPACT) else T


def rec_fields(h, kind):
    """(n0, n1, rhs, side, status, t) arrays of a structured record array of `kind`."""
    if kind == HALFSPACE:
        rhs, t = h["d"], h["t_tau"] >> 16
    elif kind == AFFINE:
        rhs, t = h["rhs"], h["t"]
    elif kind == HALFSPACE_COMPACT:
        rhs, t = h["rhs"], h["t_tau"] >> 16
    else:
        rhs, t = h["rhs"], h["t_tau"]
    return (h["n0"].astype(np.float64), h["n1"].astype(np.float64), rhs.astype(np.float64),
            h["side"].astype(np.float64), h["status"].astype(np.int64), t.astype(np.int64))


def compact(h, kind):
    """ccmpc_compact_records on the host: 128-byte records -> ccmpc_gather_rec."""
    n0, n1, rhs, side, status, _ = rec_fields(h, kind)
    g = np.zeros(h.shape, GATHER_DTYPE)
    g["n0"], g["n1"], g["rhs"] = n0, n1, rhs
    g["side"], g["status"] = side.astype(np.int16), status.astype(np.int16)
    g["t_tau"] = h["t_tau"] if kind == HALFSPACE else h["t"]
    return g


def protects(n0, n1, rhs, side, px, py, R):
    s = n0 * px + n1 * py
    v = side * (rhs - s)
    return (v >= 0) & (v * v >= (R * R) * (n0 * n0 + n1 * n1))


def audit(cells, T, R, plan=None, cell_plan=None, rec=None, kind=None):
    """cells: list of (N_c, >= T, 2) float64 world positions; plan (n_plans, T, 2) or (T, 2);
    rec: structured array [C, P] of `kind`.  Returns dict(hit, hit_any, min_d2, rec_open, open),
    None for a half that is switched off."""
    C = len(cells)
    out = dict(hit=None, hit_any=None, min_d2=None, rec_open=None, open=None)
    if plan is not None:
        plan = np.asarray(plan, np.float64)
        plan = plan[None] if plan.ndim == 2 else plan
        hit = np.zeros((C, T), np.int64)
        hit_any = np.zeros(C, np.int64)
        min_d2 = np.full((C, T), np.inf)
        for c, x in enumerate(cells):
            pl = plan[0 if cell_plan is None else int(cell_plan[c])]
            if x.shape[0] == 0:
                continue
            dx = x[:, :T, 0] - pl[None, :T, 0]
            dy = x[:, :T, 1] - pl[None, :T, 1]
            d2 = dx * dx + dy * dy
            h = d2 < R * R
            hit[c] = h.sum(0)
            hit_any[c] = h.any(1).sum()
            min_d2[c] = d2.min(0)
        out.update(hit=hit, hit_any=hit_any, min_d2=min_d2)
    if rec is not None:
        n0, n1, rhs, side, status, t = rec_fields(rec, kind)
        P = rows(kind, T)
        rec_open = np.full((C, P), -1, np.int64)
        opn = np.zeros((C, T), np.int64)
        for c, x in enumerate(cells):
            N = x.shape[0]
            prot = np.zeros((N, T), bool)
            for p in range(P):
                tp = int(t[c, p])
                if status[c, p] != 0 or not 0 <= tp < T:
                    continue
                ok = protects(n0[c, p], n1[c, p], rhs[c, p], side[c, p], x[:, tp, 0],
                              x[:, tp, 1], R)
                rec_open[c, p] = N - int(ok.sum())
                prot[:, tp] |= ok
            opn[c] = (~prot).sum(0)
        out.update(rec_open=rec_open, open=opn)
    return out
