"""NumPy restatement of ccmpc_risk_quantile's contract (include/ccmpc.h), shared by the host and
GPU calibration tests.  Every expression is float64 elementwise NumPy in the order the header
states: w from two products and a sum, q from a sort, u* by bisection over the ordered integer
images of the doubles with _audit_ref.protects as the predicate."""
import numpy as np

import _audit_ref as ar

CAL_OK, CAL_VACUOUS, CAL_SKIPPED = 0, 1, 2
_SIGN = np.uint64(1 << 63)
KEY_NEG_INF = int(~np.array(-np.inf).view(np.uint64))
KEY_POS_INF = int(np.array(np.inf).view(np.uint64) | _SIGN)


def key(x):
    """Order-preserving uint64 image of float64 values (no -0 / NaN expected)."""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | _SIGN)


def unkey(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where(k >> np.uint64(63), k & ~_SIGN, ~k).view(np.float64)


def projections(n0, n1, side, px, py):
    """w_i = side * (n0*px + n1*py) + 0.0 (the + 0.0 makes -0 a +0)."""
    s = n0 * px + n1 * py
    return side * s + 0.0


def offset(n0, n1, side, px, py, R):
    """u* per element: the smallest double u for which _audit_ref.protects holds for the
    particle (px, py) under rhs = side*u; +inf where no double does.  Arrays of equal shape."""
    n0, n1, side, px, py = (np.ascontiguousarray(a, np.float64).reshape(-1)
                            for a in np.broadcast_arrays(n0, n1, side, px, py))

    def pred(k):
        with np.errstate(all="ignore"):
            return ar.protects(n0, n1, side * unkey(k), side, px, py, R)

    lo = np.full(n0.shape, KEY_NEG_INF, np.uint64)
    hi = np.full(n0.shape, KEY_POS_INF, np.uint64)
    none, all_ = ~pred(hi), pred(lo)
    for _ in range(64):
        mid = lo + ((hi - lo) >> np.uint64(1))
        go = (hi - lo) > np.uint64(1)
        p = pred(mid)
        hi = np.where(go & p, mid, hi)
        lo = np.where(go & ~p, mid, lo)
    assert np.all(hi - lo == np.uint64(1))
    out = unkey(hi)
    out[none] = np.inf
    out[all_] = -np.inf
    return out


def quantile(cells, T, R, rec, kind, allow=None):
    """cells: list of (N_c, >= T, 2) float64 world positions; rec: structured array [C, P] of
    `kind`; allow [C] ints or None (zeros).  Returns dict(q, rhs, status [C, P], and for the
    round-trip checks n_gt = #{w > q}, n_ge = #{w >= q}; -1 where not calibrated)."""
    C = len(cells)
    n0, n1, rhs, side, status, t = ar.rec_fields(rec, kind)
    P = ar.rows(kind, T)
    allow = np.zeros(C, np.int64) if allow is None else np.asarray(allow, np.int64)
    q = np.full((C, P), np.nan)
    out_rhs = rhs[:, :P].astype(np.float64).copy()
    st = np.full((C, P), CAL_SKIPPED, np.int32)
    n_gt = np.full((C, P), -1, np.int64)
    n_ge = np.full((C, P), -1, np.int64)
    sel = []          # (c, p, px, py) of the particle that attains q
    for c, x in enumerate(cells):
        N, m = x.shape[0], int(allow[c])
        for p in range(P):
            tp = int(t[c, p])
            if (status[c, p] != 0 or not 0 <= tp < T or not np.isfinite(n0[c, p])
                    or not np.isfinite(n1[c, p]) or m < 0):
                continue
            if m >= N:
                st[c, p], q[c, p] = CAL_VACUOUS, -np.inf
                continue
            w = projections(n0[c, p], n1[c, p], side[c, p], x[:, tp, 0], x[:, tp, 1])
            order = np.argsort(w, kind="stable")
            i = order[N - 1 - m]
            st[c, p], q[c, p] = CAL_OK, w[i]
            n_gt[c, p], n_ge[c, p] = int((w > w[i]).sum()), int((w >= w[i]).sum())
            sel.append((c, p, x[i, tp, 0], x[i, tp, 1]))
    if sel:
        cs = np.array([s[0] for s in sel])
        ps = np.array([s[1] for s in sel])
        u = offset(n0[cs, ps], n1[cs, ps], side[cs, ps], np.array([s[2] for s in sel]),
                   np.array([s[3] for s in sel]), R)
        out_rhs[cs, ps] = side[cs, ps] * u
    return dict(q=q, rhs=out_rhs, status=st, n_gt=n_gt, n_ge=n_ge)
