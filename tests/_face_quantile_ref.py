"""The oracle of the box-face Monte-Carlo calibration (cc-mpc_amd/csrc/face_quantile.hip,
ccmpc_face_quantile), built on tests/_face_audit_ref.py: per cell and allow the order statistic
of the face values by a plain sort, in float64 (the contract's order) and in np.longdouble, the
particle that attains it and that particle's cut.  Not a test.
"""
import numpy as np

import _face_audit_ref as ar
from _l4_ref import LD, step_deltas, unit

HORIZONS = (1, 2, 8, 9, 12)            # 9: the first horizon past one chunk of 8 steps
VACUOUS, SKIPPED, EMPTY = 1, 2, 1      # CCMPC_CAL_VACUOUS / _SKIPPED, CCMPC_CUT_EMPTY
BUDGET = 0.003125                      # eps_ura / ph of the golden scene: 0.05 / 2 / 8
M_NAMES = ("0", "1", "budget", "N-1", "N", "-1")


def allows_of(n):
    """The allow values every cell is calibrated at: 0, 1, floor(BUDGET N), N - 1, N, -1."""
    n = int(n)
    return (0, 1, int(np.floor(BUDGET * n)), n - 1, n, -1)


def status_of(n, m):
    return SKIPPED if m < 0 else (VACUOUS if m >= n else 0)


def select(v, m):
    """(q [T, 4], arg [T, 4]) of one cell's v [n, T, 4] (float64 or longdouble) at allow m, with
    0 <= m < n: the (m + 1)-th largest v + 0.0 by a plain stable sort, and the lowest index among
    the particles that hold its value."""
    n = v.shape[0]
    assert 0 <= m < n
    w = v + v.dtype.type(0)                       # -0 becomes +0
    order = np.argsort(w, axis=0, kind="stable")
    q = np.take_along_axis(w, order[n - 1 - m][None], 0)[0]
    arg = np.argmax(w == q[None], axis=0)         # the first index holding q
    return q, arg.astype(np.int64)


def normals(c, s):
    """n [..., 4, 2]: the gradient of v_f in (X, Y) -- (-c, s), (-s, -c), (c, -s), (s, c)."""
    return np.stack([np.stack([-c, s], -1), np.stack([-s, -c], -1),
                     np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def headings(world, past_last, ld=False):
    """(c, s) [n, T] of one cell as the kernel forms them (float64) or exactly (longdouble)."""
    d = step_deltas(np.asarray(world, np.float64), past_last)
    return unit(d) if ld else ar.heading_f64(d)


def cut(world, past_last, plan, q, arg, margin, ld=False):
    """(n [T, 4, 2], rhs [T, 4]) of the cut of the arg particles: n from that particle's heading,
    rhs = ((n0 X + n1 Y) - q) - margin in the stated order (float64), or the same in longdouble
    from the exact unit vector."""
    ft = LD if ld else np.float64
    c, s = headings(world, past_last, ld)
    T = q.shape[0]
    nrm = normals(c, s)                                        # [n, T, 4, 2]
    tt, ff = np.meshgrid(np.arange(T), np.arange(4), indexing="ij")
    nsel = nrm[arg, tt, ff]                                    # [T, 4, 2]
    P = np.asarray(plan, np.float64)[:T, :2].astype(ft)
    rhs = ((nsel[..., 0] * P[:, None, 0] + nsel[..., 1] * P[:, None, 1]) - q.astype(ft)) - ft(margin)
    return nsel, rhs


def reference(T, f32, k):
    """Per cell of ar.inputs(T, f32) at its k-th allow (allows_of): dict(m, status, and where
    status == 0: q64, arg64 from the float64 values, qld, argld from the longdouble ones)."""
    ref = ar.reference(T, f32)
    out = []
    for r in ref:
        n = r["v64"].shape[0]
        m = allows_of(n)[k]
        d = dict(m=m, n=n, status=status_of(n, m))
        if d["status"] == 0:
            d["q64"], d["arg64"] = select(r["v64"], m)
            d["qld"], d["argld"] = select(r["vld"], m)
        out.append(d)
    return out


def tie_store_cells():
    """ar.tie_case() with every particle twice (index i and i + 12): every value is held by at
    least two particles, the lower index of which is the arg."""
    cells, past, plan, expect = ar.tie_case()
    return [np.concatenate([cells[0], cells[0]])], past, plan, expect
