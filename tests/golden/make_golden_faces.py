"""Generate the golden fixtures of the box-face ("TCST") generators.

Runs ONLY where the reference checkout exists.  The bodies of the reference's
compute_obstacle_constraints_GMM (v8ideal/__init__.py:966-1094), compute_robust_constraints_GMM
(:1096-1229) and compute_obstacle_constraints_GMM_approx (:1231-1376) are taken from the file's
syntax tree unchanged (make_golden.reference_function, sha256-pinned) and executed against a
recording stand-in for the slice of cvxpy they touch: temp_x[t] = [X0, X1, 1] as symbolic
affine scalars, `ndarray @` of them, cp.norm of an affine vector, the delta binaries, sum /
cp.sum, cp.Variable and comparisons.  All three run with road_boundary_constraints = True (the
robust method's other branch raises, np.zeros(T, L, dtype=float) at :1131), a stub Omicron and
segments.mask; S_big_repeated[l, t] then appears on each face row's right-hand side as a
recorded variable, which also names the face of an approx row.

Only inputs and outputs are stored: tests/golden/faces_o2_t8.npz and faces_o3_t12.npz.

Usage:  python tests/golden/make_golden_faces.py
"""
import logging
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import (_agent_self, _grid_cells, pack_cells, random_walk_cell,  # noqa: E402
                         reference_function)

orc = mg.orc
M_BIG = 10_000
CAR_R = 4.47213


# ---- the recording cvxpy ---------------------------------------------------------------------
class Expr:
    """lin . vars + const + sum_k coef_k |M_k xi_t|_2 ; vars are hashable names."""
    __array_ufunc__ = None

    def __init__(self, lin=None, const=0.0, norms=()):
        self.lin, self.const, self.norms = dict(lin or {}), float(const), list(norms)

    @staticmethod
    def of(v):
        return v if isinstance(v, Expr) else Expr(const=float(v))

    def __add__(self, o):
        o = Expr.of(o)
        lin = dict(self.lin)
        for k, c in o.lin.items():
            lin[k] = lin.get(k, 0.0) + c
        return Expr(lin, self.const + o.const, self.norms + o.norms)

    __radd__ = __add__

    def __neg__(self):
        return self * -1.0

    def __sub__(self, o):
        return self + (-Expr.of(o))

    def __rsub__(self, o):
        return Expr.of(o) + (-self)

    def __mul__(self, a):
        a = float(a)
        return Expr({k: a * c for k, c in self.lin.items()}, a * self.const,
                    [(a * c, M) for c, M in self.norms])

    __rmul__ = __mul__

    def __le__(self, o):
        return ("le", self, Expr.of(o))

    def __ge__(self, o):
        return ("ge", self, Expr.of(o))

    def __eq__(self, o):
        return ("eq", self, Expr.of(o))

    __hash__ = None


class Vec:
    """A row of expressions (cp.sum(Z, axis=0), S_big_repeated[i, :])."""
    __array_ufunc__ = None

    def __init__(self, items):
        self.items = list(items)

    def __rmul__(self, a):
        return Vec([a * e for e in self.items])

    def __eq__(self, o):
        return ("vec_eq", self, o)

    __hash__ = None


class Variable:
    _count = 0

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.name = f"V{Variable._count}"
        Variable._count += 1

    def __getitem__(self, idx):
        i, j = idx
        if isinstance(j, slice):
            return Vec([Expr({(self.name, i, jj): 1.0}) for jj in range(self.shape[1])[j]])
        return Expr({(self.name, i, j): 1.0})


def _norm(x, p=2):
    """cp.norm of a vector of affine scalars of one step: |M xi_t|_2, M's rows the entries'
    coefficients on (X0, X1, 1)."""
    assert p == 2
    rows, step = [], None
    for e in list(x):
        e = Expr.of(e)
        assert not e.norms
        row = [0.0, 0.0, e.const]
        for (tag, t, c), v in e.lin.items():
            assert tag == "x" and (step is None or step == t)
            step = t
            row[c] = v
        rows.append(row)
    return Expr(norms=[(1.0, (step, np.array(rows)))])


def _sum(x, axis=None):
    if isinstance(x, Variable):
        assert axis == 0
        return Vec([sum((x[i, j] for i in range(x.shape[0])), Expr()) for j in range(x.shape[1])])
    return sum(x, Expr())


def recording_cp():
    return types.SimpleNamespace(Variable=Variable, norm=_norm, sum=_sum)


def reference_methods():
    import scipy.linalg
    import scipy.stats
    path = os.path.join(mg.REF_MID, "v8ideal", "__init__.py")
    ns = {"np": np, "linalg": scipy.linalg, "norm": scipy.stats.norm, "cp": recording_cp(),
          "logging": logging}
    return {name: reference_function(path, name, cls="MidlevelAgent", namespace=ns)
            for name in ("compute_obstacle_constraints_GMM", "compute_robust_constraints_GMM",
                         "compute_obstacle_constraints_GMM_approx")}


def run_variant(fn, variant, cells_per_ov, yaws_per_ov, T, ref_traj, eps_ura):
    """One method on one planning step -> npz-ready arrays of its rows in append order."""
    K = [len(c) for c in cells_per_ov]
    O = len(K)
    ovs = [types.SimpleNamespace(n_states=K[o], pred_positions=list(cells_per_ov[o]),
                                 pred_yaws=list(yaws_per_ov[o])) for o in range(O)]
    params = types.SimpleNamespace(O=O, K=np.array(K))
    me = _agent_self(T, None)
    me.road_boundary_constraints = True
    setattr(me, "__control_horizon", T)
    temp_x = [[Expr({("x", t, 0): 1.0}), Expr({("x", t, 1): 1.0}), 1] for t in range(T)]
    Delta2 = {(o, k, t): [Expr({("delta", o, k, t, i): 1.0}) for i in range(4)]
              for o in range(O) for k in range(K[o]) for t in range(T)}
    n_seg = 3
    Omicron = np.arange(n_seg * T, dtype=float).reshape(n_seg, T) + 0.25
    segments = types.SimpleNamespace(mask=[False, True, False])
    Variable._count = 0
    args = [me, params, ovs, Delta2, Omicron, temp_x, eps_ura, segments, T]
    if variant == "approx":
        args.append(ref_traj)
    res = fn(*args)
    assert len(res) == 8
    cons = res[0]
    # the road-boundary prefix: mask rows Z[i, j] == Omicron[i, j] or 0, then L repeat rows
    n_pre = n_seg * T + 4
    for c in cons[:n_seg * T]:
        assert c[0] == "eq" and list(c[1].lin)[0][0] == "V0"
    for c in cons[n_seg * T:n_pre]:
        assert c[0] == "vec_eq"
    seq, okt, face, mean, root, coef, const = [], [], [], [], [], [], []
    for c in cons[n_pre:]:
        op, lhs, rhs = c
        if op == "eq":                              # sum(delta_ijt) == 1
            keys = sorted(lhs.lin)
            assert rhs.const == 1.0 and not rhs.lin and len(keys) == 4
            assert all(k[0] == "delta" and lhs.lin[k] == 1.0 for k in keys)
            seq.append(1)
            okt.append(keys[0][1:4])
            continue
        assert op == "le" and len(lhs.norms) == 1
        seq.append(0)
        g, (step, M) = lhs.norms[0]
        s_keys = [k for k in rhs.lin if k[0] == "V1"]
        assert len(s_keys) == 1 and rhs.lin[s_keys[0]] == 1.0 and s_keys[0][2] == step
        f = s_keys[0][1]
        d_keys = [k for k in rhs.lin if k[0] == "delta"]
        if variant == "approx":
            assert not d_keys and rhs.const == 0.0
            okt.append((-1, -1, step))
        else:
            assert len(d_keys) == 1 and d_keys[0][4] == f and d_keys[0][3] == step
            assert rhs.lin[d_keys[0]] == -M_BIG and rhs.const == M_BIG
            okt.append(d_keys[0][1:4])
        face.append(f)
        mean.append([lhs.lin[("x", step, 0)], lhs.lin[("x", step, 1)], lhs.const - 0.5 * CAR_R])
        const.append(lhs.const)
        root.append(M)
        coef.append(g)
    st_mean, st_cov = res[6], res[7]
    return {"seq": np.array(seq, np.int64), "okt": np.array(okt, np.int64).reshape(-1, 3),
            "face": np.array(face, np.int64), "mean": np.array(mean).reshape(-1, 3),
            "const": np.array(const), "root": np.array(root).reshape(-1, 3, 3),
            "coef": np.array(coef), "ovconstraint": np.bool_(res[4]),
            "state_mean": np.stack([_grid_cells(g, K) for g in st_mean], 1),
            "state_cov": np.stack([_grid_cells(g, K) for g in st_cov], 1)}


INSIDE, OUTSIDE = (165.0, -55.0), (215.0, -50.0)   # well clear of x = 190 and y = -80


def scene(rng, T, spec):
    """spec: per OV a list of (n_lo, n_hi, origin) per mode."""
    return [[random_walk_cell(rng, int(rng.integers(lo, hi)), T, origin=org)
             for lo, hi, org in modes] for modes in spec]


def main():
    import scipy.stats
    methods = reference_methods()
    scenes = {
        # OV 0 in the junction (two modes), OV 1 outside
        "faces_o2_t8": (8, 20261101, [[(90, 160, INSIDE), (90, 160, INSIDE)],
                                      [(90, 160, OUTSIDE)]]),
        # OV 0 outside; OV 1 inside; OV 2: first mode outside, LAST mode inside -> gated in
        "faces_o3_t12": (12, 20261102, [[(70, 120, OUTSIDE), (70, 120, OUTSIDE)],
                                        [(70, 120, INSIDE)],
                                        [(70, 120, OUTSIDE), (70, 120, INSIDE),
                                         (70, 120, INSIDE)]]),
    }
    for name, (T, seed, spec) in scenes.items():
        rng = np.random.default_rng(seed)
        cells = scene(rng, T, spec)
        pasts = np.array([[c[0][0, 0, 0] - 4.0, c[0][0, 0, 1] - 1.0] for c in cells])
        yaws = [[orc._step_yaws(c, pasts[o], T) for c in cs] for o, cs in enumerate(cells)]
        K = [len(c) for c in cells]
        eps_ura = np.zeros((len(K), max(K)))
        for o in range(len(K)):
            eps_ura[o, :] = 0.05 / len(K) * (1.0 + 0.1 * np.arange(max(K)))
        centre = np.mean([c[:, :, :].mean(0) for cs in cells for c in cs], axis=0)   # (T, 2)
        ref_traj = centre + np.array([-13.0, 6.0]) + 0.4 * np.arange(T)[:, None]
        counts, flat = pack_cells([c for cs in cells for c in cs])
        out = dict(T=T, K=np.array(K), counts=counts, positions=flat, past=pasts,
                   yaws=np.concatenate([y for ys in yaws for y in ys]), ref_traj=ref_traj,
                   eps_ura=eps_ura,
                   gamma=scipy.stats.norm.ppf(1 - eps_ura / T))
        for variant, fn in (("nominal", "compute_obstacle_constraints_GMM"),
                            ("robust", "compute_robust_constraints_GMM"),
                            ("approx", "compute_obstacle_constraints_GMM_approx")):
            r = run_variant(methods[fn], variant, cells, yaws, T, ref_traj, eps_ura)
            out.update({f"{variant}_{k}": v for k, v in r.items()})
        path = os.path.join(HERE, name + ".npz")
        np.savez(path, **out)
        print(name, os.path.getsize(path), "bytes;", {v: int((out[v + '_seq'] == 0).sum())
                                                      for v in ("nominal", "robust", "approx")})


if __name__ == "__main__":
    main()
