"""An exact (mpmath, 50 digits) restatement of what the half-space tail (constraints.hpp,
constraints.hip) and the moment reduction (moments.hip, gram.hpp) are meant to compute, the
input families of tests/test_gpu_tail_precision.py, and the float64 oracle's own error on each
family -- the yardstick the kernels are judged against.  Not a test.

Every input is taken exactly from the float64 values the device sees (for an f32 store: the
f32-rounded relative coordinates, cast to float64; the origin is added exactly, once, to the
mean -- the kernel never forms world coordinates per particle in the moment reduction, so a
per-particle rounded `rel + origin` would not be what it is meant to compute).
"""
import functools
import warnings

import mpmath as mp
import numpy as np

from oracle import ccmpc_oracle as orc

mp.mp.dps = 50
F = mp.mpf

TOL, MAXITER = 1e-8, 1000          # the cycle's own tol / maxiter
FLOOR = 1e-12                      # the level the suite calls typical (tests/test_gpu_core.py)
FACTOR = 8.0                       # <= 2 ulp primitives against IEEE's 0.5, doubled for order
BAR_Q = 1e-5                       # BASELINE.json: relative Frobenius bar on Q
MARGIN = 1e-9                      # integer decisions are compared above this exact margin


def bound(e_f):
    """The kernel's allowance for a family whose float64 oracle is e_f off the exact value."""
    return max(FACTOR * float(e_f), FLOOR)


# ---------------------------------------------------------------------------------------------
# small exact helpers: 2x2 matrices are tuples (a, b, c, d) of mpf = [[a, b], [c, d]]
# ---------------------------------------------------------------------------------------------
def m2(x):
    if isinstance(x, tuple):
        return x
    x = np.asarray(x, np.float64).reshape(4)
    return tuple(F(float(v)) for v in x)


def mul(x, y):
    return (x[0] * y[0] + x[1] * y[2], x[0] * y[1] + x[1] * y[3],
            x[2] * y[0] + x[3] * y[2], x[2] * y[1] + x[3] * y[3])


def inv(x):
    det = x[0] * x[3] - x[1] * x[2]
    if det == 0:
        return None
    return (x[3] / det, -x[1] / det, -x[2] / det, x[0] / det)


def fro(x):
    return mp.sqrt(sum(v * v for v in x))


def rel_fro(got, want):
    """|got - want|_F / |want|_F as a float; got: floats, want: mpf."""
    got = [F(float(v)) for v in np.asarray(got, np.float64).reshape(-1)]
    num = mp.sqrt(sum((g - w) ** 2 for g, w in zip(got, want)))
    den = mp.sqrt(sum(w * w for w in want))
    return float(num / den) if den != 0 else float(num)


def rel(got, want, scale=None):
    want = F(want)
    s = abs(want) if scale is None else F(scale)
    d = abs(F(float(got)) - want)
    return float(d / s) if s != 0 else float(d)


def ulp_err(got, want):
    """|got - want| in units of the last place of the float64 nearest `want` (a normal)."""
    want = F(want)
    _, e = mp.frexp(want)                       # want = m 2^e, 0.5 <= |m| < 1
    return float(abs(F(float(got)) - want) / mp.ldexp(F(1), int(e) - 53))


# ---------------------------------------------------------------------------------------------
# makeconstraint.py, exactly
# ---------------------------------------------------------------------------------------------
def compute_mvoe(S1, S2, tol=TOL, maxiter=MAXITER, iters=None):
    """makeconstraint.py:7-38 with the same iteration and stop rule; None where S1 is singular.
    dict(beta, Q, steps [|next - beta| per iteration], iters, clear, lam).  iters: run exactly
    that many iterations instead (the neighbours of a stop that is not clear)."""
    S1, S2 = m2(S1), m2(S2)
    i1 = inv(S1)
    if i1 is None:
        return None
    M = mul(i1, S2)
    half_tr, hd = (M[0] + M[3]) / 2, (M[0] - M[3]) / 2
    disc = hd * hd + M[1] * M[2]
    sd = mp.sqrt(disc) if disc >= 0 else F(0)       # .real of a complex pair
    lam = (half_tr + sd, half_tr - sd)
    tol = F(float(tol))
    beta, steps = F(1), []
    while len(steps) < maxiter:
        w = [1 + beta * l for l in lam]
        nxt = mp.sqrt(sum(1 / x for x in w) / sum(l / x for l, x in zip(lam, w)))
        steps.append(abs(nxt - beta))
        beta = nxt
        if (steps[-1] < tol) if iters is None else (len(steps) >= iters):
            break
    Q = tuple((1 + 1 / beta) * a + (1 + beta) * b for a, b in zip(S1, S2))
    clear = (steps[-1] < tol / 2 and (len(steps) < 2 or steps[-2] > 2 * tol))
    return dict(beta=beta, Q=Q, steps=steps, iters=len(steps), clear=bool(clear), lam=lam,
                S1=S1, S2=S2, converged=bool(steps[-1] < tol))


def q_slack(r, dbeta):
    """The relative Frobenius change of Q for a change dbeta of beta: |S2 - S1 / beta^2|_F
    dbeta / |Q|_F."""
    b = r["beta"]
    dq = tuple(s2 - s1 / (b * b) for s1, s2 in zip(r["S1"], r["S2"]))
    return float(fro(dq) * F(float(dbeta)) / fro(r["Q"]))


def predict_moments(C, t=1, tau=0):
    """makeconstraint.py:41-70 from a (2n x 2n) covariance whose 2x2 blocks are indexed like the
    device's: (cov_infer, cov_mu, c_t), or None where the tau block is singular."""
    C = np.asarray(C, np.float64)

    def blk(i, j):
        return m2(C[2 * i:2 * i + 2, 2 * j:2 * j + 2])
    it = inv(blk(tau, tau))
    if it is None:
        return None
    c_t = blk(t, t)
    cov_mu = mul(mul(blk(t, tau), it), blk(tau, t))
    return tuple(a - b for a, b in zip(c_t, cov_mu)), cov_mu, c_t


def _alpha_beta(cov_infer, cov_mu, c_t):
    root = mp.sqrt(fro(c_t))
    return mp.sqrt(fro(cov_infer)) / root, mp.sqrt(fro(cov_mu)) / root


def compute_lower_bound(cov_infer, cov_mu, c_t, gamma):
    """makeconstraint.py:282-303: chi2_2 cdf of (Gamma (1 - alpha) / beta)^2."""
    al, be = _alpha_beta(cov_infer, cov_mu, c_t)
    if be == 0:
        return mp.nan
    x = F(float(gamma)) * (1 - al) / be
    return -mp.expm1(-x * x / 2)


def compute_scale(cov_infer, cov_mu, c_t, gamma, chi_p):
    """makeconstraint.py:259-280."""
    al, be = _alpha_beta(cov_infer, cov_mu, c_t)
    x = mp.sqrt(F(float(chi_p))) * be / F(float(gamma)) + al
    return x * x


def closest_tangent(mu, Sigma, c, m, a):
    """tangent_lines_of_slope_m + choose_closest_tangent (makeconstraint.py:134-207) and the
    side test n.mean <= d.  None where n^T Sigma n <= 0.  dict(d, which, side, margin (exact
    |dist0 - dist1| / max), side_margin (|d - n.mu| / max(|d|, |n.mu|)), scale (|n.mu| +
    |c sqrt(n^T Sigma n)|: what d's error is measured against), cands)."""
    S = m2(Sigma) if not isinstance(Sigma, tuple) else Sigma
    mu0, mu1, a0, a1 = (v if isinstance(v, mp.mpf) else F(float(v))
                        for v in (mu[0], mu[1], a[0], a[1]))
    m = m if isinstance(m, mp.mpf) else F(float(m))
    c = c if isinstance(c, mp.mpf) else F(float(c))
    n0, n1 = -m, F(1)
    q = n0 * (S[0] * n0 + S[1] * n1) + n1 * (S[2] * n0 + S[3] * n1)
    if q <= 0:
        return None
    proj, delta = n0 * mu0 + n1 * mu1, c * mp.sqrt(q)
    cands = (proj + delta, proj - delta)
    nrm, na = mp.sqrt(n0 * n0 + n1 * n1), n0 * a0 + n1 * a1
    dist = [abs(na - d) / nrm for d in cands]
    which = 1 if dist[1] < dist[0] else 0
    d = cands[which]
    big = max(dist)
    return dict(d=d, which=which, side=1 if proj <= d else -1,
                margin=float(abs(dist[0] - dist[1]) / big) if big != 0 else 0.0,
                side_margin=float(abs(d - proj) / max(abs(d), abs(proj))),
                scale=abs(proj) + abs(delta), cands=cands, proj=proj, n0=n0)


def sqrtm2(c):
    """The principal square root of a symmetric PSD 2x2 (a, b, c, d): (A + sqrt(det) I) /
    sqrt(tr + 2 sqrt(det)); None unless det >= 0 and tr > 0."""
    det, tr = c[0] * c[3] - c[1] * c[2], c[0] + c[3]
    if det < 0 or tr <= 0:
        return None
    sd = mp.sqrt(det)
    tau = mp.sqrt(tr + 2 * sd)
    return ((c[0] + sd) / tau, c[1] / tau, c[2] / tau, (c[3] + sd) / tau)


def slope(mean, ref):
    """m = -(ref_x - mean_x) / (ref_y - mean_y), exact; None where ref_y == mean_y."""
    dy = ref[1] - mean[1]
    return None if dy == 0 else -(ref[0] - mean[0]) / dy


def affine_record(mean, cov, ref, gamma, R):
    """The GMM-affine record (v8ideal/__init__.py:1476-1515) from exact mean (2 mpf), cov
    (a, b, c, d) mpf and the float64 ref / gamma / R: dict(m, d, which, side, margin, rhs,
    tangent) or None where the covariance is not PSD or the slope is infinite."""
    ref = [F(float(v)) for v in ref]
    s = sqrtm2(cov)
    m = slope(mean, ref)
    if s is None or m is None:
        return None
    g = F(float(gamma))
    v0, v1 = s[0] * m - s[1], s[2] * m - s[3]
    margin = g * mp.sqrt(v0 * v0 + v1 * v1)
    tg = closest_tangent(mean, (F(1), F(0), F(0), F(1)), F(float(R)), m, ref)
    rhs = tg["d"] + margin if tg["side"] > 0 else tg["d"] - margin
    return dict(m=m, d=tg["d"], which=tg["which"], side=tg["side"], margin=margin, rhs=rhs,
                tangent=tg, sqrtm=s)


# ---------------------------------------------------------------------------------------------
# exact and modelled moments of a store's cells
# ---------------------------------------------------------------------------------------------
def stored(cell, f32=False, origin=None):
    """(n, 2T) float64: what the store holds of one (n, T, 2) cell (for f32: relative to origin,
    rounded to f32), and the origin (2,) to add to the mean (zeros for an f64 store)."""
    c = np.asarray(cell, np.float64)
    o = np.zeros(2) if origin is None else np.asarray(origin, np.float64).reshape(2)
    if origin is not None:
        c = c - o
    if f32:
        c = c.astype(np.float32).astype(np.float64)
    return c.reshape(c.shape[0], -1), o


def exact_moments(X, origin=None):
    """Exact mean (2T mpf, origin added exactly) and ddof = 1 covariance (2T x 2T list of mpf)
    of the stored values X (n, 2T) float64, by integer arithmetic on the values' own bits."""
    X = np.asarray(X, np.float64)
    n, D = X.shape
    cols, ks = [], []
    for r in range(D):
        ratios = [float(v).as_integer_ratio() for v in X[:, r]]
        k = max(d.bit_length() - 1 for _, d in ratios)
        cols.append([p << (k - (d.bit_length() - 1)) for p, d in ratios])
        ks.append(k)
    S = [sum(c) for c in cols]
    o = [F(0), F(0)] if origin is None else [F(float(v)) for v in origin]
    mean = [mp.ldexp(F(S[r]) / n, -ks[r]) + o[r & 1] for r in range(D)]
    cov = [[None] * D for _ in range(D)]
    for i in range(D):
        for j in range(i, D):
            G = sum(a * b for a, b in zip(cols[i], cols[j]))
            num = n * G - S[i] * S[j]                               # exact integer
            v = mp.ldexp(F(num) / (n * (n - 1)), -(ks[i] + ks[j])) if n > 1 else mp.nan
            cov[i][j] = cov[j][i] = v
    return mean, cov


def onepass_model(X, origin=None, shift=True):
    """Plain float64 NumPy model of the moment kernel's formula: shift by the cell's first
    particle, sum, Gram, (G - S S^T / n) / (n - 1); mean = (first + S / n) + origin.
    shift=False: the unshifted one-pass form (the premise of the conditioning test)."""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    sh = X[0].copy() if shift else np.zeros(X.shape[1])
    Y = X - sh
    S = Y.sum(axis=0)
    G = Y.T @ Y
    o = np.zeros(2) if origin is None else np.asarray(origin, np.float64)
    mean = (sh + S / n) + np.tile(o, X.shape[1] // 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = (G - np.outer(S, S) / n) / (n - 1.0)
    return mean, cov


def cov_err(got, cov):
    """max_ij |got_ij - cov_ij| / sqrt(cov_ii cov_jj): the covariance's error in units of the
    coordinates' own spreads (a correlation-scale error)."""
    got = np.asarray(got, np.float64)
    D = got.shape[0]
    sd = [mp.sqrt(cov[i][i]) for i in range(D)]
    return float(max(abs(F(float(got[i, j])) - cov[i][j]) / (sd[i] * sd[j])
                     for i in range(D) for j in range(D)))


def mean_err(got, mean, cov):
    """max_r |got_r - mean_r| / (1e-14 |mean_r| + the spread's share 1e-14 sd_r): <= 1 passes."""
    got = np.asarray(got, np.float64).reshape(-1)
    return float(max(abs(F(float(got[r])) - mean[r])
                     / (F("1e-14") * abs(mean[r]) + F("1e-14") * mp.sqrt(cov[r][r]))
                     for r in range(len(mean))))


# ---------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------
def _rot(th):
    return np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])


def spd(rng, scale, aspect, th=None):
    """A symmetrised R diag(l, l / aspect) R^T with l in [0.5, 2) scale."""
    th = rng.uniform(0, np.pi) if th is None else th
    l1 = scale * rng.uniform(0.5, 2.0)
    A = _rot(th) @ np.diag([l1, l1 / aspect]) @ _rot(th).T
    return 0.5 * (A + A.T)


@functools.lru_cache(maxsize=None)
def prim_inputs():
    """(n, 2) float64 (a, b): ~4000 log-uniform in [2^-200, 2^200], powers of two with the
    values one ulp either side, and 1, 2, 3, 4."""
    rng = np.random.default_rng(20261019)
    rnd = 2.0 ** rng.uniform(-200, 200, (4000, 2))
    p2 = np.ldexp(1.0, np.arange(-200, 201, 4))
    sp = np.concatenate([p2, np.nextafter(p2, 0), np.nextafter(p2, np.inf), [1.0, 2.0, 3.0, 4.0]])
    return np.concatenate([rnd, np.stack([np.roll(sp, 7)[::-1], sp], -1)])


MVOE_SCALES = (1e-10, 1e-6, 1e-2, 1.0, 1e2, 1e6)
MVOE_RATIOS = (1e-8, 1e-4, 1.0, 1e4, 1e8)
MVOE_ASPECTS = (1.0, 1e3, 1e6)
R_COLLISION = 3.4


MVOE_PER_CELL, MVOE_NONCLEAR_PER_CELL, MVOE_DRAWS = 8, 2, 24


def mvoe_aspect(asp, ratio):
    """The aspect actually used in a grid cell.  Narrowed: at aspect 1e6 and S2 / S1 >= 1e4 the
    float64 oracle alone is 1e-6 .. 3e-6 off the exact Q (8 e_f would pass the 1e-5 bar), so
    those two columns run at aspect 1e5."""
    return 1e5 if (asp == 1e6 and ratio >= 1e4) else asp


def _mvoe_cell(rng, draw, family, tag):
    """Up to MVOE_PER_CELL cases of one grid cell, of which at most MVOE_NONCLEAR_PER_CELL are
    not clear stops of the exact iteration: where the fixed point contracts by less than 4x per
    step no stop is clear (the step before a last step < tol / 2 is then < 2 tol), so such cells
    are thinned to their MVOE_NONCLEAR_PER_CELL cases instead of the cap being raised."""
    got, loose = [], 0
    for k in range(MVOE_DRAWS):
        if len(got) == MVOE_PER_CELL:
            break
        S1, S2 = draw(rng)
        r = compute_mvoe(S1, S2)
        if not r["clear"]:
            if loose == MVOE_NONCLEAR_PER_CELL:
                continue
            loose += 1
        got.append(dict(S1=S1, S2=S2, family=family, tag=tag + (k,), ref=r))
    return got


@functools.lru_cache(maxsize=None)
def mvoe_cases():
    """list of dict(S1, S2, family, tag, ref (the exact compute_mvoe)).  Families: 'aspect1',
    'aspect1000', 'aspect1e+06' (the scale x ratio grid), 'second' (Q, R^2 I over Q scales
    1e-8 .. 1e4) and 'slow' (S1 / S2 ratios 1e-12 and 1e12, aspect 1e3)."""
    rng = np.random.default_rng(20261020)
    out = []
    for asp in MVOE_ASPECTS:
        for sc in MVOE_SCALES:
            for ratio in MVOE_RATIOS:
                a = mvoe_aspect(asp, ratio)
                out += _mvoe_cell(rng, lambda g: (spd(g, sc, a), spd(g, sc * ratio, a)),
                                  f"aspect{asp:g}", (sc, ratio, asp))
    for sc in (1e-8, 1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e4):
        out += _mvoe_cell(rng, lambda g: (spd(g, sc, 10 ** g.uniform(0, 3)),
                                          R_COLLISION ** 2 * np.eye(2)), "second", (sc,))
    for ratio in (1e-12, 1e12):                         # S1 / S2
        S1, S2 = spd(rng, 1.0, 1e3), spd(rng, 1.0 / ratio, 1e3)
        out.append(dict(S1=S1, S2=S2, family="slow", tag=(ratio,), ref=compute_mvoe(S1, S2)))
    return out


@functools.lru_cache(maxsize=None)
def mvoe_reference():
    """Per case of mvoe_cases(): the exact result, the float64 oracle's result and its errors
    (e_beta relative, e_q relative Frobenius, same_iters).  Treat as read-only."""
    out = []
    for c in mvoe_cases():
        r = c["ref"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            b, Q, it = orc.compute_mvoe(c["S1"], c["S2"], TOL, MAXITER)
        out.append(dict(ref=r, o_beta=b, o_Q=Q, o_iters=it, e_beta=rel(b, r["beta"]),
                        e_q=rel_fro(Q, r["Q"]), same_iters=it == r["iters"]))
    return out


def mvoe_allowance(r, fam_err):
    """(beta relative, Q relative Frobenius) allowed for one case given its family's oracle
    errors {e_beta, e_q}: the rounding allowance bound(e_f), plus -- on a stop that is not
    clear -- tol on beta and what tol on beta moves Q."""
    ab, aq = bound(fam_err["e_beta"]), bound(fam_err["e_q"])
    if not r["clear"]:
        ab += TOL / float(r["beta"])
        aq += q_slack(r, TOL)
    return ab, aq


def family_errors(cases, refs, keys, only=lambda c, r: True):
    """{family: {key: worst of refs[i][key] over the family's cases that pass `only`}}."""
    out = {}
    for c, r in zip(cases, refs):
        if not only(c, r):
            continue
        f = out.setdefault(c["family"], {k: 0.0 for k in keys})
        for k in keys:
            v = r[k]
            if v == v:
                f[k] = max(f[k], v)
    return out


PAIR_RHO = (0.0, 1e-3, 0.5, 1 - 1e-3, 1 - 1e-6, 1 - 1e-9)
PAIR_SCALES = (1e-8, 1e-4, 1.0, 1e4)
PAIR_ASPECTS = (1.0, 1e3, 1e6)
PAIR_GAMMA, PAIR_CHI_P = 2.7344, 18.420680743952584     # norm.ppf(1 - .05 / 16), chi2.ppf(.9999)


@functools.lru_cache(maxsize=None)
def pair_cases():
    """list of dict(C (4, 4) rows (x_tau, y_tau, x_t, y_t), rho, family 'rho<v>/aspect<a>', tag).
    C_x = rho L_t W L_tau^T with Cholesky factors L and a rotation W, so every canonical
    correlation between the blocks is rho; 12 cases per (rho, aspect) over the block scales."""
    rng = np.random.default_rng(20261021)
    out = []
    for rho in PAIR_RHO:
        for asp in PAIR_ASPECTS:
            for k in range(12):
                ct = spd(rng, PAIR_SCALES[rng.integers(4)], asp)
                cu = spd(rng, PAIR_SCALES[rng.integers(4)], asp)
                cx = rho * np.linalg.cholesky(ct) @ _rot(rng.uniform(0, 2 * np.pi)) \
                    @ np.linalg.cholesky(cu).T
                C = np.block([[cu, cx.T], [cx, ct]])
                out.append(dict(C=C, rho=rho, asp=asp, family=f"rho{rho!r}/aspect{asp:g}",
                                tag=(rho, asp, k)))
    return out


def pair_exact(C):
    pm = predict_moments(C, 1, 0)
    return dict(pm=pm, lb=compute_lower_bound(*pm, PAIR_GAMMA),
                scale=compute_scale(*pm, PAIR_GAMMA, PAIR_CHI_P))


def pair_errors(ci, cm, ct, lb, sc, ex):
    """Errors of one (cov_infer, cov_mu, c_t, lower bound, scale) against pair_exact's dict.
    The blocks are measured against |c_t|_F (cov_infer + cov_mu = c_t: the backward-stable
    scale of the Schur complement) and, for the conditioning it leaves, against themselves."""
    pm = ex["pm"]
    nt = fro(pm[2])
    e = dict(e_infer=float(fro(tuple(F(float(g)) - w for g, w in
                                     zip(np.reshape(ci, 4), pm[0]))) / nt),
             e_mu=float(fro(tuple(F(float(g)) - w for g, w in zip(np.reshape(cm, 4), pm[1]))) / nt),
             e_t=rel_fro(ct, pm[2]),
             e_scale=rel(sc, ex["scale"]))
    if mp.isnan(ex["lb"]):
        e["e_lb"] = 0.0 if np.isnan(lb) else np.inf
    else:
        e["e_lb"] = rel(lb, ex["lb"]) if ex["lb"] != 0 else abs(float(lb))
    return e


@functools.lru_cache(maxsize=None)
def pair_reference():
    out = []
    for c in pair_cases():
        ex = pair_exact(c["C"])
        C = c["C"]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            cm = C[2:4, 0:2] @ np.linalg.inv(C[0:2, 0:2]) @ C[0:2, 2:4]
            ct = C[2:4, 2:4]
            ci = ct - cm
            root = np.sqrt(np.linalg.norm(ct, 'fro'))
            al = np.sqrt(np.linalg.norm(ci, 'fro')) / root
            be = np.sqrt(np.linalg.norm(cm, 'fro')) / root
            x = PAIR_GAMMA * (1 - al) / be
            lb = orc.scipy.stats.chi2.cdf(x ** 2, df=2)
            sc = (np.sqrt(PAIR_CHI_P) * be / PAIR_GAMMA + al) ** 2
        out.append(dict(ex=ex, **pair_errors(ci, cm, ct, lb, sc, ex)))
    return out


PAIR_KEYS = ("e_infer", "e_mu", "e_t", "e_lb", "e_scale")

TANGENT_M = (0.0, -0.0, 1e-8, -1e-8, 1.0, -1.0, 1e4, -1e4, 1e8, -1e8)
TANGENT_DIST = (1e-6, 1e-4, 1e-2, 1.0, 1e2, 1e4)


@functools.lru_cache(maxsize=None)
def tangent_cases():
    """list of dict(mu, Sigma, c, m, a, family 'tangent', tag): every slope x Sigma aspect
    {1, 1e3, 1e6} x (the reference point at six distances from the mean and on each of the two
    candidate lines), two draws each."""
    rng = np.random.default_rng(20261022)
    out = []
    for m in TANGENT_M:
        for asp in (1.0, 1e3, 1e6):
            for rep in range(2):
                for where in TANGENT_DIST + ("line0", "line1"):
                    mu = rng.uniform(-200, 200, 2)
                    Sig = spd(rng, 10 ** rng.uniform(-2, 2), asp)
                    c = (1.0, R_COLLISION)[rng.integers(2)]
                    if isinstance(where, float):
                        th = rng.uniform(0, 2 * np.pi)
                        a = mu + where * np.array([np.cos(th), np.sin(th)])
                    else:
                        n = np.array([-m, 1.0])
                        delta = c * np.sqrt(n @ Sig @ n) * (1 if where == "line0" else -1)
                        a = mu + delta * n / (n @ n) + rng.uniform(-5, 5) * np.array([1.0, m]) \
                            / np.hypot(1.0, m)
                    out.append(dict(mu=mu, Sigma=Sig, c=c, m=m, a=a, family="tangent",
                                    tag=(m, asp, rep, where)))
    return out


@functools.lru_cache(maxsize=None)
def tangent_reference():
    out = []
    for c in tangent_cases():
        ex = closest_tangent(c["mu"], c["Sigma"], c["c"], c["m"], c["a"])
        n, d, which = orc.choose_closest_tangent(c["mu"], c["Sigma"], c["c"], c["m"], c["a"])[:3]
        out.append(dict(ex=ex, o_d=d, o_which=which, o_side=1 if n @ c["mu"] <= d else -1,
                        e_d=rel(d, ex["cands"][which], ex["scale"])))
    return out


def tangent_rows(cases):
    return np.array([[*c["mu"], *np.reshape(c["Sigma"], 4), c["c"], c["m"], *c["a"]]
                     for c in cases])


# ---- near-singular covariances of ccmpc_affine ------------------------------------------------
SING_T = 12
SING_SCALES = (1e-4, 1.0, 1e4)
SING_KINDS = ("rank1", "rank1+1e-12", "aspect1e8")
SING_GAMMA, SING_MEAN, SING_REF_OFF = 2.5, (190.0, -80.0), (-9.0, 4.0)


@functools.lru_cache(maxsize=None)
def singular_scene():
    """Injected moments of 9 cells x T = 12: cell = (kind, scale), step t = rotation angle
    t pi / 12 + 0.1.  dict(mean (C, T, 2), cov (C, 2T, 2T), ref (T, 2), gamma (C,), blocks
    [(cell, t, (a, b, c, d) floats)])."""
    cells = [(k, s) for k in SING_KINDS for s in SING_SCALES]
    C, T = len(cells), SING_T
    mean = np.tile(np.asarray(SING_MEAN), (C, T, 1)) + np.arange(T)[None, :, None] * 0.5
    cov = np.zeros((C, 2 * T, 2 * T))
    for ci, (kind, s) in enumerate(cells):
        for t in range(T):
            th = t * np.pi / 12 + 0.1
            v = s * np.array([np.cos(th), np.sin(th)])
            if kind == "aspect1e8":
                B = _rot(th) @ np.diag([s * s, s * s * 1e-8]) @ _rot(th).T
                B = 0.5 * (B + B.T)
            else:
                B = np.outer(v, v)
                if kind == "rank1+1e-12":
                    B = B + 1e-12 * s * s * np.eye(2)
            cov[ci, 2 * t:2 * t + 2, 2 * t:2 * t + 2] = B
    ref = mean[0] + np.asarray(SING_REF_OFF)
    return dict(cells=cells, mean=mean, cov=cov, ref=ref, gamma=np.full(C, SING_GAMMA))


def plain_det(a, b, c, d):
    """float64 a d - b c as the affine kernel formed it before the compensated product."""
    return float(np.float64(a) * np.float64(d) - np.float64(b) * np.float64(c))


def _rn(x):
    """An exact rational rounded to the nearest float64 (CPython rounds int / int correctly)."""
    return x.numerator / x.denominator


def kahan_det(a, b, c, d):
    """w = b c; e = fma(-b, c, w); f = fma(a, d, -w); det = f + e -- each fma one rounding of
    the exact value, emulated with rationals."""
    from fractions import Fraction as Q
    a, b, c, d = (Q(float(v)) for v in (a, b, c, d))
    w = Q(_rn(b * c))
    e = Q(_rn(w - b * c))
    f = Q(_rn(a * d - w))
    return _rn(f + e)


def affine_model(mean, B, ref, gamma, R, det):
    """float64 NumPy model of the affine kernel's record (constraints.hip) for a given value of
    the determinant: (status_ok, margin, rhs).  sqrt and division are IEEE on both sides."""
    a, b, d = float(B[0, 0]), float(B[0, 1]), float(B[1, 1])
    if not (det >= 0.0 and a + d > 0.0):
        return False, np.nan, np.nan
    sd = np.sqrt(det)
    it = 1.0 / np.sqrt(a + d + 2.0 * sd)
    s00, s01, s11 = (a + sd) * it, b * it, (d + sd) * it
    m = -(ref[0] - mean[0]) / (ref[1] - mean[1])
    v0, v1 = s00 * m - s01, s01 * m - s11
    margin = gamma * np.sqrt(v0 * v0 + v1 * v1)
    n, dd, _ = orc.choose_closest_tangent(np.asarray(mean), np.identity(2), R, m,
                                          np.asarray(ref))[:3]
    return True, float(margin), float(dd + margin if n @ np.asarray(mean) <= dd else dd - margin)


@functools.lru_cache(maxsize=None)
def singular_reference():
    """Per (cell, t): dict(block, det_sign (of the float64 entries taken exactly), psd, ex
    (affine_record or None), plain (plain_det), kahan (kahan_det), o_margin / o_rhs (scipy
    sqrtm, as the reference computes them), e_margin, e_rhs)."""
    import scipy.linalg
    sc = singular_scene()
    out = []
    for ci in range(len(sc["cells"])):
        for t in range(SING_T):
            B = sc["cov"][ci, 2 * t:2 * t + 2, 2 * t:2 * t + 2]
            blk = m2(B)
            det = blk[0] * blk[3] - blk[1] * blk[2]
            psd = bool(det >= 0 and blk[0] + blk[3] > 0)
            mean = [F(float(v)) for v in sc["mean"][ci, t]]
            ex = affine_record(mean, blk, sc["ref"][t], sc["gamma"][ci], R_COLLISION) if psd \
                else None
            r = dict(cell=ci, t=t, det_sign=int(mp.sign(det)), psd=psd, ex=ex,
                     plain=plain_det(*B.reshape(4)), kahan=kahan_det(*B.reshape(4)))
            if psd:
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    m = -(sc["ref"][t][0] - sc["mean"][ci, t, 0]) / \
                        (sc["ref"][t][1] - sc["mean"][ci, t, 1])
                    root = scipy.linalg.sqrtm(B)
                    margin = float(np.real(sc["gamma"][ci] * np.linalg.norm(
                        root @ np.array([m, -1.0]), 2)))
                    n, d, _ = orc.choose_closest_tangent(sc["mean"][ci, t], np.identity(2),
                                                         R_COLLISION, m, sc["ref"][t])[:3]
                    rhs = d + margin if n @ sc["mean"][ci, t] <= d else d - margin
                r.update(e_margin=rel(margin, ex["margin"]),
                         e_rhs=rel(rhs, ex["rhs"], ex["tangent"]["scale"] + ex["margin"]))
                for name in ("plain", "kahan"):     # the kernel's formula with either det
                    _, mg, rh = affine_model(sc["mean"][ci, t], B, sc["ref"][t],
                                             sc["gamma"][ci], R_COLLISION, r[name])
                    r[name + "_margin"] = rel(mg, ex["margin"])
                    r[name + "_rhs"] = rel(rh, ex["rhs"], ex["tangent"]["scale"] + ex["margin"])
            out.append(r)
    return out


# ---- moments conditioning ---------------------------------------------------------------------
MOM_T = 3
MOM_COUNTS = (2, 5, 64, 257, 4100)
MOM_CONDS = ((1e2, 1.0), (1e4, 1e-2), (1e6, 1e-3))       # offset / spread
MOM_OUTLIER_CELL = 3                                      # the 257-particle cell


@functools.lru_cache(maxsize=None)
def moments_scene(ci, f32=False):
    """One store of the conditioning test: cells of MOM_COUNTS particles, T = 3, at offset /
    spread MOM_CONDS[ci]; the first particle of cell MOM_OUTLIER_CELL lies 1e3 spreads away.
    f32: an f32 store whose origin is the offset.  dict(cells, origin or None, f32)."""
    off, spread = MOM_CONDS[ci]
    rng = np.random.default_rng(20261023 + 10 * ci + int(f32))
    cells = []
    for j, n in enumerate(MOM_COUNTS):
        base = np.array([off, -0.7 * off]) + rng.uniform(-1, 1, 2) * spread
        drift = np.arange(1, MOM_T + 1)[None, :, None] * np.array([2.0, 0.5]) * spread
        walk = np.cumsum(rng.normal(0, spread, (n, MOM_T, 2)), axis=1)
        c = base + drift + walk
        if j == MOM_OUTLIER_CELL:
            c[0] += 1e3 * spread
        cells.append(c)
    origin = np.tile([off, -0.7 * off], (len(cells), 1)) if f32 else None
    return dict(cells=cells, origin=origin, f32=f32)


MOM_STORES = tuple((ci, False) for ci in range(len(MOM_CONDS))) + ((2, True),)


@functools.lru_cache(maxsize=None)
def moments_reference(ci, f32=False):
    """Per cell of moments_scene(ci, f32): dict(X, origin, mean, cov (exact), e_model (the
    shifted one-pass NumPy model's cov_err), e_unshifted, e_npcov, m_model (its mean_err))."""
    sc = moments_scene(ci, f32)
    out = []
    for j, c in enumerate(sc["cells"]):
        X, o = stored(c, f32, None if sc["origin"] is None else sc["origin"][j])
        mean, cov = exact_moments(X, o)
        mm, mc = onepass_model(X, o)
        _, uc = onepass_model(X, o, shift=False)
        out.append(dict(X=X, origin=o, mean=mean, cov=cov, e_model=cov_err(mc, cov),
                        e_unshifted=cov_err(uc, cov), e_npcov=cov_err(np.cov(X.T), cov),
                        m_model=mean_err(mm, mean, cov)))
    return out


# ---- whole records ------------------------------------------------------------------------------
REC_T = 4
REC_COUNTS = (64, 65, 300)
REC_TRANSLATIONS = (0.0, 1e3, 1e6)
REC_SCALES = (2.0 ** -10, 1.0, 2.0 ** 10)
REC_SQUEEZE = 1e3                                  # aspect, along a 30 degree axis
REC_EPS = 0.05 / REC_T
REC_FIELDS = ("mean", "m", "d", "q", "qr", "beta1", "beta2", "lb")
AFF_FIELDS = ("m", "d", "margin", "rhs", "s")
SCL_FIELDS = ("d", "margin", "rhs", "sf", "fro")


@functools.lru_cache(maxsize=None)
def record_base():
    """The base cloud (three cells around the origin, sub-metre spread growing with t) and its
    reference trajectory, before the similarity transforms."""
    rng = np.random.default_rng(20261024)
    cells = []
    for j, n in enumerate(REC_COUNTS):
        drift = np.arange(1, REC_T + 1)[None, :, None] * np.array([2.0 + j, 0.5 - j])
        walk = np.cumsum(rng.normal(0, 0.3, (n, REC_T, 2)), axis=1)
        cells.append(np.array([1.0 * j, -2.0 * j]) + drift + walk)
    ref = np.array([[-12.0 + 4.0 * (t + 1), 3.0 + 0.5 * (t + 1)] for t in range(REC_T)])
    return cells, ref


@functools.lru_cache(maxsize=None)
def record_scene(tr, scale, squeeze, f32):
    """One store of the whole-record test: x -> scale A x + (tr, -0.7 tr) with A the squeeze
    (or I), ref_traj and R scaled along; the f32 store's origin is the translation."""
    cells, ref = record_base()
    A = _rot(np.pi / 6) @ np.diag([1.0, 1.0 / REC_SQUEEZE]) @ _rot(np.pi / 6).T if squeeze \
        else np.eye(2)
    shift = np.array([tr, -0.7 * tr])
    out = [scale * (c @ A.T) + shift for c in cells]
    origin = np.tile(shift, (len(out), 1)) if f32 else None
    return dict(cells=out, ref=scale * ref + shift, R=scale * R_COLLISION, origin=origin, f32=f32,
                risk=np.tile(orc.risk_constants(REC_EPS), (len(out), 1)))


def _blk(cov, i, j):
    return (cov[2 * i][2 * j], cov[2 * i][2 * j + 1], cov[2 * i + 1][2 * j],
            cov[2 * i + 1][2 * j + 1])


def _pair_mp(cov, t, tau):
    it = inv(_blk(cov, tau, tau))
    c_t = _blk(cov, t, t)
    cov_mu = mul(mul(_blk(cov, t, tau), it), _blk(cov, tau, t))
    return tuple(a - b for a, b in zip(c_t, cov_mu)), cov_mu, c_t


def _neighbours(S1, S2):
    """The exact compute_mvoe and, where its stop is not clear, the runs one iterate shorter
    and longer: an implementation with small rounding error stops on one of them."""
    r = compute_mvoe(S1, S2)
    if r["clear"]:
        return [r]
    return [r] + [compute_mvoe(S1, S2, iters=k) for k in (r["iters"] - 1, r["iters"] + 1)
                  if 1 <= k <= MAXITER]


@functools.lru_cache(maxsize=None)
def record_reference(tr, scale, squeeze, f32):
    """The exact pipeline on the store's actual values and the float64 oracle's errors against
    it.  dict(mink [cell][pair] -> list of candidate records (one per admissible stop iterate;
    the first is the exact stop), prob_lower [cell][t], affine [cell][t], scaled / unscaled
    [cell][t], e_mink / e_affine / e_scaled {field: worst oracle error}, clear (count),
    pairs (count)).  Treat as read-only."""
    import scipy.linalg
    sc = record_scene(tr, scale, squeeze, f32)
    T, R = REC_T, F(float(sc["R"]))
    RR = (R * R, F(0), F(0), R * R)
    eye = (F(1), F(0), F(0), F(1))
    out = dict(mink=[], prob_lower=[], affine=[], scaled=[], unscaled=[], clear=0, pairs=0,
               e_mink={k: 0.0 for k in REC_FIELDS}, e_affine={k: 0.0 for k in AFF_FIELDS},
               e_scaled={k: 0.0 for k in SCL_FIELDS})
    for j, c in enumerate(sc["cells"]):
        X, o = stored(c, f32, None if sc["origin"] is None else sc["origin"][j])
        mean, cov = exact_moments(X, o)
        chi_r, chi_p, gamma = (float(v) for v in sc["risk"][j])
        W = (X.reshape(-1, T, 2) + o)                     # what the float64 reference would see
        recs_o, pl_o = orc.minkowski_cell(W.reshape(-1, 2), T, T, sc["ref"], REC_EPS, chi_r,
                                          chi_p, sc["R"])
        pairs, pl, aff, scl, uns = [], [], [], [], []
        k = 0
        for t in range(T):
            mt = (mean[2 * t], mean[2 * t + 1])
            sd = mp.sqrt(cov[2 * t][2 * t] + cov[2 * t + 1][2 * t + 1])
            rt = [F(float(v)) for v in sc["ref"][t]]
            m = slope(mt, rt)
            lbs, scales = [F(1)], [F(1)]
            for tau in range(t):
                pm = _pair_mp(cov, t, tau)
                lb = compute_lower_bound(*pm, gamma)
                lbs.append(lb)
                scales.append(compute_scale(*pm, gamma, chi_p))
                cands = []
                for r1 in _neighbours(tuple(F(chi_r) * v for v in pm[0]),
                                      tuple(F(chi_p) * v for v in pm[1])):
                    for r2 in _neighbours(r1["Q"], RR):
                        tg = closest_tangent(mt, r2["Q"], F(1), m, rt)
                        cands.append(dict(mean=mt, sd=sd, m=m, lb=lb, r1=r1, r2=r2, tg=tg,
                                          clear=r1["clear"] and r2["clear"]))
                pairs.append(cands)
                out["pairs"] += 1
                out["clear"] += cands[0]["clear"]
                ro = recs_o[k]
                k += 1
                e = min((record_errors(dict(
                    mean0=ro["mean"][0], mean1=ro["mean"][1], n0=ro["n"][0], d=ro["d"],
                    q00=ro["Q"][0, 0], q01=ro["Q"][0, 1], q11=ro["Q"][1, 1], r00=ro["QR"][0, 0],
                    r01=ro["QR"][0, 1], r11=ro["QR"][1, 1], beta1=ro["beta1"],
                    beta2=ro["beta2"], lower_bound=ro["lb"]), cd) for cd in cands),
                    key=lambda e: max(e.values()))
                for f in REC_FIELDS:
                    out["e_mink"][f] = max(out["e_mink"][f], e[f])
            pl.append(min(lbs))
            # the affine records of step t
            ex = affine_record(mt, _blk(cov, t, t), sc["ref"][t], gamma, sc["R"])
            aff.append(ex)
            p0, p1 = W[:, t, 0], W[:, t, 1]
            mo, co = np.array([np.mean(p0), np.mean(p1)]), np.cov([p0, p1])
            mf = -(sc["ref"][t][0] - mo[0]) / (sc["ref"][t][1] - mo[1])
            n, d, _ = orc.choose_closest_tangent(mo, np.identity(2), sc["R"], mf, sc["ref"][t])[:3]
            root = np.real(scipy.linalg.sqrtm(co))
            mg = gamma * np.linalg.norm(root @ np.array([mf, -1.0]), 2)
            e = affine_errors(dict(m=mf, d=d, margin=mg, rhs=d + mg if n @ mo <= d else d - mg,
                                   s00=root[0, 0], s01=root[0, 1], s11=root[1, 1]), ex)
            for f in AFF_FIELDS:
                out["e_affine"][f] = max(out["e_affine"][f], e[f])
            for scaled, dst in ((True, scl), (False, uns)):
                sf = max(scales) if scaled else F(1)
                fr = mp.sqrt(fro(tuple(sf * v for v in _blk(cov, t, t))))
                margin = F(gamma) * fr * mp.sqrt(m * m + 1)
                tg = ex["tangent"]
                dst.append(dict(sf=sf, fro=fr, margin=margin, tangent=tg, d=tg["d"],
                                which=tg["which"], side=tg["side"],
                                rhs=tg["d"] + margin if tg["side"] > 0 else tg["d"] - margin))
                sfo = 1.0
                for tau in range(t):
                    pmo = orc.predict_moments([p0, p1, W[:, tau, 0], W[:, tau, 1]])
                    sfo = max(sfo, ((np.sqrt(chi_p) * np.sqrt(np.linalg.norm(pmo[1], 'fro'))
                                     / np.sqrt(np.linalg.norm(pmo[2], 'fro')) / gamma
                                     + np.sqrt(np.linalg.norm(pmo[0], 'fro'))
                                     / np.sqrt(np.linalg.norm(pmo[2], 'fro'))) ** 2)
                                    if scaled else 1.0)
                fo = np.sqrt(np.linalg.norm(sfo * co, 'fro'))
                mgo = gamma * fo * np.linalg.norm(np.array([mf, -1.0]), 2)
                e = scaled_errors(dict(d=d, margin=mgo, s00=sfo, s01=fo,
                                       rhs=d + mgo if n @ mo <= d else d - mgo), dst[-1])
                for f in SCL_FIELDS:
                    out["e_scaled"][f] = max(out["e_scaled"][f], e[f])
        out["mink"].append(pairs)
        out["prob_lower"].append(pl)
        out["affine"].append(aff)
        out["scaled"].append(scl)
        out["unscaled"].append(uns)
        np.testing.assert_allclose(pl_o, [float(v) for v in pl], rtol=1e-5)
    return out


def record_errors(h, cd):
    """Errors of one half-space record h (mapping of ccmpc_halfspace's fields) against one
    candidate of record_reference: the mean against |mean| + spread, m relative, d against
    |n.mu| + |sqrt(n QR n)|, Q / QR relative Frobenius, betas and the lower bound relative."""
    tg = cd["tg"]
    em = max(rel(h["mean0"], cd["mean"][0], abs(cd["mean"][0]) + cd["sd"]),
             rel(h["mean1"], cd["mean"][1], abs(cd["mean"][1]) + cd["sd"]))
    return dict(mean=em, m=rel(-h["n0"], cd["m"]), d=rel(h["d"], tg["d"], tg["scale"]),
                q=rel_fro([h["q00"], h["q01"], h["q01"], h["q11"]], cd["r1"]["Q"]),
                qr=rel_fro([h["r00"], h["r01"], h["r01"], h["r11"]], cd["r2"]["Q"]),
                beta1=rel(h["beta1"], cd["r1"]["beta"]), beta2=rel(h["beta2"], cd["r2"]["beta"]),
                lb=rel(h["lower_bound"], cd["lb"]))


def affine_errors(h, ex):
    tg = ex["tangent"]
    return dict(m=rel(h["m"], ex["m"]), d=rel(h["d"], ex["d"], tg["scale"]),
                margin=rel(h["margin"], ex["margin"]),
                rhs=rel(h["rhs"], ex["rhs"], tg["scale"] + ex["margin"]),
                s=rel_fro([h["s00"], h["s01"], h["s01"], h["s11"]], ex["sqrtm"]))


def scaled_errors(h, ex):
    tg = ex["tangent"]
    return dict(d=rel(h["d"], ex["d"], tg["scale"]), margin=rel(h["margin"], ex["margin"]),
                rhs=rel(h["rhs"], ex["rhs"], tg["scale"] + ex["margin"]),
                sf=rel(h["s00"], ex["sf"]), fro=rel(h["s01"], ex["fro"]))
