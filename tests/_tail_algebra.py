"""Plain float64 NumPy restatements of compute_mvoe's arithmetic (constraints.hpp), one
operation per device operation and in the device's order: the set-up by trace and determinant,
the earlier set-up (LU inverse, product, eigenvalues) for comparison, the loop and Q.  IEEE
1 / x and 1 / sqrt(x) stand for the device's refined reciprocal and its reciprocal-square-root
estimate, and each fma is a product and a sum, so a model is a few ulp from the device, not
bit-equal to it.  Shared by tests/test_tail_algebra_host.py and tests/test_gpu_tail_algebra.py.
Not a test."""
import functools

import numpy as np

import _tail_ref as ref

f64 = np.float64


def step(s, p2, b):
    """One update of the fixed point from beta = b (mvoe_step)."""
    N, D = s * b + f64(2.0), p2 * b + s
    x = N * D
    y = f64(1.0) / np.sqrt(x)
    g = x * y
    r = f64(1.0) - g * y
    A = N * y
    return A * r * (f64(0.375) * r + f64(0.5)) + A


def loop(s, p2, tol=ref.TOL, maxiter=ref.MAXITER):
    """The loop from beta = 1: (beta, iterations)."""
    b, it = f64(1.0), 0
    while it < maxiter:
        bn = step(s, p2, b)
        it += 1
        done = not (abs(bn - b) >= tol)
        b = bn
        if done:
            break
    return b, it


def setup_trdet(S1, S2):
    """s = tr(adj(S1) S2) / det S1 and p2 = 2 det S2 / det S1 with one reciprocal."""
    a, b, c, d = (f64(v) for v in np.reshape(S1, 4))
    e, f, g, h = (f64(v) for v in np.reshape(S2, 4))
    r = f64(1.0) / (a * d - b * c)
    s = ((d * e - b * g) + (a * h - c * f)) * r
    p2 = f64(2.0) * ((e * h - f * g) * r)
    return s, p2


def setup_lu(S1, S2):
    """The earlier set-up: LU inverse with partial pivoting, M = S1^-1 S2, its two eigenvalues
    through a square root, s = l1 + l2 and p2 = 2 l1 l2."""
    a, b, c, d = (f64(v) for v in np.reshape(S1, 4))
    piv = abs(c) > abs(a)
    p0, p1, q0, q1 = (c, d, a, b) if piv else (a, b, c, d)
    i11 = f64(1.0) / p0
    l = q0 * i11
    u22 = q1 - l * p1
    i22 = f64(1.0) / u22
    i12 = -p1 * i11 * i22
    x11, x12, x21, x22 = i11 - i12 * l, i12, -i22 * l, i22
    inv = (x12, x11, x22, x21) if piv else (x11, x12, x21, x22)
    e, f, g, h = (f64(v) for v in np.reshape(S2, 4))
    Ma, Mb = inv[0] * e + inv[1] * g, inv[0] * f + inv[1] * h
    Mc, Md = inv[2] * e + inv[3] * g, inv[2] * f + inv[3] * h
    half_tr, hd = f64(0.5) * (Ma + Md), f64(0.5) * (Ma - Md)
    disc = hd * hd + Mb * Mc
    sd = np.sqrt(disc) if disc >= 0.0 else f64(0.0)
    l1, l2 = half_tr + sd, half_tr - sd
    return l1 + l2, f64(2.0) * (l1 * l2)


def mvoe(S1, S2, form="trdet", tol=ref.TOL, maxiter=ref.MAXITER):
    """compute_mvoe with the set-up in the given form ('trdet': the present one; 'lu': the
    earlier one): dict(s, p2, beta, Q (4,), iters)."""
    with np.errstate(all="ignore"):
        s, p2 = (setup_trdet if form == "trdet" else setup_lu)(S1, S2)
        b, it = loop(s, p2, tol, maxiter)
        Q = np.reshape(S1, 4) * (f64(1.0) + f64(1.0) / b) + np.reshape(S2, 4) * (f64(1.0) + b)
    return dict(s=s, p2=p2, beta=b, Q=Q, iters=it)


# ---- the two columns of the MVOE grid that tests/_tail_ref.py runs at aspect 1e5 ---------------
WIDE_ASPECT, WIDE_RATIO = 1e6, 1e8
WIDE_SCALES = (1e-6, 1.0, 1e6)
WIDE_CLEAR, WIDE_DRAWS, WIDE_SEED = 8, 16, 1      # seed 1: 8 clear stops in 10, 12 and 10 draws


@functools.lru_cache(maxsize=None)
def wide_cases():
    """Per scale of WIDE_SCALES: draws at aspect 1e6 with S2 / S1 = 1e8 until WIDE_CLEAR clear
    stops of the exact iteration, at most WIDE_DRAWS draws; only the clear stops are kept.
    list of dict(S1, S2, scale, ref (the exact compute_mvoe))."""
    rng = np.random.default_rng(WIDE_SEED)
    out = []
    for sc in WIDE_SCALES:
        got = 0
        for _ in range(WIDE_DRAWS):
            if got == WIDE_CLEAR:
                break
            S1 = ref.spd(rng, sc, WIDE_ASPECT)
            S2 = ref.spd(rng, sc * WIDE_RATIO, WIDE_ASPECT)
            r = ref.compute_mvoe(S1, S2)
            if r["clear"]:
                got += 1
                out.append(dict(S1=S1, S2=S2, scale=sc, ref=r))
    return out
