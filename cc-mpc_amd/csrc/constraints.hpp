// Per-record math of the half-space generators, shared by the standalone kernels
// (constraints.hip) and the fused moments -> half-space kernels (moments.hip, rollout.hip).
//
// Every step that decides an integer output follows the reference's operation order (which
// matrix is formed first, the strict '<' tie-break, the side test n.mean <= d) so that which and
// side match bit-for-bit and the floating outputs match to rounding.  The MVOE fixed point is
// the exception: it is set up and iterated in a shorter algebraic form (mvoe_chain), held to
// the exact reference by tests/test_gpu_tail_precision.py and tests/test_gpu_tail_algebra.py.
#pragma once
#include "ccmpc_common.hpp"

namespace ccmpc {


struct M2 {
  double a, b, c, d;  // [[a, b], [c, d]]
};

__device__ __forceinline__ M2 mul(const M2 &x, const M2 &y) {
  return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c,
          x.c * y.b + x.d * y.d};
}
__device__ __forceinline__ M2 scale(const M2 &x, double s) {
  return {x.a * s, x.b * s, x.c * s, x.d * s};
}
__device__ __forceinline__ M2 sub(const M2 &x, const M2 &y) {
  return {x.a - y.a, x.b - y.b, x.c - y.c, x.d - y.d};
}
__device__ __forceinline__ M2 add(const M2 &x, const M2 &y) {
  return {x.a + y.a, x.b + y.b, x.c + y.c, x.d + y.d};
}
__device__ __forceinline__ M2 transpose(const M2 &x) { return {x.a, x.c, x.b, x.d}; }

// Latency-lean f64 reciprocal and square root for the MVOE chain (a serial dependency chain per
// record, so each IEEE div / sqrt fix-up sequence is pure latency): hardware estimate + Newton /
// Goldschmidt refinement, <= 2 ulp (tests/test_gpu_tail_precision.py asserts it over
// [2^-200, 2^200] and measures 0.5), against the 1e-5 relative Frobenius parity bar on Q.
// The tangent choice and side test keep IEEE division, so which / side stay decided exactly
// as the reference decides them.
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}

__device__ __forceinline__ double div_nr(double a, double b) {
  const double r = rcp_nr(b);
  const double q = a * r;
  return fma(fma(-b, q, a), r, q);  // one residual correction
}

__device__ __forceinline__ double sqrt_gs(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = fma(-g, h, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  const double d = fma(-g, g, x);
  return x > 0.0 ? fma(d, h, g) : (x == 0.0 ? 0.0 : NAN);
}

// Inverse by LU with partial pivoting, as LAPACK getrf/getri does it for 2x2.  Branch-free:
// the pivot row is selected, not branched on (lanes of a wave pick different pivots, and a
// branch would run both LU paths back to back); the arithmetic per pivot choice is unchanged.
__device__ __forceinline__ bool inv2(const M2 &m, M2 &out) {
  const bool piv = fabs(m.c) > fabs(m.a);
  const double p0 = piv ? m.c : m.a, p1 = piv ? m.d : m.b;  // pivot row of P m
  const double q0 = piv ? m.a : m.c, q1 = piv ? m.b : m.d;  // other row
  const double i11 = rcp_nr(p0);
  const double l = q0 * i11;
  const double u22 = q1 - l * p1;
  const double i22 = rcp_nr(u22);
  const double i12 = -p1 * i11 * i22;
  // inv(U) = [[i11, i12], [0, i22]]; inv(L) = [[1, 0], [-l, 1]]; inv(P m) = inv(U) inv(L)
  const double x11 = i11 - i12 * l, x12 = i12, x21 = -i22 * l, x22 = i22;
  out = piv ? M2{x12, x11, x22, x21} : M2{x11, x12, x21, x22};  // inv(m) = inv(P m) P
  return p0 != 0.0 && u22 != 0.0;
}

// solve(S1, S2) = S1^{-1} S2 by the same LU (scipy.linalg.solve -> gesv)
__device__ __forceinline__ bool solve2(const M2 &s1, const M2 &s2, M2 &out) {
  M2 inv;
  if (!inv2(s1, inv)) return false;
  out = mul(inv, s2);
  return true;
}

// Build knob (profiles/r14): compute_mvoe's set-up from trace and determinant (0: by the LU
// inverse, the product and its eigenvalues, as before r14).
#ifndef CCMPC_MVOE_TRDET
#define CCMPC_MVOE_TRDET 1
#endif

// Whether the LU with partial pivoting of m (inv2, as LAPACK's getrf) meets no zero pivot: the
// `ok` flag of the tail's inverse and solve, by inv2's own instructions, for the forms that no
// longer run the LU.  It decides the record's status and its NaNs, never a value of the chain.
__device__ __forceinline__ bool lu_ok(const M2 &m) {
  const bool piv = fabs(m.c) > fabs(m.a);
  const double p0 = piv ? m.c : m.a, p1 = piv ? m.d : m.b;
  const double q0 = piv ? m.a : m.c, q1 = piv ? m.b : m.d;
  const double i11 = rcp_nr(p0);
  const double l = q0 * i11;
  const double u22 = q1 - l * p1;
  return p0 != 0.0 && u22 != 0.0;
}

// One update of the MVOE fixed point, beta' = N rsqrt(N D) with N = 2 + s beta and
// D = s + p2 beta (p2 = 2 l1 l2); see mvoe_chain.  Shared with CCMPC_SELFTEST_PRIM.
__device__ __forceinline__ double mvoe_step(double s, double p2, double b) {
  const double N = fma(s, b, 2.0), D = fma(p2, b, s);
  const double x = N * D;
  const double y = __builtin_amdgcn_rsq(x);
  // y = rsqrt(x) (1 + e) gives r = 1 - x y^2 = -(2 e + e^2), and (1 + e) (1 + r / 2 + 3/8 r^2) =
  // 1 + O(e^3): the second-order step on A = N y.  The first-order one, (1 + r / 2), is 3/2 e^2
  // off -- 17 ulp with the hardware estimate's e ~ 2^-24 -- at the same number of operations
  // and the same depth of chain (a product and an fma after r; A does not wait for r).
  const double g = x * y;
  const double r = fma(-g, y, 1.0);
  const double A = N * y;
  return fma(A * r, fma(0.375, r, 0.5), A);
}

// The serial part of compute_mvoe: the set-up (s, p2) and the fixed point's beta, with the `ok`
// flag, which nothing here waits for.
struct MvoeChain {
  double s, p2, beta;
  double prev;  // beta before the last update (CCMPC_SELFTEST_CHAIN; dead code elsewhere)
  bool ok;
};

// Set-up.  With l1, l2 the eigenvalues of M = S1^-1 S2 the fixed point needs only s = l1 + l2 =
// tr(M) and p2 = 2 l1 l2 = 2 det(M), and
//   tr(S1^-1 S2) = tr(adj(S1) S2) / det S1,   det(M) = det S2 / det S1,
// so one refined reciprocal of det S1 serves both: about 8 dependent f64 operations with one
// transcendental.  (Until r14 the LU inverse of S1, the product M and M's eigenvalues through a
// Goldschmidt square root stood here -- about 34 with three, twice per record -- and
// l2 = tr / 2 - sqrt(disc) cancelled at high aspect; tests/test_tail_algebra_host.py holds both
// forms against the exact reference.)  Plain products and differences: a compensated
// determinant is deeper, and the accuracy tests do not ask for it.  `ok` is still the LU's
// pivot test, so status is what it was on every input.
//
// Loop.  beta' = sqrt(sum 1/w / sum l/w), w = 1 + beta l  ==  sqrt(N / D) with N = w1 + w2 =
// 2 + s beta and D = l1 w2 + l2 w1 = s + 2 p beta (p = l1 l2)  ==  N rsqrt(N D): the same fixed
// point, each step one product, one hardware rsqrt and one second-order Goldschmidt step (7
// dependent f64 operations, against 17 for an IEEE division + square root; the iteration is a
// serial chain per record, so its latency is the tail's critical path).  One step is within a
// few ulp of the exact sqrt(N / D): <= 2 ulp of rounding plus O(e^3)
// (tests/test_gpu_tail_precision.py asserts <= 8 and gives the measured figure).  The stop test
// is written "not |step| >= tol": the same boolean as "|step| < tol" on every ordered pair, and
// a NaN update (a singular S1) leaves at once instead of running maxiter iterations that the LU
// form's early return used to skip.
__device__ __forceinline__ MvoeChain mvoe_chain(const M2 &S1, const M2 &S2, double tol,
                                                int maxiter) {
  MvoeChain c;
#if CCMPC_MVOE_TRDET
  c.ok = lu_ok(S1);
  const double rdet = rcp_nr(S1.a * S1.d - S1.b * S1.c);
  c.s = ((S1.d * S2.a - S1.b * S2.c) + (S1.a * S2.d - S1.c * S2.b)) * rdet;
  c.p2 = 2.0 * ((S2.a * S2.d - S2.b * S2.c) * rdet);
#else
  M2 inv;
  c.ok = inv2(S1, inv);
  const M2 M = mul(inv, S2);
  const double half_tr = 0.5 * (M.a + M.d);
  const double hd = 0.5 * (M.a - M.d);
  const double disc = hd * hd + M.b * M.c;
  // complex pair (disc < 0): .real keeps the real part of both
  const double sd = disc >= 0.0 ? sqrt_gs(disc) : 0.0;
  const double l1 = half_tr + sd, l2 = half_tr - sd;
  c.s = l1 + l2;
  c.p2 = 2.0 * (l1 * l2);
#endif
  double b = 1.0, prev = 1.0;
  for (int it = 0; it < maxiter; ++it) {
    const double bn = mvoe_step(c.s, c.p2, b);
    const bool done = !(fabs(bn - b) >= tol);
    prev = b;
    b = bn;
    if (done) break;
  }
  c.beta = b;
  c.prev = prev;
  return c;
}

// makeconstraint.py:7-38: beta by the fixed point, Q = S1 (1 + 1 / beta) + S2 (1 + beta).
// Returns ok_in && the LU pivot test of S1; where that is false, beta and Q are NaN, by selects
// on values the chain does not wait for (Q's through its S1 factor).
__device__ bool compute_mvoe(const M2 &S1, const M2 &S2, double tol, int maxiter, double &beta,
                             M2 &Q, bool ok_in = true) {
  const MvoeChain c = mvoe_chain(S1, S2, tol, maxiter);
  const bool ok = ok_in && c.ok;
  const M2 S1n = {ok ? S1.a : NAN, ok ? S1.b : NAN, ok ? S1.c : NAN, ok ? S1.d : NAN};
  beta = ok ? c.beta : NAN;
  Q = add(scale(S1n, 1.0 + rcp_nr(c.beta)), scale(S2, 1.0 + c.beta));
  return ok;
}

__device__ __forceinline__ double fro(const M2 &m) {
  return sqrt(m.a * m.a + m.b * m.b + m.c * m.c + m.d * m.d);
}

__device__ __forceinline__ M2 block(const double *cov, int rows, int i, int j) {
  const double *p = cov + (2 * i) * rows + 2 * j;
  return {p[0], p[1], p[rows], p[rows + 1]};
}

// Pair index p -> (t, tau), tau < t, p = t (t - 1) / 2 + tau.  For p < 2^20 the float estimate
// is within one of t (1 + 8 p < 2^23 + 1 is exact in float, a correctly rounded square root is
// exact at the squares (2 t - 1)^2 and the next row's start is >= 4 / (2 t + 1) > 5 ulp away),
// so one select-based correction is exact; two data-dependent while loops here compiled to
// exec-mask loops at the head of every record's chain (C2 bench step 8.93 us with the loops,
// 8.85 without, profiles/r11).  Build knob (0: the loops).
#ifndef CCMPC_PAIR_CLOSED
#define CCMPC_PAIR_CLOSED 1
#endif
__device__ __forceinline__ void pair_of(int p, int &t, int &tau) {
  int tt = static_cast<int>((1.0f + sqrtf(1.0f + 8.0f * static_cast<float>(p))) * 0.5f);
#if CCMPC_PAIR_CLOSED
  const int lo = tt * (tt - 1) / 2;  // row tt holds p in [lo, lo + tt)
  tt += lo > p ? -1 : (lo + tt <= p ? 1 : 0);
#else
  while (tt * (tt - 1) / 2 > p) --tt;
  while ((tt + 1) * tt / 2 <= p) ++tt;
#endif
  t = tt;
  tau = p - tt * (tt - 1) / 2;
}

// The same map as a table where the horizon is a compile-time constant with at most 32 pairs
// (TC <= 8): t in 4-bit fields of two 64-bit constants (pairs 0 .. 15 and 16 .. 31), the row's
// start t (t - 1) / 2 in 8-bit fields of a third, indexed by t.  Two selects, two 64-bit shifts and
// two masks in place of the closed form's float square root with its fix-up and two integer
// multiplies, which stood at the head of every record's chain.  p must be below TC (TC - 1) / 2.
// Build knob (0: the closed form everywhere).
#ifndef CCMPC_PAIR_TABLE
#define CCMPC_PAIR_TABLE 1
#endif
template <int TC>
struct PairTable {
  static constexpr int P = TC * (TC - 1) / 2;
  static constexpr bool kFits = CCMPC_PAIR_TABLE != 0 && TC >= 2 && P <= 32;
  static constexpr uint64_t t_word(int w) {
    uint64_t x = 0;
    for (int t = 1; t < TC; ++t)
      for (int tau = 0; tau < t; ++tau) {
        const int p = t * (t - 1) / 2 + tau;
        if ((p >> 4) == w) x |= static_cast<uint64_t>(t) << (4 * (p & 15));
      }
    return x;
  }
  static constexpr uint64_t start_word() {
    uint64_t x = 0;
    for (int t = 1; t < TC && t < 8; ++t) x |= static_cast<uint64_t>(t * (t - 1) / 2) << (8 * t);
    return x;
  }
};
template <int TC>
__device__ __forceinline__ void pair_of_tc(int p, int &t, int &tau) {
  if constexpr (PairTable<TC>::kFits) {
    constexpr uint64_t lo = PairTable<TC>::t_word(0), hi = PairTable<TC>::t_word(1);
    constexpr uint64_t start = PairTable<TC>::start_word();
    t = static_cast<int>(((p < 16 ? lo : hi) >> (4 * (p & 15))) & 15);
    tau = p - static_cast<int>((start >> (8 * t)) & 255);
  } else {
    pair_of(p, t, tau);
  }
}


// 16-byte store of two adjacent record fields (records are 128-byte aligned).
static_assert(sizeof(ccmpc_halfspace) == 128, "record size");
static_assert(offsetof(ccmpc_halfspace, d) == 16 && offsetof(ccmpc_halfspace, q01) == 32 &&
                  offsetof(ccmpc_halfspace, r00) == 48 && offsetof(ccmpc_halfspace, r11) == 64 &&
                  offsetof(ccmpc_halfspace, mean0) == 96 && offsetof(ccmpc_halfspace, which) == 112,
              "16-byte field pairs of ccmpc_halfspace");
__device__ __forceinline__ void store_pair(double *p, double a, double b) {
  *reinterpret_cast<double2 *>(p) = make_double2(a, b);
}

struct MinkParams {
  const double *ref_traj;    // [n_ref][T][2]
  const int32_t *cell_ref;   // [n_cells] or NULL
  const double *cell_risk;   // [n_cells][3] chi_r, chi_p, gamma
  double R, tol;
  int maxiter;
  ccmpc_halfspace *out_rec;  // [n_cells][P]
  double *out_prob_lower;    // [n_cells][T]
};

// predict_moments (makeconstraint.py:41-70) from blocks of the 2T x 2T covariance:
// cov_mu = C_t,tau C_tau^-1 C_tau,t and cov_infer = C_t - cov_mu.
struct PairMoments {
  M2 c_t, cov_mu, cov_infer;
  bool ok;
};

// The inverse of the diagonal block C_tau,tau with its `ok` flag: it depends on tau alone, so a
// cell has T of them for its T (T - 1) / 2 pairs.
struct BlockInverse {
  M2 inv;
  bool ok;
};
__device__ __forceinline__ BlockInverse block_inverse(const M2 &c_tau) {
  BlockInverse bi;
  bi.ok = inv2(c_tau, bi.inv);
  return bi;
}

__device__ __forceinline__ PairMoments pair_moments(const double *C, int rows, int t, int tau) {
  PairMoments pm;
  const BlockInverse bi = block_inverse(block(C, rows, tau, tau));
  pm.c_t = block(C, rows, t, t);
  const M2 c_x = block(C, rows, t, tau);
  const M2 c_xT = block(C, rows, tau, t);
  pm.ok = bi.ok;
  pm.cov_mu = mul(mul(c_x, bi.inv), c_xT);
  pm.cov_infer = sub(pm.c_t, pm.cov_mu);
  return pm;
}

// compute_lower_bound (makeconstraint.py:282-303):
// alpha = sqrt|cov_infer|_F / sqrt|C_t|_F, beta likewise with cov_mu, p = chi2_2 cdf
// ((Gamma (1 - alpha) / beta)^2) = 1 - exp(-x / 2).
__device__ __forceinline__ double pair_lower_bound(const PairMoments &pm, double gamma) {
  const double root_t = sqrt(fro(pm.c_t));
  const double al = sqrt(fro(pm.cov_infer)) / root_t;
  const double be = sqrt(fro(pm.cov_mu)) / root_t;
  const double x = gamma * (1.0 - al) / be;
  return -expm1(-0.5 * (x * x));
}

// compute_scale (makeconstraint.py:259-280): (sqrt(chi_p) beta / Gamma + alpha)^2.
__device__ __forceinline__ double pair_scale(const PairMoments &pm, double chi_p, double gamma) {
  const double root_t = sqrt(fro(pm.c_t));
  const double alpha = sqrt(fro(pm.cov_infer)) / root_t;
  const double beta = sqrt(fro(pm.cov_mu)) / root_t;
  const double x = sqrt(chi_p) * beta / gamma + alpha;
  return x * x;
}

// tangent_lines_of_slope_m + choose_closest_tangent (makeconstraint.py:134-207) for the normal
// n = [n0, n1] = [-m, 1] of a finite slope m, with the quantities that depend only on the mean
// and the point a precomputed by the caller: proj = n.mu, nrm = |n|, na = n.a.  Picks the
// candidate d = proj +- c sqrt(n^T S n) nearer to a under the reference's strict '<' (ties and
// NaN distances keep index 0).  Returns 0, or CCMPC_REC_NO_TANGENT where the reference returns
// its None tuple (n^T S n <= 0; a NaN n^T S n gives NaN candidates, decided by the caller's
// finiteness check).
__device__ __forceinline__ int closest_tangent(const M2 &S, double c, double n0, double n1,
                                               double proj, double nrm, double na, double &d,
                                               int &which) {
  const double sn0 = S.a * n0 + S.b * n1, sn1 = S.c * n0 + S.d * n1;
  const double q = n0 * sn0 + n1 * sn1;
  if (q <= 0.0) {
    d = NAN;
    which = 0;
    return CCMPC_REC_NO_TANGENT;
  }
  const double delta = c * sqrt(q);
  const double d1 = proj + delta, d2 = proj - delta;
  const double dist0 = fabs(na - d1) / nrm, dist1 = fabs(na - d2) / nrm;
  which = (dist1 < dist0) ? 1 : 0;
  d = which ? d2 : d1;
  return 0;
}

// The tangent's slope at step t and everything else that depends only on the step's mean
// (m0, m1) and reference point (a0, a1): the normal n = [n0, 1] = [-m, 1], proj = n.mu,
// nrm = |n|, na = n.a.  A cell has T of them for its T (T - 1) / 2 pairs.
struct TangentFrame {
  double m, n0, proj, nrm, na;
};
__device__ __forceinline__ TangentFrame tangent_frame(double m0, double m1, double a0, double a1) {
  TangentFrame f;
  f.m = -(a0 - m0) / (a1 - m1);
  f.n0 = -f.m;
  const double n1 = 1.0;
  f.proj = f.n0 * m0 + n1 * m1;
  f.nrm = sqrt(f.n0 * f.n0 + n1 * n1);
  f.na = f.n0 * a0 + n1 * a1;
  return f;
}

// One (cell, t, tau) record except its lower bound, from the cell's 2T x 2T covariance C (row
// stride `rows`) and mean mu (v8ideal/__init__.py:893-943), written straight to `out`.
// TC: the compile-time horizon (0 = run-time; see minkowski_cell), which makes the row stride of
// every covariance block an immediate.
template <int TC = 0>
__device__ void minkowski_pair(const double *C, const double *mu, const double *ref, int rows_arg,
                               int t, int tau, double chi_r, double chi_p, double R, double tol,
                               int maxiter, ccmpc_halfspace *out) {
  const int rows = TC ? 2 * TC : rows_arg;
  // the tangent frame: computed ahead of the MVOE fixed points (straight-line code the
  // scheduler overlaps with the pair-moment chain; after the data-dependent loops it would be
  // pure latency).  The compiler still sinks |n|'s square root behind the second loop and each
  // `ok` flag's chain behind its loop; holding them in front with an empty asm was built and
  // measured 0.02-0.04 us on the bench step, inside the spread (profiles/r25), and is not kept.
  const double m0 = mu[2 * t], m1 = mu[2 * t + 1];
  const TangentFrame f = tangent_frame(m0, m1, ref[2 * t], ref[2 * t + 1]);
  const double m = f.m, n0 = f.n0, n1 = 1.0, proj = f.proj, nrm = f.nrm, na = f.na;
  // the record goes out in 16-byte pairs (the lower bound at byte 88 belongs to another
  // thread), the fields known early ahead of the chain, so few stores follow its end
  store_pair(&out->n0, n0, n1);
  store_pair(&out->mean0, m0, m1);
  const PairMoments pm = pair_moments(C, rows, t, tau);
  int status = 0;
  // two MVOE calls (:915, :917-918)
  double b1 = NAN, b2 = NAN;
  M2 Q = {NAN, NAN, NAN, NAN}, QR = {NAN, NAN, NAN, NAN};
  // (a failed flag makes this call's and the next one's outputs NaN by selects; no branch sits
  // between the chains)
  bool ok = compute_mvoe(scale(pm.cov_infer, chi_r), scale(pm.cov_mu, chi_p), tol, maxiter, b1, Q,
                         pm.ok);
  store_pair(&out->q01, Q.b, Q.d);
  ok = compute_mvoe(Q, M2{R * R, 0.0, 0.0, R * R}, tol, maxiter, b2, QR, ok);
  if (!ok) status = CCMPC_REC_SINGULAR;
  store_pair(&out->r00, QR.a, QR.b);
  store_pair(&out->r11, QR.d, b1);
  out->beta2 = b2;
  // slope-m tangent of the QR ellipse closest to the reference point (:920-924)
  double d = NAN;
  int which = 0, side = 0;
  if (!isfinite(m)) {
    if (status == 0) status = CCMPC_REC_NONFINITE;
  } else {
    const int ts = closest_tangent(QR, 1.0, n0, n1, proj, nrm, na, d, which);
    if (ts != 0) {
      if (status == 0) status = ts;
    } else if (isfinite(d)) {
      side = (proj <= d) ? 1 : -1;  // (:926) n.mean <= d  ->  n.x >= d
    }
  }
  if (status == 0 && !(isfinite(d) && isfinite(Q.a) && isfinite(QR.a) && isfinite(m0)))
    status = CCMPC_REC_NONFINITE;
  store_pair(&out->d, d, Q.a);
  *reinterpret_cast<int4 *>(&out->which) = make_int4(which, side, status, (t << 16) | tau);
}

// All pairs of one cell by the threads [0, NTH) of the calling group (NTH: the kernel's
// compile-time workgroup size, never blockDim.x -- see gram.hpp), with the cell's
// reference trajectory `ref` ([T][2]) and risk constants already at hand; lb_s has room for
// T(T-1)/2 doubles.  The record of a pair is a serial chain (two MVOE fixed points, then the
// tangent) on one lane; its lower bound does not depend on that chain, so with >= 2 waves the
// lower bounds run on the upper half of the group -- other waves, i.e. truly concurrently --
// and write their record field themselves.  Up to 128 pairs that lower-bound wave also takes
// the per-t minimum (no workgroup barrier: callers must not rely on one after this call); past
// that, the barrier needed before the per-t minimum is included.
// TC, the compile-time horizon (0 = the run-time T): with it P and `half` are constants, so the
// instance holds the one path its pair count takes (at T = 8 the 28 records on threads 0 .. 27,
// the lower bounds on one wave of the other half) and not the generic pair loop beside it.
template <int NTH, int TC = 0>
__device__ void minkowski_cell(const double *C, const double *mu, int T_arg, int cell,
                               const double *ref, double chi_r, double chi_p, double gamma,
                               const MinkParams &mp, double *lb_s, int tid) {
  constexpr int nthreads = NTH;
  const int T = TC ? TC : T_arg;
  const int rows = 2 * T;
  const int P = T * (T - 1) / 2;
  ccmpc_halfspace *rec = mp.out_rec + static_cast<int64_t>(cell) * P;
  // lower bounds on the other half of the group (other waves: truly concurrent with the MVOE
  // chains) while the records fit half the threads; beyond that every thread takes whole pairs
  // (a record's chain is the tail's critical path, so fewer rounds of chains win: T = 40's 780
  // pairs on 512 threads take 2 rounds instead of 4)
  const int half = (nthreads >= 128 && P <= nthreads / 2) ? nthreads / 2 : 0;
  if (half && P <= 2 * 64) {
    // One lower-bound wave (threads [half, half + 64), up to two pairs per lane) also takes the
    // per-t minimum from its own LDS writes, so nobody waits on a workgroup barrier: the record
    // waves end with their chains (the barrier and the minimum after it used to follow the
    // longest chain).  fmin ignores NaN as the reference's min(prob_lower, x) does, in any order.
    if (tid < half) {
      if (tid < P) {
        int t, tau;
        pair_of_tc<TC>(tid, t, tau);
        minkowski_pair<TC>(C, mu, ref, rows, t, tau, chi_r, chi_p, mp.R, mp.tol, mp.maxiter,
                           rec + tid);
      }
      return;
    }
    const int lane = tid - half;
    if (lane >= 64) return;
    for (int p = lane; p < P; p += 64) {
      int t, tau;
      pair_of_tc<TC>(p, t, tau);
      const double lb = pair_lower_bound(pair_moments(C, rows, t, tau), gamma);
      lb_s[p] = lb;
      rec[p].lower_bound = lb;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes, in order
    if (lane < T) {
      double v = 1.0;
      for (int tau = 0; tau < lane; ++tau) v = fmin(v, lb_s[lane * (lane - 1) / 2 + tau]);
      mp.out_prob_lower[static_cast<int64_t>(cell) * T + lane] = v;
    }
    return;
  }
  const bool lb_side = half && tid >= half;
  const int base = lb_side ? tid - half : tid, stride = half ? half : nthreads;
  for (int p = base; p < P; p += stride) {
    int t, tau;
    pair_of_tc<TC>(p, t, tau);
    if (lb_side || !half) {
      const double lb = pair_lower_bound(pair_moments(C, rows, t, tau), gamma);
      lb_s[p] = lb;
      rec[p].lower_bound = lb;
    }
    if (!lb_side)
      minkowski_pair<TC>(C, mu, ref, rows, t, tau, chi_r, chi_p, mp.R, mp.tol, mp.maxiter, rec + p);
  }
  __syncthreads();
  for (int t = tid; t < T; t += nthreads) {
    double v = 1.0;
    for (int tau = 0; tau < t; ++tau) v = fmin(v, lb_s[t * (t - 1) / 2 + tau]);
    mp.out_prob_lower[static_cast<int64_t>(cell) * T + t] = v;
  }
}

// Same, reading the reference trajectory and risk constants from global memory.
template <int NTH>
__device__ void minkowski_cell(const double *C, const double *mu, int T, int cell,
                               const MinkParams &mp, double *lb_s, int tid) {
  const int rsel = mp.cell_ref ? mp.cell_ref[cell] : 0;
  const double *ref = mp.ref_traj + static_cast<int64_t>(rsel) * (2 * T);
  minkowski_cell<NTH>(C, mu, T, cell, ref, mp.cell_risk[3 * cell + 0],
                      mp.cell_risk[3 * cell + 1], mp.cell_risk[3 * cell + 2], mp, lb_s, tid);
}

// The unfused half-space launch (constraints.hip): one wave per (cell, t), lanes = the row's pairs.
void launch_minkowski_rows(const double *mean, const double *cov, int T, int n_cells,
                           const MinkParams &mp, hipStream_t s);

}  // namespace ccmpc
