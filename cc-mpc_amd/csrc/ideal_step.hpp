// predict_ideal's per-step plan and sample recursion, shared by the kernels that generate the
// rollout's samples: ideal_rollout_kernel / ideal_gram_kernel (rollout.hip) and
// ideal_audit_kernel (ideal_audit.hip).  A sample is a pure function of (seed, rng, i, t) and
// the source moments, so every kernel that calls these in this order holds the same bits.
#pragma once
#include "ccmpc_common.hpp"

namespace ccmpc {

struct StepPlan {
  double a00, a01, a10, a11;  // A_t
  double l00, l10, l11;       // L_t (lower)
  double mu0, mu1;            // mu_t
  double nu0, nu1;            // mu_{t+1}
};

// Builds plan[t] for t < T (called by lanes t < T).  Returns a CCMPC_REC_* code or 0.  On a
// code every field of the plan is NaN: the plan lives in LDS, which keeps what the last
// workgroup left there, and both kernels advance through a failed step like any other -- so a
// failed cell's outputs are NaN from that step on, whatever ran before (ccmpc.h).
__device__ int build_step(const double *__restrict__ mean, const double *__restrict__ cov,
                          int rows_src, int t, StepPlan &sp) {
  auto fail = [&](int code) {
    sp.a00 = sp.a01 = sp.a10 = sp.a11 = NAN;
    sp.l00 = sp.l10 = sp.l11 = NAN;
    sp.mu0 = sp.mu1 = sp.nu0 = sp.nu1 = NAN;
    return code;
  };
  auto blk = [&](int i, int j, double &a, double &b, double &c, double &d) {
    const double *p = cov + (2 * i) * rows_src + 2 * j;
    a = p[0];
    b = p[1];
    c = p[rows_src];
    d = p[rows_src + 1];
  };
  double s0, s1, s2, s3, n0, n1, n2, n3, c0, c1, c2, c3;
  blk(t, t, s0, s1, s2, s3);          // cov_tau
  blk(t + 1, t + 1, n0, n1, n2, n3);  // cov_next
  blk(t + 1, t, c0, c1, c2, c3);      // C_t_tp1 = cross_cov[t+1][t]
  const double det = s0 * s3 - s1 * s2;
  if (det == 0.0 || !isfinite(det)) return fail(CCMPC_REC_SINGULAR);
  const double inv_det = 1.0 / det;
  const double i0 = s3 * inv_det, i1 = -s1 * inv_det, i2 = -s2 * inv_det, i3 = s0 * inv_det;
  sp.a00 = c0 * i0 + c1 * i2;
  sp.a01 = c0 * i1 + c1 * i3;
  sp.a10 = c2 * i0 + c3 * i2;
  sp.a11 = c2 * i1 + c3 * i3;
  // cond_cov = cov_next - A C^T ; Cholesky reads the lower triangle (potrf 'L')
  const double k00 = n0 - (sp.a00 * c0 + sp.a01 * c1);
  const double k10 = n2 - (sp.a10 * c0 + sp.a11 * c1);
  const double k11 = n3 - (sp.a10 * c2 + sp.a11 * c3);
  if (!(k00 > 0.0)) return fail(CCMPC_REC_NOT_PD);
  sp.l00 = sqrt(k00);
  sp.l10 = k10 / sp.l00;
  const double r = k11 - sp.l10 * sp.l10;
  if (!(r > 0.0)) return fail(CCMPC_REC_NOT_PD);
  sp.l11 = sqrt(r);
  sp.mu0 = mean[2 * t];
  sp.mu1 = mean[2 * t + 1];
  sp.nu0 = mean[2 * t + 2];
  sp.nu1 = mean[2 * t + 3];
  return 0;
}

// x0 = given, or mean_0 + chol(cov_0) z with z = Philox pair (0, 0, rng, X0 stream)
__device__ void initial_draw(const double *__restrict__ mean, const double *__restrict__ cov,
                             int rows_src, const double *__restrict__ x0, int cell, uint32_t rng,
                             uint64_t seed, double &x, double &y, int &status) {
  if (x0) {
    x = x0[2 * cell];
    y = x0[2 * cell + 1];
    return;
  }
  const double a = cov[0], b = cov[rows_src], d = cov[rows_src + 1];
  double z0, z1;
  normal_pair(0u, 0u, rng, STREAM_IDEAL_X0, seed, z0, z1);
  if (!(a > 0.0) || !(d - (b / sqrt(a)) * (b / sqrt(a)) > 0.0)) {
    status = CCMPC_REC_NOT_PD;
    x = y = NAN;
    return;
  }
  const double l00 = sqrt(a), l10 = b / l00, l11 = sqrt(d - l10 * l10);
  x = mean[0] + l00 * z0;
  y = mean[1] + (l10 * z0 + l11 * z1);
}

__device__ __forceinline__ void advance(const StepPlan &sp, double z0, double z1, double &x,
                                        double &y) {
  const double d0 = x - sp.mu0, d1 = y - sp.mu1;
  const double c0 = sp.nu0 + (d0 * sp.a00 + d1 * sp.a01);
  const double c1 = sp.nu1 + (d0 * sp.a10 + d1 * sp.a11);
  x = c0 + (z0 * sp.l00);
  y = c1 + (z0 * sp.l10 + z1 * sp.l11);
}

}  // namespace ccmpc
