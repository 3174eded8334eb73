// Kelley cuts of the box-face second-order-cone rows (ccmpc_face_cuts).
//
// The approx generator's rows, or any fixed choice of one face per (cell, t), are convex in the
// ego position of step t:  g(x) = mean . xi + Gamma |root xi|_2 + 0.5 car_r <= 0, xi = (x, y, 1).
// The reference hands them to cvxpy / CPLEX as cone rows (v8ideal/__init__.py:1353-1363); here
// every row is linearised at the current plan, a . x_t <= b with a a subgradient of g there, and
// the planning QP (qp.hip, unchanged) solves over all cuts so far: outer approximation, one
// launch of this kernel per round.
//
// One wave per scene, no atomics, no workspace, nothing to initialise:
//  pass 1  lanes stride over the scene's (cell, t) rows: pick the face, evaluate g at the plan,
//          write out_g, keep the largest g (and whether a row was bad or NaN);
//  reduce  a butterfly over the 64 lanes (max is exact, so its order cannot change a bit);
//  decide  the scene's sticky state from the previous call's (round > 0) and this maximum;
//  pass 2  the same rows again (the same arithmetic, the same bits): a cut or an empty record
//          into region `round` of the scene's pool; round 0 also empties every later region.
#include "socp.hpp"

namespace ccmpc {

struct CutRow {
  double g, a0, a1, b;
  int kind;  // 0: a row, 1: no row selected, 2: a bad row
};

// Row r = ci * T + t of the scene whose first cell is c0, at the plan point of step t.  All
// float64, in this order (the header documents it):
//   w = root xi;  nw = sqrt((w0 w0 + w1 w1) + w2 w2);  g = (((m0 x + m1 y) + m2) + Gamma nw) + half_r
//   v = (root w)[0:2];  a = m[0:2] + (Gamma v) / nw  (a = m[0:2] where nw == 0);  b = (a0 x + a1 y) - g
__device__ __forceinline__ CutRow cut_row(const FaceCutArgs &a, int64_t c0, const double *plan,
                                          int64_t r) {
  const double qnan = __builtin_nan("");
  const int T = a.T;
  const int64_t ci = r / T;
  const int t = static_cast<int>(r - ci * T);
  const int64_t cell = c0 + ci;
  const ccmpc_face_rec *q = a.rec + (cell * T + t) * 4;
  int f = -1;
  if (a.face_sel) {
    f = a.face_sel[cell * T + t];
    if (f == -1) return {-INFINITY, 0.0, 0.0, 0.0, 1};
    if (f < 0 || f > 3) return {qnan, qnan, qnan, qnan, 2};
  } else {
    bool none = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned ch = q[k].t_face_chosen & 0xffu;
      none = none || ch == CCMPC_FACE_NO_CHOICE;
      if (ch == 1u && f < 0) f = k;
    }
    if (none || f < 0) return {qnan, qnan, qnan, qnan, 2};
  }
  const ccmpc_face_rec *p = q + f;
  if (p->status != 0) return {qnan, qnan, qnan, qnan, 2};
  const double m0 = p->mean[0], m1 = p->mean[1], m2 = p->mean[2];
  const double r00 = p->root[0], r01 = p->root[1], r02 = p->root[2], r11 = p->root[3],
               r12 = p->root[4], r22 = p->root[5];
  const double gm = a.gamma[cell], half_r = 0.5 * a.car_r;
  const double x = plan[static_cast<int64_t>(t) * a.ld_plan],
               y = plan[static_cast<int64_t>(t) * a.ld_plan + 1];
  const double w0 = r00 * x + r01 * y + r02;
  const double w1 = r01 * x + r11 * y + r12;
  const double w2 = r02 * x + r12 * y + r22;
  const double nw = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  CutRow o;
  o.kind = 0;
  o.g = m0 * x + m1 * y + m2 + gm * nw + half_r;
  o.a0 = m0;
  o.a1 = m1;
  if (nw != 0.0) {
    const double v0 = r00 * w0 + r01 * w1 + r02 * w2;
    const double v1 = r01 * w0 + r11 * w1 + r12 * w2;
    o.a0 = m0 + gm * v0 / nw;
    o.a1 = m1 + gm * v1 / nw;
  }
  o.b = o.a0 * x + o.a1 * y - o.g;
  return o;
}

// ccmpc_gather_rec as one 32-byte value: n0, n1, rhs, then side (int16) | status (int16) << 16 |
// t_tau << 32 (compact_records_kernel's packing)
__device__ __forceinline__ double4 cut_pack(double n0, double n1, double rhs, int status, int t) {
  const uint64_t tail = (static_cast<uint64_t>(static_cast<uint32_t>(t)) << 32) |
                        (static_cast<uint32_t>(static_cast<uint16_t>(status)) << 16) | 0xFFFFu;
  return double4{n0, n1, rhs, __builtin_bit_cast(double, tail)};
}

__global__ __launch_bounds__(64) void face_cuts_kernel(FaceCutArgs a) {
  const int lane = threadIdx.x, T = a.T;
  const int64_t s = blockIdx.x;
  const int prev = a.round > 0 ? a.out_state[s] : CCMPC_SOCP_CUT;
  const int64_t c0 = a.scene_cell[s], nc = a.scene_cell[s + 1] - c0;
  const int64_t p0 = a.pool_cell[s], np = a.pool_cell[s + 1] - p0;
  const int64_t regions = static_cast<int64_t>(a.max_rounds) + 1;
  // a pool that is not (max_rounds + 1) x the scene's cells is never written
  const bool layout_ok = nc >= 0 && np == regions * nc;
  const int64_t rows = nc > 0 ? nc * T : 0;
  const double *plan = a.plan + s * T * a.ld_plan;

  double m = -INFINITY;
  int bad = 0, isnan_ = 0;
  for (int64_t r = lane; r < rows; r += 64) {
    const CutRow row = cut_row(a, c0, plan, r);
    a.out_g[c0 * T + r] = row.g;
    if (row.kind == 2) {
      bad = 1;
    } else if (row.kind == 0) {
      if (row.g != row.g) isnan_ = 1;
      else if (row.g > m) m = row.g;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  bad = __any(bad);
  isnan_ = __any(isnan_);
  const double viol = (bad || isnan_) ? __builtin_nan("") : m;

  int state;
  if (!layout_ok) state = CCMPC_SOCP_BAD_LAYOUT;
  else if (bad || prev == CCMPC_SOCP_BAD_ROW) state = CCMPC_SOCP_BAD_ROW;
  else if (prev == CCMPC_SOCP_OK) state = CCMPC_SOCP_OK;
  // round 0 judges the linearisation point, not a plan of the programme: it never ends a scene
  else if (a.round > 0 && viol <= a.tol_g) state = CCMPC_SOCP_OK;
  else state = CCMPC_SOCP_CUT;
  if (lane == 0) {
    a.out_viol[s] = viol;
    a.out_state[s] = state;
  }
  if (!layout_ok) return;

  const bool cut = state == CCMPC_SOCP_CUT;
  const bool all = a.round == 0 || a.only_violated == 0;
  double4 *reg = a.pool + (p0 + a.round * nc) * T;
  for (int64_t r = lane; r < rows; r += 64) {
    const int t = static_cast<int>(r % T);
    double4 v = cut_pack(0.0, 0.0, 0.0, CCMPC_CUT_EMPTY, t);
    if (cut) {
      const CutRow row = cut_row(a, c0, plan, r);
      if (row.kind == 0 && (all || row.g > 0.0)) v = cut_pack(row.a0, row.a1, row.b, 0, t);
    }
    reg[r] = v;
  }
  if (a.round == 0) {
    double4 *later = a.pool + (p0 + nc) * T;
    const int64_t n = static_cast<int64_t>(a.max_rounds) * rows;
    for (int64_t i = lane; i < n; i += 64)
      later[i] = cut_pack(0.0, 0.0, 0.0, CCMPC_CUT_EMPTY, static_cast<int>(i % T));
  }
}

void launch_face_cuts(const FaceCutArgs &a, int64_t n_scenes, hipStream_t s) {
  hipLaunchKernelGGL(face_cuts_kernel, dim3(static_cast<unsigned>(n_scenes)), dim3(64), 0, s, a);
}

}  // namespace ccmpc
