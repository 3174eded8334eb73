// Box-face chance constraints ("TCST" family): the moments of the per-particle face coefficient
// vectors and the second-order-cone row data built from them (ccmpc_face_constraints).
//
// Replaces, for every (cell, t), v8ideal/__init__.py:1051-1075 (nominal), :1183-1208 (robust)
// and :1317-1352 (approx): four 3 x N coefficient arrays stacked from the particles, np.mean and
// np.cov of each, sqrtm or sqrt(|C|_F) of the covariance, and the approx variant's choice of the
// face with the smallest left-hand side at the reference point.
//
// Two launches, no atomics, no arrival counters, nothing to initialise:
//  * face_moments_kernel: a (chunk, t) grid.  Work item = one workgroup of 4 waves over one step
//    of 256 W G = 2048 consecutive particles of one cell, W = 2 (f64) or 4 (f32) per 16-byte load,
//    G = 4 or 2 loads per lane and plane (4 loads of f32 took every register: 256 VGPRs, one wave
//    per SIMD, and ran 1.5 times slower than the f64 store with half the bytes), located on the device from cell_off / cell_cnt (locate_item; blockIdx.y is the step);
//    every lane's load is 16 bytes of one plane, addresses past the cell clamped and their lanes
//    masked (the audit's idioms).  A lane reads its particles at step t and at step t - 1 (the
//    step delta), all 4 G loads requested before any arithmetic, so every plane but the last
//    pair is read twice: (2 T - 1) / T times the bytes ccmpc_moments reads, the second read out
//    of the cache the first one filled.  (One pass over all T steps per chunk, the previous
//    step in registers, reads each plane once but reduces 18 sums across the wave at every step
//    for W particles per lane and has T times fewer workgroups: measured 1.5 to 2 times slower
//    on the C2 and C4 stores)  The lane's 18 sums (two coefficient families x
//    (3 + 6)) are reduced in the wave by DPP row sums and the four rows in order, then the four
//    waves in wave order through LDS: one partial per (cell, t, chunk) in the workspace.
//  * face_finalize_kernel: one wave per (cell, t).  Lanes 0..17 add the chunk partials in chunk
//    order; lanes 0 and 1 each finish one family (faces 0 / 2 and 1 / 3): mean and ddof = 1
//    covariance of the shifted coefficients, the shift undone by the congruence L C L^T, the
//    principal root by a cyclic Jacobi eigen-decomposition of 8 sweeps, the four left-hand
//    sides at the reference point exchanged through LDS for the approx choice.
// The sums run over v - K with v = (-c, s, c x' - s y') and (-s, -c, s x' + c y'), (x', y') the
// position minus the cell's first particle's position at that step and K the first particle's
// own coefficient vector (the project's shift idiom: positions sit near 200 m, spreads are
// centimetres to metres).
#include "faces.hpp"

#include <type_traits>

#include "audit.hpp"

namespace ccmpc {

constexpr int kFaceThreads = 256;
constexpr int kFaceWaves = kFaceThreads / 64;
constexpr int kFaceSweeps = 8;
constexpr int kFaceLanePart = 8;  // particles per lane: 4 (f64) or 2 (f32) 16-byte loads per plane

template <typename P>
__global__ __launch_bounds__(kFaceThreads) void face_moments_kernel(FaceArgs a) {
  using V = AuditVec<P>;
  constexpr int W = V::W;
  constexpr int LG = W == 2 ? kFaceLgChunk64 : kFaceLgChunk32;
  constexpr int G = kFaceLanePart / W;
  static_assert((1 << LG) == kFaceThreads * W * G, "chunk = threads x lane width x groups");
  __shared__ double red[kFaceWaves][kFaceAcc];

  ItemLoc loc;
  if (!locate_item(blockIdx.x, a.cnt, a.off, a.n_cells, LG, loc)) return;  // uniform
  const int64_t cnt = loc.cnt;
  if (cnt <= 0) return;  // the finaliser reports the cell without reading the workspace
  const int T = a.T, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t cell = loc.cell, ld = a.ld;
  const P *cellp = static_cast<const P *>(a.pos) + loc.off;
  // this step's planes and the previous step's (step 0: its own, unused -- past_last instead)
  const P *pl_x = cellp + static_cast<int64_t>(2 * t) * ld, *pl_y = pl_x + ld;
  const P *pv_x = t == 0 ? pl_x : pl_x - 2 * ld, *pv_y = pv_x + ld;

  double o0 = 0.0, o1 = 0.0;
  if (std::is_same_v<P, float> && a.origin) {
    o0 = a.origin[2 * cell];
    o1 = a.origin[2 * cell + 1];
  }
  const double past_x = a.past_last[2 * cell], past_y = a.past_last[2 * cell + 1];

  // ---- the lane's particles: G groups of W, every load requested before any arithmetic --------
  const int64_t idx0 = (static_cast<int64_t>(loc.chunk_idx) << LG) + static_cast<int64_t>(W) * tid;
  const int64_t qlast = (cnt - 1) & ~static_cast<int64_t>(W - 1);
  V cx[G], cy[G], qx[G], qy[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t idx = idx0 + static_cast<int64_t>(g) * (kFaceThreads * W);
    const int64_t at = idx < qlast ? idx : qlast;  // clamped: stays inside the cell's last run
    cx[g].load(pl_x + at);
    cy[g].load(pl_y + at);
    qx[g].load(pv_x + at);
    qy[g].load(pv_y + at);
  }

  // ---- the shift: the cell's first particle at this step and its coefficient vector (the same
  // address in every lane: one broadcast load each) ----------------------------------------------
  const double hx = face_world(pl_x[0], o0), hy = face_world(pl_y[0], o1);
  const double hpx = t == 0 ? past_x : face_world(pv_x[0], o0);
  const double hpy = t == 0 ? past_y : face_world(pv_y[0], o1);
  double hs, hc;
  face_heading(hx - hpx, hy - hpy, hs, hc);
  if (loc.chunk_idx == 0 && tid == 0) {
    *reinterpret_cast<double4 *>(a.head + (cell * T + t) * 4) = double4{hx, hy, hc, hs};
    if (t == 0) a.first[cell] = loc.first;
  }

  double acc[kFaceAcc];
#pragma unroll
  for (int k = 0; k < kFaceAcc; ++k) acc[k] = 0.0;
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int64_t idx = idx0 + static_cast<int64_t>(g) * (kFaceThreads * W);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const bool valid = idx + j < cnt;
      const double x = face_world(cx[g][j], o0), y = face_world(cy[g][j], o1);
      const double xp = t == 0 ? past_x : face_world(qx[g][j], o0);
      const double yp = t == 0 ? past_y : face_world(qy[g][j], o1);
      double S, C;
      face_heading(x - xp, y - yp, S, C);
      const double xr = x - hx, yr = y - hy;
      // v - K: family 0 (-c, s, c x' - s y') - (-c0, s0, 0), family 1 (-s, -c, s x' + c y') -
      // (-s0, -c0, 0); a masked lane adds zeros
      const double dc = valid ? hc - C : 0.0, ds = valid ? S - hs : 0.0;
      const double w0 = valid ? C * xr - S * yr : 0.0;
      const double w1 = valid ? S * xr + C * yr : 0.0;
      const double u[2][3] = {{dc, ds, w0}, {-ds, dc, w1}};
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        double *q = acc + 9 * f;
        q[0] += u[f][0];
        q[1] += u[f][1];
        q[2] += u[f][2];
        q[3] += u[f][0] * u[f][0];
        q[4] += u[f][0] * u[f][1];
        q[5] += u[f][0] * u[f][2];
        q[6] += u[f][1] * u[f][1];
        q[7] += u[f][1] * u[f][2];
        q[8] += u[f][2] * u[f][2];
      }
    }
  }
  // in the wave: DPP row sums, then the four rows in order (register moves, no LDS round trips;
  // every lane of the wave is active here); then the four waves in wave order
#pragma unroll
  for (int k = 0; k < kFaceAcc; ++k) {
    const double sum = wave_sum_dpp_f64(acc[k]);
    if (lane == 0) red[wave][k] = sum;
  }
  __syncthreads();
  if (tid < kFaceAcc) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kFaceWaves; ++w) s += red[w][tid];
    // item blockIdx.x < max_items by the grid
    a.part[(static_cast<int64_t>(blockIdx.x) * T + t) * kFaceAcc + tid] = s;
  }
}

// One Jacobi rotation of the symmetric 3 x 3 in the (p, q) plane, r the third index: zeroes apq;
// the eigenvector columns p and q of V turn with it.  A huge |theta| (apq tiny beside the
// diagonal gap) gives t = 0 through 1 / inf: the rotation is the identity and apq is dropped.
__device__ __forceinline__ void face_jrot(double &app, double &aqq, double &apq, double &arp,
                                          double &arq, double &v0p, double &v0q, double &v1p,
                                          double &v1q, double &v2p, double &v2q) {
  if (apq == 0.0) return;
  const double th = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  double u = arp;
  arp = c * u - s * arq;
  arq = s * u + c * arq;
  u = v0p;
  v0p = c * u - s * v0q;
  v0q = s * u + c * v0q;
  u = v1p;
  v1p = c * u - s * v1q;
  v1q = s * u + c * v1q;
  u = v2p;
  v2p = c * u - s * v2q;
  v2q = s * u + c * v2q;
}

// Principal square root of the symmetric c = {c00 c01 c02 c11 c12 c22}: V diag(sqrt(lambda)) V^T.
// Eigenvalues in [-64 eps lambda_max, 0) count as 0; anything lower: false (sqrtm is complex).
__device__ __forceinline__ bool face_root(const double (&c)[6], double (&r)[6]) {
  double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0,
         v22 = 1.0;
  for (int sweep = 0; sweep < kFaceSweeps; ++sweep) {
    face_jrot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
    face_jrot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
    face_jrot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
  }
  const double lmax = fmax(a00, fmax(a11, a22));
  const double floor_ = -64.0 * 0x1p-52 * lmax;
  if (a00 < floor_ || a11 < floor_ || a22 < floor_) return false;
  const double s0 = sqrt(fmax(a00, 0.0)), s1 = sqrt(fmax(a11, 0.0)), s2 = sqrt(fmax(a22, 0.0));
  r[0] = s0 * v00 * v00 + s1 * v01 * v01 + s2 * v02 * v02;
  r[1] = s0 * v00 * v10 + s1 * v01 * v11 + s2 * v02 * v12;
  r[2] = s0 * v00 * v20 + s1 * v01 * v21 + s2 * v02 * v22;
  r[3] = s0 * v10 * v10 + s1 * v11 * v11 + s2 * v12 * v12;
  r[4] = s0 * v10 * v20 + s1 * v11 * v21 + s2 * v12 * v22;
  r[5] = s0 * v20 * v20 + s1 * v21 * v21 + s2 * v22 * v22;
  return true;
}

// mean . xi + Gamma |root xi|_2 + 0.5 car_r at xi = (rx, ry, 1)
__device__ __forceinline__ double face_value(const double (&m)[3], const double (&r)[6],
                                             double gamma, double half_r, double rx, double ry) {
  const double y0 = r[0] * rx + r[1] * ry + r[2];
  const double y1 = r[1] * rx + r[3] * ry + r[4];
  const double y2 = r[2] * rx + r[4] * ry + r[5];
  const double nrm = sqrt(y0 * y0 + y1 * y1 + y2 * y2);
  return m[0] * rx + m[1] * ry + m[2] + gamma * nrm + half_r;
}

__device__ __forceinline__ bool face_finite3(double a, double b, double c) {
  return isfinite(a) && isfinite(b) && isfinite(c);
}

__global__ __launch_bounds__(64) void face_finalize_kernel(FaceArgs a) {
  __shared__ double sums[kFaceAcc];
  __shared__ double vals[4];
  __shared__ int stat[2];
  const int T = a.T, lane = threadIdx.x;
  const int ct = blockIdx.x, cell = ct / T, t = ct - cell * T;
  const int64_t cnt = a.cnt[cell];
  const int lg = a.dtype == CCMPC_F64 ? kFaceLgChunk64 : kFaceLgChunk32;
  const int64_t nch = cnt > 0 ? ((cnt + (int64_t(1) << lg) - 1) >> lg) : 0;
  // counts beyond the caller's bound have no partials: the cell fails instead of reading past
  // the workspace
  int64_t first = 0;
  bool have = false;
  if (cnt >= 2) {
    first = a.first[cell];
    have = first >= 0 && first + nch <= a.max_items;
  }
  if (lane < kFaceAcc) {
    double s = 0.0;
    if (have) {
      const double *p = a.part + (first * T + t) * kFaceAcc + lane;
      for (int64_t k = 0; k < nch; ++k) s += p[k * T * kFaceAcc];  // chunk order
    }
    sums[lane] = s;
  }
  __syncthreads();

  const double qnan = __builtin_nan("");
  double mean[2][3], C[6], R[6];
  int status = CCMPC_REC_NONFINITE;
  double val[2] = {qnan, qnan};
  const bool with_ref = a.ref != nullptr;
  if (lane < 2) {
    const int g = lane;
    if (have) {
      const double4 h = *reinterpret_cast<const double4 *>(a.head + (static_cast<int64_t>(cell) * T + t) * 4);
      const double x0 = h.x, y0 = h.y, c0 = h.z, s0 = h.w;
      const double n = static_cast<double>(cnt);
      const double *q = sums + 9 * g;
      const double S0 = q[0], S1 = q[1], S2 = q[2];
      const double d = n - 1.0;
      const double u00 = (q[3] - S0 * S0 / n) / d, u01 = (q[4] - S0 * S1 / n) / d,
                   u02 = (q[5] - S0 * S2 / n) / d, u11 = (q[6] - S1 * S1 / n) / d,
                   u12 = (q[7] - S1 * S2 / n) / d, u22 = (q[8] - S2 * S2 / n) / d;
      // the shifted mean back to v: K = (-c0, s0, 0) or (-s0, -c0, 0)
      const double m0 = (g == 0 ? -c0 : -s0) + S0 / n;
      const double m1 = (g == 0 ? s0 : -c0) + S1 / n;
      const double m2 = S2 / n;
      // the position shift undone: a = L v + (0, 0, half), L = [[1,0,0],[0,1,0],[-x0,-y0,1]]
      const double half = 0.5 * (g == 0 ? a.extent[1] : a.extent[0]);
      const double lm2 = m2 - x0 * m0 - y0 * m1;
      mean[0][0] = m0;
      mean[0][1] = m1;
      mean[0][2] = lm2 + half;
      mean[1][0] = -m0;  // the mirror face: a_{f+2} = -L v + (0, 0, half)
      mean[1][1] = -m1;
      mean[1][2] = half - lm2;
      const double e02 = u02 - x0 * u00 - y0 * u01;  // (L C)_20 = (L C L^T)_02
      const double e12 = u12 - x0 * u01 - y0 * u11;
      const double e22 = (u22 - x0 * u02 - y0 * u12) - x0 * e02 - y0 * e12;
      C[0] = u00;
      C[1] = u01;
      C[2] = e02;
      C[3] = u11;
      C[4] = e12;
      C[5] = e22;
      const bool fin = face_finite3(mean[0][0], mean[0][1], mean[0][2]) &&
                       face_finite3(C[0], C[1], C[2]) && face_finite3(C[3], C[4], C[5]);
      if (fin) {
        status = 0;
        if (a.kind == CCMPC_FACE_ROBUST) {
          const double f2 = C[0] * C[0] + C[3] * C[3] + C[5] * C[5] +
                            2.0 * (C[1] * C[1] + C[2] * C[2] + C[4] * C[4]);
          const double s = sqrt(sqrt(f2));
          R[0] = s;
          R[1] = 0.0;
          R[2] = 0.0;
          R[3] = s;
          R[4] = 0.0;
          R[5] = s;
          if (!isfinite(s)) status = CCMPC_REC_NONFINITE;
        } else if (!face_root(C, R)) {
          status = CCMPC_REC_NOT_PSD;
        }
      }
      if (status == 0 && with_ref) {
        const int64_t r = a.cell_ref ? a.cell_ref[cell] : 0;
        const double rx = a.ref[(r * T + t) * 2], ry = a.ref[(r * T + t) * 2 + 1];
        const double gm = a.gamma[cell], hr = 0.5 * a.car_r;
        val[0] = face_value(mean[0], R, gm, hr, rx, ry);
        val[1] = face_value(mean[1], R, gm, hr, rx, ry);
      }
    }
    vals[g] = val[0];      // faces g and g + 2
    vals[g + 2] = val[1];
    stat[g] = status;
  }
  __syncthreads();
  if (lane < 2) {
    const int g = lane;
    int best = -1;
    if (with_ref && stat[0] == 0 && stat[1] == 0) {
      best = 0;
      for (int f = 1; f < 4; ++f)
        if (vals[f] < vals[best]) best = f;  // first index on equality
    }
    for (int m = 0; m < 2; ++m) {
      const int face = g + 2 * m;
      ccmpc_face_rec out;
      for (int i = 0; i < 3; ++i) out.mean[i] = status == 0 ? mean[m][i] : qnan;
      for (int i = 0; i < 6; ++i) {
        out.root[i] = status == 0 ? R[i] : qnan;
        out.C[i] = status == 0 ? C[i] : qnan;
      }
      out.status = status;
      const unsigned chosen = best < 0 ? CCMPC_FACE_NO_CHOICE : (best == face ? 1u : 0u);
      out.t_face_chosen = (static_cast<unsigned>(t) << 16) | (static_cast<unsigned>(face) << 8) |
                          chosen;
      a.rec[(static_cast<int64_t>(cell) * T + t) * 4 + face] = out;
    }
  }
}

int launch_face_constraints(FaceArgs a, int64_t n_bound, void *workspace, hipStream_t s) {
  const int lg = a.dtype == CCMPC_F64 ? kFaceLgChunk64 : kFaceLgChunk32;
  const int64_t items = max_items(a.n_cells, n_bound, int64_t(1) << lg);
  const int64_t nct = static_cast<int64_t>(a.n_cells) * a.T;
  if (items >= (int64_t(1) << 31) || nct >= (int64_t(1) << 31)) return CCMPC_ERR_ARG;
  size_t o_head, o_part;
  face_layout(a.T, a.n_cells, items, &o_head, &o_part);
  char *w = static_cast<char *>(workspace);
  a.max_items = items;
  a.first = reinterpret_cast<int32_t *>(w);
  a.head = reinterpret_cast<double *>(w + o_head);
  a.part = reinterpret_cast<double *>(w + o_part);
  const dim3 g(static_cast<unsigned>(items), static_cast<unsigned>(a.T)), b(kFaceThreads);
  if (a.dtype == CCMPC_F64)
    hipLaunchKernelGGL((face_moments_kernel<double>), g, b, 0, s, a);
  else
    hipLaunchKernelGGL((face_moments_kernel<float>), g, b, 0, s, a);
  hipLaunchKernelGGL(face_finalize_kernel, dim3(static_cast<unsigned>(nct)), dim3(64), 0, s, a);
  return CCMPC_OK;
}

}  // namespace ccmpc
