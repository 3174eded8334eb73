// Lane, wave and workgroup primitives of the planning QP's kernels (qp.hip): DPP lane moves and
// the reductions built on them, the workgroup's barrier, and the dense Cholesky and triangular
// solves in their LDS (wave-level) and register-resident forms.
#pragma once
#include "ccmpc_common.hpp"

namespace ccmpc {

// Lane moves inside a row of 16 (DPP; f64 as two 32-bit halves).  `old` is what a lane keeps
// if its source is out of range -- never the case for the controls used here, with the whole
// wave active (every caller reduces in wave-uniform control flow).
template <int CTRL>
__device__ __forceinline__ double qp_dpp(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo =
      __builtin_amdgcn_update_dpp(0u, static_cast<uint32_t>(u), CTRL, 0xf, 0xf, false);
  const uint32_t hi =
      __builtin_amdgcn_update_dpp(0u, static_cast<uint32_t>(u >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, (static_cast<uint64_t>(hi) << 32) | lo);
}
constexpr int kDppQuad1 = 0xB1;        // quad_perm [1,0,3,2]
constexpr int kDppQuad2 = 0x4E;        // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // lane i of 8 <- lane 7-i: the other quad
constexpr int kDppMirror = 0x140;      // lane i of 16 <- lane 15-i: the other half-row

__device__ __forceinline__ double lane_bcast(double v, int src) {  // src wave-uniform
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(u), src);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(u >> 32), src);
  return __builtin_bit_cast(double, (static_cast<uint64_t>(hi) << 32) | lo);
}

// Sum over each group of 4 / 8 consecutive lanes (every lane of the group gets it)
__device__ __forceinline__ double sum4(double v) {
  v += qp_dpp<kDppQuad1>(v);
  return v + qp_dpp<kDppQuad2>(v);
}
__device__ __forceinline__ double sum8(double v) {
  v = sum4(v);
  return v + qp_dpp<kDppHalfMirror>(v);
}

// Whole-wave reductions: four DPP steps reduce each row of 16, then the four row results are
// combined in a fixed order from lanes 0, 16, 32, 48 (uniform result, no LDS round trips)
__device__ __forceinline__ double wave_sum(double v) {
  v = sum8(v);
  v += qp_dpp<kDppMirror>(v);
  return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, qp_dpp<kDppQuad1>(v));
  v = fmax(v, qp_dpp<kDppQuad2>(v));
  v = fmax(v, qp_dpp<kDppHalfMirror>(v));
  v = fmax(v, qp_dpp<kDppMirror>(v));
  return fmax(fmax(lane_bcast(v, 0), lane_bcast(v, 16)), fmax(lane_bcast(v, 32), lane_bcast(v, 48)));
}
__device__ __forceinline__ double wave_min(double v) {
  v = fmin(v, qp_dpp<kDppQuad1>(v));
  v = fmin(v, qp_dpp<kDppQuad2>(v));
  v = fmin(v, qp_dpp<kDppHalfMirror>(v));
  v = fmin(v, qp_dpp<kDppMirror>(v));
  return fmin(fmin(lane_bcast(v, 0), lane_bcast(v, 16)), fmin(lane_bcast(v, 32), lane_bcast(v, 48)));
}

// Block reductions of up to 2 values (every thread gets the result); two barriers.  NW = 1
// (one wave per scene): the wave reduction alone, no LDS and no barrier.
template <int NW>
__device__ __forceinline__ void block_max2(double &a, double &b, double *red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  a = wave_max(a);
  b = wave_max(b);
  if (NW == 1) return;
  if (lane == 0) {
    red[2 * w] = a;
    red[2 * w + 1] = b;
  }
  __syncthreads();
  a = red[0];
  b = red[1];
  for (int k = 1; k < NW; ++k) {
    a = fmax(a, red[2 * k]);
    b = fmax(b, red[2 * k + 1]);
  }
  __syncthreads();
}
template <int NW>
__device__ __forceinline__ double block_sum(double a, double *red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  a = wave_sum(a);
  if (NW == 1) return a;
  if (lane == 0) red[w] = a;
  __syncthreads();
  a = red[0];
  for (int k = 1; k < NW; ++k) a += red[k];
  __syncthreads();
  return a;
}
template <int NW>
__device__ __forceinline__ double block_min(double a, double *red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  a = wave_min(a);
  if (NW == 1) return a;
  if (lane == 0) red[w] = a;
  __syncthreads();
  a = red[0];
  for (int k = 1; k < NW; ++k) a = fmin(a, red[k]);
  __syncthreads();
  return a;
}

// Block argmax (largest value, smallest index on ties); every thread gets the result.
template <int NW>
__device__ __forceinline__ void block_argmax(double &v, double &idx, double *red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64), oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
  }
  if (NW == 1) return;
  if (lane == 0) {
    red[2 * w] = v;
    red[2 * w + 1] = idx;
  }
  __syncthreads();
  v = red[0];
  idx = red[1];
  for (int k = 1; k < NW; ++k) {
    if (red[2 * k] > v || (red[2 * k] == v && red[2 * k + 1] < idx)) {
      v = red[2 * k];
      idx = red[2 * k + 1];
    }
  }
  __syncthreads();
}

// wave-level ordering of LDS traffic between the lanes of wave 0 (one wave executes its LDS
// instructions in order; this keeps the compiler from moving them across the step)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The workgroup's barrier; with one wave per scene, the wave-level ordering above (a wave runs
// its LDS instructions in order, so every lane then sees every other lane's writes)
template <int NW>
__device__ __forceinline__ void qp_sync() {
  if (NW == 1)
    wave_sync();
  else
    __syncthreads();
}

// Wave-level dense Cholesky and triangular solves (called by one whole wave; lane = row, two
// rows per lane, so N <= 128).  A holds the lower triangle, row stride ld; it is overwritten by
// L, and dinv[j] = 1 / L[j][j].  With pivot_skip a pivot that cancellation drove to <= 0 is
// replaced by a huge one (see the IPM in qp.hip); otherwise it fails.  Returns true on failure.
__device__ inline bool wave_cholesky(double *A, int N, int ld, double *dinv, bool pivot_skip) {
  const int lane = threadIdx.x & 63;
  bool fail = false;
  for (int j = 0; j < N; ++j) {
    double sv[2];
    const double ajj = A[j * ld + j];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = j + lane + 64 * h;
      double v = 0.0;
      if (i < N) {
        v = A[i * ld + j];
        for (int k = 0; k < j; ++k) v -= A[i * ld + k] * A[j * ld + k];
      }
      sv[h] = v;
    }
    double dj = lane_bcast(sv[0], 0);
    fail = fail || !isfinite(dj) || !isfinite(ajj);
    if (!(dj > 1e-30 * ajj)) {
      fail = fail || !pivot_skip;
      dj = 1e128;
    }
    const double ljj = sqrt(dj), inv = 1.0 / ljj;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = j + lane + 64 * h;
      if (i < N) A[i * ld + j] = (i == j) ? ljj : sv[h] * inv;
    }
    if (lane == 0) dinv[j] = inv;
    wave_sync();
  }
  return fail;
}

// b <- L^{-1} b (b[h] is row lane + 64 h)
__device__ __forceinline__ void wave_forward(const double *L, int N, int ld, const double *dinv,
                                             double b[2]) {
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < N; ++j) {
    const double yj = lane_bcast((j >> 6) ? b[1] : b[0], j & 63) * dinv[j];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i == j) b[h] = yj;
      else if (i > j && i < N) b[h] -= L[i * ld + j] * yj;
    }
  }
}

// b <- L^{-T} b
__device__ __forceinline__ void wave_backward(const double *L, int N, int ld, const double *dinv,
                                              double b[2]) {
  const int lane = threadIdx.x & 63;
  for (int j = N - 1; j >= 0; --j) {
    const double xj = lane_bcast((j >> 6) ? b[1] : b[0], j & 63) * dinv[j];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i == j) b[h] = xj;
      else if (i < j) b[h] -= L[j * ld + i] * xj;
    }
  }
}

__device__ __forceinline__ void wave_load2(const double *x, int N, double b[2]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int h = 0; h < 2; ++h) b[h] = (lane + 64 * h < N) ? x[lane + 64 * h] : 0.0;
}
__device__ __forceinline__ void wave_store2(double *x, int N, const double b[2]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (lane + 64 * h < N) x[lane + 64 * h] = b[h];
}

// Register-resident variants for n <= NM (one row per lane of the calling wave): the
// IPM factors and solves twice per iteration, and with L in registers a column step is a
// readlane and an FMA instead of a dependent LDS round trip.  a[k] = L[lane][k] (row form),
// dl = 1 / L[lane][lane]; the L^T solve reads L's rows from LDS (independent of the chain, so
// the unrolled loads issue ahead of it).  The matrix is padded to NM x NM with the identity
// (rows and columns >= n; the right-hand side 0 there), so every step runs unconditionally:
// straight-line code, no per-column branch on a runtime n.
//
// a <- the lower triangle of the n x n matrix A in LDS (row stride ld), lane = row, padded with
// the identity; every lane loads an in-bounds entry, then selects
template <int NM>
__device__ __forceinline__ void reg_load_lower(const double *A, int ld, int n, double (&a)[NM]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NM; ++k) {
    const double v = A[(lane < n ? lane : 0) * ld + (k < n ? k : 0)];
    a[k] = (lane < n && k <= lane) ? v : (k == lane ? 1.0 : 0.0);
  }
}
// the n x n part of a back over A's lower triangle (the padding is never stored)
template <int NM>
__device__ __forceinline__ void reg_store_lower(double *A, int ld, int n, const double (&a)[NM]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NM; ++k)
    if (k < n && lane < n && k <= lane) A[lane * ld + k] = a[k];
}
template <int NM, bool SKIP = true>
__device__ __forceinline__ bool reg_cholesky(double (&a)[NM], double &dl) {
  const int lane = threadIdx.x & 63;
  bool fail = false;
  double diag0 = 0.0;  // the lane's original diagonal (for the pivot-skip threshold)
#pragma unroll
  for (int k = 0; k < NM; ++k)
    if (k == lane) diag0 = a[k];
  fail = __ballot(lane < NM && !isfinite(diag0)) != 0;
#pragma unroll
  for (int j = 0; j < NM; ++j) {
    {
      double d = lane_bcast(a[j], j);
      // lane j's pivot against its own original diagonal, as a ballot bit (no broadcast)
      const bool tiny = (__ballot(!(a[j] > 1e-30 * diag0)) >> j) & 1;
      fail = fail || !isfinite(d);
      if (tiny) {  // pivot skip (the IPM), or a failure (SKIP = false)
        fail = fail || !SKIP;
        d = 1e128;
      }
      // sqrt and 1/sqrt from the hardware rsqrt + one Goldschmidt step (~1 ulp; the IPM's
      // factor needs no IEEE rounding, the polish recomputes the answer from H exactly)
      const double y = __builtin_amdgcn_rsq(d);
      double g = d * y, h = 0.5 * y;
      const double rr = fma(-g, h, 0.5);
      g = fma(g, rr, g);
      h = fma(h, rr, h);
      const double ljj = g, inv = 2.0 * h;
      const double lij = lane > j ? a[j] * inv : (lane == j ? ljj : 0.0);
      a[j] = lij;
      if (lane == j) dl = inv;
      // trailing update without an exec-mask branch: rows above k pick up values in their
      // (never read) upper triangle; lij = 0 for rows < j keeps their finished rows intact
#pragma unroll
      for (int k = j + 1; k < NM; ++k) a[k] = fma(-lij, lane_bcast(lij, k), a[k]);
    }
  }
  return fail;
}

// lt[j] = L[j][lane], the L^T solve's column (from L's lower triangle in LDS, row stride ld)
template <int NM>
__device__ __forceinline__ void reg_load_lt(const double *L, int ld, int n, double (&lt)[NM]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NM; ++j) {  // every lane loads (in-bounds index), then selects
    const double v = L[(j < n ? j : 0) * ld + (lane < j ? lane : 0)];
    lt[j] = (lane < j && j < n) ? v : 0.0;
  }
}
template <int NM>  // b <- L^{-1} b (b on lane = row)
__device__ __forceinline__ double reg_forward(const double (&a)[NM], double dl, double b) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NM; ++j) {
    const double yj = lane_bcast(b * dl, j);  // lane j's b is final: one broadcast
    const double upd = fma(-a[j], yj, b);
    b = lane == j ? yj : (lane > j ? upd : b);
  }
  return b;
}
template <int NM>  // b <- L^{-T} b
__device__ __forceinline__ double reg_backward(const double (&lt)[NM], double dl, double b) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = NM - 1; j >= 0; --j) {
    const double xj = lane_bcast(b * dl, j);
    const double upd = fma(-lt[j], xj, b);
    b = lane == j ? xj : (lane < j ? upd : b);
  }
  return b;
}
template <int NM>
__device__ __forceinline__ double reg_solve(const double (&a)[NM], const double *L, int ld,
                                            double dl, int n, double b) {
  double lt[NM];  // read ahead of the chain
  reg_load_lt(L, ld, n, lt);
  return reg_backward(lt, dl, reg_forward(a, dl, b));
}

}  // namespace ccmpc
