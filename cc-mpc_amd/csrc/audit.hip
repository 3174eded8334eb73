// Monte-Carlo risk audit: count, on the particles the constraints were built from, how many a
// plan hits and how many each half-space record leaves unprotected (ccmpc_risk_audit; no
// reference counterpart -- the reference never counts particles against its risk budget).
//
// One streaming pass over planes 0 .. 2T-1 of the store, the bytes ccmpc_moments reads:
//  * Work item = one workgroup of 4 waves over 256 W consecutive particles of one cell, W = 2
//    (f64) or 4 (f32): every lane's load is 16 bytes of one plane, a wave's 1 KiB contiguous.
//    Items are found on the device from cell_off / cell_cnt (locate_item, as the moments
//    kernel), the grid is sized by n_particles_bound.
//  * A lane owns its W particles for all T steps: the "hit at any step" bit and the step's
//    "protected by some record" bit stay in registers.  Steps are loaded four at a time, the
//    next four in flight while these are evaluated; the first four are requested before the
//    workgroup stages its records, right behind the staging's own small loads.
//  * The cell's status-0 records are staged once per workgroup in LDS, bucketed by their step
//    (counting sort over t): side*n0, side*n1, side*rhs and R^2 |n|^2, 32 bytes each, with the
//    record's row for the flush.  v = side (rhs - n.p) is formed as side*rhs - (side*n).p: the
//    same bits, because rounding is symmetric in sign.
//  * Counts are wave ballots + population counts added to LDS integers (one LDS atomic per
//    wave per record / step); the workgroup flushes every non-zero count with one 64-bit
//    integer atomic add, min_d2 with an unsigned 64-bit atomic min on the bit pattern of the
//    non-negative double (bit order = value order).  No float atomics: the results do not
//    depend on arrival order.
//  * Lanes past cell_cnt load a clamped address (the cell's last aligned run) and are masked
//    out of every ballot, so the padding between cells is never counted.
// A first small launch of the same call writes the initial values (0, +inf, and -1 for records
// that are not audited), so the caller prepares nothing.
#include "audit.hpp"

#include <type_traits>

namespace ccmpc {

constexpr int kAuditThreads = 256;
constexpr int kAuditU = 4;  // steps per load group

__device__ __forceinline__ void add_i64(int64_t *p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

// Initial values of every enabled output.
__global__ __launch_bounds__(kAuditThreads) void audit_init_kernel(AuditArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t C = a.n_cells, CT = C * a.T;
  if (a.plan) {
    if (i < CT) {
      a.hit[i] = 0;
      a.min_d2[i] = __builtin_huge_val();
    }
    if (i < C) a.hit_any[i] = 0;
  }
  if (a.rec) {
    if (i < CT) a.open[i] = 0;
    if (i < C * a.P)
      a.rec_open[i] = audit_rec_valid(audit_read_rec(a.rec, a.kind, i), a.T) ? 0 : -1;
  }
}

template <typename P, bool PLAN, bool REC>
__global__ __launch_bounds__(kAuditThreads) void audit_kernel(AuditArgs a) {
  using V = AuditVec<P>;
  constexpr int W = V::W;
  constexpr int LG = W == 2 ? 8 + 1 : 8 + 2;  // log2 particles per item (kAuditThreads * W)
  constexpr int U = kAuditU;
  __shared__ double4 stg[REC ? kAuditMaxRec : 1];  // side*n0, side*n1, side*rhs, R^2 |n|^2
  __shared__ int ridx[REC ? kAuditMaxRec : 1];     // the staged record's row in the cell
  __shared__ int rcount[REC ? kAuditMaxRec : 1];   // particles it leaves open
  // staged records of step t: [tstart[t], tstart[t + 1])
  __shared__ int tstart[REC ? kAuditMaxT + 1 : 1];
  __shared__ int tfill[REC ? kAuditMaxT : 1];
  __shared__ int open_s[REC ? kAuditMaxT : 1];
  __shared__ double plan_s[PLAN ? 2 * kAuditMaxT : 1];
  __shared__ int hit_s[PLAN ? kAuditMaxT : 1];
  __shared__ unsigned long long min_s[PLAN ? kAuditMaxT : 1];
  __shared__ int any_s;

  ItemLoc loc;
  if (!locate_item(blockIdx.x, a.cnt, a.off, a.n_cells, LG, loc, a.cell_plan)) return;  // uniform
  const int64_t cnt = loc.cnt;
  if (cnt <= 0) return;  // an empty cell keeps its initial values
  const int T = a.T, tid = threadIdx.x, lane = tid & 63;
  const int64_t cell = loc.cell;

  // ---- the lane's particles; their first load group is in flight while the workgroup stages --
  const int64_t idx = (static_cast<int64_t>(loc.chunk_idx) << LG) + static_cast<int64_t>(W) * tid;
  const int64_t qlast = (cnt - 1) & ~static_cast<int64_t>(W - 1);
  const P *base = static_cast<const P *>(a.pos) + loc.off + (idx < qlast ? idx : qlast);
  bool valid[W], any[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    valid[j] = idx + j < cnt;
    any[j] = false;
  }
  double o0 = 0.0, o1 = 0.0;
  if (std::is_same_v<P, float> && a.origin) {
    o0 = a.origin[2 * cell];
    o1 = a.origin[2 * cell + 1];
  }
  const double R2 = a.R2;
  const int64_t ld = a.ld;

  auto load_steps = [&](V (&b)[U][2], int t0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u < T ? t0 + u : T - 1;
      b[u][0].load(base + static_cast<int64_t>(2 * t) * ld);
      b[u][1].load(base + static_cast<int64_t>(2 * t + 1) * ld);
    }
  };

  // The workgroup's small inputs are requested first and the particles' first load group right
  // behind them (loads return in order): the stream is in flight while the workgroup stages.
  double plan_v = 0.0;
  if (PLAN && tid < 2 * T) plan_v = a.plan[static_cast<int64_t>(loc.ref_sel) * 2 * T + tid];
  const int64_t r0 = cell * a.P;
  AuditRec q0{};  // the thread's first record (all of them up to 256 rows per cell)
  q0.status = 1;
  if (REC && tid < a.P) q0 = audit_read_rec(a.rec, a.kind, r0 + tid);
  V cur[U][2], nxt[U][2];
  load_steps(cur, 0);

  // ---- stage the plan row and the cell's audited records ------------------------------------
  if (PLAN) {
    if (tid < 2 * T) plan_s[tid] = plan_v;
    if (tid < T) {
      hit_s[tid] = 0;
      min_s[tid] = __builtin_bit_cast(unsigned long long, __builtin_huge_val());
    }
    if (tid == 0) any_s = 0;
  }
  if (REC) {
    if (tid < T) {
      tfill[tid] = 0;
      open_s[tid] = 0;
    }
    __syncthreads();
    for (int r = tid; r < a.P; r += kAuditThreads) {
      const AuditRec q = r == tid ? q0 : audit_read_rec(a.rec, a.kind, r0 + r);
      if (audit_rec_valid(q, T)) atomicAdd(&tfill[q.t], 1);
      rcount[r] = 0;  // every slot the flush may visit holds a row of this cell
      ridx[r] = 0;
    }
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int t = 0; t < T; ++t) {
        tstart[t] = s;
        s += tfill[t];
        tfill[t] = 0;
      }
      tstart[T] = s;
    }
    __syncthreads();
    for (int r = tid; r < a.P; r += kAuditThreads) {
      const AuditRec q = r == tid ? q0 : audit_read_rec(a.rec, a.kind, r0 + r);
      if (!audit_rec_valid(q, T)) continue;
      const int k = tstart[q.t] + atomicAdd(&tfill[q.t], 1);
      if (k >= tstart[q.t + 1]) continue;  // records rewritten under the call: stay in bounds
      const double sd = static_cast<double>(q.side);
      stg[k] = double4{sd * q.n0, sd * q.n1, sd * q.rhs, a.R2 * (q.n0 * q.n0 + q.n1 * q.n1)};
      ridx[k] = r;
    }
  }
  __syncthreads();

  auto step = [&](int t, const V (&b)[2]) {
    double px[W], py[W];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      if constexpr (std::is_same_v<P, float>) {
        px[j] = b[0][j] + o0;
        py[j] = b[1][j] + o1;
      } else {
        px[j] = b[0][j];
        py[j] = b[1][j];
      }
    }
    if (PLAN) {
      const double ax = plan_s[2 * t], ay = plan_s[2 * t + 1];
      double m = __builtin_huge_val();
      int nh = 0;
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const double dx = px[j] - ax, dy = py[j] - ay;
        const double d2 = dx * dx + dy * dy;
        const bool h = valid[j] && d2 < R2;
        any[j] = any[j] || h;
        nh += __popcll(__ballot(h));
        m = (valid[j] && d2 < m) ? d2 : m;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double x = __shfl_xor(m, o, 64);
        m = x < m ? x : m;
      }
      if (lane == 0) {
        if (nh) atomicAdd(&hit_s[t], nh);
        atomicMin(&min_s[t], __builtin_bit_cast(unsigned long long, m));
      }
    }
    if (REC) {
      bool prot[W];
#pragma unroll
      for (int j = 0; j < W; ++j) prot[j] = false;
      const int k1 = tstart[t + 1];
      for (int k = tstart[t]; k < k1; ++k) {
        const double4 q = stg[k];
        int no = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          const double s = q.x * px[j] + q.y * py[j];
          const bool p = audit_protects(q.z - s, q.w);
          prot[j] = prot[j] || p;
          no += __popcll(__ballot(valid[j] && !p));
        }
        if (lane == 0 && no) atomicAdd(&rcount[k], no);
      }
      int no = 0;
#pragma unroll
      for (int j = 0; j < W; ++j) no += __popcll(__ballot(valid[j] && !prot[j]));
      if (lane == 0 && no) atomicAdd(&open_s[t], no);
    }
  };

  for (int t0 = 0; t0 < T; t0 += U) {
    if (t0 + U < T) load_steps(nxt, t0 + U);  // uniform
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (t0 + u < T) step(t0 + u, cur[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cur[u][0] = nxt[u][0];
      cur[u][1] = nxt[u][1];
    }
  }
  if (PLAN) {
    int na = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) na += __popcll(__ballot(any[j]));
    if (lane == 0 && na) atomicAdd(&any_s, na);
  }
  __syncthreads();

  // ---- one flush per output -----------------------------------------------------------------
  if (PLAN) {
    if (tid < T) {
      if (hit_s[tid]) add_i64(a.hit + cell * T + tid, hit_s[tid]);
      atomicMin(reinterpret_cast<unsigned long long *>(a.min_d2 + cell * T + tid), min_s[tid]);
    }
    if (tid == 0 && any_s) add_i64(a.hit_any + cell, any_s);
  }
  if (REC) {
    if (tid < T && open_s[tid]) add_i64(a.open + cell * T + tid, open_s[tid]);
    const int ns = tstart[T];
    for (int k = tid; k < ns; k += kAuditThreads)
      if (rcount[k]) add_i64(a.rec_open + cell * a.P + ridx[k], rcount[k]);
  }
}

template <typename P>
static void launch_typed(const AuditArgs &a, unsigned grid, hipStream_t s) {
  const dim3 g(grid), b(kAuditThreads);
  if (a.plan && a.rec)
    hipLaunchKernelGGL((audit_kernel<P, true, true>), g, b, 0, s, a);
  else if (a.plan)
    hipLaunchKernelGGL((audit_kernel<P, true, false>), g, b, 0, s, a);
  else
    hipLaunchKernelGGL((audit_kernel<P, false, true>), g, b, 0, s, a);
}

int launch_risk_audit(const AuditArgs &a, hipStream_t s) {
  const int64_t C = a.n_cells;
  int64_t n_init = C * a.T;
  if (a.rec && C * a.P > n_init) n_init = C * a.P;
  const int64_t init_blocks = (n_init + kAuditThreads - 1) / kAuditThreads;
  const int lg = a.dtype == CCMPC_F64 ? 9 : 10;
  const int64_t items = max_items(C, a.n_bound, int64_t(1) << lg);
  if (init_blocks >= (int64_t(1) << 31) || items >= (int64_t(1) << 31)) return CCMPC_ERR_ARG;
  hipLaunchKernelGGL(audit_init_kernel, dim3(static_cast<unsigned>(init_blocks)),
                     dim3(kAuditThreads), 0, s, a);
  if (a.dtype == CCMPC_F64)
    launch_typed<double>(a, static_cast<unsigned>(items), s);
  else
    launch_typed<float>(a, static_cast<unsigned>(items), s);
  return CCMPC_OK;
}

}  // namespace ccmpc
