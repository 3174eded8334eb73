// Monte-Carlo risk audit on the ideal rollout's samples, never materialised
// (ccmpc_ideal_risk_audit; no reference counterpart, as ccmpc_risk_audit).
//
// The contract is one sentence: the outputs are those of ccmpc_ideal_rollout (Z = NULL)
// followed by ccmpc_risk_audit on that store.  A sample of the rollout is a pure function of
// (seed, rng_cell[c], i, t) and the source moments, so this kernel regenerates it in registers
// with the rollout's own functions (ideal_step.hpp, normal_pair) in the rollout's order and
// evaluates audit_kernel's step arithmetic on it, word for word; the library is compiled
// without contraction, so the same source gives the same bits.
//  * Work item = one workgroup of 4 waves over a chunk of one cell's samples, one sample per
//    lane per trip (i = base + lane), about CCMPC_IDEAL_AUDIT_ITEMS items per launch.  Every
//    workgroup builds the cell's StepPlan[T] in LDS and stages the cell's status-0 records
//    bucketed by step, as audit_kernel does.
//  * The lane keeps its hit-at-any-step bit and the step's protected bit in registers across
//    t; counts are wave ballots + population counts added to LDS integers, flushed once per
//    workgroup with 64-bit integer atomic adds.  min_d2 is an unsigned 64-bit minimum on the
//    bit pattern of the non-negative double, in LDS and then in memory: a wave reduces its 64
//    values only when one of them is below the workgroup's running minimum (a stale read of
//    that minimum is only ever too large, so it costs a reduction and never a result).  No
//    float atomics: no output bit depends on arrival order.
//  * Lanes past n_samples run the recursion like any other and are masked out of every ballot.
// A first small launch writes the initial values (0, +inf, -1 for records that are not
// audited), so the caller prepares nothing; there is no workspace.
#include <string>

#include "audit.hpp"
#include "ideal_step.hpp"

namespace ccmpc {

constexpr int kIdealAuditThreads = 256;
// work items per launch (all cells): four workgroups per CU of a 256-CU part fit side by side
// (LDS 38 KB each with records), so every sample is in flight in one round
#ifndef CCMPC_IDEAL_AUDIT_ITEMS
#define CCMPC_IDEAL_AUDIT_ITEMS 1024
#endif

struct IdealAuditArgs {
  // the rollout
  const double *prev_mean, *prev_cov;
  int T_src;
  const int32_t *src_cell;
  int n_cells, T;
  int64_t n, chunk, items_per_cell;
  const double *x0;
  uint64_t seed;
  const uint64_t *seed_dev;
  const int32_t *rng_cell;
  // the audit
  const double *plan;        // [r][T][2] or null: no plan half
  const int32_t *cell_plan;  // [n_cells] or null: row 0
  const unsigned char *rec;  // [n_cells][P] records of `kind`, or null: no record half
  int kind, P;
  double R2;                 // R * R
  int64_t *hit, *hit_any;
  double *min_d2;
  int64_t *rec_open, *open;
  int32_t *status;
};

__device__ __forceinline__ void add_u64(int64_t *p, unsigned v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

// Initial values of every enabled output (audit_init_kernel's).
__global__ __launch_bounds__(kIdealAuditThreads) void ideal_audit_init_kernel(IdealAuditArgs a) {
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

template <bool PLAN, bool REC>
__global__ __launch_bounds__(kIdealAuditThreads) void ideal_audit_kernel(IdealAuditArgs a) {
  __shared__ StepPlan sp_s[kAuditMaxT];
  __shared__ double x0_s[2];
  __shared__ int status_s;
  __shared__ double4 stg[REC ? kAuditMaxRec : 1];   // side*n0, side*n1, side*rhs, R^2 |n|^2
  __shared__ int ridx[REC ? kAuditMaxRec : 1];      // the staged record's row in the cell
  __shared__ unsigned rcount[REC ? kAuditMaxRec : 1];  // samples it leaves open
  // staged records of step t: [tstart[t], tstart[t + 1])
  __shared__ int tstart[REC ? kAuditMaxT + 1 : 1];
  __shared__ int tfill[REC ? kAuditMaxT : 1];
  __shared__ unsigned open_s[REC ? kAuditMaxT : 1];
  __shared__ double plan_s[PLAN ? 2 * kAuditMaxT : 1];
  __shared__ unsigned hit_s[PLAN ? kAuditMaxT : 1];
  __shared__ unsigned long long min_s[PLAN ? kAuditMaxT : 1];
  __shared__ unsigned any_s;

  const int T = a.T, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t item = blockIdx.x;
  const int cell = static_cast<int>(item / a.items_per_cell);
  const int64_t cidx = item % a.items_per_cell;
  const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
  const int rows_src = 2 * a.T_src;
  const int src = a.src_cell ? a.src_cell[cell] : cell;
  const double *mu = a.prev_mean + static_cast<int64_t>(src) * rows_src;
  const double *cv = a.prev_cov + static_cast<int64_t>(src) * rows_src * rows_src;
  const uint32_t rng =
      a.rng_cell ? static_cast<uint32_t>(a.rng_cell[cell]) : static_cast<uint32_t>(cell);

  // ---- the cell's step plan and x0, as ideal_rollout_kernel builds them ---------------------
  if (tid == 0) status_s = 0;
  __syncthreads();
  if (tid < T) {
    const int st = build_step(mu, cv, rows_src, tid, sp_s[tid]);
    if (st) atomicMin(&status_s, st);
  }
  if (tid == 64) {
    int st = 0;
    initial_draw(mu, cv, rows_src, a.x0, cell, rng, seed, x0_s[0], x0_s[1], st);
    if (st) atomicMin(&status_s, st);
  }

  // ---- stage the plan row and the cell's audited records (audit_kernel's staging) -----------
  if (PLAN) {
    const int sel = a.cell_plan ? a.cell_plan[cell] : 0;
    if (tid < 2 * T) plan_s[tid] = a.plan[static_cast<int64_t>(sel) * 2 * T + tid];
    if (tid < T) {
      hit_s[tid] = 0;
      min_s[tid] = __builtin_bit_cast(unsigned long long, __builtin_huge_val());
    }
    if (tid == 0) any_s = 0;
  }
  if (REC) {
    const int64_t r0 = static_cast<int64_t>(cell) * a.P;
    if (tid < T) {
      tfill[tid] = 0;
      open_s[tid] = 0;
    }
    __syncthreads();
    for (int r = tid; r < a.P; r += kIdealAuditThreads) {
      const AuditRec q = audit_read_rec(a.rec, a.kind, r0 + r);
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
    for (int r = tid; r < a.P; r += kIdealAuditThreads) {
      const AuditRec q = audit_read_rec(a.rec, a.kind, r0 + r);
      if (!audit_rec_valid(q, T)) continue;
      const int k = tstart[q.t] + atomicAdd(&tfill[q.t], 1);
      if (k >= tstart[q.t + 1]) continue;  // records rewritten under the call: stay in bounds
      const double sd = static_cast<double>(q.side);
      stg[k] = double4{sd * q.n0, sd * q.n1, sd * q.rhs, a.R2 * (q.n0 * q.n0 + q.n1 * q.n1)};
      ridx[k] = r;
    }
  }
  __syncthreads();
  if (cidx == 0 && tid == 0 && a.status) a.status[cell] = status_s;

  // ---- the samples --------------------------------------------------------------------------
  const double R2 = a.R2;
  const double x0x = x0_s[0], x0y = x0_s[1];
  // i0 .. i1 are this item's samples.  Inside the loop every index is 32 bits (span and i fit:
  // n_samples < 2^32), which keeps the loop's uniform state out of SGPR pairs.
  const int64_t i0 = cidx * a.chunk;
  const int64_t i1 = (i0 + a.chunk < a.n) ? i0 + a.chunk : a.n;
  const uint32_t span = static_cast<uint32_t>(i1 - i0);
  const uint32_t first = 64u * w;  // the wave's first sample of the item
  const uint32_t trips =
      span > first ? (span - first + kIdealAuditThreads - 1) / kIdealAuditThreads : 0u;
  unsigned na = 0;  // this wave's samples hit at any step (wave-uniform)
  // no barrier inside: the trip count differs between waves at the tail
  for (uint32_t trip = 0, off = first; trip < trips; ++trip, off += kIdealAuditThreads) {
    // a lane past the item wraps at most to a small index: it is masked out of every ballot
    const uint32_t i = static_cast<uint32_t>(i0) + off + lane;
    const bool valid = static_cast<uint32_t>(lane) < span - off;
    double px = x0x, py = x0y;
    bool any = false;
    for (int t = 0; t < T; ++t) {
      double z0, z1;
      normal_pair(i, static_cast<uint32_t>(t), rng, STREAM_IDEAL_Z, seed, z0, z1);
      advance(sp_s[t], z0, z1, px, py);
      if (PLAN) {
        const double ax = plan_s[2 * t], ay = plan_s[2 * t + 1];
        const double dx = px - ax, dy = py - ay;
        const double d2 = dx * dx + dy * dy;
        const bool h = valid && d2 < R2;
        any = any || h;
        const unsigned nh = __popcll(__ballot(h));
        if (lane == 0 && nh) atomicAdd(&hit_s[t], nh);
        // the workgroup's minimum so far; another wave may lower it meanwhile, which only
        // makes this test pass where it need not
        const double seen = __builtin_bit_cast(double, min_s[t]);
        if (__ballot(valid && d2 < seen)) {  // wave-uniform, rare after the first trips
          double m = __builtin_huge_val();
          m = (valid && d2 < m) ? d2 : m;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const double x = __shfl_xor(m, o, 64);
            m = x < m ? x : m;
          }
          if (lane == 0) atomicMin(&min_s[t], __builtin_bit_cast(unsigned long long, m));
        }
      }
      if (REC) {
        bool prot = false;
        const int k1 = tstart[t + 1];
        for (int k = tstart[t]; k < k1; ++k) {
          const double4 q = stg[k];
          const double s = q.x * px + q.y * py;
          const bool p = audit_protects(q.z - s, q.w);
          prot = prot || p;
          const unsigned no = __popcll(__ballot(valid && !p));
          if (lane == 0 && no) atomicAdd(&rcount[k], no);
        }
        const unsigned no = __popcll(__ballot(valid && !prot));
        if (lane == 0 && no) atomicAdd(&open_s[t], no);
      }
    }
    if (PLAN) na += __popcll(__ballot(any));
  }
  if (PLAN && lane == 0 && na) atomicAdd(&any_s, na);
  __syncthreads();

  // ---- one flush per output -----------------------------------------------------------------
  // The output pointers are read from the argument block here: held in SGPRs across the sample
  // loop, beside the Philox round keys and the constants of log and sincos, they were spilled
  // to VGPR lanes.
  const IdealAuditArgs *o = (const IdealAuditArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(o));
  int ft = tid;  // likewise: the staging's `tid < T` masks are not kept for the flush
  asm volatile("" : "+v"(ft));
  const int64_t cT = static_cast<int64_t>(cell) * T;
  if (PLAN) {
    if (ft < T) {
      if (hit_s[ft]) add_u64(o->hit + cT + ft, hit_s[ft]);
      atomicMin(reinterpret_cast<unsigned long long *>(o->min_d2 + cT + ft), min_s[ft]);
    }
    if (ft == 0 && any_s) add_u64(o->hit_any + cell, any_s);
  }
  if (REC) {
    if (ft < T && open_s[ft]) add_u64(o->open + cT + ft, open_s[ft]);
    const int ns = tstart[T];
    for (int k = ft; k < ns; k += kIdealAuditThreads)
      if (rcount[k]) add_u64(o->rec_open + static_cast<int64_t>(cell) * o->P + ridx[k], rcount[k]);
  }
}

// samples per work item: a multiple of the workgroup's 256, about CCMPC_IDEAL_AUDIT_ITEMS items
// per launch.  items_per_cell * n_cells <= CCMPC_IDEAL_AUDIT_ITEMS + n_cells, so the grid fits.
inline int64_t ideal_audit_chunk(int64_t n_cells, int64_t n) {
  int64_t c = (n_cells * n + CCMPC_IDEAL_AUDIT_ITEMS - 1) / CCMPC_IDEAL_AUDIT_ITEMS;
  c = ((c + kIdealAuditThreads - 1) / kIdealAuditThreads) * kIdealAuditThreads;
  return c < kIdealAuditThreads ? kIdealAuditThreads : c;
}

}  // namespace ccmpc

using namespace ccmpc;

extern "C" int ccmpc_ideal_risk_audit(const double *prev_mean, const double *prev_cov,
                                      int64_t T_src, const int32_t *src_cell, int64_t n_cells,
                                      int64_t T, int64_t n_samples, const double *x0,
                                      uint64_t seed, const uint64_t *seed_dev,
                                      const int32_t *rng_cell, const double *plan,
                                      const int32_t *cell_plan, const void *rec, int rec_kind,
                                      double R, int64_t *out_hit, int64_t *out_hit_any,
                                      double *out_min_d2, int64_t *out_rec_open,
                                      int64_t *out_open, int32_t *out_status,
                                      ccmpc_stream_t stream) {
  static_assert(kAuditMaxT >= 39, "the audit's tables hold every rollout horizon");
  CCMPC_REQUIRE(T_src >= 2 && T_src <= 40, "T_src must be in [2, 40]");
  CCMPC_REQUIRE(T >= 1 && T <= T_src - 1, "T must be in [1, T_src - 1]");
  CCMPC_REQUIRE(n_cells >= 0 && n_cells < 65536, "bad n_cells");
  CCMPC_REQUIRE(n_samples >= 1 && n_samples < (int64_t(1) << 32), "bad n_samples");
  CCMPC_REQUIRE(std::isfinite(R) && R > 0.0, "R must be finite and positive");
  CCMPC_REQUIRE(plan || rec, "nothing to audit: plan and rec are both null");
  int P = 0;
  if (rec) {
    P = audit_rows(rec_kind, T);
    CCMPC_REQUIRE(P >= 0, "unknown rec_kind");
    // P == 0 (T = 1 of the half-space kinds): out_rec_open has no rows and may be null
    CCMPC_REQUIRE((out_rec_open || P == 0) && out_open,
                  "record half needs out_rec_open and out_open");
    CCMPC_REQUIRE(aligned(rec, 16), "records must be 16-byte aligned");
  }
  if (plan) {
    CCMPC_REQUIRE(out_hit && out_hit_any && out_min_d2,
                  "plan half needs out_hit, out_hit_any and out_min_d2");
    CCMPC_REQUIRE(aligned(plan, 8), "plan must be 8-byte aligned");
  }
  if (n_cells == 0) return CCMPC_OK;
  CCMPC_REQUIRE(prev_mean && prev_cov, "null pointer");
  CCMPC_REQUIRE(aligned(prev_mean, 8) && aligned(prev_cov, 8) && aligned(x0, 8) &&
                    aligned(seed_dev, 8) && aligned(src_cell, 4) && aligned(rng_cell, 4) &&
                    aligned(cell_plan, 4) && aligned(out_status, 4),
                "misaligned input");
  CCMPC_REQUIRE(aligned(out_hit, 8) && aligned(out_hit_any, 8) && aligned(out_min_d2, 8) &&
                    aligned(out_rec_open, 8) && aligned(out_open, 8),
                "outputs must be 8-byte aligned");
  const int64_t chunk = ideal_audit_chunk(n_cells, n_samples);
  const int64_t ipc = (n_samples + chunk - 1) / chunk;
  const IdealAuditArgs a{prev_mean, prev_cov, static_cast<int>(T_src), src_cell,
                         static_cast<int>(n_cells), static_cast<int>(T), n_samples, chunk, ipc,
                         x0, seed, seed_dev, rng_cell, plan, cell_plan,
                         static_cast<const unsigned char *>(rec), rec_kind, P, R * R, out_hit,
                         out_hit_any, out_min_d2, out_rec_open, out_open, out_status};
  int64_t n_init = n_cells * T;
  if (rec && n_cells * P > n_init) n_init = n_cells * P;
  const dim3 b(kIdealAuditThreads);
  const dim3 gi(static_cast<unsigned>((n_init + kIdealAuditThreads - 1) / kIdealAuditThreads));
  const dim3 g(static_cast<unsigned>(ipc * n_cells));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(ideal_audit_init_kernel, gi, b, 0, s, a);
  if (plan && rec)
    hipLaunchKernelGGL((ideal_audit_kernel<true, true>), g, b, 0, s, a);
  else if (plan)
    hipLaunchKernelGGL((ideal_audit_kernel<true, false>), g, b, 0, s, a);
  else
    hipLaunchKernelGGL((ideal_audit_kernel<false, true>), g, b, 0, s, a);
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}
