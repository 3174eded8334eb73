// Monte-Carlo calibration of half-space offsets on the ideal rollout's samples, never
// materialised (ccmpc_ideal_risk_quantile; no reference counterpart, as ccmpc_risk_quantile).
//
// The contract is one sentence: out_q, out_rhs and out_status are those of ccmpc_ideal_rollout
// (Z = NULL) followed by ccmpc_risk_quantile on that store.  A sample of the rollout is a pure
// function of (seed, rng_cell[c], i, t) and the source moments, so every counting pass
// regenerates it in registers with the rollout's own functions (ideal_step.hpp, normal_pair) in
// the rollout's order, as ideal_audit_kernel does, and forms quantile_count_kernel's projection
// and key on it, word for word; the library is compiled without contraction, so the same source
// gives the same bits.  The selection is the store call's radix select, 8 bits per pass:
//  * ideal_quantile_init_kernel, one workgroup per cell: builds the step plan and the initial
//    draw for the rollout's status and the first failed step f(c), decides SKIPPED (the store
//    call's rule, and every record of a step >= f(c)) / VACUOUS and writes those outputs, writes
//    the QuantRecs with their ranks m + 1 and zeroes the cell's bins.
//  * ideal_quantile_count_kernel, once per digit: ideal_audit_kernel's sample loop (a 4-wave
//    workgroup over a chunk of one cell's samples, one sample per lane per trip) times a second
//    grid dimension over chunks of <= 32 records, staged in LDS bucketed by step.  A chunk
//    generates steps only up to the largest step among its live records, and a workgroup with
//    nothing live returns before it builds a plan or generates a sample.  Every sample whose
//    key matches a record's prefix adds 1 to the record's 256-bin LDS histogram of the next
//    digit, with quantile_count_kernel's in-wave aggregation; non-zero bins are flushed with
//    32-bit integer atomic adds.
//  * ideal_quantile_narrow_kernel, after each count: one workgroup per record; its first wave
//    picks the digit where the count from the top reaches the rank (quant_pick_digit).
//  * The candidate list.  Every digit costs a regeneration of the whole rollout, so a record
//    leaves the digit loop as early as it can: when its selected bin holds at most kIqListCap
//    samples, the next counting pass has every matching sample append its whole key to the
//    record's list (an integer atomic counter gives the slot; the order is arbitrary), and the
//    narrowing launch picks the rank-th largest key of the list directly, ties included.  The
//    result depends on the multiset only, so every bit stays determined.  A resolved record
//    (kIqDone) has its outputs and is staged no more.  CCMPC_IDEAL_QUANT_LIST = 0 leaves a list
//    of one: the store call's single-candidate hand-over.
// Integer atomics only: nothing depends on arrival order.  The launch sequence is fixed.
#include "ideal_step.hpp"
#include "quantile.hpp"

namespace ccmpc {

#ifndef CCMPC_QUANTILE_AGG
#define CCMPC_QUANTILE_AGG 1
#endif
// capacity of a record's candidate list; 0: off (one candidate, as ccmpc_risk_quantile)
#ifndef CCMPC_IDEAL_QUANT_LIST
#define CCMPC_IDEAL_QUANT_LIST 1024
#endif
// work items per counting launch and record chunk (all cells), as CCMPC_IDEAL_AUDIT_ITEMS
#ifndef CCMPC_IDEAL_QUANT_ITEMS
#define CCMPC_IDEAL_QUANT_ITEMS 1024
#endif

constexpr int kIqThreads = 256;
constexpr uint32_t kIqListCap = CCMPC_IDEAL_QUANT_LIST > 0 ? CCMPC_IDEAL_QUANT_LIST : 1;
// QuantRec.t of a live record: its step in the low byte, and
constexpr int kIqList = 0x100;  // the next pass appends the matching keys to the record's list
constexpr int kIqDone = 0x200;  // resolved: the outputs are written

// Workspace: [C P] QuantRec, [C P][256] bins (uint32), [C P] remaining ranks (int64),
// [C P][kIqListCap] candidate keys (uint64), [C P] list lengths (uint32).
constexpr size_t kIqBytesPerRec =
    kQuantBytesPerRec + kIqListCap * sizeof(uint64_t) + sizeof(uint32_t);
inline size_t ideal_quantile_workspace_bytes(int64_t n_cells, int P) {
  return static_cast<size_t>(n_cells) * static_cast<size_t>(P) * kIqBytesPerRec + 64;
}

struct IdealQuantArgs {
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
  // the calibration
  const unsigned char *rec;  // [n_cells][P] records of `kind`
  int kind, P;
  double R2;                 // R * R
  const int64_t *allow;      // [n_cells] or null: zeros
  QuantRec *qrec;            // workspace
  uint32_t *bins;
  int64_t *rank;
  uint64_t *list;
  uint32_t *lcnt;
  double *out_q, *out_rhs;
  int32_t *out_status, *out_cell_status;
};

// First launch, one workgroup per cell.
__global__ __launch_bounds__(kIqThreads) void ideal_quantile_init_kernel(IdealQuantArgs a) {
  __shared__ int status_s, fail_s;
  const int T = a.T, tid = threadIdx.x;
  const int cell = blockIdx.x;
  const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
  const int rows_src = 2 * a.T_src;
  const int src = a.src_cell ? a.src_cell[cell] : cell;
  const double *mu = a.prev_mean + static_cast<int64_t>(src) * rows_src;
  const double *cv = a.prev_cov + static_cast<int64_t>(src) * rows_src * rows_src;
  const uint32_t rng =
      a.rng_cell ? static_cast<uint32_t>(a.rng_cell[cell]) : static_cast<uint32_t>(cell);
  if (tid == 0) {
    status_s = 0;
    fail_s = T;
  }
  __syncthreads();
  // the rollout's status, and f(c): the first step whose samples are NaN
  if (tid < T) {
    StepPlan sp;
    const int st = build_step(mu, cv, rows_src, tid, sp);
    if (st) {
      atomicMin(&status_s, st);
      atomicMin(&fail_s, tid);
    }
  }
  if (tid == 64) {
    int st = 0;
    double x, y;
    initial_draw(mu, cv, rows_src, a.x0, cell, rng, seed, x, y, st);
    if (st) {
      atomicMin(&status_s, st);
      atomicMin(&fail_s, 0);
    }
  }
  __syncthreads();
  if (tid == 0 && a.out_cell_status) a.out_cell_status[cell] = status_s;
  const int fail = fail_s;
  const int P = a.P;
  const int64_t r0 = static_cast<int64_t>(cell) * P;
  uint4 *b4 = reinterpret_cast<uint4 *>(a.bins) + r0 * 64;
  for (int i = tid; i < P * 64; i += kIqThreads) b4[i] = uint4{0u, 0u, 0u, 0u};
  const int64_t N = a.n;
  for (int k = tid; k < P; k += kIqThreads) {
    const int64_t i = r0 + k;
    const AuditRec r = audit_read_rec(a.rec, a.kind, i);
    const int64_t m = a.allow ? a.allow[cell] : 0;
    const bool cal = audit_rec_valid(r, T) && isfinite(r.n0) && isfinite(r.n1) && m >= 0 &&
                     r.t < fail;
    int32_t st = 0;
    if (!cal)
      st = CCMPC_CAL_SKIPPED;
    else if (m >= N)
      st = CCMPC_CAL_VACUOUS;
    QuantRec q;
    q.n0 = r.n0;
    q.n1 = r.n1;
    q.prefix = 0;
    q.side = r.side;
    q.t = st == 0 ? r.t : -1;
    a.qrec[i] = q;
    a.rank[i] = st == 0 ? m + 1 : 0;
    a.out_status[i] = st;
    if (st != 0) {
      a.out_q[i] = st == CCMPC_CAL_VACUOUS ? -__builtin_huge_val() : __builtin_nan("");
      a.out_rhs[i] = r.rhs;
    }
  }
}

__global__ __launch_bounds__(kIqThreads) void ideal_quantile_count_kernel(IdealQuantArgs a,
                                                                          int pass,
                                                                          int rows_per_chunk) {
  constexpr int RC = kQuantMaxChunk;
  __shared__ uint32_t bins[RC * 256];  // the next digit's histogram of every staged record
  __shared__ double4 stg[RC];          // n0, n1, (double)side, the prefix's bits
  __shared__ int ridx[RC];             // the staged record's row in the chunk
  __shared__ int list_s[RC];           // kIqList: append the matching keys, count nothing
  // staged records of step t: [tstart[t], tstart[t + 1])
  __shared__ int tstart[kAuditMaxT + 1];
  __shared__ int tfill[kAuditMaxT];
  __shared__ StepPlan sp_s[kAuditMaxT];
  __shared__ double x0_s[2];
  __shared__ int tend_s;  // one past the largest step that has a staged record

  const int T = a.T, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t item = blockIdx.x;
  const int cell = static_cast<int>(item / a.items_per_cell);
  const int64_t cidx = item % a.items_per_cell;
  const int row0 = static_cast<int>(blockIdx.y) * rows_per_chunk;
  int nrows = a.P - row0;
  nrows = nrows < rows_per_chunk ? nrows : rows_per_chunk;
  nrows = nrows < RC ? nrows : RC;
  if (nrows <= 0) return;  // uniform
  const int64_t rbase = static_cast<int64_t>(cell) * a.P + row0;

  // ---- stage the chunk's live records, bucketed by step (quantile_count_kernel's staging) --
  QuantRec q0;
  q0.t = -1;
  if (tid < nrows) q0 = a.qrec[rbase + tid];
  const bool live = q0.t >= 0 && !(q0.t & kIqDone) && (q0.t & 0xff) < T;
  const int t0 = q0.t & 0xff;
  if (tid < T) tfill[tid] = 0;
  for (int i = tid; i < nrows * 256; i += kIqThreads) bins[i] = 0;
  __syncthreads();
  if (live) atomicAdd(&tfill[t0], 1);
  __syncthreads();
  if (tid == 0) {
    int s = 0, te = 0;
    for (int t = 0; t < T; ++t) {
      tstart[t] = s;
      if (tfill[t]) te = t + 1;
      s += tfill[t];
      tfill[t] = 0;
    }
    tstart[T] = s;
    tend_s = te;
  }
  __syncthreads();
  const int tend = tend_s;
  if (tend == 0) return;  // uniform: nothing of this chunk is being selected
  if (live) {
    const int k = tstart[t0] + atomicAdd(&tfill[t0], 1);  // < nrows <= RC: one add per thread
    stg[k] = double4{q0.n0, q0.n1, static_cast<double>(q0.side),
                     __builtin_bit_cast(double, q0.prefix)};
    ridx[k] = tid;
    list_s[k] = q0.t & kIqList;
  }

  // ---- the cell's step plan and x0, as ideal_rollout_kernel builds them --------------------
  // a live record's step is below f(c): every step built here succeeds, and so does the draw
  {
    const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
    const int rows_src = 2 * a.T_src;
    const int src = a.src_cell ? a.src_cell[cell] : cell;
    const double *mu = a.prev_mean + static_cast<int64_t>(src) * rows_src;
    const double *cv = a.prev_cov + static_cast<int64_t>(src) * rows_src * rows_src;
    const uint32_t rng =
        a.rng_cell ? static_cast<uint32_t>(a.rng_cell[cell]) : static_cast<uint32_t>(cell);
    if (tid < tend) build_step(mu, cv, rows_src, tid, sp_s[tid]);
    if (tid == 64) {
      int st = 0;
      initial_draw(mu, cv, rows_src, a.x0, cell, rng, seed, x0_s[0], x0_s[1], st);
    }
  }
  __syncthreads();

  // ---- the samples (ideal_audit_kernel's loop) ----------------------------------------------
  const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
  const uint32_t rng =
      a.rng_cell ? static_cast<uint32_t>(a.rng_cell[cell]) : static_cast<uint32_t>(cell);
  const double x0x = x0_s[0], x0y = x0_s[1];
  const int sh = 56 - 8 * pass;  // the digit's position in the key
  // i0 .. i1 are this item's samples; inside the loop every index is 32 bits (n_samples < 2^32)
  const int64_t i0 = cidx * a.chunk;
  const int64_t i1 = (i0 + a.chunk < a.n) ? i0 + a.chunk : a.n;
  const uint32_t span = static_cast<uint32_t>(i1 - i0);
  const uint32_t first = 64u * wv;  // the wave's first sample of the item
  const uint32_t trips = span > first ? (span - first + kIqThreads - 1) / kIqThreads : 0u;
  // no barrier inside: the trip count differs between waves at the tail
  for (uint32_t trip = 0, off = first; trip < trips; ++trip, off += kIqThreads) {
    // a lane past the item wraps at most to a small index: it is masked out of every count
    const uint32_t i = static_cast<uint32_t>(i0) + off + lane;
    const bool valid = static_cast<uint32_t>(lane) < span - off;
    double px = x0x, py = x0y;
    for (int t = 0; t < tend; ++t) {
      double z0, z1;
      normal_pair(i, static_cast<uint32_t>(t), rng, STREAM_IDEAL_Z, seed, z0, z1);
      advance(sp_s[t], z0, z1, px, py);
      const int k1 = tstart[t + 1];
      for (int k = tstart[t]; k < k1; ++k) {
        const double4 q = stg[k];
        const uint64_t prefix = __builtin_bit_cast(uint64_t, q.w);
        const double s = q.x * px + q.y * py;
        const double w = q.z * s + 0.0;  // -0 becomes +0: bit order = value order
        const uint64_t key = quant_key(w);
        const uint64_t head = pass ? key >> (sh + 8) : 0;
        const bool act = valid && head == prefix;
        if (list_s[k]) {  // uniform: the few candidates left hand their keys over
          if (act) {
            const int64_t ri = rbase + ridx[k];
            const uint32_t at = atomicAdd(a.lcnt + ri, 1u);
            if (at < kIqListCap) a.list[ri * kIqListCap + at] = key;
          }
          continue;
        }
        uint32_t *h = bins + k * 256;
        const int dig = static_cast<int>((key >> sh) & 255u);
#if CCMPC_QUANTILE_AGG
        const unsigned long long am = __ballot(act);
        if (am) {  // uniform
          const int fl = __ffsll(static_cast<long long>(am)) - 1;
          const int d0 = __builtin_amdgcn_readlane(dig, fl);
          if (__ballot(act && dig == d0) == am) {
            if (lane == fl) atomicAdd(&h[d0], static_cast<uint32_t>(__popcll(am)));
          } else if (act) {
            atomicAdd(&h[dig], 1u);
          }
        }
#else
        if (act) atomicAdd(&h[dig], 1u);
#endif
      }
    }
  }
  __syncthreads();

  // ---- flush the non-zero bins --------------------------------------------------------------
  const IdealQuantArgs *o = (const IdealQuantArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(o));
  const int ns = tstart[T];
  uint32_t *g = o->bins + rbase * 256;
  for (int i = tid; i < ns * 256; i += kIqThreads) {
    const uint32_t v = bins[i];
    if (v) atomicAdd(g + static_cast<int64_t>(ridx[i >> 8]) * 256 + (i & 255), v);
  }
}

// q and the offset of record i from q's key (quantile.hip's quant_finish).
__device__ __forceinline__ void ideal_quant_finish(const IdealQuantArgs &a, int64_t i,
                                                   const QuantRec &q, uint64_t key) {
  const double qv = quant_unkey(key);
  const double sd = static_cast<double>(q.side);
  const double r2n = a.R2 * (q.n0 * q.n0 + q.n1 * q.n1);
  a.out_q[i] = qv;
  a.out_rhs[i] = sd * quant_unkey(quant_offset_key(qv, sd, r2n));
}

// One workgroup per record: the rank-th largest key of its list, or (first wave) the digit
// where the count from the top reaches the rank.
__global__ __launch_bounds__(kIqThreads) void ideal_quantile_narrow_kernel(IdealQuantArgs a,
                                                                           int pass) {
  __shared__ uint64_t keys[kIqListCap];
  __shared__ unsigned long long ans_s;
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const QuantRec q = a.qrec[i];
  if (q.t < 0 || (q.t & kIqDone)) return;  // uniform: nothing to select, or resolved
  const uint64_t r = static_cast<uint64_t>(a.rank[i]);
  if (q.t & kIqList) {  // uniform: this pass's candidates stored their keys
    uint32_t n = a.lcnt[i];
    n = n < kIqListCap ? n : kIqListCap;
    const uint64_t *l = a.list + i * kIqListCap;
    for (uint32_t j = tid; j < n; j += kIqThreads) keys[j] = l[j];
    // a list that does not reach the rank cannot happen (the bin's count was exact): defined
    if (tid == 0) ans_s = q.prefix << (64 - 8 * pass);
    __syncthreads();
    for (uint32_t j = tid; j < n; j += kIqThreads) {
      const uint64_t x = keys[j];
      uint32_t gt = 0, ge = 0;
      for (uint32_t k = 0; k < n; ++k) {
        const uint64_t y = keys[k];
        gt += y > x;
        ge += y >= x;
      }
      if (gt < r && r <= ge) ans_s = x;  // ties write the same bits
    }
    __syncthreads();
    if (tid == 0) {
      const uint64_t key = ans_s;
      a.qrec[i].prefix = key;
      a.qrec[i].t = (q.t & 0xff) | kIqDone;
      ideal_quant_finish(a, i, q, key);
    }
    return;
  }
  if (tid >= 64) return;
  const bool last = pass + 1 == kQuantDigits;
  uint4 *b4 = reinterpret_cast<uint4 *>(a.bins) + i * 64 + lane;
  const uint4 c = *b4;  // digits 4 lane .. 4 lane + 3
  if (!last) *b4 = uint4{0u, 0u, 0u, 0u};
  const QuantPick p = quant_pick_digit(c, r, lane);
  bool mine = p.mine;
  uint64_t run = p.run;
  if (!mine && lane == 0 && (r == 0 || r > p.grand)) {  // cannot happen: stay defined
    mine = true;
    run = r ? r - 1 : 0;
  }
  if (!mine) return;
  const uint64_t prefix = (q.prefix << 8) | static_cast<uint64_t>(4 * lane + p.dsel);
  if (last) {
    ideal_quant_finish(a, i, q, prefix);
    return;
  }
  a.qrec[i].prefix = prefix;
  a.rank[i] = static_cast<int64_t>(r - run);
  if (p.csel >= 1 && p.csel <= kIqListCap) {
    a.qrec[i].t = q.t | kIqList;
    a.lcnt[i] = 0;
  }
}

// samples per work item: a multiple of the workgroup's 256, about CCMPC_IDEAL_QUANT_ITEMS items
// per record chunk.  items_per_cell * n_cells <= CCMPC_IDEAL_QUANT_ITEMS + n_cells: the grid fits.
inline int64_t ideal_quant_chunk(int64_t n_cells, int64_t n) {
  int64_t c = (n_cells * n + CCMPC_IDEAL_QUANT_ITEMS - 1) / CCMPC_IDEAL_QUANT_ITEMS;
  c = ((c + kIqThreads - 1) / kIqThreads) * kIqThreads;
  return c < kIqThreads ? kIqThreads : c;
}

inline bool ideal_quant_shape_ok(int64_t T, int rec_kind, int64_t n_cells) {
  return T >= 1 && T <= 39 && n_cells >= 0 && n_cells < 65536 && audit_rows(rec_kind, T) >= 0;
}

}  // namespace ccmpc

using namespace ccmpc;

extern "C" size_t ccmpc_ideal_risk_quantile_workspace_bytes(int64_t T, int rec_kind,
                                                            int64_t n_cells) {
  if (!ideal_quant_shape_ok(T, rec_kind, n_cells)) return 0;
  return ideal_quantile_workspace_bytes(n_cells, audit_rows(rec_kind, T));
}

extern "C" int ccmpc_ideal_risk_quantile(const double *prev_mean, const double *prev_cov,
                                         int64_t T_src, const int32_t *src_cell, int64_t n_cells,
                                         int64_t T, int64_t n_samples, const double *x0,
                                         uint64_t seed, const uint64_t *seed_dev,
                                         const int32_t *rng_cell, const void *rec, int rec_kind,
                                         double R, const int64_t *cell_allow, void *workspace,
                                         size_t workspace_bytes, double *out_q, double *out_rhs,
                                         int32_t *out_status, int32_t *out_cell_status,
                                         ccmpc_stream_t stream) {
  static_assert(kAuditMaxT >= 39, "the tables hold every rollout horizon");
  CCMPC_REQUIRE(T_src >= 2 && T_src <= 40, "T_src must be in [2, 40]");
  CCMPC_REQUIRE(T >= 1 && T <= T_src - 1, "T must be in [1, T_src - 1]");
  CCMPC_REQUIRE(n_cells >= 0 && n_cells < 65536, "bad n_cells");
  CCMPC_REQUIRE(n_samples >= 1 && n_samples < (int64_t(1) << 32), "bad n_samples");
  CCMPC_REQUIRE(std::isfinite(R) && R > 0.0, "R must be finite and positive");
  const int P = audit_rows(rec_kind, T);
  CCMPC_REQUIRE(P >= 0, "unknown rec_kind");
  CCMPC_REQUIRE(rec, "rec is null");
  // P == 0 (T = 1 of the half-space kinds): no rows, at most out_cell_status is written
  CCMPC_REQUIRE(P == 0 || (out_q && out_rhs && out_status),
                "null output: out_q, out_rhs and out_status are needed");
  CCMPC_REQUIRE(workspace_bytes >= ideal_quantile_workspace_bytes(n_cells, P),
                "workspace too small");
  CCMPC_REQUIRE(aligned(workspace, 16), "workspace must be 16-byte aligned");
  if (n_cells == 0) return CCMPC_OK;
  if (P == 0 && !out_cell_status) return CCMPC_OK;
  CCMPC_REQUIRE(prev_mean && prev_cov, "null pointer");
  CCMPC_REQUIRE(P == 0 || workspace, "workspace is null");
  CCMPC_REQUIRE(aligned(prev_mean, 8) && aligned(prev_cov, 8) && aligned(x0, 8) &&
                    aligned(seed_dev, 8) && aligned(src_cell, 4) && aligned(rng_cell, 4) &&
                    aligned(cell_allow, 8) && aligned(out_cell_status, 4),
                "misaligned input");
  CCMPC_REQUIRE(aligned(rec, 16), "records must be 16-byte aligned");
  CCMPC_REQUIRE(aligned(out_q, 8) && aligned(out_rhs, 8) && aligned(out_status, 4),
                "outputs must be 8-byte (status 4-byte) aligned");
  const int64_t chunk = ideal_quant_chunk(n_cells, n_samples);
  const int64_t ipc = (n_samples + chunk - 1) / chunk;
  const size_t CP = static_cast<size_t>(n_cells) * static_cast<size_t>(P);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  const IdealQuantArgs a{prev_mean, prev_cov, static_cast<int>(T_src), src_cell,
                         static_cast<int>(n_cells), static_cast<int>(T), n_samples, chunk, ipc,
                         x0, seed, seed_dev, rng_cell, static_cast<const unsigned char *>(rec),
                         rec_kind, P, R * R, cell_allow, reinterpret_cast<QuantRec *>(ws),
                         reinterpret_cast<uint32_t *>(ws + CP * sizeof(QuantRec)),
                         reinterpret_cast<int64_t *>(ws + CP * (sizeof(QuantRec) + 1024)),
                         reinterpret_cast<uint64_t *>(ws + CP * kQuantBytesPerRec),
                         reinterpret_cast<uint32_t *>(
                             ws + CP * (kQuantBytesPerRec + kIqListCap * sizeof(uint64_t))),
                         out_q, out_rhs, out_status, out_cell_status};
  hipStream_t s = as_stream(stream);
  const dim3 b(kIqThreads);
  hipLaunchKernelGGL(ideal_quantile_init_kernel, dim3(static_cast<unsigned>(n_cells)), b, 0, s,
                     a);
  if (P > 0) {
    const int chunks = (P + kQuantMaxChunk - 1) / kQuantMaxChunk;
    const int rows = (P + chunks - 1) / chunks;
    const dim3 g(static_cast<unsigned>(ipc * n_cells), static_cast<unsigned>(chunks));
    for (int pass = 0; pass < kQuantDigits; ++pass) {
      hipLaunchKernelGGL(ideal_quantile_count_kernel, g, b, 0, s, a, pass, rows);
      hipLaunchKernelGGL(ideal_quantile_narrow_kernel, dim3(static_cast<unsigned>(CP)), b, 0, s,
                         a, pass);
    }
  }
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}
