// Monte-Carlo calibration of half-space offsets to a risk budget (ccmpc_risk_quantile; no
// reference counterpart): for every record of every cell, the (m+1)-th largest projection
// w = side * (n . p) + 0.0 of the cell's particles at the record's step, and the smallest offset
// for which ccmpc_risk_audit's own predicate protects a particle at that projection.
//
// The selection is a radix select on the order-preserving 64-bit key of w (a negative double
// has all bits flipped, any other its sign bit set), 8 bits per pass, most significant first:
//  * quantile_init_kernel: one thread per record decides SKIPPED / VACUOUS (and writes those
//    outputs), writes the record as the passes read it (QuantRec: n0, n1, side, t, prefix = 0)
//    with its rank m + 1, and zeroes the bins.  The caller prepares nothing.
//  * quantile_count_kernel, once per digit: the audit's streaming geometry -- a workgroup of 4
//    waves over 256 W particles of one cell (locate_item), 16 bytes per lane per plane, clamped
//    loads and masked tail lanes, the next load group in flight while this one is evaluated --
//    times a second grid dimension over chunks of <= 32 records.  The chunk's live records are
//    staged in LDS bucketed by step (counting sort), so records of one step share the particle
//    loads and only the planes of steps the chunk uses are read.  Every particle whose key
//    matches a record's prefix adds 1 to the record's 256-bin LDS histogram of the next digit.
//    Where all matching lanes of a wave hold the same digit (the sign / exponent bytes) the
//    wave issues one add of the population count instead of 64 same-address atomics.  Non-zero
//    bins are flushed with 32-bit integer atomic adds.
//  * quantile_narrow_kernel, after each count: one wave per record scans the 256 counts from
//    the top, extends the prefix by the digit where the running count reaches the rank, reduces
//    the rank and clears the bins.  After the last digit the prefix is q's key: the wave's
//    deciding lane writes q and searches the offset (an estimate, a few adjacent doubles, else
//    bisection over the ordered bit patterns) with the audit's predicate.
//  * A record whose selected bin holds exactly one particle needs no further digits: the next
//    counting pass has that particle store its whole key (kQuantSingle), after which the record
//    is resolved (kQuantDone) and no pass stages it any more.  A workgroup whose chunk has
//    nothing left to stage returns before it loads a particle, so once the low mantissa bytes
//    are reached the passes cost little more than their launches.  The launch sequence stays
//    fixed; ties (several particles with q's exact bits) simply run all eight digits.
// Integer atomics only: nothing depends on arrival order, every output bit is determined.
#include "quantile.hpp"

#include <type_traits>

namespace ccmpc {

#ifndef CCMPC_QUANTILE_AGG
#define CCMPC_QUANTILE_AGG 1  // 0: always per-lane LDS adds (tools/time_quantile.py's A/B)
#endif

constexpr int kQuantThreads = 256;
// QuantRec.t of a live record: its step in the low byte, and
constexpr int kQuantSingle = 0x100;  // one candidate left: the next pass stores its key in rank[]
constexpr int kQuantDone = 0x200;    // prefix is q's whole key
constexpr int kQuantU = 4;  // steps per load group

// First launch: statuses, the outputs of records that select nothing, the staged records, the
// ranks and empty bins.
__global__ __launch_bounds__(kQuantThreads) void quantile_init_kernel(QuantArgs a) {
  const int64_t CP = static_cast<int64_t>(a.n_cells) * a.P;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint4 *b4 = reinterpret_cast<uint4 *>(a.bins);
  for (int64_t i = i0; i < CP * 64; i += stride) b4[i] = uint4{0u, 0u, 0u, 0u};
  for (int64_t i = i0; i < CP; i += stride) {
    const int64_t c = i / a.P;
    const AuditRec r = audit_read_rec(a.rec, a.kind, i);
    const int64_t N = a.cnt[c], m = a.allow ? a.allow[c] : 0;
    const bool cal = audit_rec_valid(r, a.T) && isfinite(r.n0) && isfinite(r.n1) && m >= 0;
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

template <typename P>
__global__ __launch_bounds__(kQuantThreads) void quantile_count_kernel(QuantArgs a, int pass,
                                                                       int rows_per_chunk) {
  using V = AuditVec<P>;
  constexpr int W = V::W;
  constexpr int LG = W == 2 ? 8 + 1 : 8 + 2;  // log2 particles per item (kQuantThreads * W)
  constexpr int U = kQuantU;
  constexpr int RC = kQuantMaxChunk;
  __shared__ uint32_t bins[RC * 256];  // the next digit's histogram of every staged record
  __shared__ double4 stg[RC];          // n0, n1, (double)side, the prefix's bits
  __shared__ int ridx[RC];             // the staged record's row in the chunk
  __shared__ int single_s[RC];         // kQuantSingle: store the matching key, count nothing
  // staged records of step t: [tstart[t], tstart[t + 1]); tlist: the steps that have any
  __shared__ int tstart[kAuditMaxT + 1];
  __shared__ int tfill[kAuditMaxT];
  __shared__ int tlist[kAuditMaxT];
  __shared__ int nsteps_s;

  ItemLoc loc;
  if (!locate_item(blockIdx.x, a.cnt, a.off, a.n_cells, LG, loc)) return;  // uniform
  const int64_t cnt = loc.cnt;
  if (cnt <= 0) return;  // an empty cell's records are VACUOUS or SKIPPED
  const int T = a.T, tid = threadIdx.x;
  [[maybe_unused]] const int lane = tid & 63;
  const int64_t cell = loc.cell;
  const int row0 = static_cast<int>(blockIdx.y) * rows_per_chunk;
  int nrows = a.P - row0;
  nrows = nrows < rows_per_chunk ? nrows : rows_per_chunk;
  nrows = nrows < RC ? nrows : RC;
  if (nrows <= 0) return;  // uniform

  // ---- stage the chunk's live records, bucketed by step ------------------------------------
  QuantRec q0;
  q0.t = -1;
  if (tid < nrows) q0 = a.qrec[cell * a.P + row0 + tid];
  const bool live = q0.t >= 0 && !(q0.t & kQuantDone) && (q0.t & 0xff) < T;
  const int t0 = q0.t & 0xff;
  if (tid < T) tfill[tid] = 0;
  for (int i = tid; i < nrows * 256; i += kQuantThreads) bins[i] = 0;
  __syncthreads();
  if (live) atomicAdd(&tfill[t0], 1);
  __syncthreads();
  if (tid == 0) {
    int s = 0, ns = 0;
    for (int t = 0; t < T; ++t) {
      tstart[t] = s;
      if (tfill[t]) tlist[ns++] = t;
      s += tfill[t];
      tfill[t] = 0;
    }
    tstart[T] = s;
    nsteps_s = ns;
  }
  __syncthreads();
  const int nsteps = nsteps_s;
  if (nsteps == 0) return;  // uniform: nothing of this chunk is being selected
  if (live) {
    const int k = tstart[t0] + atomicAdd(&tfill[t0], 1);  // < nrows <= RC: one add per thread
    stg[k] = double4{q0.n0, q0.n1, static_cast<double>(q0.side),
                     __builtin_bit_cast(double, q0.prefix)};
    ridx[k] = tid;
    single_s[k] = q0.t & kQuantSingle;
  }

  // ---- the lane's particles ------------------------------------------------------------------
  const int64_t idx = (static_cast<int64_t>(loc.chunk_idx) << LG) + static_cast<int64_t>(W) * tid;
  const int64_t qlast = (cnt - 1) & ~static_cast<int64_t>(W - 1);
  const P *base = static_cast<const P *>(a.pos) + loc.off + (idx < qlast ? idx : qlast);
  bool valid[W];
#pragma unroll
  for (int j = 0; j < W; ++j) valid[j] = idx + j < cnt;
  double o0 = 0.0, o1 = 0.0;
  if (std::is_same_v<P, float> && a.origin) {
    o0 = a.origin[2 * cell];
    o1 = a.origin[2 * cell + 1];
  }
  const int64_t ld = a.ld;
  const int sh = 56 - 8 * pass;  // the digit's position in the key

  auto load_steps = [&](V (&b)[U][2], int i0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = tlist[i0 + u < nsteps ? i0 + u : nsteps - 1];
      b[u][0].load(base + static_cast<int64_t>(2 * t) * ld);
      b[u][1].load(base + static_cast<int64_t>(2 * t + 1) * ld);
    }
  };
  V cur[U][2], nxt[U][2];
  load_steps(cur, 0);
  __syncthreads();  // stg / ridx are staged

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
    const int k1 = tstart[t + 1];
    for (int k = tstart[t]; k < k1; ++k) {
      const double4 q = stg[k];
      const uint64_t prefix = __builtin_bit_cast(uint64_t, q.w);
      uint32_t *h = bins + k * 256;
      const bool single = single_s[k] != 0;  // uniform
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const double s = q.x * px[j] + q.y * py[j];
        const double w = q.z * s + 0.0;  // -0 becomes +0: bit order = value order
        const uint64_t key = quant_key(w);
        const uint64_t head = pass ? key >> (sh + 8) : 0;
        const bool act = valid[j] && head == prefix;
        const int dig = static_cast<int>((key >> sh) & 255u);
        if (single) {  // the one candidate left (one lane of the whole grid) hands its key over
          if (act) a.rank[cell * a.P + row0 + ridx[k]] = static_cast<int64_t>(key);
          continue;
        }
#if CCMPC_QUANTILE_AGG
        const unsigned long long am = __ballot(act);
        if (am) {  // uniform
          const int first = __ffsll(static_cast<long long>(am)) - 1;
          const int d0 = __builtin_amdgcn_readlane(dig, first);
          if (__ballot(act && dig == d0) == am) {
            if (lane == first) atomicAdd(&h[d0], static_cast<uint32_t>(__popcll(am)));
          } else if (act) {
            atomicAdd(&h[dig], 1u);
          }
        }
#else
        if (act) atomicAdd(&h[dig], 1u);
#endif
      }
    }
  };

  for (int i0 = 0; i0 < nsteps; i0 += U) {
    if (i0 + U < nsteps) load_steps(nxt, i0 + U);  // uniform
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u < nsteps) step(tlist[i0 + u], cur[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cur[u][0] = nxt[u][0];
      cur[u][1] = nxt[u][1];
    }
  }
  __syncthreads();

  // ---- flush the non-zero bins ---------------------------------------------------------------
  const int ns = tstart[T];
  uint32_t *g = a.bins + (cell * a.P + row0) * 256;
  for (int i = tid; i < ns * 256; i += kQuantThreads) {
    const uint32_t v = bins[i];
    if (v) atomicAdd(g + static_cast<int64_t>(ridx[i >> 8]) * 256 + (i & 255), v);
  }
}

// q and the offset of record i from q's key.
__device__ __forceinline__ void quant_finish(const QuantArgs &a, int64_t i, const QuantRec &q,
                                             uint64_t key) {
  const double qv = quant_unkey(key);
  const double sd = static_cast<double>(q.side);
  const double r2n = a.R2 * (q.n0 * q.n0 + q.n1 * q.n1);
  a.out_q[i] = qv;
  a.out_rhs[i] = sd * quant_unkey(quant_offset_key(qv, sd, r2n));
}

// One wave per record: the digit where the count from the top reaches the rank.
__global__ __launch_bounds__(kQuantThreads) void quantile_narrow_kernel(QuantArgs a, int pass) {
  const int64_t CP = static_cast<int64_t>(a.n_cells) * a.P;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * (kQuantThreads / 64) + (threadIdx.x >> 6);
  if (i >= CP) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const QuantRec q = a.qrec[i];
  if (q.t < 0) return;  // wave-uniform: its bins were never touched
  const bool last = pass + 1 == kQuantDigits;
  if (q.t & (kQuantDone | kQuantSingle)) {  // wave-uniform: nothing was counted for it
    if (lane != 0) return;
    uint64_t key = q.prefix;
    if (q.t & kQuantSingle) {  // this pass's candidate stored its key
      key = static_cast<uint64_t>(a.rank[i]);
      a.qrec[i].prefix = key;
      a.qrec[i].t = (q.t & 0xff) | kQuantDone;
    }
    if (last) quant_finish(a, i, q, key);
    return;
  }
  uint4 *b4 = reinterpret_cast<uint4 *>(a.bins) + i * 64 + lane;
  const uint4 c = *b4;  // digits 4 lane .. 4 lane + 3
  if (!last) *b4 = uint4{0u, 0u, 0u, 0u};
  const uint64_t r = static_cast<uint64_t>(a.rank[i]);
  const uint32_t tot = c.x + c.y + c.z + c.w;
  const uint32_t incl = static_cast<uint32_t>(wave_incl_scan_i32(static_cast<int32_t>(tot)));
  const uint32_t grand = static_cast<uint32_t>(lane_i32(static_cast<int32_t>(incl), 63));
  const uint64_t above = grand - incl;  // the count of all larger digits
  bool mine = above < r && r <= above + tot;
  int dsel = 0;
  uint32_t csel = 0;  // the selected digit's count
  uint64_t run = above;
  if (mine) {
    if (run + c.w >= r) {
      dsel = 3;
      csel = c.w;
    } else if (run + c.w + c.z >= r) {
      run += c.w;
      dsel = 2;
      csel = c.z;
    } else if (run + c.w + c.z + c.y >= r) {
      run += static_cast<uint64_t>(c.w) + c.z;
      dsel = 1;
      csel = c.y;
    } else {
      run += static_cast<uint64_t>(c.w) + c.z + c.y;
      csel = c.x;
    }
  } else if (lane == 0 && (r == 0 || r > grand)) {
    // counts that do not reach the rank (the store was rewritten under the call): stay defined
    mine = true;
    run = r ? r - 1 : 0;
  }
  if (!mine) return;
  const uint64_t prefix = (q.prefix << 8) | static_cast<uint64_t>(4 * lane + dsel);
  if (last) {
    quant_finish(a, i, q, prefix);
    return;
  }
  a.qrec[i].prefix = prefix;
  a.rank[i] = static_cast<int64_t>(r - run);
  if (csel == 1) a.qrec[i].t = q.t | kQuantSingle;
}

int launch_risk_quantile(const QuantArgs &a, hipStream_t s) {
  const int64_t CP = static_cast<int64_t>(a.n_cells) * a.P;
  const int lg = a.dtype == CCMPC_F64 ? 9 : 10;
  const int64_t items = max_items(a.n_cells, a.n_bound, int64_t(1) << lg);
  const int chunks = (a.P + kQuantMaxChunk - 1) / kQuantMaxChunk;
  const int rows = (a.P + chunks - 1) / chunks;
  const int64_t narrow_blocks = (CP + kQuantThreads / 64 - 1) / (kQuantThreads / 64);
  if (items >= (int64_t(1) << 31) || narrow_blocks >= (int64_t(1) << 31) || chunks > 65535)
    return CCMPC_ERR_ARG;
  int64_t init_blocks = (CP * 64 + kQuantThreads - 1) / kQuantThreads;
  init_blocks = init_blocks < 4096 ? init_blocks : 4096;
  hipLaunchKernelGGL(quantile_init_kernel, dim3(static_cast<unsigned>(init_blocks)),
                     dim3(kQuantThreads), 0, s, a);
  const dim3 g(static_cast<unsigned>(items), static_cast<unsigned>(chunks)), b(kQuantThreads);
  for (int pass = 0; pass < kQuantDigits; ++pass) {
    if (a.dtype == CCMPC_F64)
      hipLaunchKernelGGL(quantile_count_kernel<double>, g, b, 0, s, a, pass, rows);
    else
      hipLaunchKernelGGL(quantile_count_kernel<float>, g, b, 0, s, a, pass, rows);
    hipLaunchKernelGGL(quantile_narrow_kernel, dim3(static_cast<unsigned>(narrow_blocks)),
                       dim3(kQuantThreads), 0, s, a, pass);
  }
  return CCMPC_OK;
}

}  // namespace ccmpc
