// Monte-Carlo calibration of the box-face rows to a risk budget (ccmpc_face_quantile; no
// reference counterpart): for every (cell, t, face) the (m+1)-th largest face value v_f + 0.0 of
// the cell's particles at a plan -- the distance by which the row misses (> 0) or clears (<= 0)
// the budget of m open particles --, the particle that attains it, and that particle's own
// half-space v_f(x) <= 0 shifted to the budget, as a record the planning QP reads.
//
// The values are ccmpc_face_audit's (face_values, face_audit.hpp: the same inline function, the
// same bits); the selection is ccmpc_risk_quantile's radix select on the order-preserving key of
// the double (quantile.hpp), 8 bits per pass, most significant first.  Rows are (cell, t, face):
//  * face_quantile_init_kernel: one thread per row decides SKIPPED / VACUOUS, writes every
//    output's initial value (an empty cut, arg -1) and the row's workspace (prefix 0, rank m + 1,
//    no arg yet), and zeroes the bins.  The caller prepares nothing.
//  * face_quantile_pass_kernel<P, false>, once per digit: face_audit_kernel's streaming geometry
//    -- a workgroup of 4 waves over 256 W particles of one cell (locate_item), 16 bytes per lane
//    per plane, clamped loads and masked tail lanes, the next four steps in flight while these
//    are evaluated, the previous step kept in registers for the heading -- times a second grid
//    dimension over chunks of 8 steps = 32 rows, one 1 KiB LDS histogram each.  A chunk that
//    starts at t > 0 reads the step before it once more for its first heading.  Every particle
//    whose key matches a row's prefix adds 1 to the row's histogram of the next digit; where all
//    matching lanes of a wave hold the same digit (the sign / exponent bytes) the wave issues
//    one add of the population count.  Non-zero bins are flushed with 32-bit integer atomics.
//  * face_quantile_narrow_kernel, after each count: one wave per row scans the 256 counts from
//    the top (DPP scan), extends the prefix by the digit where the running count reaches the
//    rank, reduces the rank and clears the bins.  A row whose selected bin holds one particle
//    needs no further digits: the next pass has that particle store its whole key.  A chunk with
//    nothing left to select returns before it loads a particle.  After the last digit the prefix
//    is q's key and out_q is written.
//  * face_quantile_pass_kernel<P, true>: one more pass in which every particle whose key equals
//    q's lowers the row's arg to its index within the cell (a 32-bit integer atomic minimum, in
//    LDS and then in the workspace): the lowest index that holds q's bits.
//  * face_quantile_cut_kernel: one thread per row forms the heading of the arg particle again
//    (two positions, the same face_heading) and writes out_arg and the cut.
// Integer atomics only: nothing depends on arrival order, every output bit is determined.
#include "face_quantile.hpp"

#include <type_traits>

namespace ccmpc {

constexpr int kFaceQuantThreads = 256;
constexpr int kFaceQuantU = 4;  // steps per load group
// a row's state in the workspace
constexpr int kFqDead = -1;    // VACUOUS or SKIPPED: nothing to select
constexpr int kFqLive = 0;     // digits are being counted
constexpr int kFqSingle = 1;   // one candidate left: the next pass stores its key in rank[]
constexpr int kFqDone = 2;     // prefix is q's whole key
constexpr uint32_t kFqNoArg = 0xFFFFFFFFu;

// ccmpc_gather_rec as two 16-byte halves: n0, n1 | rhs, side (int16, -1) | status (int16) << 16
// | t_tau << 32: ccmpc_face_cuts' packing.
__device__ __forceinline__ void face_quant_store_cut(double2 *out, int64_t i, double n0, double n1,
                                                     double rhs, int status, int t) {
  const uint64_t tail = (static_cast<uint64_t>(static_cast<uint32_t>(t)) << 32) |
                        (static_cast<uint32_t>(static_cast<uint16_t>(status)) << 16) | 0xFFFFu;
  out[2 * i] = double2{n0, n1};
  out[2 * i + 1] = double2{rhs, __builtin_bit_cast(double, tail)};
}

// First launch: statuses, every output's initial value, the rows' workspace and empty bins.
__global__ __launch_bounds__(kFaceQuantThreads) void face_quantile_init_kernel(FaceQuantArgs a) {
  const int64_t R = static_cast<int64_t>(a.n_cells) * a.T * 4;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint4 *b4 = reinterpret_cast<uint4 *>(a.bins);
  for (int64_t i = i0; i < R * 64; i += stride) b4[i] = uint4{0u, 0u, 0u, 0u};
  for (int64_t i = i0; i < R; i += stride) {
    const int64_t ct = i >> 2, c = ct / a.T;
    const int t = static_cast<int>(ct - c * a.T);
    const int64_t N = a.cnt[c], m = a.allow ? a.allow[c] : 0;
    int32_t st = 0;
    if (m < 0)
      st = CCMPC_CAL_SKIPPED;
    else if (m >= N)
      st = CCMPC_CAL_VACUOUS;
    a.prefix[i] = 0;
    a.rank[i] = st == 0 ? m + 1 : 0;
    a.arg[i] = kFqNoArg;
    a.state[i] = st == 0 ? kFqLive : kFqDead;
    if ((i & 3) == 0) a.out_status[ct] = st;
    a.out_q[i] = st == CCMPC_CAL_SKIPPED ? __builtin_nan("") : -__builtin_huge_val();
    a.out_arg[i] = -1;
    face_quant_store_cut(a.out_cut, i, 0.0, 0.0, 0.0, CCMPC_CUT_EMPTY, t);
  }
}

// ARG = false: the counting pass of digit `pass`.  ARG = true: the lowest index holding q's key.
template <typename P, bool ARG>
__global__ __launch_bounds__(kFaceQuantThreads) void face_quantile_pass_kernel(FaceQuantArgs a,
                                                                              int pass) {
  using V = AuditVec<P>;
  constexpr int W = V::W;
  constexpr int LG = W == 2 ? 8 + 1 : 8 + 2;  // log2 particles per item (threads * W)
  constexpr int U = kFaceQuantU;
  constexpr int TS = kFaceQuantSteps;
  constexpr int RC = 4 * TS;
  static_assert(TS % U == 0, "whole load groups");
  // the next digit's histogram of every row; ARG: the row's lowest matching index
  __shared__ uint32_t bins[ARG ? RC : RC * 256];
  __shared__ unsigned long long pre_s[RC];  // the row's prefix (ARG: q's key)
  __shared__ int st_s[RC];                  // 0: not staged, 1: staged, 2: staged, kFqSingle
  __shared__ double plan_s[2 * TS];

  ItemLoc loc;
  if (!locate_item(blockIdx.x, a.cnt, a.off, a.n_cells, LG, loc, a.cell_plan)) return;  // uniform
  const int64_t cnt = loc.cnt;
  if (cnt <= 0) return;  // an empty cell's rows are VACUOUS or SKIPPED
  const int T = a.T, tid = threadIdx.x;
  [[maybe_unused]] const int lane = tid & 63;
  const int64_t cell = loc.cell;
  const int t0 = static_cast<int>(blockIdx.y) * TS;
  int nst = T - t0;
  nst = nst < TS ? nst : TS;
  if (nst <= 0) return;  // uniform
  const int nrows = 4 * nst;
  const int64_t rb = (cell * T + t0) * 4;  // the chunk's first row

  // ---- stage the chunk's rows ------------------------------------------------------------------
  int st = 0;
  unsigned long long pre = 0;
  if (tid < nrows) {
    const int s = a.state[rb + tid];
    pre = a.prefix[rb + tid];
    if (ARG)
      st = s == kFqDone ? 1 : 0;
    else
      st = s == kFqLive ? 1 : s == kFqSingle ? 2 : 0;
  }
  if (tid < RC) {
    pre_s[tid] = pre;
    st_s[tid] = st;
  }
  if (!__syncthreads_or(st != 0)) return;  // uniform: nothing of this chunk is being selected

  // ---- the lane's particles ----------------------------------------------------------------------
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
  [[maybe_unused]] const int sh = 56 - 8 * pass;  // the digit's position in the key

  auto load_steps = [&](V (&b)[U][2], int u0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + (u0 + u < nst ? u0 + u : nst - 1);
      b[u][0].load(base + static_cast<int64_t>(2 * t) * ld);
      b[u][1].load(base + static_cast<int64_t>(2 * t + 1) * ld);
    }
  };

  double plan_v = 0.0;
  if (tid < 2 * nst)
    plan_v = a.plan[(static_cast<int64_t>(loc.ref_sel) * T + t0 + (tid >> 1)) * a.ld_plan +
                    (tid & 1)];
  const double past_x = a.past_last[2 * cell], past_y = a.past_last[2 * cell + 1];
  const double half_r = 0.5 * a.car_r;
  const double hlon = 0.5 * a.extent[0] + half_r, hlat = 0.5 * a.extent[1] + half_r;
  V cur[U][2], nxt[U][2], prev[2];
  {
    const int tp = t0 > 0 ? t0 - 1 : 0;  // the step before the chunk (unused at t = 0)
    prev[0].load(base + static_cast<int64_t>(2 * tp) * ld);
    prev[1].load(base + static_cast<int64_t>(2 * tp + 1) * ld);
  }
  load_steps(cur, 0);

  if (tid < 2 * nst) plan_s[tid] = plan_v;
  if (ARG) {
    if (tid < RC) bins[tid] = kFqNoArg;
  } else {
    for (int i = tid; i < nrows * 256; i += kFaceQuantThreads) bins[i] = 0;
  }
  __syncthreads();

  auto step = [&](int tl, const V (&b)[2], const V (&pb)[2]) {
    const int t = t0 + tl, k0 = 4 * tl;
    if ((st_s[k0] | st_s[k0 + 1] | st_s[k0 + 2] | st_s[k0 + 3]) == 0) return;  // uniform
    const double X = plan_s[2 * tl], Y = plan_s[2 * tl + 1];
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double x = face_world(b[0][j], o0), y = face_world(b[1][j], o1);
      const double xp = t == 0 ? past_x : face_world(pb[0][j], o0);
      const double yp = t == 0 ? past_y : face_world(pb[1][j], o1);
      double S, C, v[4];
      face_values(x, y, xp, yp, X, Y, hlat, hlon, S, C, v[0], v[1], v[2], v[3]);
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int k = k0 + f, sk = st_s[k];
        if (sk == 0) continue;  // uniform
        const uint64_t key = quant_key(v[f] + 0.0);  // -0 becomes +0: bit order = value order
        const uint64_t prefix = pre_s[k];
        if constexpr (ARG) {
          if (valid[j] && key == prefix) atomicMin(&bins[k], static_cast<uint32_t>(idx + j));
        } else {
          const uint64_t head = pass ? key >> (sh + 8) : 0;
          const bool act = valid[j] && head == prefix;
          const int dig = static_cast<int>((key >> sh) & 255u);
          if (sk == 2) {  // the one candidate left (one lane of the whole grid) hands its key over
            if (act) a.rank[rb + k] = static_cast<int64_t>(key);
            continue;
          }
          uint32_t *h = bins + k * 256;
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
        }
      }
    }
  };

  for (int u0 = 0; u0 < nst; u0 += U) {
    if (u0 + U < nst) load_steps(nxt, u0 + U);  // uniform
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u0 + u < nst) step(u0 + u, cur[u], u == 0 ? prev : cur[u ? u - 1 : 0]);
    prev[0] = cur[U - 1][0];
    prev[1] = cur[U - 1][1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cur[u][0] = nxt[u][0];
      cur[u][1] = nxt[u][1];
    }
  }
  __syncthreads();

  // ---- flush ---------------------------------------------------------------------------------------
  if constexpr (ARG) {
    if (tid < nrows && bins[tid] != kFqNoArg) atomicMin(a.arg + rb + tid, bins[tid]);
  } else {
    uint32_t *g = a.bins + rb * 256;
    for (int i = tid; i < nrows * 256; i += kFaceQuantThreads) {
      const uint32_t v = bins[i];
      if (v) atomicAdd(g + i, v);
    }
  }
}

// One wave per row: the digit where the count from the top reaches the rank.
__global__ __launch_bounds__(kFaceQuantThreads) void face_quantile_narrow_kernel(FaceQuantArgs a,
                                                                                int pass) {
  const int64_t R = static_cast<int64_t>(a.n_cells) * a.T * 4;
  const int64_t i =
      static_cast<int64_t>(blockIdx.x) * (kFaceQuantThreads / 64) + (threadIdx.x >> 6);
  if (i >= R) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int st = a.state[i];
  if (st == kFqDead) return;  // wave-uniform: its bins were never touched
  const bool last = pass + 1 == kQuantDigits;
  const uint64_t pre = a.prefix[i];
  if (st != kFqLive) {  // wave-uniform: nothing was counted for it
    if (lane != 0) return;
    uint64_t key = pre;
    if (st == kFqSingle) {  // this pass's candidate stored its key
      key = static_cast<uint64_t>(a.rank[i]);
      a.prefix[i] = key;
      a.state[i] = kFqDone;
    }
    if (last) a.out_q[i] = quant_unkey(key);
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
  const uint64_t prefix = (pre << 8) | static_cast<uint64_t>(4 * lane + dsel);
  a.prefix[i] = prefix;
  if (last) {
    a.state[i] = kFqDone;
    a.out_q[i] = quant_unkey(prefix);
    return;
  }
  a.rank[i] = static_cast<int64_t>(r - run);
  if (csel == 1) a.state[i] = kFqSingle;
}

// One thread per row: out_arg and the cut from the arg particle's own heading.
template <typename P>
__global__ __launch_bounds__(kFaceQuantThreads) void face_quantile_cut_kernel(FaceQuantArgs a) {
  const int64_t R = static_cast<int64_t>(a.n_cells) * a.T * 4;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= R) return;
  if (a.state[i] != kFqDone) return;  // the initial values stand
  const uint32_t ai = a.arg[i];
  if (ai == kFqNoArg) return;  // no particle holds q's bits (the store was rewritten under the call)
  const int f = static_cast<int>(i & 3);
  const int64_t ct = i >> 2, c = ct / a.T;
  const int t = static_cast<int>(ct - c * a.T);
  if (static_cast<int64_t>(ai) >= a.cnt[c]) return;
  const P *p = static_cast<const P *>(a.pos) + a.off[c] + ai;
  double o0 = 0.0, o1 = 0.0;
  if (std::is_same_v<P, float> && a.origin) {
    o0 = a.origin[2 * c];
    o1 = a.origin[2 * c + 1];
  }
  const double x = face_world(p[static_cast<int64_t>(2 * t) * a.ld], o0);
  const double y = face_world(p[static_cast<int64_t>(2 * t + 1) * a.ld], o1);
  const int tp = t > 0 ? t - 1 : 0;
  const double xp = t == 0 ? a.past_last[2 * c] : face_world(p[static_cast<int64_t>(2 * tp) * a.ld], o0);
  const double yp =
      t == 0 ? a.past_last[2 * c + 1] : face_world(p[static_cast<int64_t>(2 * tp + 1) * a.ld], o1);
  double S, C;
  face_heading(x - xp, y - yp, S, C);
  const int r = a.cell_plan ? a.cell_plan[c] : 0;
  const double *pl = a.plan + (static_cast<int64_t>(r) * a.T + t) * a.ld_plan;
  const double X = pl[0], Y = pl[1];
  // the gradient of v_f in (X, Y): (-c, s), (-s, -c), (c, -s), (s, c)
  const double n0 = f == 0 ? -C : f == 1 ? -S : f == 2 ? C : S;
  const double n1 = f == 0 ? S : f == 1 ? -C : f == 2 ? -S : C;
  const double q = a.out_q[i];
  a.out_arg[i] = static_cast<int64_t>(ai);
  if (q + a.margin <= 0.0) return;  // the row already meets the budget: the empty record stands
  const double rhs = ((n0 * X + n1 * Y) - q) - a.margin;
  face_quant_store_cut(a.out_cut, i, n0, n1, rhs, 0, t);
}

int launch_face_quantile(const FaceQuantArgs &a, hipStream_t s) {
  const int64_t R = static_cast<int64_t>(a.n_cells) * a.T * 4;
  const int lg = a.dtype == CCMPC_F64 ? 9 : 10;
  const int64_t items = max_items(a.n_cells, a.n_bound, int64_t(1) << lg);
  const int chunks = (a.T + kFaceQuantSteps - 1) / kFaceQuantSteps;
  const int64_t narrow_blocks = (R + kFaceQuantThreads / 64 - 1) / (kFaceQuantThreads / 64);
  const int64_t cut_blocks = (R + kFaceQuantThreads - 1) / kFaceQuantThreads;
  if (items >= (int64_t(1) << 31) || narrow_blocks >= (int64_t(1) << 31)) return CCMPC_ERR_ARG;
  int64_t init_blocks = (R * 64 + kFaceQuantThreads - 1) / kFaceQuantThreads;
  init_blocks = init_blocks < 4096 ? init_blocks : 4096;
  const dim3 b(kFaceQuantThreads);
  hipLaunchKernelGGL(face_quantile_init_kernel, dim3(static_cast<unsigned>(init_blocks)), b, 0, s,
                     a);
  const dim3 g(static_cast<unsigned>(items), static_cast<unsigned>(chunks));
  const bool f64 = a.dtype == CCMPC_F64;
  for (int pass = 0; pass < kQuantDigits; ++pass) {
    if (f64)
      hipLaunchKernelGGL((face_quantile_pass_kernel<double, false>), g, b, 0, s, a, pass);
    else
      hipLaunchKernelGGL((face_quantile_pass_kernel<float, false>), g, b, 0, s, a, pass);
    hipLaunchKernelGGL(face_quantile_narrow_kernel, dim3(static_cast<unsigned>(narrow_blocks)), b,
                       0, s, a, pass);
  }
  if (f64) {
    hipLaunchKernelGGL((face_quantile_pass_kernel<double, true>), g, b, 0, s, a, 0);
    hipLaunchKernelGGL(face_quantile_cut_kernel<double>, dim3(static_cast<unsigned>(cut_blocks)), b,
                       0, s, a);
  } else {
    hipLaunchKernelGGL((face_quantile_pass_kernel<float, true>), g, b, 0, s, a, 0);
    hipLaunchKernelGGL(face_quantile_cut_kernel<float>, dim3(static_cast<unsigned>(cut_blocks)), b,
                       0, s, a);
  }
  return CCMPC_OK;
}

}  // namespace ccmpc
