// Monte-Carlo audit of the box-face rows: count, on the particles the face records were built
// from, how many violate each face's inequality at a plan, and how far the worst one stands
// beyond it (ccmpc_face_audit; no reference counterpart -- the reference replaces the count by
// mean . xi + Gamma |root xi| + 0.5 car_r <= 0 under a Gaussian assumption).
//
// One streaming pass over planes 0 .. 2T-1 of the store, on the geometry of audit_kernel:
//  * Work item = one workgroup of 4 waves over 256 W consecutive particles of one cell, W = 2
//    (f64) or 4 (f32): every lane's load is 16 bytes of one plane (AuditVec).  Items are found
//    on the device (locate_item), the grid is sized by n_particles_bound.  Lanes past cell_cnt
//    load a clamped address and are masked out of every ballot and out of the maxima.
//  * A lane owns its W particles for all T steps.  The previous step's stored pair stays in
//    registers for the heading (past_last at t = 0), so every plane is read once: 16 T (f64) or
//    8 T (f32) bytes per particle, the audit's figure, not the (2T - 1) / T of
//    face_moments_kernel's (chunk, t) grid.  Steps are loaded four at a time, the next four in
//    flight while these are evaluated.  The "in the box at any step" and "open under the
//    selected row at any step" bits are registers: one wave mask per particle slot, kept in
//    scalar registers and updated with scalar instructions from the step's ballots.
//  * The heading is faces.hpp's face_heading, the one ccmpc_face_constraints forms: bit for bit
//    the unit vector the records' coefficients were built from.  The four face values come from
//    face_values (face_audit.hpp), the inline function face_quantile.hip evaluates too.
//  * Once per workgroup the cell's plan row (2T doubles) and face_sel row (T ints) are staged in
//    LDS.
//  * Counts are wave ballots + population counts; lanes 0..4 of a wave add the step's five
//    counts (four faces, in box) to LDS integers with one LDS atomic.  The selected row's count
//    is the selected face's: the flush reads it from the same integers.  The four maxima of a
//    step are reduced in the lane over its W particles, then over each 16-lane row of the wave
//    in one transposed DPP tree (register moves; a maximum is exact, so no order can change it),
//    then the last quad of every row raises the step's LDS keys (quant_key: unsigned key order
//    = value order).
//  * One flush per workgroup: every non-zero count with one 64-bit integer atomic add, every
//    (step, face) maximum with one 64-bit integer atomic.  No float atomics: no output bit
//    depends on arrival order.
// A first small launch of the same call writes the initial values (0, -inf, and -1 for the
// steps without a row), so the caller prepares nothing.
#include "face_audit.hpp"

#include <type_traits>

#include "faces.hpp"
#include "quantile.hpp"

namespace ccmpc {

constexpr int kFaceAuditThreads = 256;
constexpr int kFaceAuditU = 4;    // steps per load group
constexpr int kFaceAuditCnt = 5;  // counts per step: faces 0..3, in box

__device__ __forceinline__ void face_audit_add(int64_t *p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

// *p = the larger of *p and the double of `key`, in key order, on the double's own bits (the
// min_d2 idiom widened to signed values): among sign-clear patterns the larger integer is the
// larger double and every one of them is above every sign-set pattern (a signed maximum);
// among sign-set patterns the smaller unsigned integer is the larger double and every one of
// them is above every sign-clear pattern as an unsigned integer (an unsigned minimum).  Either
// way the stored pattern's key becomes max(key of *p, key): the unsigned maximum of the key.
__device__ __forceinline__ void face_audit_max(double *p, uint64_t key) {
  const uint64_t b = __builtin_bit_cast(uint64_t, quant_unkey(key));
  if (b >> 63)
    atomicMin(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(b));
  else
    atomicMax(reinterpret_cast<long long *>(p), static_cast<long long>(b));
}

__device__ __forceinline__ bool face_sel_valid(int32_t f) { return f >= 0 && f <= 3; }

// Lanes without a source (the first lanes of a row) keep their own value.
template <int CTRL>
__device__ __forceinline__ double face_audit_dpp(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t l = static_cast<uint32_t>(u), h = static_cast<uint32_t>(u >> 32);
  const uint32_t lo = __builtin_amdgcn_update_dpp(l, l, CTRL, 0xf, 0xf, false);
  const uint32_t hi = __builtin_amdgcn_update_dpp(h, h, CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, (static_cast<uint64_t>(hi) << 32) | lo);
}

// The four per-lane maxima of a step, reduced over the 16 lanes of a DPP row in one transposed
// tree (register moves only): after the two exchanges inside a quad (with lane ^ 1, then
// lane ^ 2) lane k of every quad holds the quad's maximum of face face_audit_lane_face(k), and
// two row shifts (4, 8 lanes: the lane's place in its quad is kept) leave the row's maximum of
// that face in lanes 12..15.  Seven moves of a double where four separate wave reductions take
// sixteen and as many lane reads.  All 64 lanes must be active.
__device__ __forceinline__ double face_audit_row_max4(double m0, double m1, double m2, double m3,
                                                      int lane) {
  const bool odd = lane & 1, up = lane & 2;
  double a = odd ? m2 : m0, b = odd ? m3 : m1;          // kept: faces (0, 1) or (2, 3)
  const double sa = odd ? m0 : m2, sb = odd ? m1 : m3;  // the partner keeps these
  a = fmax(a, face_audit_dpp<0xB1>(sa));                // quad_perm [1, 0, 3, 2]
  b = fmax(b, face_audit_dpp<0xB1>(sb));
  double c = up ? b : a;
  const double sc = up ? a : b;
  c = fmax(c, face_audit_dpp<0x4E>(sc));                // quad_perm [2, 3, 0, 1]
  c = fmax(c, face_audit_dpp<0x114>(c));                // row_shr:4
  c = fmax(c, face_audit_dpp<0x118>(c));                // row_shr:8
  return c;
}
// The face whose maximum face_audit_row_max4 leaves in a lane.
__device__ __forceinline__ int face_audit_lane_face(int lane) {
  return ((lane & 1) << 1) | ((lane >> 1) & 1);
}

// Initial values of every enabled output.
__global__ __launch_bounds__(kFaceAuditThreads) void face_audit_init_kernel(FaceAuditArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t C = a.n_cells, CT = C * a.T;
  if (i < 4 * CT) {
    a.face_open[i] = 0;
    if (a.worst) a.worst[i] = -__builtin_huge_val();
  }
  if (i < CT) {
    a.in_box[i] = 0;
    if (a.face_sel) a.sel_open[i] = face_sel_valid(a.face_sel[i]) ? 0 : -1;
  }
  if (i < C) {
    a.in_box_any[i] = 0;
    if (a.face_sel) a.sel_open_any[i] = 0;
  }
}

template <typename P, bool SEL, bool WORST>
__global__ __launch_bounds__(kFaceAuditThreads) void face_audit_kernel(FaceAuditArgs a) {
  using V = AuditVec<P>;
  constexpr int W = V::W;
  constexpr int LG = W == 2 ? 8 + 1 : 8 + 2;  // log2 particles per item (threads * W)
  constexpr int U = kFaceAuditU;
  constexpr int NC = kFaceAuditCnt;
  __shared__ double plan_s[2 * kAuditMaxT];
  __shared__ int sel_s[SEL ? kAuditMaxT : 1];
  __shared__ int cnt_s[NC * kAuditMaxT];
  __shared__ unsigned long long worst_s[WORST ? 4 * kAuditMaxT : 1];
  __shared__ int any_s[2];  // in box at any step, open under the selected row at any step
  static_assert(NC * kAuditMaxT <= kFaceAuditThreads, "one thread per LDS count");

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
  // per particle slot j, as wave masks (one bit per lane, wave-uniform values): the lanes whose
  // particle exists, and the two any-step bits
  bool valid[W];
  unsigned long long vmask[W], box_any[W], sel_any[W];
#pragma unroll
  for (int j = 0; j < W; ++j) {
    valid[j] = idx + j < cnt;
    vmask[j] = __ballot(valid[j]);
    box_any[j] = 0;
    sel_any[j] = 0;
  }
  double o0 = 0.0, o1 = 0.0;
  if (std::is_same_v<P, float> && a.origin) {
    o0 = a.origin[2 * cell];
    o1 = a.origin[2 * cell + 1];
  }
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
  if (tid < 2 * T)
    plan_v = a.plan[(static_cast<int64_t>(loc.ref_sel) * T + (tid >> 1)) * a.ld_plan + (tid & 1)];
  int sel_v = -1;
  if (SEL && tid < T) sel_v = a.face_sel[cell * T + tid];
  const double past_x = a.past_last[2 * cell], past_y = a.past_last[2 * cell + 1];
  const double half_r = 0.5 * a.car_r;
  const double hlon = 0.5 * a.extent[0] + half_r, hlat = 0.5 * a.extent[1] + half_r;
  V cur[U][2], nxt[U][2], prev[2];
  load_steps(cur, 0);
  prev[0] = cur[0][0];  // unused at t = 0
  prev[1] = cur[0][1];

  // ---- stage the plan row, the face_sel row and the empty counts ------------------------------
  if (tid < 2 * T) plan_s[tid] = plan_v;
  if (SEL && tid < T) sel_s[tid] = sel_v;
  if (tid < NC * T) cnt_s[tid] = 0;
  if (WORST && tid < 4 * T) worst_s[tid] = kKeyNegInf;
  if (tid < 2) any_s[tid] = 0;
  __syncthreads();

  auto step = [&](int t, const V (&b)[2], const V (&pb)[2]) {
    const double X = plan_s[2 * t], Y = plan_s[2 * t + 1];
    // the selected face as four wave-uniform masks: all ones for that face, else zero
    const int fs = SEL ? __builtin_amdgcn_readfirstlane(sel_s[t]) : -1;
    const unsigned long long k0 = fs == 0 ? ~0ull : 0ull, k1 = fs == 1 ? ~0ull : 0ull,
                             k2 = fs == 2 ? ~0ull : 0ull, k3 = fs == 3 ? ~0ull : 0ull;
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0, nb = 0;
    double m0 = -__builtin_huge_val(), m1 = m0, m2 = m0, m3 = m0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double x = face_world(b[0][j], o0), y = face_world(b[1][j], o1);
      const double xp = t == 0 ? past_x : face_world(pb[0][j], o0);
      const double yp = t == 0 ? past_y : face_world(pb[1][j], o1);
      double S, C, v0, v1, v2, v3;
      face_values(x, y, xp, yp, X, Y, hlat, hlon, S, C, v0, v1, v2, v3);
      const unsigned long long b0 = __ballot(v0 > 0.0) & vmask[j], b1 = __ballot(v1 > 0.0) & vmask[j],
                               b2 = __ballot(v2 > 0.0) & vmask[j], b3 = __ballot(v3 > 0.0) & vmask[j];
      const unsigned long long in = b0 & b1 & b2 & b3;
      n0 += __popcll(b0);
      n1 += __popcll(b1);
      n2 += __popcll(b2);
      n3 += __popcll(b3);
      nb += __popcll(in);
      box_any[j] |= in;
      if (SEL) sel_any[j] |= (b0 & k0) | (b1 & k1) | (b2 & k2) | (b3 & k3);
      const bool ok = valid[j];
      if (WORST) {
        const double ninf = -__builtin_huge_val();
        m0 = fmax(m0, ok ? v0 : ninf);
        m1 = fmax(m1, ok ? v1 : ninf);
        m2 = fmax(m2, ok ? v2 : ninf);
        m3 = fmax(m3, ok ? v3 : ninf);
      }
    }
    const int n = lane == 0 ? n0 : lane == 1 ? n1 : lane == 2 ? n2 : lane == 3 ? n3 : nb;
    if (lane < NC && n) atomicAdd(&cnt_s[NC * t + lane], n);
    if (WORST) {
      const double m = face_audit_row_max4(m0, m1, m2, m3, lane);
      if ((lane & 12) == 12)  // the last quad of each of the wave's four rows
        atomicMax(&worst_s[4 * t + face_audit_lane_face(lane)],
                  static_cast<unsigned long long>(quant_key(m)));
    }
  };

  for (int t0 = 0; t0 < T; t0 += U) {
    if (t0 + U < T) load_steps(nxt, t0 + U);  // uniform
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (t0 + u < T) step(t0 + u, cur[u], u == 0 ? prev : cur[u ? u - 1 : 0]);
    prev[0] = cur[U - 1][0];
    prev[1] = cur[U - 1][1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      cur[u][0] = nxt[u][0];
      cur[u][1] = nxt[u][1];
    }
  }
  {
    int nb = 0, ns = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) {
      nb += __popcll(box_any[j]);
      if (SEL) ns += __popcll(sel_any[j]);
    }
    const int n = lane == 0 ? nb : ns;
    if (lane < 2 && n) atomicAdd(&any_s[lane], n);
  }
  __syncthreads();

  // ---- one flush per output -----------------------------------------------------------------
  if (tid < NC * T) {
    const int t = tid / NC, k = tid - NC * t, n = cnt_s[tid];
    if (n) {
      if (k < 4) {
        face_audit_add(a.face_open + (cell * T + t) * 4 + k, n);
        if (SEL && sel_s[t] == k) face_audit_add(a.sel_open + cell * T + t, n);
      } else {
        face_audit_add(a.in_box + cell * T + t, n);
      }
    }
  }
  if (WORST && tid < 4 * T) face_audit_max(a.worst + cell * T * 4 + tid, worst_s[tid]);
  if (tid == 0 && any_s[0]) face_audit_add(a.in_box_any + cell, any_s[0]);
  if (SEL && tid == 1 && any_s[1]) face_audit_add(a.sel_open_any + cell, any_s[1]);
}

template <typename P>
static void launch_typed(const FaceAuditArgs &a, unsigned grid, hipStream_t s) {
  const dim3 g(grid), b(kFaceAuditThreads);
  const bool sel = a.face_sel != nullptr, worst = a.worst != nullptr;
  if (sel && worst)
    hipLaunchKernelGGL((face_audit_kernel<P, true, true>), g, b, 0, s, a);
  else if (sel)
    hipLaunchKernelGGL((face_audit_kernel<P, true, false>), g, b, 0, s, a);
  else if (worst)
    hipLaunchKernelGGL((face_audit_kernel<P, false, true>), g, b, 0, s, a);
  else
    hipLaunchKernelGGL((face_audit_kernel<P, false, false>), g, b, 0, s, a);
}

int launch_face_audit(const FaceAuditArgs &a, hipStream_t s) {
  const int64_t C = a.n_cells;
  const int64_t n_init = 4 * C * a.T;
  const int64_t init_blocks = (n_init + kFaceAuditThreads - 1) / kFaceAuditThreads;
  const int lg = a.dtype == CCMPC_F64 ? 9 : 10;
  const int64_t items = max_items(C, a.n_bound, int64_t(1) << lg);
  if (init_blocks >= (int64_t(1) << 31) || items >= (int64_t(1) << 31)) return CCMPC_ERR_ARG;
  hipLaunchKernelGGL(face_audit_init_kernel, dim3(static_cast<unsigned>(init_blocks)),
                     dim3(kFaceAuditThreads), 0, s, a);
  if (a.dtype == CCMPC_F64)
    launch_typed<double>(a, static_cast<unsigned>(items), s);
  else
    launch_typed<float>(a, static_cast<unsigned>(items), s);
  return CCMPC_OK;
}

}  // namespace ccmpc
