// Error plumbing and version entry points of the C ABI (include/ccmpc.h).
#include <string>

#include "audit.hpp"
#include "ccmpc_common.hpp"
#include "face_audit.hpp"
#include "face_quantile.hpp"
#include "faces.hpp"
#include "quantile.hpp"
#include "socp.hpp"

namespace ccmpc {
static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }
}  // namespace ccmpc

extern "C" int ccmpc_abi_version(void) { return CCMPC_ABI_VERSION; }

extern "C" const char *ccmpc_last_error(void) { return ccmpc::g_last_error.c_str(); }

extern "C" const char *ccmpc_status_string(int status) {
  switch (status) {
    case CCMPC_OK: return "ok";
    case CCMPC_ERR_ARG: return "invalid argument";
    case CCMPC_ERR_LAUNCH: return "kernel launch failed";
    case CCMPC_ERR_WORKSPACE: return "workspace too small";
    case CCMPC_ERR_UNSUPPORTED: return "unsupported configuration";
    case CCMPC_REC_SINGULAR: return "singular matrix (LinAlgError in the reference)";
    case CCMPC_REC_NO_TANGENT: return "no real tangent (n^T Sigma n <= 0)";
    case CCMPC_REC_NONFINITE: return "non-finite slope or moment";
    case CCMPC_REC_NOT_PD: return "conditional covariance not positive definite";
    case CCMPC_REC_NOT_PSD: return "covariance not positive semi-definite (complex sqrtm)";
    default: return "unknown status";
  }
}

// Stream-ordered byte copy between host and device buffers (any direction; the runtime infers
// it from the pointers).  Lets a captured planning-step graph carry its packed H2D input copy
// and D2H output copy as graph nodes (ccmpc/step.py).
extern "C" int ccmpc_copy_async(void *dst, const void *src, size_t bytes, ccmpc_stream_t stream) {
  CCMPC_REQUIRE(dst && src, "null pointer");
  if (bytes == 0) return CCMPC_OK;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, ccmpc::as_stream(stream));
  if (e != hipSuccess) {
    ccmpc::set_error(std::string("ccmpc_copy_async: ") + hipGetErrorString(e));
    return CCMPC_ERR_LAUNCH;
  }
  return CCMPC_OK;
}

// The same copy as a kernel of 16-byte lanes that reads / writes the pinned host side directly
// (host allocations are device-accessible by their host address on this platform): a graph
// kernel node instead of a memcpy node (ccmpc/step.py measures both).  bytes % 16 == 0 and
// 16-byte aligned pointers.
__global__ __launch_bounds__(256) void copy16_kernel(uint4 *__restrict__ dst,
                                                     const uint4 *__restrict__ src, size_t n) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<size_t>(gridDim.x) * blockDim.x)
    dst[i] = src[i];
}

extern "C" int ccmpc_copy_kernel_async(void *dst, const void *src, size_t bytes,
                                       ccmpc_stream_t stream) {
  CCMPC_REQUIRE(dst && src, "null pointer");
  CCMPC_REQUIRE(bytes % 16 == 0 && ccmpc::aligned(dst, 16) && ccmpc::aligned(src, 16),
                "bytes and pointers must be 16-byte aligned");
  if (bytes == 0) return CCMPC_OK;
  const size_t n = bytes / 16;
  const unsigned blocks = static_cast<unsigned>(n < 64 * 256 ? (n + 255) / 256 : 64);
  hipLaunchKernelGGL(copy16_kernel, dim3(blocks), dim3(256), 0, ccmpc::as_stream(stream),
                     static_cast<uint4 *>(dst), static_cast<const uint4 *>(src), n);
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// One 8-byte value from device memory to a pinned host word, made visible to the host after
// everything this stream wrote before it: a system-scope release (which writes back the L2, so
// an earlier kernel's writes to host memory land first), then a system-scope store.  The host
// polls the word instead of synchronising the stream (ccmpc/step.py: a step's records are on
// the host as soon as their copy-out is, while the L4 branch of the same graph still runs).
__global__ __launch_bounds__(64) void signal_host_kernel(int64_t *dst, const int64_t *src) {
  if (threadIdx.x != 0) return;
  const int64_t v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __atomic_thread_fence(__ATOMIC_RELEASE);  // system scope (the default)
  __hip_atomic_store(dst, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Copy-out and signal in one single-workgroup kernel: every wave copies its share, waits for
// its stores (vmcnt(0)), the workgroup meets at a barrier, then one thread makes everything the
// CU wrote visible at system scope (the release writes back this XCD's L2, where all of this
// kernel's stores went) and stores the value.  One launch less on a planning step's critical
// path than ccmpc_copy_kernel_async followed by ccmpc_signal_host.
__global__ __launch_bounds__(1024) void copy16_signal_kernel(uint4 *__restrict__ dst,
                                                             const uint4 *__restrict__ src,
                                                             size_t n, int64_t *host_word,
                                                             const int64_t *value) {
  constexpr int U = 4;  // 4 loads in flight per thread before the stores (64 KB in one pass)
  for (size_t base = 0; base < n; base += U * blockDim.x) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + u * blockDim.x + threadIdx.x;
      if (i < n) v[u] = src[i];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = base + u * blockDim.x + threadIdx.x;
      if (i < n) dst[i] = v[u];
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's stores have landed in L2
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t v = __hip_atomic_load(value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_thread_fence(__ATOMIC_RELEASE);  // system scope
    __hip_atomic_store(host_word, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

extern "C" int ccmpc_copy_signal_async(void *dst, const void *src, size_t bytes,
                                       int64_t *host_word, const int64_t *value,
                                       ccmpc_stream_t stream) {
  CCMPC_REQUIRE(dst && src && host_word && value, "null pointer");
  CCMPC_REQUIRE(bytes % 16 == 0 && ccmpc::aligned(dst, 16) && ccmpc::aligned(src, 16) &&
                    ccmpc::aligned(host_word, 8) && ccmpc::aligned(value, 8),
                "bytes and pointers must be 16-byte (words 8-byte) aligned");
  hipLaunchKernelGGL(copy16_signal_kernel, dim3(1), dim3(1024), 0, ccmpc::as_stream(stream),
                     static_cast<uint4 *>(dst), static_cast<const uint4 *>(src), bytes / 16,
                     host_word, value);
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

extern "C" int ccmpc_signal_host(int64_t *host_word, const int64_t *value, ccmpc_stream_t stream) {
  CCMPC_REQUIRE(host_word && value, "null pointer");
  CCMPC_REQUIRE(ccmpc::aligned(host_word, 8) && ccmpc::aligned(value, 8),
                "pointers must be 8-byte aligned");
  hipLaunchKernelGGL(signal_host_kernel, dim3(1), dim3(64), 0, ccmpc::as_stream(stream),
                     host_word, value);
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// Stream capture into an executable graph, replay and release (ccmpc/step.py's planning-step
// graphs capture only this library's calls and event record / wait pairs, so they need no
// framework graph object).  Relaxed capture mode: calls of other threads are not affected.
extern "C" int ccmpc_graph_capture_begin(ccmpc_stream_t stream) {
  const hipError_t e = hipStreamBeginCapture(ccmpc::as_stream(stream), hipStreamCaptureModeRelaxed);
  if (e != hipSuccess) {
    ccmpc::set_error(std::string("ccmpc_graph_capture_begin: ") + hipGetErrorString(e));
    return CCMPC_ERR_LAUNCH;
  }
  return CCMPC_OK;
}

extern "C" int ccmpc_graph_capture_end(ccmpc_stream_t stream, void **out_exec) {
  CCMPC_REQUIRE(out_exec, "null pointer");
  *out_exec = nullptr;
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(ccmpc::as_stream(stream), &g);
  if (e == hipSuccess) {
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e == hipSuccess) *out_exec = x;
  }
  if (e != hipSuccess) {
    ccmpc::set_error(std::string("ccmpc_graph_capture_end: ") + hipGetErrorString(e));
    return CCMPC_ERR_LAUNCH;
  }
  return CCMPC_OK;
}

extern "C" int ccmpc_graph_launch(void *exec, ccmpc_stream_t stream) {
  CCMPC_REQUIRE(exec, "null graph");
  const hipError_t e = hipGraphLaunch(static_cast<hipGraphExec_t>(exec), ccmpc::as_stream(stream));
  if (e != hipSuccess) {
    ccmpc::set_error(std::string("ccmpc_graph_launch: ") + hipGetErrorString(e));
    return CCMPC_ERR_LAUNCH;
  }
  return CCMPC_OK;
}

extern "C" int ccmpc_graph_destroy(void *exec) {
  if (!exec) return CCMPC_OK;
  const hipError_t e = hipGraphExecDestroy(static_cast<hipGraphExec_t>(exec));
  if (e != hipSuccess) {
    ccmpc::set_error(std::string("ccmpc_graph_destroy: ") + hipGetErrorString(e));
    return CCMPC_ERR_LAUNCH;
  }
  return CCMPC_OK;
}

// ---- compact records for the multi-GPU exchange ---------------------------------------------
// One thread per record: the five fields the QP reads (n, rhs, side, status, t_tau) out of the
// 128-byte record into a 32-byte ccmpc_gather_rec, as two 16-byte stores.
__global__ __launch_bounds__(256) void compact_records_kernel(const unsigned char *__restrict__ rec,
                                                              int affine, int64_t n,
                                                              double4 *__restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned char *r = rec + i * 128;
  const double2 nn = *reinterpret_cast<const double2 *>(r);
  const double rhs = *reinterpret_cast<const double *>(r + (affine ? 32 : 16));
  const int4 tail = *reinterpret_cast<const int4 *>(r + 112);  // which, side, status, t_tau
  const uint32_t ss = (static_cast<uint32_t>(static_cast<uint16_t>(tail.y))) |
                      (static_cast<uint32_t>(static_cast<uint16_t>(tail.z)) << 16);
  double4 v;
  v.x = nn.x;
  v.y = nn.y;
  v.z = rhs;
  v.w = __builtin_bit_cast(double, (static_cast<uint64_t>(static_cast<uint32_t>(tail.w)) << 32) |
                                       ss);
  out[i] = v;
}

extern "C" int ccmpc_compact_records(const void *rec, int rec_kind, int64_t n_rec,
                                     ccmpc_gather_rec *out, ccmpc_stream_t stream) {
  CCMPC_REQUIRE(rec_kind == CCMPC_REC_KIND_HALFSPACE || rec_kind == CCMPC_REC_KIND_AFFINE,
                "rec_kind must be CCMPC_REC_KIND_HALFSPACE or _AFFINE");
  CCMPC_REQUIRE(n_rec >= 0, "bad n_rec");
  if (n_rec == 0) return CCMPC_OK;
  CCMPC_REQUIRE(rec && out, "null pointer");
  CCMPC_REQUIRE(ccmpc::aligned(rec, 16) && ccmpc::aligned(out, 32), "misaligned records");
  const int64_t blocks = (n_rec + 255) / 256;
  CCMPC_REQUIRE(blocks < (int64_t(1) << 31), "too many records");
  hipLaunchKernelGGL(compact_records_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                     ccmpc::as_stream(stream), static_cast<const unsigned char *>(rec),
                     rec_kind == CCMPC_REC_KIND_AFFINE ? 1 : 0, n_rec,
                     reinterpret_cast<double4 *>(out));
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// ---- Monte-Carlo risk audit (audit.hip) -----------------------------------------------------
extern "C" int ccmpc_risk_audit(const void *positions, int dtype, int64_t ld, int64_t T,
                                const double *origin, const int64_t *cell_off,
                                const int64_t *cell_cnt, int64_t n_cells,
                                int64_t n_particles_bound, const double *plan,
                                const int32_t *cell_plan, const void *rec, int rec_kind, double R,
                                int64_t *out_hit, int64_t *out_hit_any, double *out_min_d2,
                                int64_t *out_rec_open, int64_t *out_open,
                                ccmpc_stream_t stream) {
  CCMPC_REQUIRE(T >= 1 && T <= ccmpc::kAuditMaxT, "T must be in [1, 40]");
  CCMPC_REQUIRE(std::isfinite(R) && R > 0.0, "R must be finite and positive");
  CCMPC_REQUIRE(plan || rec, "nothing to audit: plan and rec are both null");
  int P = 0;
  if (rec) {
    P = ccmpc::audit_rows(rec_kind, T);
    CCMPC_REQUIRE(P >= 0, "unknown rec_kind");
    // P == 0 (T = 1 of the half-space kinds): out_rec_open has no rows and may be null
    CCMPC_REQUIRE((out_rec_open || P == 0) && out_open,
                  "record half needs out_rec_open and out_open");
    CCMPC_REQUIRE(ccmpc::aligned(rec, 16), "records must be 16-byte aligned");
  }
  if (plan) {
    CCMPC_REQUIRE(out_hit && out_hit_any && out_min_d2,
                  "plan half needs out_hit, out_hit_any and out_min_d2");
    CCMPC_REQUIRE(ccmpc::aligned(plan, 8), "plan must be 8-byte aligned");
  }
  CCMPC_REQUIRE(n_cells >= 0 && n_cells < (1 << 30), "bad n_cells");
  CCMPC_REQUIRE(n_particles_bound >= 0, "bad n_particles_bound");
  CCMPC_REQUIRE(dtype == CCMPC_F64 || dtype == CCMPC_F32, "bad dtype");
  CCMPC_REQUIRE(ld % 4 == 0 && ld > 0, "ld must be a positive multiple of 4");
  if (n_cells == 0) return CCMPC_OK;
  CCMPC_REQUIRE(positions && cell_off && cell_cnt, "null pointer");
  CCMPC_REQUIRE(ccmpc::aligned(positions, 16), "positions must be 16-byte aligned");
  CCMPC_REQUIRE(ccmpc::aligned(out_hit, 8) && ccmpc::aligned(out_hit_any, 8) &&
                    ccmpc::aligned(out_min_d2, 8) && ccmpc::aligned(out_rec_open, 8) &&
                    ccmpc::aligned(out_open, 8),
                "outputs must be 8-byte aligned");
  const ccmpc::AuditArgs a{positions, dtype, ld, static_cast<int>(T), origin, cell_off, cell_cnt,
                           static_cast<int>(n_cells), n_particles_bound, plan, cell_plan,
                           static_cast<const unsigned char *>(rec), rec_kind, P, R * R,
                           out_hit, out_hit_any, out_min_d2, out_rec_open, out_open};
  const int rc = ccmpc::launch_risk_audit(a, ccmpc::as_stream(stream));
  CCMPC_REQUIRE(rc == CCMPC_OK, "too many work items for one grid");
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// ---- Box-face chance constraints (faces.hip) ------------------------------------------------
extern "C" size_t ccmpc_face_workspace_bytes(int64_t T, int64_t n_cells,
                                             int64_t n_particles_bound) {
  if (T < 1 || T > ccmpc::kFaceMaxT || n_cells < 0 || n_cells >= (1 << 30) ||
      n_particles_bound < 0)
    return 0;
  return ccmpc::face_workspace_bytes(T, n_cells, n_particles_bound);
}

extern "C" int ccmpc_face_constraints(const void *positions, int dtype, int64_t ld, int64_t T,
                                      const double *origin, const int64_t *cell_off,
                                      const int64_t *cell_cnt, int64_t n_cells,
                                      int64_t n_particles_bound, const double *past_last,
                                      const double *extent, const double *cell_gamma,
                                      const double *ref_traj, const int32_t *cell_ref, int kind,
                                      double car_r, void *workspace, size_t workspace_bytes,
                                      ccmpc_face_rec *out_rec, ccmpc_stream_t stream) {
  static_assert(sizeof(ccmpc_face_rec) == 128, "ccmpc_face_rec is 128 bytes");
  CCMPC_REQUIRE(T >= 1 && T <= ccmpc::kFaceMaxT, "T must be in [1, 40]");
  CCMPC_REQUIRE(kind == CCMPC_FACE_NOMINAL || kind == CCMPC_FACE_ROBUST, "unknown kind");
  CCMPC_REQUIRE(std::isfinite(car_r), "car_r must be finite");
  CCMPC_REQUIRE(n_cells >= 0 && n_cells < (1 << 30), "bad n_cells");
  CCMPC_REQUIRE(n_particles_bound >= 0, "bad n_particles_bound");
  CCMPC_REQUIRE(dtype == CCMPC_F64 || dtype == CCMPC_F32, "bad dtype");
  CCMPC_REQUIRE(ld % 4 == 0 && ld > 0, "ld must be a positive multiple of 4");
  if (n_cells == 0) return CCMPC_OK;
  CCMPC_REQUIRE(positions && cell_off && cell_cnt && past_last && extent && cell_gamma && out_rec,
                "null pointer");
  CCMPC_REQUIRE(ccmpc::aligned(positions, 16), "positions must be 16-byte aligned");
  CCMPC_REQUIRE(ccmpc::aligned(out_rec, 8), "out_rec must be 8-byte aligned");
  CCMPC_REQUIRE(workspace && ccmpc::aligned(workspace, 256), "workspace must be 256-byte aligned");
  if (workspace_bytes < ccmpc::face_workspace_bytes(T, n_cells, n_particles_bound)) {
    ccmpc::set_error("ccmpc_face_constraints: workspace too small");
    return CCMPC_ERR_WORKSPACE;
  }
  ccmpc::FaceArgs a{};
  a.pos = positions;
  a.dtype = dtype;
  a.ld = ld;
  a.T = static_cast<int>(T);
  a.origin = origin;
  a.off = cell_off;
  a.cnt = cell_cnt;
  a.n_cells = static_cast<int>(n_cells);
  a.past_last = past_last;
  a.extent = extent;
  a.gamma = cell_gamma;
  a.ref = ref_traj;
  a.cell_ref = cell_ref;
  a.kind = kind;
  a.car_r = car_r;
  a.rec = out_rec;
  const int rc = ccmpc::launch_face_constraints(a, n_particles_bound, workspace,
                                                ccmpc::as_stream(stream));
  CCMPC_REQUIRE(rc == CCMPC_OK, "too many work items for one grid");
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// ---- Monte-Carlo audit of the box-face rows (face_audit.hip) ---------------------------------
extern "C" int ccmpc_face_audit(const void *positions, int dtype, int64_t ld, int64_t T,
                                const double *origin, const int64_t *cell_off,
                                const int64_t *cell_cnt, int64_t n_cells,
                                int64_t n_particles_bound, const double *past_last,
                                const double *extent, double car_r, const double *plan,
                                int64_t ld_plan, const int32_t *cell_plan,
                                const int32_t *face_sel, int64_t *out_face_open,
                                int64_t *out_in_box, int64_t *out_in_box_any,
                                int64_t *out_sel_open, int64_t *out_sel_open_any,
                                double *out_worst, ccmpc_stream_t stream) {
  CCMPC_REQUIRE(T >= 1 && T <= ccmpc::kAuditMaxT, "T must be in [1, 40]");
  CCMPC_REQUIRE(std::isfinite(car_r), "car_r must be finite");
  CCMPC_REQUIRE(ld_plan >= 2, "ld_plan must be >= 2");
  CCMPC_REQUIRE(n_cells >= 0 && n_cells < (1 << 30), "bad n_cells");
  CCMPC_REQUIRE(n_particles_bound >= 0, "bad n_particles_bound");
  CCMPC_REQUIRE(dtype == CCMPC_F64 || dtype == CCMPC_F32, "bad dtype");
  CCMPC_REQUIRE(ld % 4 == 0 && ld > 0, "ld must be a positive multiple of 4");
  CCMPC_REQUIRE(positions && cell_off && cell_cnt && past_last && extent && plan, "null pointer");
  CCMPC_REQUIRE(out_face_open && out_in_box && out_in_box_any,
                "out_face_open, out_in_box and out_in_box_any are required");
  CCMPC_REQUIRE(!face_sel || (out_sel_open && out_sel_open_any),
                "face_sel needs out_sel_open and out_sel_open_any");
  CCMPC_REQUIRE(ccmpc::aligned(positions, 16), "positions must be 16-byte aligned");
  CCMPC_REQUIRE(ccmpc::aligned(plan, 8) && ccmpc::aligned(past_last, 8) &&
                    ccmpc::aligned(extent, 8),
                "plan, past_last and extent must be 8-byte aligned");
  CCMPC_REQUIRE(ccmpc::aligned(out_face_open, 8) && ccmpc::aligned(out_in_box, 8) &&
                    ccmpc::aligned(out_in_box_any, 8) && ccmpc::aligned(out_sel_open, 8) &&
                    ccmpc::aligned(out_sel_open_any, 8) && ccmpc::aligned(out_worst, 8),
                "outputs must be 8-byte aligned");
  if (n_cells == 0) return CCMPC_OK;
  const ccmpc::FaceAuditArgs a{positions, dtype, ld, static_cast<int>(T), origin, cell_off,
                               cell_cnt, static_cast<int>(n_cells), n_particles_bound, past_last,
                               extent, car_r, plan, ld_plan, cell_plan, face_sel, out_face_open,
                               out_in_box, out_in_box_any, face_sel ? out_sel_open : nullptr,
                               face_sel ? out_sel_open_any : nullptr, out_worst};
  const int rc = ccmpc::launch_face_audit(a, ccmpc::as_stream(stream));
  CCMPC_REQUIRE(rc == CCMPC_OK, "too many work items for one grid");
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// ---- Monte-Carlo calibration of the box-face rows (face_quantile.hip) ------------------------
extern "C" size_t ccmpc_face_quantile_workspace_bytes(int64_t T, int64_t n_cells) {
  if (T < 1 || T > ccmpc::kAuditMaxT || n_cells < 0 || n_cells >= (1 << 30)) return 0;
  return ccmpc::face_quantile_workspace_bytes(T, n_cells);
}

extern "C" int ccmpc_face_quantile(const void *positions, int dtype, int64_t ld, int64_t T,
                                   const double *origin, const int64_t *cell_off,
                                   const int64_t *cell_cnt, int64_t n_cells,
                                   int64_t n_particles_bound, const double *past_last,
                                   const double *extent, double car_r, const double *plan,
                                   int64_t ld_plan, const int32_t *cell_plan,
                                   const int64_t *cell_allow, double margin, void *workspace,
                                   size_t workspace_bytes, double *out_q, int64_t *out_arg,
                                   ccmpc_gather_rec *out_cut, int32_t *out_status,
                                   ccmpc_stream_t stream) {
  static_assert(sizeof(ccmpc_gather_rec) == 32, "ccmpc_gather_rec is 32 bytes");
  CCMPC_REQUIRE(T >= 1 && T <= ccmpc::kAuditMaxT, "T must be in [1, 40]");
  CCMPC_REQUIRE(std::isfinite(car_r), "car_r must be finite");
  CCMPC_REQUIRE(std::isfinite(margin) && margin >= 0.0, "margin must be finite and >= 0");
  CCMPC_REQUIRE(ld_plan >= 2, "ld_plan must be >= 2");
  CCMPC_REQUIRE(n_cells >= 0 && n_cells < (1 << 30), "bad n_cells");
  CCMPC_REQUIRE(n_particles_bound >= 0 && n_particles_bound < (int64_t(1) << 32),
                "n_particles_bound must be in [0, 2^32)");
  CCMPC_REQUIRE(dtype == CCMPC_F64 || dtype == CCMPC_F32, "bad dtype");
  CCMPC_REQUIRE(ld % 4 == 0 && ld > 0, "ld must be a positive multiple of 4");
  CCMPC_REQUIRE(positions && cell_off && cell_cnt && past_last && extent && plan, "null pointer");
  CCMPC_REQUIRE(out_q && out_arg && out_cut && out_status, "null output");
  CCMPC_REQUIRE(ccmpc::aligned(positions, 16), "positions must be 16-byte aligned");
  CCMPC_REQUIRE(ccmpc::aligned(plan, 8) && ccmpc::aligned(past_last, 8) &&
                    ccmpc::aligned(extent, 8) && ccmpc::aligned(cell_allow, 8),
                "plan, past_last, extent and cell_allow must be 8-byte aligned");
  CCMPC_REQUIRE(ccmpc::aligned(out_q, 8) && ccmpc::aligned(out_arg, 8) &&
                    ccmpc::aligned(out_cut, 16) && ccmpc::aligned(out_status, 4),
                "outputs must be 8-byte (out_cut 16-byte, out_status 4-byte) aligned");
  if (workspace_bytes < ccmpc::face_quantile_workspace_bytes(T, n_cells)) {
    ccmpc::set_error("ccmpc_face_quantile: workspace too small");
    return CCMPC_ERR_ARG;
  }
  if (n_cells == 0) return CCMPC_OK;
  CCMPC_REQUIRE(workspace && ccmpc::aligned(workspace, 16),
                "workspace must be non-null and 16-byte aligned");
  const size_t R = static_cast<size_t>(n_cells) * static_cast<size_t>(T) * 4;
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  ccmpc::FaceQuantArgs a{};
  a.pos = positions;
  a.dtype = dtype;
  a.ld = ld;
  a.T = static_cast<int>(T);
  a.origin = origin;
  a.off = cell_off;
  a.cnt = cell_cnt;
  a.n_cells = static_cast<int>(n_cells);
  a.n_bound = n_particles_bound;
  a.past_last = past_last;
  a.extent = extent;
  a.car_r = car_r;
  a.plan = plan;
  a.ld_plan = ld_plan;
  a.cell_plan = cell_plan;
  a.allow = cell_allow;
  a.margin = margin;
  a.bins = reinterpret_cast<uint32_t *>(ws);
  a.prefix = reinterpret_cast<uint64_t *>(ws + R * 1024);
  a.rank = reinterpret_cast<int64_t *>(ws + R * (1024 + 8));
  a.arg = reinterpret_cast<uint32_t *>(ws + R * (1024 + 16));
  a.state = reinterpret_cast<int32_t *>(ws + R * (1024 + 20));
  a.out_q = out_q;
  a.out_arg = out_arg;
  a.out_cut = reinterpret_cast<double2 *>(out_cut);
  a.out_status = out_status;
  const int rc = ccmpc::launch_face_quantile(a, ccmpc::as_stream(stream));
  CCMPC_REQUIRE(rc == CCMPC_OK, "too many work items for one grid");
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// ---- Outer-approximation cuts of the face rows (socp.hip) -----------------------------------
extern "C" int ccmpc_face_cuts(const ccmpc_face_rec *rec, int64_t T, int64_t n_scenes,
                               const int64_t *scene_cell, const int32_t *face_sel,
                               const double *cell_gamma, double car_r, const double *plan,
                               int64_t ld_plan, int32_t round, int32_t max_rounds, double tol_g,
                               int32_t only_violated, ccmpc_gather_rec *pool,
                               const int64_t *pool_cell, double *out_g, double *out_viol,
                               int32_t *out_state, ccmpc_stream_t stream) {
  static_assert(sizeof(ccmpc_gather_rec) == 32, "ccmpc_gather_rec is 32 bytes");
  CCMPC_REQUIRE(T >= 1 && T <= ccmpc::kCutMaxT, "T must be in [1, 40]");
  CCMPC_REQUIRE(std::isfinite(tol_g), "tol_g must be finite");
  CCMPC_REQUIRE(std::isfinite(car_r), "car_r must be finite");
  CCMPC_REQUIRE(max_rounds >= 0 && max_rounds < (1 << 15), "max_rounds must be in [0, 2^15)");
  CCMPC_REQUIRE(round >= 0 && round <= max_rounds, "round must be in [0, max_rounds]");
  CCMPC_REQUIRE(ld_plan >= 2, "ld_plan must be >= 2");
  CCMPC_REQUIRE(n_scenes >= 0 && n_scenes < (int64_t(1) << 31), "bad n_scenes");
  CCMPC_REQUIRE(pool && out_g && out_viol && out_state, "null output");
  CCMPC_REQUIRE(rec && scene_cell && cell_gamma && plan && pool_cell, "null pointer");
  CCMPC_REQUIRE(ccmpc::aligned(rec, 8) && ccmpc::aligned(pool, 16), "misaligned records");
  if (n_scenes == 0) return CCMPC_OK;
  const ccmpc::FaceCutArgs a{rec, static_cast<int>(T), scene_cell, face_sel, cell_gamma, car_r,
                             plan, ld_plan, round, max_rounds, tol_g, only_violated,
                             reinterpret_cast<double4 *>(pool), pool_cell, out_g, out_viol,
                             out_state};
  ccmpc::launch_face_cuts(a, n_scenes, ccmpc::as_stream(stream));
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}

// ---- Monte-Carlo calibration of the offsets (quantile.hip) ----------------------------------
extern "C" size_t ccmpc_risk_quantile_workspace_bytes(int64_t T, int rec_kind, int64_t n_cells) {
  if (T < 1 || T > ccmpc::kAuditMaxT || n_cells < 0 || n_cells >= (1 << 30)) return 0;
  const int P = ccmpc::audit_rows(rec_kind, T);
  if (P < 0) return 0;
  return ccmpc::quantile_workspace_bytes(n_cells, P);
}

extern "C" int ccmpc_risk_quantile(const void *positions, int dtype, int64_t ld, int64_t T,
                                   const double *origin, const int64_t *cell_off,
                                   const int64_t *cell_cnt, int64_t n_cells,
                                   int64_t n_particles_bound, const void *rec, int rec_kind,
                                   double R, const int64_t *cell_allow, void *workspace,
                                   size_t workspace_bytes, double *out_q, double *out_rhs,
                                   int32_t *out_status, ccmpc_stream_t stream) {
  CCMPC_REQUIRE(T >= 1 && T <= ccmpc::kAuditMaxT, "T must be in [1, 40]");
  CCMPC_REQUIRE(std::isfinite(R) && R > 0.0, "R must be finite and positive");
  const int P = ccmpc::audit_rows(rec_kind, T);
  CCMPC_REQUIRE(P >= 0, "unknown rec_kind");
  CCMPC_REQUIRE(n_cells >= 0 && n_cells < (1 << 30), "bad n_cells");
  CCMPC_REQUIRE(n_particles_bound >= 0 && n_particles_bound < (int64_t(1) << 32),
                "n_particles_bound must be in [0, 2^32)");
  CCMPC_REQUIRE(dtype == CCMPC_F64 || dtype == CCMPC_F32, "bad dtype");
  CCMPC_REQUIRE(ld % 4 == 0 && ld > 0, "ld must be a positive multiple of 4");
  // P == 0 (T = 1 of the half-space kinds): no rows, nothing is written
  CCMPC_REQUIRE(P == 0 || (out_q && out_rhs && out_status), "null output");
  if (workspace_bytes < ccmpc::quantile_workspace_bytes(n_cells, P)) {
    ccmpc::set_error("ccmpc_risk_quantile: workspace too small");
    return CCMPC_ERR_ARG;
  }
  if (n_cells == 0 || P == 0) return CCMPC_OK;
  CCMPC_REQUIRE(positions && cell_off && cell_cnt && rec && workspace, "null pointer");
  CCMPC_REQUIRE(ccmpc::aligned(positions, 16) && ccmpc::aligned(rec, 16) &&
                    ccmpc::aligned(workspace, 16),
                "positions, records and workspace must be 16-byte aligned");
  CCMPC_REQUIRE(ccmpc::aligned(out_q, 8) && ccmpc::aligned(out_rhs, 8) &&
                    ccmpc::aligned(out_status, 4) && ccmpc::aligned(cell_allow, 8),
                "outputs must be 8-byte (status 4-byte) aligned");
  const size_t CP = static_cast<size_t>(n_cells) * static_cast<size_t>(P);
  unsigned char *ws = static_cast<unsigned char *>(workspace);
  ccmpc::QuantArgs a{positions, dtype, ld, static_cast<int>(T), origin, cell_off, cell_cnt,
                     static_cast<int>(n_cells), n_particles_bound,
                     static_cast<const unsigned char *>(rec), rec_kind, P, R * R, cell_allow,
                     reinterpret_cast<ccmpc::QuantRec *>(ws),
                     reinterpret_cast<uint32_t *>(ws + CP * sizeof(ccmpc::QuantRec)),
                     reinterpret_cast<int64_t *>(ws + CP * (sizeof(ccmpc::QuantRec) + 1024)),
                     out_q, out_rhs, out_status};
  const int rc = ccmpc::launch_risk_quantile(a, ccmpc::as_stream(stream));
  CCMPC_REQUIRE(rc == CCMPC_OK, "too many work items for one grid");
  CCMPC_LAUNCH_CHECK();
  return CCMPC_OK;
}
