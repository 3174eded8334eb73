// Monte-Carlo risk audit of a plan and of half-space records on a particle store (audit.hip);
// the C entry point with its argument checks is ccmpc_risk_audit in capi.hip.
#pragma once
#include "ccmpc_common.hpp"
#include "gram.hpp"

namespace ccmpc {

constexpr int kAuditMaxT = 40;
constexpr int kAuditMaxRec = kAuditMaxT * (kAuditMaxT - 1) / 2;  // half-space rows of one cell

struct AuditArgs {
  const void *pos;
  int dtype;
  int64_t ld;
  int T;
  const double *origin;
  const int64_t *off, *cnt;
  int n_cells;
  int64_t n_bound;
  const double *plan;        // [r][T][2] or null: no plan half
  const int32_t *cell_plan;  // [n_cells] or null: row 0
  const unsigned char *rec;  // [n_cells][P] records of `kind`, or null: no record half
  int kind, P;
  double R2;                 // R * R
  int64_t *hit, *hit_any;
  double *min_d2;
  int64_t *rec_open, *open;
};

// rows per cell of a record kind at horizon T (-1: unknown kind)
inline int audit_rows(int kind, int64_t T) {
  switch (kind) {
    case CCMPC_REC_KIND_HALFSPACE:
    case CCMPC_REC_KIND_HALFSPACE_COMPACT: return static_cast<int>(T * (T - 1) / 2);
    case CCMPC_REC_KIND_AFFINE:
    case CCMPC_REC_KIND_AFFINE_COMPACT: return static_cast<int>(T);
    default: return -1;
  }
}

// A lane's 16-byte load of one plane: W particles, widened to double on use.
template <typename P>
struct AuditVec;
template <>
struct AuditVec<double> {
  static constexpr int W = 2;
  double2 v;
  __device__ __forceinline__ void load(const double *p) { v = stream_load2<true>(p); }
  __device__ __forceinline__ double operator[](int j) const { return j ? v.y : v.x; }
};
template <>
struct AuditVec<float> {
  static constexpr int W = 4;
  float4 v;
  __device__ __forceinline__ void load(const float *p) {
    const ccmpc_f4v t = __builtin_nontemporal_load(reinterpret_cast<const ccmpc_f4v *>(p));
    v = make_float4(t.x, t.y, t.z, t.w);
  }
  __device__ __forceinline__ double operator[](int j) const {
    return static_cast<double>(j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w);
  }
};

// The fields of a record the audit reads, from any of the four kinds.
struct AuditRec {
  double n0, n1, rhs;
  int side, status, t;
};
__device__ __forceinline__ AuditRec audit_read_rec(const unsigned char *__restrict__ rec,
                                                   int kind, int64_t i) {
  AuditRec q;
  if (kind == CCMPC_REC_KIND_HALFSPACE || kind == CCMPC_REC_KIND_AFFINE) {
    const unsigned char *r = rec + i * 128;
    const double2 nn = *reinterpret_cast<const double2 *>(r);
    const int4 tail = *reinterpret_cast<const int4 *>(r + 112);  // which, side, status, t(_tau)
    q.n0 = nn.x;
    q.n1 = nn.y;
    q.rhs = *reinterpret_cast<const double *>(r + (kind == CCMPC_REC_KIND_AFFINE ? 32 : 16));
    q.side = tail.y;
    q.status = tail.z;
    q.t = kind == CCMPC_REC_KIND_AFFINE ? tail.w : (tail.w >> 16);
  } else {  // ccmpc_gather_rec
    const unsigned char *r = rec + i * 32;
    const double2 nn = *reinterpret_cast<const double2 *>(r);
    const uint2 w = *reinterpret_cast<const uint2 *>(r + 24);
    q.n0 = nn.x;
    q.n1 = nn.y;
    q.rhs = *reinterpret_cast<const double *>(r + 16);
    q.side = static_cast<int16_t>(w.x & 0xffffu);
    q.status = static_cast<int16_t>(w.x >> 16);
    const int tt = static_cast<int>(w.y);
    q.t = kind == CCMPC_REC_KIND_AFFINE_COMPACT ? tt : (tt >> 16);
  }
  return q;
}
__device__ __forceinline__ bool audit_rec_valid(const AuditRec &q, int T) {
  return q.status == 0 && q.t >= 0 && q.t < T;
}

// The audit's predicate on v = side * (rhs - n.p) and r2n = (R*R) * |n|^2: the record protects
// the particle.  Shared with the quantile's offset search (quantile.hip).
__device__ __forceinline__ bool audit_protects(double v, double r2n) {
  return v >= 0.0 && v * v >= r2n;
}

// Two launches on `s` (initial values, then the streaming pass); CCMPC_OK or CCMPC_ERR_ARG when
// the grid would not fit.  No allocation, no synchronisation.
int launch_risk_audit(const AuditArgs &a, hipStream_t s);

}  // namespace ccmpc
