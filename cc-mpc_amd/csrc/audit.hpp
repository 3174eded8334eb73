// Monte-Carlo risk audit of a plan and of half-space records on a particle store (audit.hip);
// the C entry point with its argument checks is ccmpc_risk_audit in capi.hip.
#pragma once
#include "ccmpc_common.hpp"

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

// Two launches on `s` (initial values, then the streaming pass); CCMPC_OK or CCMPC_ERR_ARG when
// the grid would not fit.  No allocation, no synchronisation.
int launch_risk_audit(const AuditArgs &a, hipStream_t s);

}  // namespace ccmpc
