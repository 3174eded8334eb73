// Outer-approximation cuts of the box-face second-order-cone rows (socp.hip): one half-space
// per selected (cell, t) row, linearised at a plan, written as ccmpc_gather_rec into a pool the
// planning QP reads in place; the C entry point with its argument checks is ccmpc_face_cuts in
// capi.hip.
#pragma once
#include "ccmpc_common.hpp"

namespace ccmpc {

constexpr int kCutMaxT = 40;

struct FaceCutArgs {
  const ccmpc_face_rec *rec;   // [cells][T][4]
  int T;
  const int64_t *scene_cell;   // [S + 1]
  const int32_t *face_sel;     // [cells][T] or null: the record's own chosen flag
  const double *gamma;         // [cells]
  double car_r;
  const double *plan;          // [S][T][ld_plan]
  int64_t ld_plan;
  int round, max_rounds;
  double tol_g;
  int only_violated;
  double4 *pool;               // ccmpc_gather_rec, 32 bytes each
  const int64_t *pool_cell;    // [S + 1]
  double *out_g;               // [cells][T]
  double *out_viol;            // [S]
  int32_t *out_state;          // [S]
};

// One launch of n_scenes workgroups on `s`.  No allocation, no synchronisation, no atomics.
void launch_face_cuts(const FaceCutArgs &a, int64_t n_scenes, hipStream_t s);

}  // namespace ccmpc
