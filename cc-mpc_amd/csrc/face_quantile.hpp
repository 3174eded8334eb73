// Monte-Carlo calibration of the box-face rows to a risk budget: per (cell, t, face) an exact
// order statistic of the face values v_f on the particle store at a plan, the particle that
// attains it and that particle's own half-space (face_quantile.hip); the C entry point with its
// argument checks is ccmpc_face_quantile in capi.hip.
#pragma once
#include "face_audit.hpp"
#include "quantile.hpp"

namespace ccmpc {

constexpr int kFaceQuantSteps = 8;  // steps per counting workgroup: 8 x 4 faces = kQuantMaxChunk rows
static_assert(4 * kFaceQuantSteps == kQuantMaxChunk, "one 1 KiB LDS histogram per row");

// Workspace, per row (cell, t, face): [256] bins (uint32) | prefix (uint64: the digits of q's
// key found so far, then the key) | rank (int64: the rank left below the prefix; a single
// candidate's key in transit) | arg (uint32: the lowest index holding q's bits) | state (int32).
constexpr size_t kFaceQuantBytesPerRow =
    256 * sizeof(uint32_t) + sizeof(uint64_t) + sizeof(int64_t) + sizeof(uint32_t) + sizeof(int32_t);
inline size_t face_quantile_workspace_bytes(int64_t T, int64_t n_cells) {
  return static_cast<size_t>(n_cells) * static_cast<size_t>(T) * 4 * kFaceQuantBytesPerRow + 64;
}

struct FaceQuantArgs {
  const void *pos;
  int dtype;
  int64_t ld;
  int T;
  const double *origin;
  const int64_t *off, *cnt;
  int n_cells;
  int64_t n_bound;
  const double *past_last;   // [c][2]
  const double *extent;      // {lon, lat}
  double car_r;
  const double *plan;        // [r][T][ld_plan]
  int64_t ld_plan;
  const int32_t *cell_plan;  // [c] or null: row 0
  const int64_t *allow;      // [c] or null: zeros
  double margin;
  uint32_t *bins;            // workspace
  uint64_t *prefix;
  int64_t *rank;
  uint32_t *arg;
  int32_t *state;
  double *out_q;             // [c][T][4]
  int64_t *out_arg;          // [c][T][4]
  double2 *out_cut;          // [c][T][4] ccmpc_gather_rec, as two 16-byte halves
  int32_t *out_status;       // [c][T]
};

// 3 + 2 * kQuantDigits launches on `s`: the initial values, per digit a counting pass over the
// store and the narrowing of every row's prefix, one more pass for the lowest index that holds
// q's bits, and the cuts.  The sequence depends on (T, n_cells, n_bound) only.  CCMPC_OK or
// CCMPC_ERR_ARG when a grid would not fit.  No allocation, no synchronisation.
int launch_face_quantile(const FaceQuantArgs &a, hipStream_t s);

}  // namespace ccmpc
