// Box-face chance constraints on a particle store (faces.hip): the moments of the per-particle
// heading-dependent face coefficients and the second-order-cone row data built from them; the C
// entry point with its argument checks is ccmpc_face_constraints in capi.hip.
#pragma once
#include "ccmpc_common.hpp"
#include "gram.hpp"

namespace ccmpc {

constexpr int kFaceMaxT = 40;
constexpr int kFaceAcc = 18;       // two families x (3 sums + 6 products) per (cell, t)
constexpr int kFaceLgChunk64 = 11;  // particles per item: 256 lanes x 4 groups x 2 (f64) ...
constexpr int kFaceLgChunk32 = 11;  // ... or x 2 groups x 4 (f32): 16 bytes per lane and load

struct FaceArgs {
  const void *pos;
  int dtype;
  int64_t ld;
  int T;
  const double *origin;
  const int64_t *off, *cnt;
  int n_cells;
  const double *past_last;   // [c][2]
  const double *extent;      // {lon, lat}
  const double *gamma;       // [c]
  const double *ref;         // [r][T][2] or null
  const int32_t *cell_ref;   // [c] or null: row 0
  int kind;
  double car_r;
  int64_t max_items;         // capacity of `part` in items (= the grid of the first launch)
  int32_t *first;            // [c]: the cell's first item
  double *head;              // [c][T][4]: x0, y0, cos, sin of the cell's first particle
  double *part;              // [item][T][kFaceAcc]
  ccmpc_face_rec *rec;       // [c][T][4]
};

// cos / sin of the heading of a step delta, as l4.hip's heading_cs_rsq forms them (restated, so
// that file keeps its bits): (dx, dy) / |(dx, dy)| from the hardware rsqrt with two Newton steps;
// a delta whose squared norm would be subnormal is first scaled by 2^600 (exact); a zero step or
// an overflowing norm keeps sincos of atan2 (atan2(0, 0) = 0: c = 1, s = 0).
__device__ __forceinline__ void face_heading(double dx, double dy, double &S, double &C) {
  double n2 = dx * dx + dy * dy;
  if (n2 < 0x1p-960) {
    dx *= 0x1p600;
    dy *= 0x1p600;
    n2 = dx * dx + dy * dy;
  }
  if (n2 > 0.0 && n2 < INFINITY) {
    double r = __builtin_amdgcn_rsq(n2);
    r = r * fma(-0.5 * n2 * r, r, 1.5);
    r = r * fma(-0.5 * n2 * r, r, 1.5);
    C = dx * r;
    S = dy * r;
  } else {
    sincos(atan2(dy, dx), &S, &C);
  }
}

template <typename P>
__device__ __forceinline__ double face_world(P v, double o) {
  return static_cast<double>(v) + o;  // as world() in l4.hip
}

inline size_t face_round256(size_t b) { return (b + 255) / 256 * 256; }

// Workspace: first | head | part, each 256-byte aligned.  `items` = max_items at the chunk used.
inline size_t face_layout(int64_t T, int64_t n_cells, int64_t items, size_t *o_head,
                          size_t *o_part) {
  size_t o = face_round256(static_cast<size_t>(n_cells) * sizeof(int32_t));
  *o_head = o;
  o += face_round256(static_cast<size_t>(n_cells) * T * 4 * sizeof(double));
  *o_part = o;
  o += face_round256(static_cast<size_t>(items) * T * kFaceAcc * sizeof(double));
  return o;
}

// Bytes for either dtype (the f64 chunk is the smaller one, so it has the most items).
inline size_t face_workspace_bytes(int64_t T, int64_t n_cells, int64_t n_bound) {
  size_t oh, op;
  return face_layout(T, n_cells, max_items(n_cells, n_bound, int64_t(1) << kFaceLgChunk64), &oh,
                     &op);
}

// Two launches on `s` (moments of the chunks, then one wave per (cell, t)); CCMPC_OK or
// CCMPC_ERR_ARG when a grid would not fit.  No allocation, no synchronisation, no atomics.
int launch_face_constraints(FaceArgs a, int64_t n_bound, void *workspace, hipStream_t s);

}  // namespace ccmpc
