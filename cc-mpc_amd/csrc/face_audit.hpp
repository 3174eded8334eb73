// Monte-Carlo audit of the box-face rows on a particle store (face_audit.hip): per (cell, t),
// the particles each face's inequality leaves open at a plan; the C entry point with its
// argument checks is ccmpc_face_audit in capi.hip.
#pragma once
#include "audit.hpp"
#include "faces.hpp"

namespace ccmpc {

// The four face values of one particle at one step, as ccmpc_face_audit's contract states them
// (include/ccmpc.h): (x, y) the particle's world position, (xp, yp) its previous one (past_last
// at step 0), (X, Y) the plan point.  Float64, no contraction, products before sums.  S, C: the
// heading's sine and cosine (face_heading).  Shared by face_audit.hip and face_quantile.hip, so
// both form the same bits.
__device__ __forceinline__ void face_values(double x, double y, double xp, double yp, double X,
                                            double Y, double hlat, double hlon, double &S,
                                            double &C, double &v0, double &v1, double &v2,
                                            double &v3) {
  face_heading(x - xp, y - yp, S, C);
  const double ex = X - x, ey = Y - y;
  const double p = C * ex - S * ey, q = S * ex + C * ey;
  v0 = hlat - p;
  v1 = hlon - q;
  v2 = hlat + p;
  v3 = hlon + q;
}

struct FaceAuditArgs {
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
  const int32_t *face_sel;   // [c][T] or null: no selected-row outputs
  int64_t *face_open;        // [c][T][4]
  int64_t *in_box;           // [c][T]
  int64_t *in_box_any;       // [c]
  int64_t *sel_open;         // [c][T]   (face_sel)
  int64_t *sel_open_any;     // [c]      (face_sel)
  double *worst;             // [c][T][4] or null
};

// Two launches on `s` (initial values, then the streaming pass); CCMPC_OK or CCMPC_ERR_ARG when
// a grid would not fit.  No allocation, no synchronisation.
int launch_face_audit(const FaceAuditArgs &a, hipStream_t s);

}  // namespace ccmpc
