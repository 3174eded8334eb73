// Monte-Carlo calibration of half-space offsets to a risk budget: an exact batched selection on
// the particle store (quantile.hip); the C entry point with its argument checks is
// ccmpc_risk_quantile in capi.hip.
#pragma once
#include "audit.hpp"

namespace ccmpc {

constexpr int kQuantDigits = 8;     // 8-bit digits of the 64-bit key, most significant first
constexpr int kQuantMaxChunk = 32;  // records per counting workgroup: 1 KiB of LDS bins each

// The order-preserving 64-bit key of a double: unsigned key order = value order (-0 below +0).
// The radix select works on it; the face audit (face_audit.hip) takes its maxima on it.
constexpr uint64_t kSignBit = uint64_t(1) << 63;
constexpr uint64_t kKeyNegInf = ~0xFFF0000000000000ull;            // key of -inf
constexpr uint64_t kKeyPosInf = 0x7FF0000000000000ull | kSignBit;  // key of +inf

__device__ __forceinline__ uint64_t quant_key(double w) {
  const uint64_t b = __builtin_bit_cast(uint64_t, w);
  return (b >> 63) ? ~b : (b | kSignBit);
}
__device__ __forceinline__ double quant_unkey(uint64_t k) {
  return __builtin_bit_cast(double, (k >> 63) ? (k & ~kSignBit) : ~k);
}

// The smallest u (as its key) for which the audit's predicate protects a particle with
// s = side*q under rhs = side*u; the key of +inf where no double does.  Shared by the narrowing
// launches of quantile.hip and ideal_quantile.hip.
__device__ __forceinline__ uint64_t quant_offset_key(double q, double sd, double r2n) {
  auto pred = [&](uint64_t k) {
    const double u = quant_unkey(k);
    const double rhs = sd * u, s = sd * q;
    return audit_protects(sd * (rhs - s), r2n);
  };
  uint64_t lo = kKeyNegInf, hi = kKeyPosInf;
  if (!pred(hi)) return hi;
  if (pred(lo)) return lo;
  // invariant: !pred(lo), pred(hi), lo < hi
  const double est = q + sqrt(r2n);
  if (isfinite(est)) {
    const uint64_t ke = quant_key(est);
    if (pred(ke)) {
      hi = ke;
      for (int i = 0; i < 4; ++i) {
        if (hi - 1 > lo && pred(hi - 1)) {
          --hi;
        } else {
          lo = hi - 1;
          break;
        }
      }
    } else {
      lo = ke;
      for (int i = 0; i < 4; ++i) {
        if (lo + 1 < hi && !pred(lo + 1)) {
          ++lo;
        } else {
          hi = lo + 1;
          break;
        }
      }
    }
  }
  while (hi - lo > 1) {  // at most 64 halvings
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (pred(mid))
      hi = mid;
    else
      lo = mid;
  }
  return hi;
}

// One wave over a record's 256 counts, lane l holding digits 4 l .. 4 l + 3 in c: the digit
// where the count from the top reaches the rank r (1-based).  `mine` on the one lane that holds
// it, with the digit's place in the lane, its count and the count of all larger digits; on no
// lane where r is 0 or above `grand`, the sum of all counts.  quantile_narrow_kernel keeps its
// own, older statement of the same lines: routed through this helper its registers were
// allocated differently, and that kernel's instruction stream is pinned.
struct QuantPick {
  bool mine;
  int dsel;
  uint32_t csel, grand;
  uint64_t run;
};
__device__ __forceinline__ QuantPick quant_pick_digit(const uint4 &c, uint64_t r, int lane) {
  const uint32_t tot = c.x + c.y + c.z + c.w;
  const uint32_t incl = static_cast<uint32_t>(wave_incl_scan_i32(static_cast<int32_t>(tot)));
  const uint32_t grand = static_cast<uint32_t>(lane_i32(static_cast<int32_t>(incl), 63));
  const uint64_t above = grand - incl;  // the count of all larger digits
  QuantPick p;
  p.mine = above < r && r <= above + tot;
  p.dsel = 0;
  p.csel = 0;
  p.grand = grand;
  p.run = above;
  if (p.mine) {
    if (p.run + c.w >= r) {
      p.dsel = 3;
      p.csel = c.w;
    } else if (p.run + c.w + c.z >= r) {
      p.run += c.w;
      p.dsel = 2;
      p.csel = c.z;
    } else if (p.run + c.w + c.z + c.y >= r) {
      p.run += static_cast<uint64_t>(c.w) + c.z;
      p.dsel = 1;
      p.csel = c.y;
    } else {
      p.run += static_cast<uint64_t>(c.w) + c.z + c.y;
      p.csel = c.x;
    }
  }
  return p;
}

// A record as the counting passes read it (written by the call's first launch, its prefix
// extended by every narrowing launch).  t < 0: nothing to select (VACUOUS or SKIPPED); else the
// step in the low byte and the selection state above it (quantile.hip).
struct QuantRec {
  double n0, n1;
  uint64_t prefix;  // the digits of q's key found so far
  int32_t side, t;
};
static_assert(sizeof(QuantRec) == 32, "QuantRec is read as two 16-byte loads");

// Workspace: [C P] QuantRec, [C P][256] bins (uint32), [C P] remaining ranks (int64).
constexpr size_t kQuantBytesPerRec = sizeof(QuantRec) + sizeof(int64_t) + 256 * sizeof(uint32_t);
inline size_t quantile_workspace_bytes(int64_t n_cells, int P) {
  return static_cast<size_t>(n_cells) * static_cast<size_t>(P) * kQuantBytesPerRec + 64;
}

struct QuantArgs {
  const void *pos;
  int dtype;
  int64_t ld;
  int T;
  const double *origin;
  const int64_t *off, *cnt;
  int n_cells;
  int64_t n_bound;
  const unsigned char *rec;  // [n_cells][P] records of `kind`
  int kind, P;
  double R2;                 // R * R
  const int64_t *allow;      // [n_cells] or null: zeros
  QuantRec *qrec;            // workspace
  uint32_t *bins;
  int64_t *rank;
  double *out_q, *out_rhs;
  int32_t *out_status;
};

// 1 + 2 * kQuantDigits launches on `s`: the initial values, then per digit a counting pass over
// the store and the narrowing of every record's prefix (the last one writes the outputs).  The
// sequence depends on (T, kind, n_cells, n_bound) only.  CCMPC_OK or CCMPC_ERR_ARG when a grid
// would not fit.  No allocation, no synchronisation.
int launch_risk_quantile(const QuantArgs &a, hipStream_t s);

}  // namespace ccmpc
