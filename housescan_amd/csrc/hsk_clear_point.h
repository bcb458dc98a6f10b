// hsk_clear_point.h -- the clearance field (DESIGN.md 8l the rule, 3.18 the kernels): which voxels are obstacles, the nearest set
// bit of a row's obstacle mask, the border term, the windowed minimum every axis pass runs -- templated on its load -- and the
// voxel of a world point.  Plain C++ with no HIP type in it, so that tests/clear_point_harness.cpp compiles the same text for the
// host and tests/test_clearance_host.py compares the field it makes with the numpy twin (tests/clearance_twin.py).  All integers.
//
// THE BOUND every loop below rests on: a reach is at most CLEAR_MAX_REACH = 255 voxels, a weight at most 1024, so max_d2 <
// 256^2 * 1024 = 2^26 and every sum formed below stays under 2^30 + 2^26: nothing wraps.  A value above max_d2 is kept as
// CLEAR_INF between the passes (it can never be part of a minimum that is at most max_d2) and leaves as CLEAR_FAR.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hsk_sample.h"

#define CLEAR_FAR 0xffffffffu      // the field's "farther than max_d2, or no obstacle at all" (HSK_CLEARANCE_FAR)
#define CLEAR_OUTSIDE 0xfffffffeu  // a point lookup outside the grid (HSK_CLEARANCE_OUTSIDE)
#define CLEAR_INF 0x40000000u      // "above max_d2" between the passes
#define CLEAR_DX_NONE 0xffffu      // the x pass: no obstacle within reach in this row
#define CLEAR_MAX_REACH 255
#define CLEAR_FLAG_UNKNOWN 1u      // HSK_CLEAR_UNKNOWN
#define CLEAR_MASK_BITS 64u        // voxels of a row per mask word: the seams of the x pass
#define CLEAR_AXIS_SEG 16u         // consecutive outputs along the axis a wave of an axis pass makes: the seams of the y and z passes

#if defined(__HIPCC__)
#define CLEAR_ROLLED _Pragma("unroll 1")  // (a rolled loop of divergent trips keeps one saved lane mask, not one per trip)
#else
#define CLEAR_ROLLED
#endif

// 8i's states from the pair word: SOLID = observed with raw <= 0; with the flag an UNSEEN voxel (weight 0) is an obstacle too
HSK_HD bool clear_obstacle(unsigned word, unsigned flags) {
  const int w = hsk_pair_wgt(word);
  return w == 0 ? (flags & CLEAR_FLAG_UNKNOWN) != 0u : hsk_pair_raw(word) <= 0;
}

// the distance to the grid's outside along one axis of n voxels: min(i + 1, n - i)
HSK_HD unsigned clear_border(unsigned i, unsigned n) { return i + 1u < n - i ? i + 1u : n - i; }

// The distance from bit x to the nearest set bit of mask[0, nw) -- a row's obstacle bits, bit x & 63 of word x >> 6 -- when that
// is at most R, else CLEAR_DX_NONE.  Each loop looks at the words of one side: it ends after at most (R >> 6) + 1 <= 4 further
// words (R <= 255) or at the end of the row.
HSK_HD unsigned clear_nearest_bit(const unsigned long long* mask, unsigned nw, unsigned x, unsigned R) {
  const unsigned wi = x >> 6, b = x & 63u;
  unsigned best = CLEAR_DX_NONE;
  {  // at or below x
    unsigned long long m = mask[wi] & (~0ull >> (63u - b));
    unsigned w = wi, base = 0u;  // base: the distance from x to bit 63 of word w
CLEAR_ROLLED
    for (unsigned trip = 0u; trip <= ((unsigned)CLEAR_MAX_REACH >> 6) + 1u; ++trip) {
      if (m) {
        best = (trip == 0u ? b : base + 63u) - (63u - (unsigned)__builtin_clzll(m));
        break;
      }
      if (w == 0u) break;
      base = trip == 0u ? b + 1u : base + 64u;
      if (base > R) break;
      w -= 1u;
      m = mask[w];
    }
  }
  {  // above x
    unsigned long long m = b == 63u ? 0ull : mask[wi] & (~0ull << (b + 1u));
    unsigned w = wi, base = 0u;  // base: the distance from x to bit 0 of word w
CLEAR_ROLLED
    for (unsigned trip = 0u; trip <= ((unsigned)CLEAR_MAX_REACH >> 6) + 1u; ++trip) {
      if (m) {
        const unsigned d = trip == 0u ? (unsigned)__builtin_ctzll(m) - b : base + (unsigned)__builtin_ctzll(m);
        best = d < best ? d : best;
        break;
      }
      if (w + 1u >= nw) break;
      base = trip == 0u ? 64u - b : base + 64u;
      if (base > R || base >= best) break;
      w += 1u;
      m = mask[w];
    }
  }
  return best <= R ? best : CLEAR_DX_NONE;
}

// the x pass's value of a voxel: the distance to the row's nearest obstacle and, with the flag, to the outside
HSK_HD unsigned clear_row_dx(const unsigned long long* mask, unsigned nw, unsigned x, unsigned X, unsigned R, unsigned flags) {
  unsigned d = clear_nearest_bit(mask, nw, x, R);
  if (flags & CLEAR_FLAG_UNKNOWN) {
    const unsigned e = clear_border(x, X);
    d = (e <= R && e < d) ? e : d;
  }
  return d;
}
// ... as a squared distance: what the y pass reads
HSK_HD unsigned clear_dx_value(unsigned dx, unsigned wx) { return dx == CLEAR_DX_NONE ? CLEAR_INF : wx * dx * dx; }

// above max_d2 -> `far` (CLEAR_INF between the passes, CLEAR_FAR in the field)
HSK_HD unsigned clear_cap(unsigned v, unsigned max_d2, unsigned far) { return v <= max_d2 ? v : far; }

// One axis pass at position i of n along the axis: min over |j| <= R of in(i + j) + w j^2, positions outside the row left out,
// and with the flag the border term w min(i + 1, n - i)^2.  `in` gives a value that is at most max_d2 or CLEAR_INF.
template <class Load>
HSK_HD unsigned clear_window_min(const Load& in, unsigned i, unsigned n, unsigned w, unsigned R, unsigned flags) {
  unsigned best = in(i);
  if (flags & CLEAR_FLAG_UNKNOWN) {
    const unsigned e = clear_border(i, n);
    if (e <= R) {  // (beyond the reach the term is above max_d2 anyway, and e * e * w might not fit)
      const unsigned c = w * e * e;
      best = c < best ? c : best;
    }
  }
  // (bounded: R <= CLEAR_MAX_REACH = 255 trips; it ends sooner once the step alone costs as much as the best so far)
  for (unsigned j = 1u; j <= R; ++j) {
    const unsigned c = w * j * j;
    if (c >= best) break;
    const unsigned a = i >= j ? in(i - j) : CLEAR_INF, b = i + j < n ? in(i + j) : CLEAR_INF;
    const unsigned m = (a < b ? a : b) + c;
    best = m < best ? m : best;
  }
  return best;
}

// the reach of an axis: the largest r with w r^2 <= max_d2, as floor(sqrt(max_d2 / w)) in binary64 (exact: the quotient of two
// integers below 2^32 is farther from the next integer than its rounding error, and the root of a perfect square is exact)
static inline unsigned clear_reach(unsigned max_d2, unsigned w) { return (unsigned)floor(sqrt((double)max_d2 / (double)w)); }

// A world point's voxel, unclamped, as cover_voxel_word (hsk_cover_point.h) takes it: `inside` says whether it lies in the grid
// (a NaN does not); x, y, z: the voxel clamped into the grid, so that the load behind it is legal whatever the point is.
template <class Vol>
HSK_HD void clear_point_voxel(const Vol& v, float px, float py, float pz, unsigned& x, unsigned& y, unsigned& z, bool& inside) {
  const int gx = hsk_vox_of_q(hsk_div_by_const(px, v.icell[0])), gy = hsk_vox_of_q(hsk_div_by_const(py, v.icell[1])),
            gz = hsk_vox_of_q(hsk_div_by_const(pz, v.icell[2]));
  inside = gx >= 0 && gx < v.X && gy >= 0 && gy < v.Y && gz >= 0 && gz < v.Z;
  x = (unsigned)hsk_min_i(hsk_max_i(gx, 0), v.X - 1);
  y = (unsigned)hsk_min_i(hsk_max_i(gy, 0), v.Y - 1);
  z = (unsigned)hsk_min_i(hsk_max_i(gz, 0), v.Z - 1);
}
