// hsk_level_solve.h -- the upright-frame estimate, the HOST's steps: functions of the integer sums the device returns,
// in binary64 with +, -, x, / and sqrt only, every expression in the written order -- the seed from the cube-map histogram, an axis
// from its signed sums, the coarse yaw from the two fourth-power sums, one refit of the frame from three axes' sums, floor and
// ceiling from the height histograms -- and level_estimate, the order in which they are asked, over any `Stages` that answers the
// three device questions.  api_level.hip gives it the kernels, tests/level_point_harness.cpp loops over hsk_level_point.h on the
// host; tests/level_twin.py restates all of it.  Plain C++, no HIP type.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/hskinfu.h"
#include "hsk_level_point.h"

static inline double level_dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static inline bool level_norm(const double v[3], double out[3]) {
  const double l = sqrt(level_dot3(v, v));
  const bool ok = l > 0.0 && l <= 1.7976931348623157e308;
  for (int k = 0; k < 3; ++k) out[k] = ok ? v[k] / l : 0.0;
  return ok;
}
static inline void level_cross(const double a[3], const double b[3], double out[3]) {
  const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  memcpy(out, c, sizeof(c));
}
// v - (v . d) d
static inline void level_proj(const double v[3], const double d[3], double out[3]) {
  const double s = level_dot3(v, d);
  const double p[3] = {v[0] - s * d[0], v[1] - s * d[1], v[2] - s * d[2]};
  memcpy(out, p, sizeof(p));
}
static inline void level_quantise_axis(const double a[3], int32_t A[3]) {
  for (int k = 0; k < 3; ++k) A[k] = (int32_t)rint(a[k] * HSK_LEVEL_A_SCALE);
}
// the hint as a unit vector; false: zero or not finite
static inline bool level_hint(const float up_hint[3], double h[3]) {
  const double v[3] = {(double)up_hint[0], (double)up_hint[1], (double)up_hint[2]};
  return level_norm(v, h);
}
static inline uint64_t level_least(float min_fraction, uint64_t n) {
  const double f = floor((double)min_fraction * (double)n);
  return f > 3.0 ? (uint64_t)f : 3u;
}

// step 2: the 2 x 2 block of bins of the largest support among those whose shared corner lies within the hint's cone; the first of
// equals in (face, j, i) order.  A block's support is its four counts plus those of the four antipodes: a ceiling votes for up as a
// floor does, and a direction on a bin corner -- the volume's own axes are, so every scan that starts level -- spreads a noisy floor
// over four bins, which one block holds.  The seed is the corner's direction, face coordinates (2 (i + 1) - 16) / 16.
static inline void level_solve_seed(const uint32_t* hist, const double hint[3], double tilt, uint64_t least, double axis[3], uint64_t* support,
                                    bool* found) {
  int64_t best = -1;
  double best_d[3] = {0.0, 0.0, 0.0};
  const int F = HSK_LEVEL_FACE;
  for (int f = 0; f < 6; ++f)
    for (int j = 0; j < F - 1; ++j)
      for (int i = 0; i < F - 1; ++i) {
        const int m = f / 2;
        double d[3] = {0.0, 0.0, 0.0};
        d[m] = (f & 1) ? -1.0 : 1.0;
        d[(m + 1) % 3] = (double)(2 * (i + 1) - F) / 16.0;
        d[(m + 2) % 3] = (double)(2 * (j + 1) - F) / 16.0;
        level_norm(d, d);
        if (!(level_dot3(d, hint) >= tilt)) continue;
        int64_t sup = 0;
        for (int jj = j; jj <= j + 1; ++jj)
          for (int ii = i; ii <= i + 1; ++ii)
            sup += (int64_t)hist[(f * F + jj) * F + ii] + (int64_t)hist[(((f ^ 1) * F) + (F - 1 - jj)) * F + (F - 1 - ii)];
        if (sup > best) best = sup, memcpy(best_d, d, sizeof(d));
      }
  *found = best >= 0 && (uint64_t)best >= least;
  *support = best > 0 ? (uint64_t)best : 0u;
  for (int k = 0; k < 3; ++k) axis[k] = *found ? best_d[k] : 0.0;
}

// step 3: S / |S|, flipped into the hint's hemisphere; false: S = 0
static inline bool level_solve_axis(const int64_t s4[4], const double hint[3], double axis[3]) {
  const double S[3] = {(double)s4[1], (double)s4[2], (double)s4[3]};
  double a[3];
  if (!level_norm(S, a)) return false;
  const bool flip = level_dot3(a, hint) < 0.0;
  for (int k = 0; k < 3; ++k) axis[k] = flip ? -a[k] : a[k];
  return true;
}

// step 4's basis: e1 from the volume axis of the smallest |a_k| (the lowest k of equals), e2 = a x e1
static inline void level_basis(const double a[3], double e1[3], double e2[3]) {
  int k = 0;
  for (int c = 1; c < 3; ++c)
    if (fabs(a[c]) < fabs(a[k])) k = c;
  double e[3] = {0.0, 0.0, 0.0};
  e[k] = 1.0;
  level_proj(e, a, e1);
  level_norm(e1, e1);
  level_cross(a, e1, e2);
}
// without a yaw: the volume's +X, or +Z where +X is degenerate, projected off a
static inline void level_plain_x(const double a[3], double x[3]) {
  const bool z = a[0] * a[0] > 0.5;
  const double e[3] = {z ? 0.0 : 1.0, 0.0, z ? 1.0 : 0.0};
  level_proj(e, a, x);
  level_norm(x, x);
}
// step 4: (c, s) = (re, im) / |(re, im)| is four times the walls' angle; two half-angle steps; of x and its quarter turns about a,
// the one with the largest component along +X (the first of equals)
static inline bool level_solve_yaw(const int64_t w3[3], uint64_t least, const double a[3], double x[3]) {
  const double re = (double)w3[1], im = (double)w3[2];
  const double r = sqrt(re * re + im * im);
  if ((uint64_t)w3[0] < least || !(r > 0.0)) {
    level_plain_x(a, x);
    return false;
  }
  double c = re / r, s = im / r;
  for (int h = 0; h < 2; ++h) {
    const double c2 = sqrt((1.0 + c) / 2.0), s2 = copysign(sqrt((1.0 - c) / 2.0), s);
    c = c2, s = s2;
  }
  double e1[3], e2[3], cand[4][3];
  level_basis(a, e1, e2);
  for (int k = 0; k < 3; ++k) cand[0][k] = c * e1[k] + s * e2[k];
  level_cross(a, cand[0], cand[1]);
  for (int k = 0; k < 3; ++k) cand[2][k] = -cand[0][k], cand[3][k] = -cand[1][k];
  int best = 0;
  for (int q = 1; q < 4; ++q)
    if (cand[q][0] > cand[best][0]) best = q;
  level_proj(cand[best], a, x);
  level_norm(x, x);
  return true;
}

// the rows of the levelled frame: x, down = -a, x x down
static inline void level_rows(const double a[3], const double x[3], double rows[3][3]) {
  for (int k = 0; k < 3; ++k) rows[0][k] = x[k], rows[1][k] = -a[k];
  level_cross(rows[0], rows[1], rows[2]);
}

// step 5: one refit of (a, x) from the three rows' counts and sums
static inline void level_solve_frame(const int64_t s12[12], uint64_t least, const double hint[3], bool yaw, double a[3], double x[3]) {
  if ((uint64_t)s12[4] >= least) {
    double a2[3];
    if (level_solve_axis(s12 + 4, hint, a2)) memcpy(a, a2, sizeof(a2));
  }
  const double d[3] = {-a[0], -a[1], -a[2]};
  double v[3] = {0.0, 0.0, 0.0};
  if (yaw) {
    if ((uint64_t)s12[0] >= least) {
      const double S[3] = {(double)s12[1], (double)s12[2], (double)s12[3]};
      level_proj(S, d, v);
    }
    if ((uint64_t)s12[8] >= least) {
      const double S[3] = {(double)s12[9], (double)s12[10], (double)s12[11]};
      double u[3];
      level_proj(S, d, u);
      level_cross(d, u, u);
      for (int k = 0; k < 3; ++k) v[k] = v[k] + u[k];
    }
  }
  double x2[3];
  if (!level_norm(v, x2)) {
    level_proj(x, d, x2);
    level_norm(x2, x2);
  }
  memcpy(x, x2, sizeof(x2));
}

// step 6: per class, among the bins that hold at least half the peak's count the outermost one (the largest t_1 for the floor, the
// smallest for the ceiling); the mean of t_1 over it and its two neighbours
static inline uint32_t level_solve_heights(const uint32_t* cnt, const int64_t* sum, uint64_t least, double* floor_m, double* ceiling_m) {
  uint32_t bits = 0;
  double out[2] = {0.0, 0.0};
  const int B = HSK_LEVEL_H_BINS;
  for (int cls = 0; cls < 2; ++cls) {
    const uint32_t* c = cnt + (size_t)cls * B;
    const int64_t* s = sum + (size_t)cls * B;
    uint64_t total = 0, peak = 0;
    for (int b = 0; b < B; ++b) {
      total += c[b];
      if (c[b] > peak) peak = c[b];
    }
    if (total < least || total == 0) continue;
    int at = -1;
    if (cls == 0) {
      for (int b = B - 1; b >= 0 && at < 0; --b)
        if (2 * (uint64_t)c[b] >= peak) at = b;
    } else {
      for (int b = 0; b < B && at < 0; ++b)
        if (2 * (uint64_t)c[b] >= peak) at = b;
    }
    const int lo = at > 0 ? at - 1 : 0, hi = at < B - 1 ? at + 1 : B - 1;
    int64_t ss = 0, cc = 0;
    for (int b = lo; b <= hi; ++b) ss += s[b], cc += c[b];
    out[cls] = ((double)ss / (double)cc) / 4194304.0;
    bits |= cls == 0 ? HSK_UPRIGHT_FLOOR : HSK_UPRIGHT_CEILING;
  }
  *floor_m = out[0];
  *ceiling_m = out[1];
  return bits;
}

// The estimate over the three device questions, each an int (HSK_OK or the error that ends the estimate):
//   st.hist(hist[1536], &n_valid)
//   st.sums(axes[3][3], n_axes, sums12, wall[3][3] or null, wall3)   -- the supporters of up to three axes; the wall points of wall[0]
//   st.extents(R[3][3], classes, box6, counts, sums)                 -- counts, sums: 2 x 16384, written when classes is set
// p: checked parameters; n > 0 points; cnt, sum: room for the height histograms.
template <class Stages>
static inline int level_estimate(Stages& st, uint64_t n, const hsk_upright_params& p, hsk_upright* out, uint32_t* hist, uint32_t* cnt, int64_t* sum) {
  double hint[3];
  level_hint(p.up_hint, hint);
  const uint64_t least = level_least(p.min_fraction, n);
  uint64_t n_valid = 0;
  if (int rc = st.hist(hist, &n_valid)) return rc;
  out->n_invalid = (uint32_t)(n - n_valid);
  double a[3], x[3];
  uint64_t support = 0;
  bool found_up = false, yaw = false;
  level_solve_seed(hist, hint, (double)p.max_tilt_cos, least, a, &support, &found_up);
  int32_t A[3][3];
  if (found_up) {
    out->found |= HSK_UPRIGHT_UP;
    out->n_axis[1] = (uint32_t)support;
    for (int r = 0; r < p.refits; ++r) {
      int64_t s12[12], w3[3];
      level_quantise_axis(a, A[0]);
      if (int rc = st.sums(A, 1, s12, nullptr, w3)) return rc;
      if ((uint64_t)s12[0] < least) break;
      double a2[3];
      if (!level_solve_axis(s12, hint, a2)) break;
      memcpy(a, a2, sizeof(a2));
    }
    level_plain_x(a, x);
    if (!(p.flags & HSK_UPRIGHT_NO_YAW)) {
      double e1[3], e2[3];
      int64_t s12[12], w3[3];
      level_basis(a, e1, e2);
      level_quantise_axis(a, A[0]), level_quantise_axis(e1, A[1]), level_quantise_axis(e2, A[2]);
      if (int rc = st.sums(A, 0, s12, A, w3)) return rc;
      out->n_walls = (uint32_t)w3[0];
      yaw = level_solve_yaw(w3, least, a, x);
      if (yaw) out->found |= HSK_UPRIGHT_YAW;
    }
    double rows[3][3];
    for (int r = 0; r < p.refits; ++r) {
      int64_t s12[12], w3[3];
      level_rows(a, x, rows);
      for (int k = 0; k < 3; ++k) level_quantise_axis(rows[k], A[k]);
      if (int rc = st.sums(A, 3, s12, nullptr, w3)) return rc;
      for (int k = 0; k < 3; ++k) out->n_axis[k] = (uint32_t)s12[4 * k];
      level_solve_frame(s12, least, hint, yaw, a, x);
    }
    level_rows(a, x, rows);
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 3; ++c) out->level[4 * k + c] = (float)rows[k][c];
  }
  for (int k = 0; k < 3; ++k) {
    const double row[3] = {(double)out->level[4 * k], (double)out->level[4 * k + 1], (double)out->level[4 * k + 2]};
    level_quantise_axis(row, A[k]);
  }
  int32_t box[6];
  if (int rc = st.extents(A, found_up, box, cnt, sum)) return rc;
  if (n_valid > 0) {
    for (int k = 0; k < 3; ++k) {
      out->box_lo[k] = (float)((double)box[k] / 4194304.0);
      out->box_hi[k] = (float)((double)box[3 + k] / 4194304.0);
    }
  }
  if (found_up) {
    double fl, ce;
    out->found |= level_solve_heights(cnt, sum, least, &fl, &ce);
    out->floor_m = (float)fl;
    out->ceiling_m = (float)ce;
  }
  return HSK_OK;
}

// an empty result: nothing found, the identity
static inline void level_clear(hsk_upright* out, uint64_t n) {
  memset(out, 0, sizeof(*out));
  out->level[0] = out->level[5] = out->level[10] = out->level[15] = 1.0f;
  out->n_points = (uint32_t)n;
}
