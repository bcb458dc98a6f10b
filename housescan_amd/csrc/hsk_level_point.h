// hsk_level_point.h -- the upright-frame estimate, the work on ONE point: a point's integers N (its normal, the cells'
// skew taken out) and P (its place), whether it is valid, its bin of the cube-map histogram, the two cone tests against an integer
// axis, what a wall point adds to the yaw's sums, its levelled coordinates and its bin of the height histograms.  level.hip's
// kernels call it per lane; like hsk_plane_point.h it is plain C++ with no HIP type in it, so that tests/level_point_harness.cpp
// compiles the same text for the host and tests/test_level_host.py compares it with the numpy twin (tests/level_twin.py) bit for
// bit, without a GPU.  One rounding per written operator: both builds forbid contraction.  Behind level_point() everything is
// integer arithmetic; the cone tests convert exact integer products to binary64 and multiply once.
//
// The bounds: |N_k| <= 2^15 and |P_k| <= 2^16, an axis A = rint(a 4096) of a unit vector has |A_k| <= 4096 and |A|^2 < 2^24 1.001.
// N . A is below 2^28.8 and its square, like |N|^2 |A|^2, below 3 2^54 1.001: an int64 holds both.  For |n| <= 1.41 (every
// producer here gives unit normals) they stay below 2^53 and the conversion to binary64 is exact; above, it rounds once to
// nearest even -- the same in the kernels, the harness and numpy.  P . R is below 2^28.8: an int32 holds it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hsk_sample.h"

#define HSK_LEVEL_REACH_M 64.0f      // |x|, |y|, |z| of a valid point
#define HSK_LEVEL_N_MAX 2.0f         // |n_k| of a valid point
#define HSK_LEVEL_N_SCALE 16384.0f   // N = rint((n w) 16384)
#define HSK_LEVEL_P_SCALE 1024.0f    // P = rint(x 1024)
#define HSK_LEVEL_A_SCALE 4096.0     // an axis: A = rint(a 4096)
#define HSK_LEVEL_FACE 16            // the cube map: 6 faces of 16 x 16 bins
#define HSK_LEVEL_HIST_BINS (6 * HSK_LEVEL_FACE * HSK_LEVEL_FACE)
// U = (N . E1 + 2^18) >> 19: |U|, |V| <= 128 1.01 for a unit normal and U^2 + V^2 <= 3 2^16 1.001 for any valid one, so one point's
// |(U + iV)^4| = (U^2 + V^2)^2 is below 2^35.2 and the sums of 2^24 points below 2^59.2
#define HSK_LEVEL_YAW_SHIFT 19
// the height histograms: t_1 = P . R_1 counts 2^-22 m, a bin is t_1 >> 16 (1/64 m) + 8192; |t_1| >> 16 <= 7133
#define HSK_LEVEL_H_BINS 16384
#define HSK_LEVEL_H_SHIFT 16
#define HSK_LEVEL_H_ZERO 8192

struct LevelPoint {
  int N[3], P[3];
  bool valid;
};

// the six numbers finite and within their bounds (a NaN fails every comparison), and N not zero; an invalid point's integers are 0
HSK_HD LevelPoint level_point(float x, float y, float z, float nx, float ny, float nz, float wx, float wy, float wz) {
  const bool ok = (fabsf(x) <= HSK_LEVEL_REACH_M) & (fabsf(y) <= HSK_LEVEL_REACH_M) & (fabsf(z) <= HSK_LEVEL_REACH_M) &
                  (fabsf(nx) <= HSK_LEVEL_N_MAX) & (fabsf(ny) <= HSK_LEVEL_N_MAX) & (fabsf(nz) <= HSK_LEVEL_N_MAX);
  LevelPoint q;
  q.N[0] = (int)rintf(((ok ? nx : 0.0f) * wx) * HSK_LEVEL_N_SCALE);
  q.N[1] = (int)rintf(((ok ? ny : 0.0f) * wy) * HSK_LEVEL_N_SCALE);
  q.N[2] = (int)rintf(((ok ? nz : 0.0f) * wz) * HSK_LEVEL_N_SCALE);
  q.valid = ok & ((q.N[0] | q.N[1] | q.N[2]) != 0);
  q.P[0] = (int)rintf((q.valid ? x : 0.0f) * HSK_LEVEL_P_SCALE);
  q.P[1] = (int)rintf((q.valid ? y : 0.0f) * HSK_LEVEL_P_SCALE);
  q.P[2] = (int)rintf((q.valid ? z : 0.0f) * HSK_LEVEL_P_SCALE);
  return q;
}

HSK_HD int level_abs_i(int v) { return v < 0 ? -v : v; }

// the cube-map bin of a valid point's N: m = argmax |N_k| (the lowest k of equals), face 2 m + (N_m < 0), then the two other
// components, each (N_a 16 + |N_m| 16) / (2 |N_m|) cut at 15 -- a floor division of non-negative numbers
HSK_HD int level_hist_bin(const int N[3]) {
  const int a0 = level_abs_i(N[0]), a1 = level_abs_i(N[1]), a2 = level_abs_i(N[2]);
  int m = 0, nm = a0;
  if (a1 > nm) m = 1, nm = a1;
  if (a2 > nm) m = 2, nm = a2;
  const int na = N[m == 2 ? 0 : m + 1], nb = N[m == 0 ? 2 : m - 1];  // (m + 1) % 3, (m + 2) % 3
  const int f = 2 * m + (N[m] < 0 ? 1 : 0);
  const int den = nm > 0 ? 2 * nm : 1;  // (N = 0 belongs to no valid point; its bin is not used)
  const int i = hsk_min_i((na * HSK_LEVEL_FACE + nm * HSK_LEVEL_FACE) / den, HSK_LEVEL_FACE - 1);
  const int j = hsk_min_i((nb * HSK_LEVEL_FACE + nm * HSK_LEVEL_FACE) / den, HSK_LEVEL_FACE - 1);
  return (f * HSK_LEVEL_FACE + j) * HSK_LEVEL_FACE + i;
}

HSK_HD long long level_dot(const int a[3], const int b[3]) {
  return ((long long)a[0] * b[0] + (long long)a[1] * b[1]) + (long long)a[2] * b[2];
}

// the cone tests of N against the axis A: dot = N . A; supporter: (double)(dot^2) >= c2 (double)(|N|^2 |A|^2); wall point: <= with
// the squared sine in c2
HSK_HD bool level_cone(const int N[3], const int A[3], long long aa, double c2, bool inside, long long& dot) {
  dot = level_dot(N, A);
  const double lhs = (double)(dot * dot), rhs = c2 * (double)(level_dot(N, N) * aa);
  return inside ? lhs >= rhs : lhs <= rhs;
}

// what a wall point adds to the yaw's two sums: the real and the imaginary part of (U + iV)^4
HSK_HD void level_yaw_terms(const int N[3], const int E1[3], const int E2[3], long long& re, long long& im) {
  const long long half = 1ll << (HSK_LEVEL_YAW_SHIFT - 1);
  const long long U = (level_dot(N, E1) + half) >> HSK_LEVEL_YAW_SHIFT, V = (level_dot(N, E2) + half) >> HSK_LEVEL_YAW_SHIFT;
  const long long U2 = U * U, V2 = V * V;
  re = (U2 * U2 - 6 * U2 * V2) + V2 * V2;
  im = 4 * U * V * (U2 - V2);
}

// a levelled coordinate in units of 2^-22 m, and its bin of the height histograms
HSK_HD int level_t(const int P[3], const int R[3]) { return (int)level_dot(P, R); }
// (the cut never acts on an axis of |R|^2 <= 4100^2, which is all the ABI lets through: it keeps the index inside whatever comes)
HSK_HD int level_height_bin(int t1) {
  return hsk_max_i(0, hsk_min_i((t1 >> HSK_LEVEL_H_SHIFT) + HSK_LEVEL_H_ZERO, HSK_LEVEL_H_BINS - 1));
}
