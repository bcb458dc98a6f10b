// hsk_normal_point.h -- cloud normals, the work on ONE point (DESIGN.md 8v the rule, 3.28 the kernels): is the point valid, its
// coordinates on the q grid of hsk_plane_point.h, the cell of the neighbour search and its key, what a neighbour adds to the
// sums, and the solve -- matrix, eigenvectors, class, normal, orientation, curvature.  normals.hip's kernels call it per lane;
// plain C++ with no HIP type in it, so that tests/normal_point_harness.cpp compiles the same text for the host and
// tests/test_normals_host.py compares it with the numpy twin (tests/normals_twin.py) bit for bit, without a GPU.
// hsk_normal_solve (the ABI's host mirror of one point's solve) is normal_solve below.
//
// Every sum is an integer, so the order the neighbours arrive in is free.  The solve is binary64, one rounding per written
// operator (every build forbids contraction), in the order written here; the eigenvectors are hsk_simplify_point.h's rational
// Jacobi rotation, used as it stands.  Every comparison is written so that a NaN fails it.
#pragma once
#include <math.h>
#include <stddef.h>

#include "hsk_plane_point.h"
#include "hsk_simplify_point.h"

typedef long long normal_i64;

#define NORMAL_OK 0
#define NORMAL_INVALID 1
#define NORMAL_SPARSE 2
#define NORMAL_CROWDED 3
#define NORMAL_DEGENERATE 4
#define NORMAL_CLASSES 5
#define NORMAL_SUMS 10            // m, S_x S_y S_z, S_xx S_xy S_xz S_yy S_yz S_zz
#define NORMAL_Q_BIAS (1 << 18)   // |q| <= 2^18: q + 2^18 is no negative number
#define NORMAL_MIN_RQ 4           // radius_m in [1 / 1024, 0.25] on the q grid
#define NORMAL_MAX_RQ 1024
#define NORMAL_MAX_NEIGHBOURS (1 << 20)
#define NORMAL_KEY_BITS 21        // a cell coordinate is at most 2^19 / 4 = 2^17: three of them in 63 bits
#define NORMAL_KEY_EMPTY 0xFFFFFFFFFFFFFFFFull  // no key: a key's top bit is 0

// ---- the overflow arithmetic of the matrix --------------------------------------------------------------------
// A neighbour has |dq| <= r_q <= 2^10 per axis, and a point that is solved has m <= 2^20 of them: |S_a| <= 2^30, |S_ab| <= 2^40,
// m S_ab <= 2^60 and S_a S_b <= 2^60, so N_ab = m S_ab - S_a S_b lies within +-2^61.  A CROWDED lane stops at m = max + 1 <=
// 2^20 + 1 and its sums (< 2^41) are never multiplied.
static_assert((long long)NORMAL_MAX_NEIGHBOURS * NORMAL_MAX_RQ * NORMAL_MAX_RQ == (1LL << 40), "|S_ab| <= 2^40");
static_assert((long long)NORMAL_MAX_NEIGHBOURS * ((long long)NORMAL_MAX_NEIGHBOURS * NORMAL_MAX_RQ * NORMAL_MAX_RQ) == (1LL << 60), "m S_ab <= 2^60");
static_assert(3 * NORMAL_KEY_BITS < 64 && ((2 * NORMAL_Q_BIAS) / NORMAL_MIN_RQ) < (1 << NORMAL_KEY_BITS), "three cell coordinates fit a key below its top bit");

// the three coordinates finite and within reach (a NaN and an infinity fail the comparison)
HSK_HD bool normal_point_valid(float x, float y, float z) {
  return (fabsf(x) <= HSK_PLANE_REACH_M) & (fabsf(y) <= HSK_PLANE_REACH_M) & (fabsf(z) <= HSK_PLANE_REACH_M);
}
// the radius on the q grid: 4 .. 1024 for a radius_m in its range
HSK_HD int normal_radius_q(float radius_m) { return (int)rintf(radius_m * HSK_PLANE_Q_SCALE); }
// the cell of a coordinate q of a valid point, cells of edge r_q: q + 2^18 is not negative, so the division is plain
HSK_HD unsigned normal_cell(int q, int r_q) { return (unsigned)(q + NORMAL_Q_BIAS) / (unsigned)r_q; }
// the largest cell coordinate there is at this radius
HSK_HD unsigned normal_cell_max(int r_q) { return (unsigned)(2 * NORMAL_Q_BIAS) / (unsigned)r_q; }
HSK_HD unsigned long long normal_key(unsigned cx, unsigned cy, unsigned cz) {
  return (unsigned long long)cx | ((unsigned long long)cy << NORMAL_KEY_BITS) | ((unsigned long long)cz << (2 * NORMAL_KEY_BITS));
}
// where a key's probe starts in a table of mask + 1 slots (a power of two): a 64-bit mix, so that the lattice of a scan's cells
// does not walk the table in step
HSK_HD unsigned normal_hash(unsigned long long key, unsigned mask) {
  key ^= key >> 33;
  key *= 0xff51afd7ed558ccdull;
  key ^= key >> 33;
  key *= 0xc4ceb9fe1a85ec53ull;
  key ^= key >> 33;
  return (unsigned)key & mask;
}

// point j (at q_j = q_i + d) offered to point i's sums: a neighbour when |d|^2 <= r_q^2, the boundary included, in integers
// (|d| per axis is at most 2^20, the square sum fits 64 bits with room); true: it was one and s took it
HSK_HD bool normal_add(normal_i64* s, int dx, int dy, int dz, normal_i64 r2) {
  const normal_i64 x = dx, y = dy, z = dz;
  if (!(x * x + y * y + z * z <= r2)) return false;
  s[0] += 1;
  s[1] += x;
  s[2] += y;
  s[3] += z;
  s[4] += x * x;
  s[5] += x * y;
  s[6] += x * z;
  s[7] += y * y;
  s[8] += y * z;
  s[9] += z * z;
  return true;
}

// the class the neighbour count alone decides, or NORMAL_OK: the point is solved
HSK_HD int normal_count_class(normal_i64 m, unsigned min_neighbours, unsigned max_neighbours) {
  return m < (normal_i64)min_neighbours ? NORMAL_SPARSE : (m > (normal_i64)max_neighbours ? NORMAL_CROWDED : NORMAL_OK);
}

// the sign rule without a viewpoint (house.cpp's convention): the component of largest magnitude positive, the lowest index on a tie
HSK_HD bool normal_flip_by_axis(const double* n) {
  int k = 0;
  if (fabs(n[1]) > fabs(n[k])) k = 1;
  if (fabs(n[2]) > fabs(n[k])) k = 2;
  return n[k] < 0.0;
}

// The solve of a point p with 1 <= m <= 2^20 neighbours from its ten sums, taken relative to q_p: NORMAL_OK with the unit normal
// and the surface variation, or NORMAL_DEGENERATE (no plane: a collinear or coincident neighbourhood) with zeros.  viewpoints: 3
// floats each, nv of them (0: none); the nearest one to p (the lowest index on a tie) turns the normal towards itself.
HSK_HD int normal_solve(const normal_i64* s, float px, float py, float pz, const float* viewpoints, size_t nv, float line_rel, float* normal,
                        float* curvature) {
  normal[0] = normal[1] = normal[2] = 0.0f;
  *curvature = 0.0f;
  const normal_i64 m = s[0];
  // N_ab = m S_ab - S_a S_b: within +-2^61 (above), exact
  const normal_i64 nxx = m * s[4] - s[1] * s[1], nxy = m * s[5] - s[1] * s[2], nxz = m * s[6] - s[1] * s[3];
  const normal_i64 nyy = m * s[7] - s[2] * s[2], nyz = m * s[8] - s[2] * s[3], nzz = m * s[9] - s[3] * s[3];
  double a[3][3] = {{(double)nxx, (double)nxy, (double)nxz}, {(double)nxy, (double)nyy, (double)nyz}, {(double)nxz, (double)nyz, (double)nzz}};
  double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < SIMP_SWEEPS; ++sweep) {
    simp_rotate(a, v, 0, 1);
    simp_rotate(a, v, 0, 2);
    simp_rotate(a, v, 1, 2);
  }
  const double e[3] = {a[0][0], a[1][1], a[2][2]};
  // i0: the smallest, the first on a tie; i2: the larger of the other two, the first on a tie; i1: what is left
  int i0 = 0;
  if (e[1] < e[i0]) i0 = 1;
  if (e[2] < e[i0]) i0 = 2;
  const int ja = i0 == 0 ? 1 : 0, jb = i0 == 2 ? 1 : 2;
  const int i2 = e[jb] > e[ja] ? jb : ja, i1 = ja + jb - i2;
  const double l0 = e[i0] < 0.0 ? 0.0 : e[i0];
  if (!(e[i1] > (double)line_rel * e[i2])) return NORMAL_DEGENERATE;
  const double v0 = v[0][i0], v1 = v[1][i0], v2 = v[2][i0];
  const double inv = 1.0 / sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  double n[3] = {v0 * inv, v1 * inv, v2 * inv};
  bool flip;
  if (nv == 0) {
    flip = normal_flip_by_axis(n);
  } else {
    double best_d2 = 0.0, d[3] = {0.0, 0.0, 0.0};
    for (size_t w = 0; w < nv; ++w) {
      const double dx = (double)viewpoints[3 * w] - (double)px, dy = (double)viewpoints[3 * w + 1] - (double)py,
                   dz = (double)viewpoints[3 * w + 2] - (double)pz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (w == 0 || d2 < best_d2) best_d2 = d2, d[0] = dx, d[1] = dy, d[2] = dz;
    }
    const double sgn = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    flip = sgn < 0.0 ? true : (sgn == 0.0 ? normal_flip_by_axis(n) : false);
  }
  if (flip) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
  normal[0] = (float)n[0];
  normal[1] = (float)n[1];
  normal[2] = (float)n[2];
  *curvature = (float)(l0 / ((l0 + e[i1]) + e[i2]));
  return NORMAL_OK;
}
