// hsk_simplify_point.h -- the simplified mesh (DESIGN.md 8k the rule, 3.17 the kernels): what the kernels of simplify.hip and
// the host share -- the quantised vertex of a cut edge, the sums of a vertex and of a triangle, the colour pick, and the
// representative vertex of a cluster (a cyclic Jacobi of a fixed number of sweeps and the pseudo-inverse step), with its
// clamp, its way to metres, its normal and its colour.  Plain C++ with no HIP type in it: tests/simplify_point_harness.cpp
// compiles the same text for the host, simplifies a volume sequentially, and tests/test_simplify_host.py compares it with the
// numpy twin (tests/simplify_twin.py) -- every sum, every vertex, normal, colour and face.  hsk_cluster_vertex (the ABI's host
// mirror of the device solve) is simp_vertex below.
//
// Every sum is an integer (no float enters one), so the order they are taken in is free.  The solve is binary64, one rounding
// per written operator (every build forbids contraction), in the order written here, with + - x / sqrt only: do not
// re-associate it.  With anisotropic cells the error that is minimised is the GRID's (distances in voxels), not the metric one.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hsk_sample.h"

typedef long long simp_i64;

#define SIMP_UNIT 256     // positions are integers in units of 1 / 256 voxel
#define SIMP_SUMS 16      // n, sum p (3), sum N (3), sum N N^T (xx xy xz yy yz zz), sum N dN (3)
#define SIMP_REC 20       // ... and behind them sum r, sum g, sum b and the count of the coloured vertices
#define SIMP_SWEEPS 8     // cyclic Jacobi sweeps of the 3 x 3 solve, always all of them
#define SIMP_MAX_CLUSTER 16

// ---- the overflow arithmetic of the sums, for the largest cluster c = 16 -------------------------------------
// Positions are taken relative to the centre of the cluster's cell.  A triangle that touches the cluster lies in one of the
// (c + 1)^3 cubes from one cube below the cell on every axis, so its coordinates lie in [-128 c - 256, 128 c]: |p| <= 2304.
// The two edge vectors lie inside one cube, |d| <= 256 per component, so |N_i| <= 2 * 256^2 = 2^17; |dN| = |N . p0| <=
// 3 * 2^17 * 2304 < 2^30; at most 5 (c + 1)^3 = 24565 triangles: |sum N_i dN| <= 24565 * 2^17 * 3 * 2^17 * 2304 < 2^61.4.
// The other sums are smaller (sum N_i N_j < 2^49, sum p < 2^24).  Everything fits 64 bits signed: no cluster size is refused.
#define SIMP_MAX_COORD (128 * SIMP_MAX_CLUSTER + 256)
#define SIMP_MAX_N (2LL * SIMP_UNIT * SIMP_UNIT)
#define SIMP_MAX_TRIANGLES (5LL * (SIMP_MAX_CLUSTER + 1) * (SIMP_MAX_CLUSTER + 1) * (SIMP_MAX_CLUSTER + 1))
static_assert(SIMP_MAX_N == (1LL << 17), "|N_i| <= 2^17");
static_assert(3LL * SIMP_MAX_N * SIMP_MAX_COORD < (1LL << 30), "|dN| < 2^30");
static_assert(SIMP_MAX_TRIANGLES < (1LL << 15), "at most 2^15 triangles touch a cluster");
// (the product's factors one after the other, each step checked against what is left of 2^63 - 1)
static_assert(SIMP_MAX_TRIANGLES * SIMP_MAX_N <= INT64_MAX / (3LL * SIMP_MAX_N * SIMP_MAX_COORD), "sum N dN fits an int64 at c = 16");
static_assert(SIMP_MAX_TRIANGLES * SIMP_MAX_N * (3LL * SIMP_MAX_N * SIMP_MAX_COORD) < (1LL << 62), "... with a bit to spare");

// log2 of a legal cluster size, -1 for any other
HSK_HD int simp_shift(int c) { return c == 2 ? 1 : (c == 4 ? 2 : (c == 8 ? 3 : (c == 16 ? 4 : -1))); }

// where the zero crossing lies on the edge from the LOWER corner (stored TSDF fa) to the upper (fb), in 1 / 256 of the edge:
// round(256 |fa| / D), D = |fb - fa| > 0 (the ends of a cut edge differ in sign), halves up, in integers: 0 .. 256
HSK_HD int simp_q(int fa, int fb) {
  const int a = fa < 0 ? -fa : fa, d = fb > fa ? fb - fa : fa - fb;
  return (512 * a + d) / (2 * d);
}

// the inside mask of a cube from its eight pair words (x fastest): 0 when a corner was never observed or nothing is cut
HSK_HD unsigned simp_m8(const unsigned* w) {
  unsigned m8 = 0u;
  bool ok = true;
  for (int c = 0; c < 8; ++c) {
    ok = ok && hsk_pair_wgt(w[c]) != 0;
    m8 |= (hsk_pair_raw(w[c]) < 0 ? 1u : 0u) << c;
  }
  return (!ok || m8 == 255u) ? 0u : m8;
}
// an edge code (lower corner | upper corner << 4): its lower corner, and its axis from b ^ a (1, 2 or 4)
HSK_HD int simp_code_low(unsigned code) { return (int)(code & 15u); }
HSK_HD int simp_code_axis(unsigned code) {
  const int ab = (int)((code >> 4) ^ code) & 7;
  return ab == 1 ? 0 : (ab == 2 ? 1 : 2);
}
// the raw TSDF of corner c of the eight words, without an indexed array (a kernel keeps the words in registers)
HSK_HD int simp_corner_raw(const unsigned* w, int c) {
  unsigned v = 0u;
  for (int i = 0; i < 8; ++i) v = i == c ? w[i] : v;
  return hsk_pair_raw(v);
}

// the indexed mesh's colour selection on an edge (extract.hip: attr_color): the word of the end with the smaller |tsdf| (the
// lower corner a on a tie), of the other end when that one has colour weight 0; 0 when neither has
HSK_HD unsigned simp_color_pick(int ta, int tb, unsigned ca, unsigned cb) {
  const bool take_a = (ta < 0 ? -ta : ta) <= (tb < 0 ? -tb : tb);
  unsigned cw = take_a ? ca : cb;
  if ((cw >> 24) == 0u) cw = take_a ? cb : ca;
  return (cw >> 24) == 0u ? 0u : cw;
}

// the position of the vertex of the edge (lower corner g, axis, TSDF fa -> fb) relative to the centre of the cell of edge c
// whose first voxel is `base`, in units of 1 / 256 voxel
HSK_HD void simp_position(const int* g, int axis, int fa, int fb, const int* base, int c, simp_i64* p) {
  const int q = simp_q(fa, fb);
  for (int i = 0; i < 3; ++i) p[i] = (simp_i64)SIMP_UNIT * (g[i] - base[i]) - (SIMP_UNIT / 2) * c + (i == axis ? q : 0);
}
// one vertex of the cluster into its record: the count and the position sums, and its colour word (0: uncoloured or no colour)
HSK_HD void simp_add_vertex(simp_i64* rec, const simp_i64* p, unsigned cw) {
  rec[0] += 1;
  rec[1] += p[0];
  rec[2] += p[1];
  rec[3] += p[2];
  if ((cw >> 24) != 0u) {
    rec[16] += (simp_i64)(cw & 255u);
    rec[17] += (simp_i64)((cw >> 8) & 255u);
    rec[18] += (simp_i64)((cw >> 16) & 255u);
    rec[19] += 1;
  }
}
// one triangle that touches the cluster (once per cluster): N = (p1 - p0) x (p2 - p0), twice the area times the normal in
// the soup's winding, dN = N . p0
HSK_HD void simp_add_triangle(simp_i64* rec, const simp_i64* p0, const simp_i64* p1, const simp_i64* p2) {
  const simp_i64 u0 = p1[0] - p0[0], u1 = p1[1] - p0[1], u2 = p1[2] - p0[2];
  const simp_i64 v0 = p2[0] - p0[0], v1 = p2[1] - p0[1], v2 = p2[2] - p0[2];
  const simp_i64 n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
  const simp_i64 dn = n0 * p0[0] + n1 * p0[1] + n2 * p0[2];
  rec[4] += n0;
  rec[5] += n1;
  rec[6] += n2;
  rec[7] += n0 * n0;
  rec[8] += n0 * n1;
  rec[9] += n0 * n2;
  rec[10] += n1 * n1;
  rec[11] += n1 * n2;
  rec[12] += n2 * n2;
  rec[13] += n0 * dn;
  rec[14] += n1 * dn;
  rec[15] += n2 * dn;
}

// one Jacobi rotation of the symmetric a that annihilates a[p][q], accumulated into the eigenvector columns of v: the
// rational formulas (Rutishauser), no trigonometry
HSK_HD void simp_rotate(double a[3][3], double v[3][3], int p, int q) {
  const double apq = a[p][q];
  if (apq != 0.0) {
    const int r = 3 - p - q;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double mag = theta < 0.0 ? -theta : theta;
    double t = 1.0 / (mag + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double app = a[p][p] - t * apq, aqq = a[q][q] + t * apq;
    const double arp = c * a[r][p] - s * a[r][q], arq = s * a[r][p] + c * a[r][q];
    a[p][p] = app;
    a[q][q] = aqq;
    a[p][q] = a[q][p] = 0.0;
    a[r][p] = a[p][r] = arp;
    a[r][q] = a[q][r] = arq;
    for (int k = 0; k < 3; ++k) {
      const double vkp = c * v[k][p] - s * v[k][q], vkq = s * v[k][p] + c * v[k][q];
      v[k][p] = vkp;
      v[k][q] = vkq;
    }
  }
}

// The representative vertex of a cluster of edge c from its 16 sums (n >= 1), relative to the centre of its cell in units of
// 1 / 256 voxel.  mode != 0 (HSK_SIMPLIFY_MEAN): the mean, rank 0.  Else the mean moved by the pseudo-inverse of A = sum N N^T
// applied to b - A mean, over the eigenvalues above floor * the largest; *rank the eigenvalues kept.  Then clamped to the cell
// grown by one voxel on every side; *clamped: a coordinate was moved by the clamp.
HSK_HD void simp_vertex(const simp_i64* s, int c, int mode, double floor_rel, double* x, int* rank, int* clamped) {
  const double n = (double)s[0];
  const double m[3] = {(double)s[1] / n, (double)s[2] / n, (double)s[3] / n};
  x[0] = m[0], x[1] = m[1], x[2] = m[2];
  *rank = 0;
  *clamped = 0;
  if (mode != 0) return;
  const double A[3][3] = {{(double)s[7], (double)s[8], (double)s[9]}, {(double)s[8], (double)s[10], (double)s[11]}, {(double)s[9], (double)s[11], (double)s[12]}};
  double a[3][3], v[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a[i][j] = A[i][j], v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SIMP_SWEEPS; ++sweep) {
    simp_rotate(a, v, 0, 1);
    simp_rotate(a, v, 0, 2);
    simp_rotate(a, v, 1, 2);
  }
  double r[3];
  for (int k = 0; k < 3; ++k) r[k] = (double)s[13 + k] - ((A[k][0] * m[0] + A[k][1] * m[1]) + A[k][2] * m[2]);
  double lmax = a[0][0];
  lmax = a[1][1] > lmax ? a[1][1] : lmax;
  lmax = a[2][2] > lmax ? a[2][2] : lmax;
  if (lmax > 0.0) {
    const double cut = floor_rel * lmax;
    for (int i = 0; i < 3; ++i) {
      if (!(a[i][i] > cut)) continue;
      const double coef = ((v[0][i] * r[0] + v[1][i] * r[1]) + v[2][i] * r[2]) / a[i][i];
      x[0] = x[0] + v[0][i] * coef;
      x[1] = x[1] + v[1][i] * coef;
      x[2] = x[2] + v[2][i] * coef;
      *rank += 1;
    }
  }
  const double lim = (double)((SIMP_UNIT / 2) * c + SIMP_UNIT);
  for (int k = 0; k < 3; ++k) {
    if (x[k] > lim) x[k] = lim, *clamped = 1;
    if (x[k] < -lim) x[k] = -lim, *clamped = 1;
  }
}

// x (simp_vertex) of cluster cl (its index on each axis) in metres: the grid-to-metre map of the soup's vertices, a voxel's
// centre at (g + 0.5) cell, in binary64 and rounded once to binary32
HSK_HD void simp_metres(const double* x, int c, const int* cl, const float* cell, float* out) {
  for (int k = 0; k < 3; ++k) {
    const double pv = (double)(c * cl[k] + c / 2) + x[k] / (double)SIMP_UNIT;
    out[k] = (float)((pv + 0.5) * (double)cell[k]);
  }
}
// the cluster's normal: sum N taken to metric space (a covector: each component over its axis's cell) and scaled to length 1 in
// binary64; false (the caller writes NaN x 3) where sum N = 0
HSK_HD bool simp_normal(const simp_i64* s, const float* cell, float* out) {
  if (s[4] == 0 && s[5] == 0 && s[6] == 0) return false;
  const double n0 = (double)s[4] / (double)cell[0], n1 = (double)s[5] / (double)cell[1], n2 = (double)s[6] / (double)cell[2];
  const double inv = 1.0 / sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  out[0] = (float)(n0 * inv);
  out[1] = (float)(n1 * inv);
  out[2] = (float)(n2 * inv);
  return true;
}
// the cluster's colour: the rounded mean of its coloured vertices per channel; false (and (0, 0, 0)) when it has none
HSK_HD bool simp_rgb(const simp_i64* rec, unsigned char* out) {
  const simp_i64 nc = rec[19];
  for (int k = 0; k < 3; ++k) out[k] = nc > 0 ? (unsigned char)((rec[16 + k] + nc / 2) / nc) : (unsigned char)0;
  return nc > 0;
}

// ---- a cube's triangles (Table: the marching-cubes table, ntri[256] and edge[256][5][3] of edge codes) ----------------------
// the lower corner of the edge `code` of the cube at (x, y, z)
HSK_HD void simp_edge_corner(unsigned code, int x, int y, int z, int* g) {
  const int a = simp_code_low(code);
  g[0] = x + (a & 1);
  g[1] = y + ((a >> 1) & 1);
  g[2] = z + (a >> 2);
}
// the clusters (shift s, CX x CY clusters per plane) of a triangle's three corners; true: all three differ -- the face survives
HSK_HD bool simp_face_clusters(const unsigned char* codes, int x, int y, int z, int s, int CX, int CY, unsigned* ids) {
  for (int q = 0; q < 3; ++q) {
    int g[3];
    simp_edge_corner(codes[q], x, y, z, g);
    ids[q] = (unsigned)(((g[2] >> s) * CY + (g[1] >> s)) * CX + (g[0] >> s));
  }
  return ids[0] != ids[1] && ids[0] != ids[2] && ids[1] != ids[2];
}
// the triangles of the cube at (x, y, z) (its eight words w, its mask m8) with a corner in cluster cl (shift s): their sums
// into rec, each triangle once
template <class Table>
HSK_HD void simp_cube_triangles(const Table& ct, const unsigned* w, unsigned m8, int x, int y, int z, int s, const int* cl, simp_i64* rec) {
  const int c = 1 << s, base[3] = {cl[0] << s, cl[1] << s, cl[2] << s};
  const int nt = m8 ? (int)ct.ntri[m8] : 0;
  for (int t = 0; t < nt; ++t) {
    simp_i64 p[3][3];
    bool touches = false;
    for (int q = 0; q < 3; ++q) {
      const unsigned code = ct.edge[m8][t][q];
      int g[3];
      simp_edge_corner(code, x, y, z, g);
      touches = touches || ((g[0] >> s) == cl[0] && (g[1] >> s) == cl[1] && (g[2] >> s) == cl[2]);
      simp_position(g, simp_code_axis(code), simp_corner_raw(w, simp_code_low(code)), simp_corner_raw(w, (int)(code >> 4)), base, c, p[q]);
    }
    if (touches) simp_add_triangle(rec, p[0], p[1], p[2]);
  }
}
