// products.cpp -- products on the file seam between KinFu and HouseScan (host-only):
//   <room>/cloud_bin.pcd, <room>/cloud_downsampled.pcd  -- read by loadRoom / cloudFromFile
//   (housescan/Main.hs:1738-1762, :1334-1345 via PCD.loadXyz :1320-1323; printed at :2437).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/hskinfu.h"

// binary PCD v0.7 with float32 x y z, the layout pcd-loader's loadXyz expects
extern "C" int hsk_write_pcd_xyz(const char* path, const float* xyz, size_t n) {
  if (!path || (!xyz && n)) return HSK_ERR_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) return HSK_ERR_STATE;
  fprintf(f,
          "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
          "WIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n",
          n, n);
  const size_t wrote = n ? fwrite(xyz, 12, n, f) : 0;
  const int rc = fclose(f);
  return (wrote == n && rc == 0) ? HSK_OK : HSK_ERR_STATE;
}

// Scene views on the file seam (hsk_render_view): binary PPM (P6, 8-bit RGB) and binary PGM (P5, maxval 65535: 16-bit samples,
// most significant byte first -- the depth image in millimetres, readable by any Netpbm tool).  Sizes as hsk_render_view's.
extern "C" int hsk_write_ppm(const char* path, const uint8_t* rgb, int w, int h) {
  if (!path || !rgb || w < 1 || h < 1 || w > 4096 || h > 4096) return HSK_ERR_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) return HSK_ERR_STATE;
  fprintf(f, "P6\n%d %d\n255\n", w, h);
  const size_t n = (size_t)w * h;
  const size_t wrote = fwrite(rgb, 3, n, f);
  const int rc = fclose(f);
  return (wrote == n && rc == 0) ? HSK_OK : HSK_ERR_STATE;
}
extern "C" int hsk_write_pgm16(const char* path, const uint16_t* depth_mm, int w, int h) {
  if (!path || !depth_mm || w < 1 || h < 1 || w > 4096 || h > 4096) return HSK_ERR_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) return HSK_ERR_STATE;
  fprintf(f, "P5\n%d %d\n65535\n", w, h);
  std::vector<uint8_t> row((size_t)w * 2);
  bool ok = true;
  for (int y = 0; y < h && ok; ++y) {
    for (int x = 0; x < w; ++x) {
      const uint16_t d = depth_mm[(size_t)y * w + x];
      row[2 * x] = (uint8_t)(d >> 8);
      row[2 * x + 1] = (uint8_t)(d & 255);
    }
    ok = fwrite(row.data(), 2, (size_t)w, f) == (size_t)w;
  }
  const int rc = fclose(f);
  return (ok && rc == 0) ? HSK_OK : HSK_ERR_STATE;
}

// binary PCD v0.7 with x y z rgb normal_x normal_y normal_z curvature, 32 B per point: the coloured form of HouseScan's cloud
// loader (Main.hs:1325-1345: XYZ first, then XYZ + RGB + normal).  rgb is PCL's packed colour, the bit pattern 0x00RRGGBB
// stored in a float field; curvature 0.  (Unverified against pcd-loader's loadXyzRgbNormal itself: it is not available here.)
extern "C" int hsk_write_pcd_xyzrgbnormal(const char* path, const float* xyz, const uint8_t* rgb, const float* normals, size_t n) {
  if (!path || (n && (!xyz || !rgb))) return HSK_ERR_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) return HSK_ERR_STATE;
  fprintf(f,
          "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb normal_x normal_y normal_z curvature\n"
          "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\n"
          "WIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n",
          n, n);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<uint32_t> rec(8 * 4096);
  size_t wrote = 0;
  for (size_t i0 = 0; i0 < n; i0 += 4096) {
    const size_t m = n - i0 < 4096 ? n - i0 : 4096;
    for (size_t j = 0; j < m; ++j) {
      const size_t i = i0 + j;
      uint32_t* r = &rec[8 * j];
      float nrm[3] = {nan, nan, nan};
      if (normals) memcpy(nrm, normals + 3 * i, 12);
      memcpy(r, xyz + 3 * i, 12);
      r[3] = ((uint32_t)rgb[3 * i] << 16) | ((uint32_t)rgb[3 * i + 1] << 8) | (uint32_t)rgb[3 * i + 2];
      memcpy(r + 4, nrm, 12);
      r[7] = 0u;  // curvature 0.0f
    }
    wrote += fwrite(rec.data(), 32, m, f);
  }
  const int rc = fclose(f);
  return (wrote == n && rc == 0) ? HSK_OK : HSK_ERR_STATE;
}

// voxel-grid centroid downsample with attributes: leaves keyed by floor(p / leaf), ordered by key (then by point), the
// centroid in binary64; the mean colour, rounded half up, and the renormalised mean of the leaf's non-NaN normals
extern "C" int hsk_voxel_downsample_attrs(const float* xyz, const uint8_t* rgb, const float* normals, size_t n, float leaf, float* out_xyz,
                                          uint8_t* out_rgb, float* out_normals, size_t cap, size_t* n_out) {
  if (!n_out || (!xyz && n) || !(leaf > 0.0f)) return HSK_ERR_ARG;
  struct Item {
    uint64_t key;
    uint32_t idx;
  };
  std::vector<Item> items;
  items.reserve(n);
  const float inv = 1.0f / leaf;
  for (size_t i = 0; i < n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (!(x == x) || !(y == y) || !(z == z)) continue;
    const int64_t ix = (int64_t)std::floor(x * inv) + (1 << 20);
    const int64_t iy = (int64_t)std::floor(y * inv) + (1 << 20);
    const int64_t iz = (int64_t)std::floor(z * inv) + (1 << 20);
    if (ix < 0 || iy < 0 || iz < 0 || ix >= (1 << 21) || iy >= (1 << 21) || iz >= (1 << 21)) continue;
    items.push_back(Item{((uint64_t)iz << 42) | ((uint64_t)iy << 21) | (uint64_t)ix, (uint32_t)i});
  }
  std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.key != b.key ? a.key < b.key : a.idx < b.idx; });
  const float nan = std::numeric_limits<float>::quiet_NaN();
  size_t m = 0;
  for (size_t i = 0; i < items.size();) {
    size_t j = i;
    double sx = 0, sy = 0, sz = 0, nx = 0, ny = 0, nz = 0;
    uint64_t cr = 0, cg = 0, cb = 0;
    size_t nn = 0;
    while (j < items.size() && items[j].key == items[i].key) {
      const size_t q = items[j].idx;
      sx += xyz[3 * q];
      sy += xyz[3 * q + 1];
      sz += xyz[3 * q + 2];
      if (rgb) {
        cr += rgb[3 * q];
        cg += rgb[3 * q + 1];
        cb += rgb[3 * q + 2];
      }
      if (normals) {
        const float a = normals[3 * q], b = normals[3 * q + 1], c = normals[3 * q + 2];
        if (a == a && b == b && c == c) {
          nx += a;
          ny += b;
          nz += c;
          ++nn;
        }
      }
      ++j;
    }
    const double c = (double)(j - i);
    if (m < cap) {
      if (out_xyz) {
        out_xyz[3 * m] = (float)(sx / c);
        out_xyz[3 * m + 1] = (float)(sy / c);
        out_xyz[3 * m + 2] = (float)(sz / c);
      }
      if (rgb && out_rgb) {
        const uint64_t cnt = (uint64_t)(j - i);
        out_rgb[3 * m] = (uint8_t)((cr + cnt / 2) / cnt);
        out_rgb[3 * m + 1] = (uint8_t)((cg + cnt / 2) / cnt);
        out_rgb[3 * m + 2] = (uint8_t)((cb + cnt / 2) / cnt);
      }
      if (normals && out_normals) {
        const double len = std::sqrt(nx * nx + ny * ny + nz * nz);
        const bool ok = nn > 0 && len > 0.0;
        out_normals[3 * m] = ok ? (float)(nx / len) : nan;
        out_normals[3 * m + 1] = ok ? (float)(ny / len) : nan;
        out_normals[3 * m + 2] = ok ? (float)(nz / len) : nan;
      }
    }
    ++m;
    i = j;
  }
  *n_out = m;
  return HSK_OK;
}

// voxel-grid centroid downsample (what produces cloud_downsampled.pcd); output ordered by leaf index.  The attribute form's
// leaves with no attributes: one implementation, so that both give the same xyz by construction
extern "C" int hsk_voxel_downsample(const float* xyz, size_t n, float leaf, float* out, size_t cap, size_t* n_out) {
  return hsk_voxel_downsample_attrs(xyz, nullptr, nullptr, n, leaf, out, nullptr, nullptr, cap, n_out);
}

// ------------------------------------------------------------------------------------------------------
// Plane detection on the fused cloud: what HouseScan's loadRoom consumes beside the cloud --
//   <room>/planes.txt               one plane per line "a b c d" in PCL form ax + by + cz + d = 0
//                                   (parsed by planeEqsFromFile, housescan/Main.hs:1379-1389, which negates d)
//   <room>/cloud_plane_hull<k>.pcd  polygon vertices of plane k in drawing order (Main.hs:1395-1400, :758-763)
// Deterministic sequential RANSAC (fixed-seed LCG) + PCA refit + 2-D convex hull of the inliers.
// ------------------------------------------------------------------------------------------------------
namespace {
struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

// smallest-eigenvalue eigenvector of a symmetric 3x3 matrix (cyclic Jacobi)
void smallest_eigvec(double A[3][3], double n[3]) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 32; ++sweep) {
    double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
    if (off < 1e-30) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (std::fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int m = 0;
  if (A[1][1] < A[m][m]) m = 1;
  if (A[2][2] < A[m][m]) m = 2;
  for (int k = 0; k < 3; ++k) n[k] = V[k][m];
}
}  // namespace

// planes_abcd: up to max_planes x 4 floats (unit normal a,b,c and d of ax+by+cz+d=0); labels (optional, n ints):
// index of the plane a point was assigned to, or -1.  Planes are reported in detection order (largest first).
extern "C" int hsk_detect_planes(const float* xyz, size_t n, float dist_thresh, float min_fraction, int max_planes,
                                 int iterations, float* planes_abcd, int* labels, int* n_planes) {
  if (!xyz || !planes_abcd || !n_planes || max_planes <= 0 || !(dist_thresh > 0.0f) || iterations <= 0) return HSK_ERR_ARG;
  std::vector<int> lab(n, -1);
  std::vector<uint32_t> rest(n);
  for (size_t i = 0; i < n; ++i) rest[i] = (uint32_t)i;
  Lcg rng{0x9E3779B97F4A7C15ull};
  const size_t min_inl = (size_t)std::max(3.0, (double)min_fraction * (double)n);
  int found = 0;
  while (found < max_planes && rest.size() >= std::max<size_t>(min_inl, 3)) {
    // score candidates on a bounded subsample of the remaining points
    const size_t m = rest.size();
    const size_t stride = std::max<size_t>(1, m / 20000);
    double best_n[3] = {0, 0, 1}, best_d = 0;
    size_t best_cnt = 0;
    for (int it = 0; it < iterations; ++it) {
      const float* p0 = xyz + 3 * (size_t)rest[rng.next() % m];
      const float* p1 = xyz + 3 * (size_t)rest[rng.next() % m];
      const float* p2 = xyz + 3 * (size_t)rest[rng.next() % m];
      const double u[3] = {(double)p1[0] - p0[0], (double)p1[1] - p0[1], (double)p1[2] - p0[2]};
      const double v[3] = {(double)p2[0] - p0[0], (double)p2[1] - p0[1], (double)p2[2] - p0[2]};
      double nn[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
      const double len = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
      if (len < 1e-9) continue;
      for (double& c : nn) c /= len;
      const double d = -(nn[0] * p0[0] + nn[1] * p0[1] + nn[2] * p0[2]);
      size_t cnt = 0;
      for (size_t i = 0; i < m; i += stride) {
        const float* p = xyz + 3 * (size_t)rest[i];
        if (std::fabs(nn[0] * p[0] + nn[1] * p[1] + nn[2] * p[2] + d) <= dist_thresh) ++cnt;
      }
      if (cnt > best_cnt) {
        best_cnt = cnt;
        best_d = d;
        best_n[0] = nn[0];
        best_n[1] = nn[1];
        best_n[2] = nn[2];
      }
    }
    if (best_cnt * stride < min_inl) break;
    // refit twice by PCA on the inliers of the current estimate
    for (int pass = 0; pass < 2; ++pass) {
      double mean[3] = {0, 0, 0};
      size_t cnt = 0;
      for (uint32_t idx : rest) {
        const float* p = xyz + 3 * (size_t)idx;
        if (std::fabs(best_n[0] * p[0] + best_n[1] * p[1] + best_n[2] * p[2] + best_d) <= dist_thresh) {
          mean[0] += p[0];
          mean[1] += p[1];
          mean[2] += p[2];
          ++cnt;
        }
      }
      if (cnt < 3) break;
      for (double& c : mean) c /= (double)cnt;
      double C[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      for (uint32_t idx : rest) {
        const float* p = xyz + 3 * (size_t)idx;
        if (std::fabs(best_n[0] * p[0] + best_n[1] * p[1] + best_n[2] * p[2] + best_d) <= dist_thresh) {
          const double q[3] = {p[0] - mean[0], p[1] - mean[1], p[2] - mean[2]};
          for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) C[a][b] += q[a] * q[b];
        }
      }
      double nn[3];
      smallest_eigvec(C, nn);
      const double len = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
      if (len < 1e-12) break;
      for (int a = 0; a < 3; ++a) best_n[a] = nn[a] / len;
      best_d = -(best_n[0] * mean[0] + best_n[1] * mean[1] + best_n[2] * mean[2]);
    }
    // assign and remove the inliers
    std::vector<uint32_t> keep;
    keep.reserve(rest.size());
    size_t cnt = 0;
    for (uint32_t idx : rest) {
      const float* p = xyz + 3 * (size_t)idx;
      if (std::fabs(best_n[0] * p[0] + best_n[1] * p[1] + best_n[2] * p[2] + best_d) <= dist_thresh) {
        lab[idx] = found;
        ++cnt;
      } else {
        keep.push_back(idx);
      }
    }
    if (cnt < min_inl) {  // the refit lost the support: undo and stop
      for (int& l : lab)
        if (l == found) l = -1;
      break;
    }
    planes_abcd[4 * found + 0] = (float)best_n[0];
    planes_abcd[4 * found + 1] = (float)best_n[1];
    planes_abcd[4 * found + 2] = (float)best_n[2];
    planes_abcd[4 * found + 3] = (float)best_d;
    ++found;
    rest.swap(keep);
  }
  if (labels)
    for (size_t i = 0; i < n; ++i) labels[i] = lab[i];
  *n_planes = found;
  return HSK_OK;
}

// Oriented plane detection (include/hskinfu.h), the host's share of a round: the generator above for api_planes.hip
// (hsk_ctx.h declares it), and one refit from the inliers' integer moments -- the same Jacobi as the detector above.
uint32_t plane_lcg_next(uint64_t* state) {
  Lcg g{*state};
  const uint32_t v = g.next();
  *state = g.s;
  return v;
}

extern "C" int hsk_plane_refit(const int64_t sums10[10], const float prev_abcd[4], float out_abcd[4], int* ok) {
  if (!sums10 || !prev_abcd || !out_abcd || !ok) return HSK_ERR_ARG;
  const int64_t lim = (int64_t)1 << 62;
  if (sums10[0] < 0 || sums10[0] > ((int64_t)1 << 24)) return HSK_ERR_ARG;
  for (int i = 1; i < 10; ++i)
    if (sums10[i] < -lim || sums10[i] > lim) return HSK_ERR_ARG;
  *ok = 0;
  float prev[4];
  memcpy(prev, prev_abcd, sizeof(prev));  // (out_abcd may be prev_abcd)
  memcpy(out_abcd, prev, sizeof(prev));
  const int64_t m = sums10[0];
  if (m < 3) return HSK_OK;
  const int64_t* S = sums10 + 1;   // the sums of q
  const int64_t* SS = sums10 + 4;  // xx xy xz yy yz zz
  static const int at[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  const double mm = (double)m * (double)m;
  double Cm[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const __int128 num = (__int128)m * (__int128)SS[at[a][b]] - (__int128)S[a] * (__int128)S[b];  // exact: below 2^87
      Cm[a][b] = (double)num / mm;
    }
  double nn[3];
  smallest_eigvec(Cm, nn);
  const double len = std::sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
  if (len < 1e-12) return HSK_OK;
  for (double& c : nn) c /= len;
  const double dot = (nn[0] * (double)prev[0] + nn[1] * (double)prev[1]) + nn[2] * (double)prev[2];
  if (dot < 0.0)
    for (double& c : nn) c = -c;
  double mean[3];
  for (int a = 0; a < 3; ++a) mean[a] = ((double)S[a] / (double)m) / 4096.0;
  const double d = -((nn[0] * mean[0] + nn[1] * mean[1]) + nn[2] * mean[2]);
  out_abcd[0] = (float)nn[0];
  out_abcd[1] = (float)nn[1];
  out_abcd[2] = (float)nn[2];
  out_abcd[3] = (float)d;
  *ok = 1;
  return HSK_OK;
}

// Convex hull (in the plane, counter-clockwise about the normal) of the points labelled `plane`; hull_xyz gets up
// to cap vertices lying exactly on the plane.
extern "C" int hsk_plane_hull(const float* xyz, size_t n, const int* labels, int plane, const float abcd[4], float* hull_xyz,
                              size_t cap, size_t* n_hull) {
  if (!xyz || !labels || !abcd || !n_hull) return HSK_ERR_ARG;
  const double nn[3] = {abcd[0], abcd[1], abcd[2]};
  // orthonormal basis (e1, e2) of the plane
  double a[3] = {1, 0, 0};
  if (std::fabs(nn[0]) > 0.9) {
    a[0] = 0;
    a[1] = 1;
  }
  double e1[3] = {a[1] * nn[2] - a[2] * nn[1], a[2] * nn[0] - a[0] * nn[2], a[0] * nn[1] - a[1] * nn[0]};
  const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
  for (double& c : e1) c /= l1;
  const double e2[3] = {nn[1] * e1[2] - nn[2] * e1[1], nn[2] * e1[0] - nn[0] * e1[2], nn[0] * e1[1] - nn[1] * e1[0]};
  struct P2 {
    double x, y;
  };
  std::vector<P2> pts;
  for (size_t i = 0; i < n; ++i)
    if (labels[i] == plane) {
      const float* p = xyz + 3 * i;
      pts.push_back({e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2], e2[0] * p[0] + e2[1] * p[1] + e2[2] * p[2]});
    }
  *n_hull = 0;
  if (pts.size() < 3) return HSK_OK;
  std::sort(pts.begin(), pts.end(), [](const P2& u, const P2& v) { return u.x != v.x ? u.x < v.x : u.y < v.y; });
  auto cross = [](const P2& o, const P2& u, const P2& v) { return (u.x - o.x) * (v.y - o.y) - (u.y - o.y) * (v.x - o.x); };
  std::vector<P2> h(2 * pts.size());
  size_t k = 0;
  for (size_t i = 0; i < pts.size(); ++i) {  // Andrew's monotone chain
    while (k >= 2 && cross(h[k - 2], h[k - 1], pts[i]) <= 0) --k;
    h[k++] = pts[i];
  }
  for (size_t i = pts.size() - 1, t = k + 1; i > 0; --i) {
    while (k >= t && cross(h[k - 2], h[k - 1], pts[i - 1]) <= 0) --k;
    h[k++] = pts[i - 1];
  }
  h.resize(k > 1 ? k - 1 : k);
  *n_hull = h.size();
  const double off = -(double)abcd[3];  // points on the plane: x = u e1 + v e2 + off * n
  for (size_t i = 0; i < h.size() && i < cap && hull_xyz; ++i)
    for (int c = 0; c < 3; ++c) hull_xyz[3 * i + c] = (float)(h[i].x * e1[c] + h[i].y * e2[c] + off * nn[c]);
  return HSK_OK;
}

// planes.txt in the format planeEqsFromFile parses (Main.hs:1379-1389): "a b c d" per line, lines separated by \n
extern "C" int hsk_write_planes_txt(const char* path, const float* planes_abcd, int n_planes) {
  if (!path || (!planes_abcd && n_planes)) return HSK_ERR_ARG;
  FILE* f = fopen(path, "w");
  if (!f) return HSK_ERR_STATE;
  for (int i = 0; i < n_planes; ++i)
    fprintf(f, "%.9g %.9g %.9g %.9g%s", planes_abcd[4 * i], planes_abcd[4 * i + 1], planes_abcd[4 * i + 2],
            planes_abcd[4 * i + 3], i + 1 < n_planes ? "\n" : "");
  return fclose(f) == 0 ? HSK_OK : HSK_ERR_STATE;
}

// ------------------------------------------------------------------------------------------------------
// Transforms on the seam back from HouseScan: HouseScan exports each room's placement as a
// row-major, LEFT-multiplicative 4x4 -- as one CSV line for `pcl_transform_point_cloud -matrix`
// (roomProjectionToString, housescan/Main.hs:2271-2284) and as a 4-line .xf file for `plyxform`
// (roomProjectionToXfFormat, Main.hs:2289-2302).  These read/write both forms and apply them to a cloud.
// ------------------------------------------------------------------------------------------------------
extern "C" int hsk_write_xf(const char* path, const float m[16]) {
  if (!path || !m) return HSK_ERR_ARG;
  FILE* f = fopen(path, "w");
  if (!f) return HSK_ERR_STATE;
  for (int r = 0; r < 4; ++r) fprintf(f, "%.9g %.9g %.9g %.9g\n", m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
  return fclose(f) == 0 ? HSK_OK : HSK_ERR_STATE;
}

// accepts the .xf layout (whitespace separated) and the CSV layout (comma separated): 16 numbers, row-major
extern "C" int hsk_read_xf(const char* path, float m[16]) {
  if (!path || !m) return HSK_ERR_ARG;
  FILE* f = fopen(path, "r");
  if (!f) return HSK_ERR_STATE;
  int n = 0;
  double v;
  while (n < 16) {
    int c = fgetc(f);
    if (c == EOF) break;
    if (c == ',' || c == ' ' || c == '\n' || c == '\t' || c == '\r') continue;
    ungetc(c, f);
    if (fscanf(f, "%lf", &v) != 1) break;
    m[n++] = (float)v;
  }
  fclose(f);
  return n == 16 ? HSK_OK : HSK_ERR_STATE;
}

// p' = M p for packed xyz points (in place allowed); w is assumed 1 and the last row (0 0 0 1)
extern "C" int hsk_transform_cloud(const float* xyz, size_t n, const float m[16], float* out) {
  if ((!xyz && n) || !m || (!out && n)) return HSK_ERR_ARG;
  for (size_t i = 0; i < n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    out[3 * i] = m[0] * x + m[1] * y + m[2] * z + m[3];
    out[3 * i + 1] = m[4] * x + m[5] * y + m[6] * z + m[7];
    out[3 * i + 2] = m[8] * x + m[9] * y + m[10] * z + m[11];
  }
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// Recorded depth streams: no OpenNI / .oni here, so the core has its own raw container.
//   bytes 0..3 "HSKD", u32 version = 1, u32 width, u32 height, u32 n_frames, f32 fx, fy, cx, cy, then
//   n_frames x (width*height) little-endian uint16 millimetres, row-major -- the frame layout of
//   takeDepthSnapshot (housescan/HoniHelper.hs:20-36).
// ------------------------------------------------------------------------------------------------------
struct hsk_depth_stream {
  FILE* f;
  uint32_t w, h, n;
  float intr[4];
  bool writing;
};

extern "C" hsk_depth_stream* hsk_stream_create(const char* path, int w, int h, float fx, float fy, float cx, float cy) {
  if (!path || w <= 0 || h <= 0) return nullptr;
  FILE* f = fopen(path, "wb");
  if (!f) return nullptr;
  hsk_depth_stream* s = new hsk_depth_stream{f, (uint32_t)w, (uint32_t)h, 0, {fx, fy, cx, cy}, true};
  const uint32_t hdr[5] = {0x444B5348u /* "HSKD" */, 1u, s->w, s->h, 0u};
  fwrite(hdr, 4, 5, f);
  fwrite(s->intr, 4, 4, f);
  return s;
}

extern "C" hsk_depth_stream* hsk_stream_open(const char* path, int* w, int* h, int* n_frames, float intr[4]) {
  if (!path) return nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) return nullptr;
  uint32_t hdr[5];
  float in4[4];
  if (fread(hdr, 4, 5, f) != 5 || fread(in4, 4, 4, f) != 4 || hdr[0] != 0x444B5348u || hdr[1] != 1u) {
    fclose(f);
    return nullptr;
  }
  hsk_depth_stream* s = new hsk_depth_stream{f, hdr[2], hdr[3], hdr[4], {in4[0], in4[1], in4[2], in4[3]}, false};
  if (w) *w = (int)s->w;
  if (h) *h = (int)s->h;
  if (n_frames) *n_frames = (int)s->n;
  if (intr)
    for (int i = 0; i < 4; ++i) intr[i] = in4[i];
  return s;
}

extern "C" int hsk_stream_write(hsk_depth_stream* s, const uint16_t* depth) {
  if (!s || !s->writing || !depth) return HSK_ERR_ARG;
  const size_t px = (size_t)s->w * s->h;
  if (fwrite(depth, 2, px, s->f) != px) return HSK_ERR_STATE;
  s->n += 1;
  return HSK_OK;
}

// frame `index` (0-based) into depth; HSK_ERR_ARG when out of range
extern "C" int hsk_stream_read(hsk_depth_stream* s, int index, uint16_t* depth) {
  if (!s || s->writing || !depth || index < 0 || (uint32_t)index >= s->n) return HSK_ERR_ARG;
  const size_t px = (size_t)s->w * s->h;
  if (fseek(s->f, (long)(36 + (size_t)index * px * 2), SEEK_SET) != 0) return HSK_ERR_STATE;
  return fread(depth, 2, px, s->f) == px ? HSK_OK : HSK_ERR_STATE;
}

extern "C" int hsk_stream_info(const hsk_depth_stream* s, int* w, int* h, int* n_frames, float intr[4]) {
  if (!s) return HSK_ERR_ARG;
  if (w) *w = (int)s->w;
  if (h) *h = (int)s->h;
  if (n_frames) *n_frames = (int)s->n;
  if (intr)
    for (int i = 0; i < 4; ++i) intr[i] = s->intr[i];
  return HSK_OK;
}

extern "C" int hsk_stream_close(hsk_depth_stream* s) {
  if (!s) return HSK_ERR_ARG;
  int rc = HSK_OK;
  if (s->writing) {  // patch the frame count
    if (fseek(s->f, 16, SEEK_SET) != 0 || fwrite(&s->n, 4, 1, s->f) != 1) rc = HSK_ERR_STATE;
  }
  if (fclose(s->f) != 0) rc = HSK_ERR_STATE;
  delete s;
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------
// mesh products: weld a triangle soup by exact vertex coordinates, write a binary .ply mesh
// ---------------------------------------------------------------------------------------------------------------
#include <cstring>
#include <unordered_map>

namespace {
struct VKey {
  uint32_t a, b, c;
  bool operator==(const VKey& o) const { return a == o.a && b == o.b && c == o.c; }
};
struct VKeyHash {
  size_t operator()(const VKey& k) const {
    uint64_t h = 0x9e3779b97f4a7c15ull ^ k.a;
    h = (h ^ (h >> 29)) * 0xbf58476d1ce4e5b9ull ^ k.b;
    h = (h ^ (h >> 32)) * 0x94d049bb133111ebull ^ k.c;
    return (size_t)(h ^ (h >> 31));
  }
};
// vertices in order of first appearance; -0.0 is folded onto +0.0 so that equal points weld
void weld(const float* tri, size_t n_tri, std::vector<float>& verts, std::vector<int32_t>& idx) {
  std::unordered_map<VKey, int32_t, VKeyHash> seen;
  seen.reserve(n_tri * 2);
  idx.resize(n_tri * 3);
  for (size_t i = 0; i < n_tri * 3; ++i) {
    float p[3] = {tri[3 * i] + 0.0f, tri[3 * i + 1] + 0.0f, tri[3 * i + 2] + 0.0f};
    VKey k;
    std::memcpy(&k, p, 12);
    auto it = seen.find(k);
    if (it == seen.end()) {
      const int32_t id = (int32_t)(verts.size() / 3);
      seen.emplace(k, id);
      verts.insert(verts.end(), p, p + 3);
      idx[i] = id;
    } else {
      idx[i] = it->second;
    }
  }
}
}  // namespace

extern "C" int hsk_weld_triangles(const float* tri_xyz, size_t n_triangles, float* vertices, size_t cap_vertices, size_t* n_vertices,
                                  int32_t* indices) {
  if ((!tri_xyz && n_triangles) || !n_vertices) return HSK_ERR_ARG;
  std::vector<float> verts;
  std::vector<int32_t> idx;
  weld(tri_xyz, n_triangles, verts, idx);
  *n_vertices = verts.size() / 3;
  if (!vertices && !indices) return HSK_OK;
  if (vertices) {
    if (cap_vertices < verts.size() / 3) return HSK_ERR_ARG;
    if (!verts.empty()) std::memcpy(vertices, verts.data(), verts.size() * 4);
  }
  if (indices && !idx.empty()) std::memcpy(indices, idx.data(), idx.size() * 4);
  return HSK_OK;
}

extern "C" int hsk_write_ply_mesh(const char* path, const float* tri_xyz, size_t n_triangles, size_t* n_vertices_out, size_t* n_faces_out) {
  if (!path || (!tri_xyz && n_triangles)) return HSK_ERR_ARG;
  std::vector<float> verts;
  std::vector<int32_t> idx;
  weld(tri_xyz, n_triangles, verts, idx);
  size_t faces = 0;
  for (size_t t = 0; t < n_triangles; ++t)
    if (idx[3 * t] != idx[3 * t + 1] && idx[3 * t + 1] != idx[3 * t + 2] && idx[3 * t] != idx[3 * t + 2]) ++faces;
  FILE* f = fopen(path, "wb");
  if (!f) return HSK_ERR_STATE;
  fprintf(f,
          "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
          "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
          verts.size() / 3, faces);
  bool ok = verts.empty() || fwrite(verts.data(), 4, verts.size(), f) == verts.size();
  for (size_t t = 0; t < n_triangles && ok; ++t) {
    if (idx[3 * t] == idx[3 * t + 1] || idx[3 * t + 1] == idx[3 * t + 2] || idx[3 * t] == idx[3 * t + 2]) continue;
    const unsigned char three = 3;
    ok = fwrite(&three, 1, 1, f) == 1 && fwrite(&idx[3 * t], 4, 3, f) == 3;
  }
  const int rc = fclose(f);
  if (n_vertices_out) *n_vertices_out = verts.size() / 3;
  if (n_faces_out) *n_faces_out = faces;
  return (ok && rc == 0) ? HSK_OK : HSK_ERR_STATE;
}

// binary little-endian PLY 1.0 of an indexed mesh: per vertex x y z [nx ny nz] [red green blue], interleaved and unpadded (NaN
// normal components written as 0); per face a uchar 3 and three int indices, every face as given -- and, with uv, a uchar 6 and
// the face's six texture coordinates behind them (the form Meshlab reads, with the atlas named in a comment line).  The indices
// are checked before the file is created.
static int write_ply_mesh(const char* path, const float* vertices, const float* normals, const uint8_t* rgb, size_t n_vertices,
                          const int32_t* faces, size_t n_faces, const char* texture_file, const float* uv) {
  if (!path || (n_vertices && !vertices) || (n_faces && !faces)) return HSK_ERR_ARG;
  for (size_t i = 0; i < 3 * n_faces; ++i)
    if (faces[i] < 0 || (size_t)faces[i] >= n_vertices) return HSK_ERR_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) return HSK_ERR_STATE;
  fprintf(f, "ply\nformat binary_little_endian 1.0\n");
  if (texture_file) fprintf(f, "comment TextureFile %s\n", texture_file);
  fprintf(f, "element vertex %zu\nproperty float x\nproperty float y\nproperty float z\n", n_vertices);
  if (normals) fprintf(f, "property float nx\nproperty float ny\nproperty float nz\n");
  if (rgb) fprintf(f, "property uchar red\nproperty uchar green\nproperty uchar blue\n");
  fprintf(f, "element face %zu\nproperty list uchar int vertex_indices\n%send_header\n", n_faces, uv ? "property list uchar float texcoord\n" : "");
  const size_t rec = 12 + (normals ? 12 : 0) + (rgb ? 3 : 0), frec = uv ? 38 : 13, batch = 8192;
  std::vector<unsigned char> buf(batch * (rec > frec ? rec : frec));
  bool ok = true;
  for (size_t i0 = 0; i0 < n_vertices && ok; i0 += batch) {
    const size_t m = n_vertices - i0 < batch ? n_vertices - i0 : batch;
    unsigned char* p = buf.data();
    for (size_t j = 0; j < m; ++j) {
      const size_t i = i0 + j;
      memcpy(p, vertices + 3 * i, 12);
      p += 12;
      if (normals) {
        for (int c = 0; c < 3; ++c) {
          const float v = normals[3 * i + c];
          const float w = v == v ? v : 0.0f;
          memcpy(p + 4 * c, &w, 4);
        }
        p += 12;
      }
      if (rgb) {
        memcpy(p, rgb + 3 * i, 3);
        p += 3;
      }
    }
    ok = fwrite(buf.data(), rec, m, f) == m;
  }
  for (size_t t0 = 0; t0 < n_faces && ok; t0 += batch) {
    const size_t m = n_faces - t0 < batch ? n_faces - t0 : batch;
    for (size_t j = 0; j < m; ++j) {
      buf[frec * j] = 3;
      memcpy(&buf[frec * j + 1], faces + 3 * (t0 + j), 12);
      if (uv) {
        buf[frec * j + 13] = 6;
        memcpy(&buf[frec * j + 14], uv + 6 * (t0 + j), 24);
      }
    }
    ok = fwrite(buf.data(), frec, m, f) == m;
  }
  const int rc = fclose(f);
  return (ok && rc == 0) ? HSK_OK : HSK_ERR_STATE;
}
extern "C" int hsk_write_ply_indexed(const char* path, const float* vertices, const float* normals, const uint8_t* rgb, size_t n_vertices,
                                     const int32_t* faces, size_t n_faces) {
  return write_ply_mesh(path, vertices, normals, rgb, n_vertices, faces, n_faces, nullptr, nullptr);
}
// ... with the atlas's file name (no line break in it) and the faces' texture coordinates (hsk_bake_texture's uv)
extern "C" int hsk_write_ply_textured(const char* path, const float* vertices, const float* normals, size_t n_vertices, const int32_t* faces,
                                      size_t n_faces, const float* uv, const char* texture_file) {
  if (!texture_file || !*texture_file || strpbrk(texture_file, "\r\n") || (n_faces && !uv)) return HSK_ERR_ARG;
  return write_ply_mesh(path, vertices, normals, nullptr, n_vertices, faces, n_faces, texture_file, uv);
}

// 8-bit RGB PNG of a w x h image (rows top to bottom): the zlib stream is made of stored deflate blocks -- no compression, so no
// library: only the chunks' crc32 and the stream's adler32 are computed
static uint32_t png_crc(uint32_t c, const unsigned char* p, size_t n) {
  static uint32_t tab[256];
  if (!tab[1])
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t v = i;
      for (int k = 0; k < 8; ++k) v = (v & 1u) ? 0xedb88320u ^ (v >> 1) : v >> 1;
      tab[i] = v;
    }
  for (size_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
  return c;
}
static void png_be32(unsigned char* p, uint32_t v) {
  p[0] = (unsigned char)(v >> 24), p[1] = (unsigned char)(v >> 16), p[2] = (unsigned char)(v >> 8), p[3] = (unsigned char)v;
}
static bool png_chunk(FILE* f, const char type[4], const unsigned char* data, size_t n) {
  unsigned char head[8], tail[4];
  png_be32(head, (uint32_t)n);
  memcpy(head + 4, type, 4);
  png_be32(tail, png_crc(png_crc(0xffffffffu, head + 4, 4), data, n) ^ 0xffffffffu);
  return fwrite(head, 1, 8, f) == 8 && (n == 0 || fwrite(data, 1, n, f) == n) && fwrite(tail, 1, 4, f) == 4;
}
extern "C" int hsk_write_png_rgb(const char* path, const uint8_t* rgb, int w, int h) {
  if (!path || !rgb || w <= 0 || h <= 0) return HSK_ERR_ARG;
  const size_t row = 1 + 3 * (size_t)w, raw = row * (size_t)h, n_blocks = (raw + 65534) / 65535;
  const size_t zbytes = 2 + raw + 5 * n_blocks + 4;
  if (zbytes > 0x7fffffffu) return HSK_ERR_ARG;  // (a chunk's length is 31 bits: one IDAT holds the image)
  std::vector<unsigned char> z;
  z.reserve(zbytes);
  z.push_back(0x78), z.push_back(0x01);
  uint32_t a = 1, b = 0;
  size_t in_block = 0, done = 0;  // bytes still to go in the open stored block; filtered bytes written so far
  auto put = [&](const unsigned char* p, size_t n) {
    while (n) {
      if (!in_block) {
        const size_t len = raw - done < 65535 ? raw - done : 65535;
        z.push_back(done + len == raw ? 1 : 0);
        z.push_back((unsigned char)len), z.push_back((unsigned char)(len >> 8));
        z.push_back((unsigned char)~len), z.push_back((unsigned char)(~len >> 8));
        in_block = len;
      }
      const size_t m = n < in_block ? n : in_block;
      z.insert(z.end(), p, p + m);
      for (size_t i = 0; i < m; ++i) {
        a += p[i];
        if (a >= 65521u) a -= 65521u;
        b += a;
        if (b >= 65521u) b -= 65521u;
      }
      p += m, n -= m, in_block -= m, done += m;
    }
  };
  const unsigned char none = 0;  // the filter byte of every row
  for (int y = 0; y < h; ++y) {
    put(&none, 1);
    put(rgb + 3 * (size_t)w * (size_t)y, 3 * (size_t)w);
  }
  unsigned char ad[4];
  png_be32(ad, (b << 16) | a);
  z.insert(z.end(), ad, ad + 4);
  FILE* f = fopen(path, "wb");
  if (!f) return HSK_ERR_STATE;
  static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  unsigned char ihdr[13];
  png_be32(ihdr, (uint32_t)w);
  png_be32(ihdr + 4, (uint32_t)h);
  ihdr[8] = 8, ihdr[9] = 2, ihdr[10] = 0, ihdr[11] = 0, ihdr[12] = 0;
  const bool ok = fwrite(sig, 1, 8, f) == 8 && png_chunk(f, "IHDR", ihdr, 13) && png_chunk(f, "IDAT", z.data(), z.size()) &&
                  png_chunk(f, "IEND", nullptr, 0);
  const int rc = fclose(f);
  return (ok && rc == 0) ? HSK_OK : HSK_ERR_STATE;
}

// n' = R n with R the rotation part of a row-major .xf matrix: hsk_transform_cloud's arithmetic without the translation, no
// renormalisation (in place allowed)
extern "C" int hsk_transform_normals(const float* n, size_t count, const float m[16], float* out) {
  if ((!n && count) || !m || (!out && count)) return HSK_ERR_ARG;
  for (size_t i = 0; i < count; ++i) {
    const float x = n[3 * i], y = n[3 * i + 1], z = n[3 * i + 2];
    out[3 * i] = m[0] * x + m[1] * y + m[2] * z;
    out[3 * i + 1] = m[4] * x + m[5] * y + m[6] * z;
    out[3 * i + 2] = m[8] * x + m[9] * y + m[10] * z;
  }
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// Section views on the host seam (include/hskinfu.h "Section views"): a house section in a room's frame, and the
// rooms' images into one.
// ------------------------------------------------------------------------------------------------------
// M = room -> house, rigid: M^-1 = (R^T, -R^T t).  Everything in binary64 from the binary32 inputs, one rounding at the end.
extern "C" int hsk_section_in_room(const hsk_section* house, const float room_xf[16], hsk_section* room) {
  if (!house || !room_xf || !room) return HSK_ERR_ARG;
  if (house->view.follow != 0) return HSK_ERR_ARG;
  if (house->n_clip < 0 || house->n_clip > HSK_MAX_CLIP) return HSK_ERR_ARG;
  const float* m = room_xf;
  if (!(m[12] == 0.0f && m[13] == 0.0f && m[14] == 0.0f && m[15] == 1.0f)) return HSK_ERR_ARG;
  double R[3][3], t[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i][j] = (double)m[4 * i + j];
    t[i] = (double)m[4 * i + 3];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = (R[0][i] * R[0][j] + R[1][i] * R[1][j]) + R[2][i] * R[2][j];
      if (!(std::fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-4)) return HSK_ERR_ARG;   // (NaN: refused)
    }
  hsk_section out = *house;
  // a point p -> R^T (p - t); a direction v -> R^T v
  auto point = [&](const double p[3], double q[3]) {
    const double e0 = p[0] - t[0], e1 = p[1] - t[1], e2 = p[2] - t[2];
    for (int i = 0; i < 3; ++i) q[i] = (R[0][i] * e0 + R[1][i] * e1) + R[2][i] * e2;
  };
  auto direction = [&](const double v[3], double q[3]) {
    for (int i = 0; i < 3; ++i) q[i] = (R[0][i] * v[0] + R[1][i] * v[1]) + R[2][i] * v[2];
  };
  // pose: the columns of its rotation are directions, its translation a point
  const float* hp = house->view.pose;
  for (int c = 0; c < 3; ++c) {
    const double v[3] = {(double)hp[c], (double)hp[4 + c], (double)hp[8 + c]};
    double q[3];
    direction(v, q);
    for (int i = 0; i < 3; ++i) out.view.pose[4 * i + c] = (float)q[i];
  }
  {
    const double p[3] = {(double)hp[3], (double)hp[7], (double)hp[11]};
    double q[3];
    point(p, q);
    for (int i = 0; i < 3; ++i) out.view.pose[4 * i + 3] = (float)q[i];
  }
  // planes: (n, d) M = (n R, n . t + d)
  for (int c = 0; c < house->n_clip; ++c) {
    const double n[3] = {(double)house->clip[c][0], (double)house->clip[c][1], (double)house->clip[c][2]};
    for (int j = 0; j < 3; ++j) out.clip[c][j] = (float)((n[0] * R[0][j] + n[1] * R[1][j]) + n[2] * R[2][j]);
    out.clip[c][3] = (float)(((n[0] * t[0] + n[1] * t[1]) + n[2] * t[2]) + (double)house->clip[c][3]);
  }
  if (!house->view.light_in_camera) {
    const double l[3] = {(double)house->view.light[0], (double)house->view.light[1], (double)house->view.light[2]};
    double q[3];
    if (house->light_directional)
      direction(l, q);
    else
      point(l, q);
    for (int i = 0; i < 3; ++i) out.view.light[i] = (float)q[i];
  }
  *room = out;
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// Volume fusion on the host seam (include/hskinfu.h "Volume fusion")
// ------------------------------------------------------------------------------------------------------
// hsk_section_in_room's test of a rigid row-major matrix; R, t in binary64
static bool rigid_parts(const float* m, double R[3][3], double t[3]) {
  if (!(m[12] == 0.0f && m[13] == 0.0f && m[14] == 0.0f && m[15] == 1.0f)) return false;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i][j] = (double)m[4 * i + j];
    t[i] = (double)m[4 * i + 3];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = (R[0][i] * R[0][j] + R[1][i] * R[1][j]) + R[2][i] * R[2][j];
      if (!(std::fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-4)) return false;   // (NaN: refused)
    }
  return true;
}

// M^-1 = (R^T, -R^T t): the rotation is a transposition (no rounding), the translation one binary64 expression rounded once
extern "C" int hsk_invert_rigid(const float m[16], float inv[16]) {
  if (!m || !inv) return HSK_ERR_ARG;
  double R[3][3], t[3];
  if (!rigid_parts(m, R, t)) return HSK_ERR_ARG;
  float out[16];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out[4 * i + j] = m[4 * j + i];
    out[4 * i + 3] = (float)(-((R[0][i] * t[0] + R[1][i] * t[1]) + R[2][i] * t[2]));
  }
  out[12] = out[13] = out[14] = 0.0f;
  out[15] = 1.0f;
  memcpy(inv, out, sizeof(out));   // (inv may be m)
  return HSK_OK;
}

// The source's interior -- the points whose voxel lies in [1, dims - 2] on every axis, where a trilinear sample exists -- is the
// box [cell, (dims - 1) cell]; its image under M lies in the box of its eight corners' images.  Binary64 from the binary32
// cells the contexts use (size / dims in binary32).
extern "C" int hsk_fuse_footprint(const int src_dims[3], const float src_size_m[3], const int dst_dims[3], const float dst_size_m[3],
                                  const float src_to_dst[16], int32_t box[6]) {
  if (!src_dims || !src_size_m || !dst_dims || !dst_size_m || !src_to_dst || !box) return HSK_ERR_ARG;
  double R[3][3], t[3];
  if (!rigid_parts(src_to_dst, R, t)) return HSK_ERR_ARG;
  double lo[3], hi[3], cd[3];
  for (int i = 0; i < 3; ++i) {
    if (src_dims[i] <= 0 || dst_dims[i] <= 0 || !(src_size_m[i] > 0.0f) || !(dst_size_m[i] > 0.0f)) return HSK_ERR_ARG;
    const double cs = (double)(src_size_m[i] / (float)src_dims[i]);
    cd[i] = (double)(dst_size_m[i] / (float)dst_dims[i]);
    lo[i] = cs;
    hi[i] = (double)(src_dims[i] - 1) * cs;
  }
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int c = 0; c < 8; ++c) {
    const double p[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
    for (int i = 0; i < 3; ++i) {
      const double q = ((R[i][0] * p[0] + R[i][1] * p[1]) + R[i][2] * p[2]) + t[i];
      if (q < mn[i]) mn[i] = q;
      if (q > mx[i]) mx[i] = q;
    }
  }
  bool empty = false;
  int32_t out[6];
  for (int i = 0; i < 3; ++i) {
    double a = std::floor(mn[i] / cd[i]) - 1.0, b = std::floor(mx[i] / cd[i]) + 2.0;
    if (!(a >= 0.0)) a = 0.0;                        // (also a NaN: an image that is not finite receives nothing)
    if (!(b <= (double)dst_dims[i])) b = (double)dst_dims[i];
    if (!(mn[i] <= mx[i]) || !(a < b)) empty = true;
    out[2 * i] = (int32_t)(a < (double)dst_dims[i] ? a : (double)dst_dims[i]);
    out[2 * i + 1] = (int32_t)(b > 0.0 ? b : 0.0);
  }
  for (int i = 0; i < 6; ++i) box[i] = empty ? 0 : out[i];
  return HSK_OK;
}

extern "C" int hsk_composite_views(int n, const uint8_t* const* rgb, const uint16_t* const* depth_mm, int w, int h,
                                   const uint8_t background[3], uint8_t* out_rgb, uint16_t* out_depth_mm, int32_t* out_index) {
  if (n < 1 || w < 1 || w > 4096 || h < 1 || h > 4096 || !depth_mm) return HSK_ERR_ARG;
  if (out_rgb && (!rgb || !background)) return HSK_ERR_ARG;
  for (int v = 0; v < n; ++v)
    if (!depth_mm[v] || (out_rgb && !rgb[v])) return HSK_ERR_ARG;
  const size_t P = (size_t)w * h;
  for (size_t i = 0; i < P; ++i) {
    int best = -1;
    unsigned bd = 0;
    for (int v = 0; v < n; ++v) {
      const unsigned d = depth_mm[v][i];
      if (d != 0 && (best < 0 || d < bd)) {
        best = v;
        bd = d;
      }
    }
    if (out_rgb) {
      const uint8_t* src = best < 0 ? background : rgb[best] + 3 * i;
      out_rgb[3 * i] = src[0];
      out_rgb[3 * i + 1] = src[1];
      out_rgb[3 * i + 2] = src[2];
    }
    if (out_depth_mm) out_depth_mm[i] = (uint16_t)bd;
    if (out_index) out_index[i] = best;
  }
  return HSK_OK;
}
