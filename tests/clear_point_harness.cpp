// clear_point_harness.cpp -- the clearance kernels' shared text (housescan_amd/csrc/hsk_clear_point.h: the obstacle predicate, the
// nearest set bit of a row mask, the border term, the windowed minimum, a point's voxel), compiled for the host: it makes a whole
// field the way clearance.hip's three passes do, sequentially, and tests/test_clearance_host.py compares it with the numpy twin
// (tests/clearance_twin.py).  Input file: dims (3 int32), weight (3 uint32), max_d2, flags (uint32), the cells' size in metres
// (3 float), the number of points (uint32), the points (x, y, z floats), then the volume's words in the device's block layout.
// Output file: the field (X Y Z uint32, row-major, x fastest), then n_obstacle, n_far, max_d2_seen (3 uint64), then the points'
// values (uint32 each).
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_clear_point.h"
#include "harness_io.h"

struct LoadDx {
  const unsigned short* p;
  size_t stride;
  unsigned wx;
  unsigned operator()(unsigned i) const { return clear_dx_value(p[(size_t)i * stride], wx); }
};
struct LoadU32 {
  const unsigned* p;
  size_t stride;
  unsigned operator()(unsigned i) const { return p[(size_t)i * stride]; }
};

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int dims[3];
  unsigned par[5], n_pts;
  float size[3];
  if (!(in.get(dims, 3) && in.get(par, 5) && in.get(size, 3) && in.get(&n_pts, 1))) return 2;
  const unsigned X = (unsigned)dims[0], Y = (unsigned)dims[1], Z = (unsigned)dims[2];
  const unsigned w[3] = {par[0], par[1], par[2]}, max_d2 = par[3], flags = par[4];
  unsigned R[3];
  for (int a = 0; a < 3; ++a) {
    R[a] = clear_reach(max_d2, w[a]);
    if (R[a] > CLEAR_MAX_REACH) return 4;
  }
  std::vector<float> pts((size_t)n_pts * 3);
  const size_t n = (size_t)X * Y * Z;
  std::vector<unsigned> vol(volume_words(X, Y, Z));
  if (!(in.get(pts) && in.get(vol))) return 2;
  unsigned long long stats[3] = {0, 0, 0};
  // the x pass: a row's obstacle bits as exactly nw mask words, then every voxel's nearest bit
  const unsigned nw = (X + CLEAR_MASK_BITS - 1u) / CLEAR_MASK_BITS;
  std::vector<unsigned short> dx(n);
  std::vector<unsigned long long> mask(nw);
  const size_t pitch = (size_t)(X >> 2) << 4;
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y) {
      for (unsigned i = 0; i < nw; ++i) mask[i] = 0ull;
      for (unsigned x = 0; x < X; ++x) {
        const size_t at = ((size_t)(z >> 2) * Y * pitch + ((size_t)(z & 3u) << 2)) + (size_t)y * pitch + (((size_t)(x >> 2) << 4) + (x & 3u));
        if (clear_obstacle(vol[at], flags)) {
          mask[x >> 6] |= 1ull << (x & 63u);
          stats[0] += 1;
        }
      }
      for (unsigned x = 0; x < X; ++x) dx[((size_t)z * Y + y) * X + x] = (unsigned short)clear_row_dx(mask.data(), nw, x, X, R[0], flags);
    }
  // the y pass, then the z pass
  std::vector<unsigned> tmp(n), field(n);
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned x = 0; x < X; ++x) {
      const LoadDx ld{dx.data() + (size_t)z * Y * X + x, (size_t)X, w[0]};
      for (unsigned y = 0; y < Y; ++y) tmp[((size_t)z * Y + y) * X + x] = clear_cap(clear_window_min(ld, y, Y, w[1], R[1], flags), max_d2, CLEAR_INF);
    }
  for (unsigned y = 0; y < Y; ++y)
    for (unsigned x = 0; x < X; ++x) {
      const LoadU32 ld{tmp.data() + (size_t)y * X + x, (size_t)X * Y};
      for (unsigned z = 0; z < Z; ++z) {
        const unsigned v = clear_cap(clear_window_min(ld, z, Z, w[2], R[2], flags), max_d2, CLEAR_FAR);
        field[((size_t)z * Y + y) * X + x] = v;
        stats[1] += v == CLEAR_FAR ? 1 : 0;
        if (v != CLEAR_FAR && v > stats[2]) stats[2] = v;
      }
    }
  // the point lookup
  SampleVol sv;
  sv.X = dims[0], sv.Y = dims[1], sv.Z = dims[2];
  for (int a = 0; a < 3; ++a) {
    sv.cell[a] = size[a] / (float)dims[a];
    sv.icell[a] = 1.0 / (double)sv.cell[a];
  }
  std::vector<unsigned> at_pts(n_pts);
  for (unsigned i = 0; i < n_pts; ++i) {
    unsigned x, y, z;
    bool inside;
    clear_point_voxel(sv, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], x, y, z, inside);
    const unsigned v = field[((size_t)z * Y + y) * X + x];
    at_pts[i] = inside ? v : CLEAR_OUTSIDE;
  }
  HarnessOut o(argv[2]);
  o.put(field.data(), n), o.put(stats, 3), o.put(at_pts.data(), n_pts);
  return o.finish();
}
