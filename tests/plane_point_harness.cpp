// plane_point_harness.cpp -- the plane kernels' work on one point against one plane (housescan_amd/csrc/hsk_plane_point.h),
// compiled for the host: tests/test_planes_host.py feeds it a cloud with normals, labels and planes, and compares every plane's
// inlier count, sum_abs and ten moments with the numpy twin.  Input file: n, n_planes (uint32), dist_m, cos_min (float), the
// planes (4 floats each), six planes of n floats (x, y, z, nx, ny, nz), n labels (int32).  Output: the number of valid points,
// then one line per plane: the count, sum_abs, the ten sums; then one line per point 0 .. 7: the plane a seed there makes.
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_plane_point.h"
#include "harness_io.h"

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 1);
  unsigned n, n_planes;
  float dist_m, cos_min;
  if (!(in.get(&n, 1) && in.get(&n_planes, 1) && in.get(&dist_m, 1) && in.get(&cos_min, 1))) return 2;
  std::vector<float> planes((size_t)n_planes * 4), soa((size_t)n * 6);
  std::vector<int> labels(n);
  if (!(in.get(planes) && in.get(soa) && in.get(labels))) return 2;
  const float *X = soa.data(), *Y = X + n, *Z = Y + n, *NX = Z + n, *NY = NX + n, *NZ = NY + n;
  unsigned long long n_valid = 0;
  for (unsigned i = 0; i < n; ++i) n_valid += plane_point_valid(X[i], Y[i], Z[i], NX[i], NY[i], NZ[i]) ? 1 : 0;
  printf("%llu\n", n_valid);
  for (unsigned j = 0; j < n_planes; ++j) {
    const float* e = &planes[(size_t)j * 4];
    long long s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long sum_abs = 0;
    for (unsigned i = 0; i < n; ++i) {
      const bool open = plane_point_valid(X[i], Y[i], Z[i], NX[i], NY[i], NZ[i]) & (labels[i] < 0);
      float as;
      if (!plane_point_inlier(open, e[0], e[1], e[2], e[3], dist_m, cos_min, X[i], Y[i], Z[i], NX[i], NY[i], NZ[i], as)) continue;
      const long long qx = plane_q(X[i]), qy = plane_q(Y[i]), qz = plane_q(Z[i]);
      s[0] += 1;
      s[1] += qx, s[2] += qy, s[3] += qz;
      s[4] += qx * qx, s[5] += qx * qy, s[6] += qx * qz;
      s[7] += qy * qy, s[8] += qy * qz, s[9] += qz * qz;
      sum_abs += plane_abs_q(as);
    }
    printf("%lld %llu %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", s[0], sum_abs, s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], s[9]);
  }
  for (unsigned i = 0; i < n && i < 8; ++i) {
    float abcd[4];
    plane_of_point(X[i], Y[i], Z[i], NX[i], NY[i], NZ[i], abcd);
    unsigned bits[4];
    for (int c = 0; c < 4; ++c) __builtin_memcpy(&bits[c], &abcd[c], 4);
    printf("%u %u %u %u\n", bits[0], bits[1], bits[2], bits[3]);
  }
  return 0;
}
