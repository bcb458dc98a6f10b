// reloc_point_harness.cpp -- the scoring kernel's work on one point under one pose (housescan_amd/csrc/hsk_reloc_point.h), compiled
// for the host: tests/test_reloc_host.py feeds it a volume in the device's block layout, a cloud and poses, and compares the
// six counts and sum_abs of every pose with the numpy twin.  Input file: dims (3 int32), size (3 float), n_poses, n (uint32),
// the poses (16 floats each, row-major), the volume's words, then three planes of n floats (x, y, z).  Output: one line per
// pose, the six counts and sum_abs.
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_reloc_point.h"
#include "harness_io.h"

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 1);
  int dims[3];
  float size[3];
  unsigned n_poses, n;
  if (!(in.get(dims, 3) && in.get(size, 3) && in.get(&n_poses, 1) && in.get(&n, 1))) return 2;
  SampleVol dv;
  dv.X = dims[0];
  dv.Y = dims[1];
  dv.Z = dims[2];
  for (int i = 0; i < 3; ++i) {
    dv.cell[i] = size[i] / (float)dims[i];
    dv.icell[i] = 1.0 / (double)dv.cell[i];
  }
  std::vector<float> poses((size_t)n_poses * 16), soa((size_t)n * 3);
  std::vector<unsigned> vol(volume_words(dv.X, dv.Y, dv.Z));
  if (!(in.get(poses) && in.get(vol) && in.get(soa))) return 2;
  for (unsigned j = 0; j < n_poses; ++j) {
    const float* m = &poses[(size_t)j * 16];
    float R[9], t[3];
    for (int i = 0; i < 3; ++i) {
      for (int c = 0; c < 3; ++c) R[3 * i + c] = m[4 * i + c];
      t[i] = m[4 * i + 3];
    }
    unsigned long long cnt[RELOC_CLASSES] = {0, 0, 0, 0, 0, 0}, sum = 0;
    for (unsigned i = 0; i < n; ++i) {
      unsigned q = 0;
      cnt[reloc_point(vol.data(), dv, R, t, soa[i], soa[n + i], soa[2 * (size_t)n + i], q)] += 1;
      sum += q;
    }
    printf("%llu %llu %llu %llu %llu %llu %llu\n", cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], sum);
  }
  return 0;
}
