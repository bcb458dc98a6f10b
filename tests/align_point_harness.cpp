// align_point_harness.cpp -- the alignment kernel's work on one point (housescan_amd/csrc/hsk_align_point.h), compiled for the
// host: tests/test_align_host.py feeds it a volume in the device's block layout and a cloud, and compares the 28 sums and the
// count with the numpy twin.  Input file: dims (3 int32), size (3 float), matrix (16 float), tau, cos_gate (float), J (int32),
// n (uint32), the volume's words, then six planes of n floats (x, y, z, nx, ny, nz).  Output: 28 integers and the count.
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_align_point.h"
#include "harness_io.h"

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 1);
  int dims[3], J;
  float size[3], m[16], tau, gate;
  unsigned n;
  if (!(in.get(dims, 3) && in.get(size, 3) && in.get(m, 16) && in.get(&tau, 1) && in.get(&gate, 1) && in.get(&J, 1) && in.get(&n, 1))) return 2;
  AlignVol dv;
  AlignArgs aa;
  dv.X = dims[0];
  dv.Y = dims[1];
  dv.Z = dims[2];
  for (int i = 0; i < 3; ++i) {
    dv.cell[i] = size[i] / (float)dims[i];
    dv.icell[i] = 1.0 / (double)dv.cell[i];
    aa.c[i] = size[i] * 0.5f;
    for (int j = 0; j < 3; ++j) aa.R[3 * i + j] = m[4 * i + j];
    aa.t[i] = m[4 * i + 3];
  }
  aa.tau = tau;
  aa.cos_gate = gate;
  aa.J = J;
  aa.n = aa.pitch = n;
  std::vector<unsigned> vol(volume_words(dv.X, dv.Y, dv.Z));
  std::vector<float> soa((size_t)n * 6);
  if (!(in.get(vol) && in.get(soa))) return 2;
  double acc[28] = {0.0};
  unsigned n_used = 0;
  for (unsigned i = 0; i < n; ++i)
    if (align_point(vol.data(), dv, aa, soa[i], soa[n + i], soa[2 * (size_t)n + i], soa[3 * (size_t)n + i], soa[4 * (size_t)n + i],
                    soa[5 * (size_t)n + i], acc))
      n_used += 1;
  for (int k = 0; k < 28; ++k) printf("%lld\n", (long long)acc[k]);
  printf("%u\n", n_used);
  return 0;
}
