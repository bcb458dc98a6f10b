// sample_harness.cpp -- the TSDF sample at a point (housescan_amd/csrc/hsk_sample.h), compiled for the host: tests/test_sample_host.py
// feeds it a volume in the device's block layout and points, and compares every piece with the numpy twins bit for bit.
// Input file: dims (3 int32), size (3 float), n (uint32), the volume's words, then three planes of n floats (x, y, z).
// Output file: per point 15 32-bit words -- the interior verdict, the containing voxel clamped to the interior (3), the lower
// corner (3), F (bits), the smallest weight, the gradient (3 x bits), the containing voxel clamped into the grid (3).
// The volume is a heap array of exactly the volume's words: the address sanitizer reports any tap outside it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../housescan_amd/csrc/hsk_sample.h"
#include "harness_io.h"

static int bits(float f) {
  int i;
  memcpy(&i, &f, 4);
  return i;
}

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int dims[3];
  float size[3];
  unsigned n;
  if (!(in.get(dims, 3) && in.get(size, 3) && in.get(&n, 1))) return 2;
  SampleVol v;
  v.X = dims[0];
  v.Y = dims[1];
  v.Z = dims[2];
  for (int i = 0; i < 3; ++i) {
    v.cell[i] = size[i] / (float)dims[i];
    v.icell[i] = 1.0 / (double)v.cell[i];
  }
  std::vector<unsigned> vol(volume_words(v.X, v.Y, v.Z));
  std::vector<float> p((size_t)n * 3);
  if (!(in.get(vol) && in.get(p))) return 2;
  std::vector<int> out((size_t)n * 15);
  for (unsigned i = 0; i < n; ++i) {
    const float px = p[i], py = p[n + i], pz = p[2 * (size_t)n + i];
    const SampleCell sc = hsk_sample_cell(v, px, py, pz);
    unsigned w[8];
    float fv[8], gx, gy, gz;
    hsk_sample_words(vol.data(), v, sc, w);
    hsk_sample_values(w, fv);
    hsk_sample_gradient(fv, sc.a, sc.b, sc.c, v.icell, gx, gy, gz);
    int* o = &out[(size_t)i * 15];
    o[0] = sc.in ? 1 : 0;
    o[1] = sc.cx, o[2] = sc.cy, o[3] = sc.cz;
    o[4] = sc.x, o[5] = sc.y, o[6] = sc.z;
    o[7] = bits(hsk_sample_blend(fv, sc.a, sc.b, sc.c));
    o[8] = hsk_sample_min_weight(w);
    o[9] = bits(gx), o[10] = bits(gy), o[11] = bits(gz);
    hsk_voxel_at(v, px, py, pz, o[12], o[13], o[14]);
  }
  HarnessOut o(argv[2]);
  o.put(out);
  return o.finish();
}
