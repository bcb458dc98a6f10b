// cover_point_harness.cpp -- the coverage kernels' work on one ray under one pose (housescan_amd/csrc/hsk_cover_point.h), compiled
// for the host: tests/test_cover_host.py feeds it a volume in the device's block layout, a probe and poses, and compares every
// ray's class, depth and gain and every pose's eye_state with the numpy twin.  Input file: dims (3 int32), size (3 float), the
// probe (width, height int32; fx, fy, cx, cy, near_m, far_m, step_m float), n_poses (uint32), the poses (16 floats each,
// row-major), the volume's words.  Output: one line per pose -- eye_state, then class, depth_mm and gain of every pixel, row-major.
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_cover_point.h"
#include "harness_io.h"

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 1);
  int dims[3], wh[2];
  float size[3], pf[7];
  unsigned n_poses;
  if (!(in.get(dims, 3) && in.get(size, 3) && in.get(wh, 2) && in.get(pf, 7) && in.get(&n_poses, 1))) return 2;
  SampleVol dv;
  dv.X = dims[0];
  dv.Y = dims[1];
  dv.Z = dims[2];
  for (int i = 0; i < 3; ++i) {
    dv.cell[i] = size[i] / (float)dims[i];
    dv.icell[i] = 1.0 / (double)dv.cell[i];
  }
  CoverProbe pr;
  pr.W = wh[0];
  pr.H = wh[1];
  pr.fx = pf[0];
  pr.fy = pf[1];
  pr.cx = pf[2];
  pr.cy = pf[3];
  pr.near_m = pf[4];
  pr.step_m = pf[6];
  pr.n = cover_sample_count(pf[4], pf[5], pf[6]);
  std::vector<float> poses((size_t)n_poses * 16);
  std::vector<unsigned> vol(volume_words(dv.X, dv.Y, dv.Z));
  if (!(in.get(poses) && in.get(vol))) return 2;
  for (unsigned j = 0; j < n_poses; ++j) {
    const float* m = &poses[(size_t)j * 16];
    float R[9], t[3];
    for (int i = 0; i < 3; ++i) {
      for (int c = 0; c < 3; ++c) R[3 * i + c] = m[4 * i + c];
      t[i] = m[4 * i + 3];
    }
    printf("%d", cover_eye_state(vol.data(), dv, t));
    for (int v = 0; v < pr.H; ++v)
      for (int u = 0; u < pr.W; ++u) {
        unsigned gain = 0, depth = 0;
        const int cls = cover_ray(vol.data(), dv, pr, R, t, u, v, gain, depth);
        printf(" %d %u %u", cls, depth, gain);
      }
    printf("\n");
  }
  return 0;
}
