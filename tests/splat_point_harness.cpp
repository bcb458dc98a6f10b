// splat_point_harness.cpp -- the cloud import's work on one point and one pixel (housescan_amd/csrc/hsk_splat_point.h), compiled for
// the host: tests/test_splat_host.py feeds it a camera, parameters, a pose and a cloud, and compares the image and the counters
// with the numpy twin.  Input file: width, height, mode, has_normals (4 int32); fx, fy, cx, cy, point_size_m, cover, min_half_px,
// max_half_px, near_m, far_m (10 float); the pose (16 floats, row-major); n (uint32); the points (3 floats each); the normals
// likewise, if any.  Output file: the image (width x height uint16, row-major), then n_invalid, n_clipped, n_backfacing,
// n_outside, n_splatted, n_pixels (uint32).  The points are taken in the file's order; a pixel keeps the smallest offer.
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_splat_point.h"
#include "harness_io.h"

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int head[4];
  float pf[10], m[16];
  unsigned n;
  if (!(in.get(head, 4) && in.get(pf, 10) && in.get(m, 16) && in.get(&n, 1))) return 2;
  const SplatCam cam = {head[0], head[1], pf[0], pf[1], pf[2], pf[3]};
  const SplatArgs args = {head[2], (0.5f * pf[4]) * pf[5], pf[6], pf[7], pf[8], pf[9]};
  SplatPose pose;
  for (int i = 0; i < 3; ++i) {
    for (int c = 0; c < 3; ++c) pose.R[3 * i + c] = m[4 * i + c];
    pose.t[i] = m[4 * i + 3];
  }
  std::vector<float> xyz((size_t)n * 3), nrm(head[3] ? (size_t)n * 3 : 0);
  if (!(in.get(xyz) && in.get(nrm))) return 2;
  std::vector<unsigned> zbuf((size_t)cam.w * (size_t)cam.h, SPLAT_EMPTY);
  unsigned counts[SPLAT_CLASSES + 1] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (unsigned i = 0; i < n; ++i) {
    SplatFoot f;
    const float* q = &xyz[(size_t)i * 3];
    const float* nn = head[3] ? &nrm[(size_t)i * 3] : q;
    const int cls = splat_point(cam, pose, args, q[0], q[1], q[2], head[3] != 0, nn[0], nn[1], nn[2], f);
    counts[cls] += 1u;
    if (cls != SPLAT_DONE) continue;
    for (int v = f.v_lo; v <= f.v_hi; ++v)
      for (int u = f.u_lo; u <= f.u_hi; ++u) {
        const unsigned offer = splat_offer(cam, f, u, v);
        if (u < 0 || u >= cam.w || v < 0 || v >= cam.h) return 3;  // (a footprint outside the image: the rule's fault)
        unsigned& word = zbuf[(size_t)v * (size_t)cam.w + (size_t)u];
        if (offer < word) word = offer;
      }
  }
  std::vector<unsigned short> image(zbuf.size());
  for (size_t i = 0; i < zbuf.size(); ++i) {
    image[i] = zbuf[i] == SPLAT_EMPTY ? (unsigned short)0 : (unsigned short)zbuf[i];
    counts[SPLAT_CLASSES] += zbuf[i] != SPLAT_EMPTY ? 1u : 0u;
  }
  HarnessOut out(argv[2]);
  out.put(image);
  out.put(counts, SPLAT_CLASSES + 1);
  return out.finish();
}
