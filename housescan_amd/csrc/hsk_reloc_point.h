// hsk_reloc_point.h -- pose scoring, the work on ONE point under ONE pose: the point moved by the candidate
// pose, one trilinear sample of the TSDF, and the class the point falls in.  reloc.hip's kernel calls it per lane; like
// hsk_align_point.h it is plain C++ with no HIP type in it, so that tests/reloc_point_harness.cpp compiles the same text for
// the host and tests/test_reloc_host.py compares it with the numpy twin (tests/reloc_twin.py) bit for bit, without a GPU.
// One rounding per written operator: both builds forbid contraction.
#pragma once
#include "hsk_sample.h"

// the six classes, in the order of hsk_pose_score's counts
#define RELOC_NEAR 0     // |F| < 1: on a surface the volume holds
#define RELOC_FREE 1     // F >= 1: a measured point in space the volume saw empty
#define RELOC_BEHIND 2   // anything else (F <= -1)
#define RELOC_UNSEEN 3   // one of the eight taps was never observed
#define RELOC_OUTSIDE 4  // the sample is the NaN of the outer shell, or beyond it
#define RELOC_SKIPPED 5  // a NaN coordinate: an invalid pixel of a vertex map
#define RELOC_CLASSES 6

// One point (x, y, z) in camera coordinates under the pose (R, t): its class, and in `q` what a near point adds to sum_abs
// (rint(|F| 65536), an integer; 0 for every other class).  Branch-free (hsk_sample.h): every tap lies inside the volume
// whatever the point is -- a NaN, an infinity, kilometres away -- and the verdict is one chain of selects behind the loads.
HSK_HD int reloc_point(const unsigned* vol, const SampleVol& dv, const float* R, const float* t, float x, float y, float z,
                       unsigned& q) {
  const float p0 = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
  const float p1 = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
  const float p2 = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
  const SampleCell sc = hsk_sample_cell(dv, p0, p1, p2);
  unsigned w[8];
  float f[8];
  hsk_sample_words(vol, dv, sc, w);
  const int Ws = hsk_sample_min_weight(w);
  hsk_sample_values(w, f);
  const float F = hsk_sample_blend(f, sc.a, sc.b, sc.c);
  const float aF = fabsf(F);
  const bool skip = (x != x) | (y != y) | (z != z);
  const bool seen = sc.in & (Ws > 0);
  const bool near = !skip & seen & (aF < 1.0f);
  int cls = F > 0.0f ? RELOC_FREE : RELOC_BEHIND;
  cls = aF < 1.0f ? RELOC_NEAR : cls;
  cls = Ws > 0 ? cls : RELOC_UNSEEN;
  cls = sc.in ? cls : RELOC_OUTSIDE;
  cls = skip ? RELOC_SKIPPED : cls;
  q = (unsigned)rint((double)(near ? aF : 0.0f) * 65536.0);  // (below 2^16: |F| < 1)
  return cls;
}
