// hsk_plane_point.h -- oriented plane detection, the work on ONE point against ONE plane: is the point valid, is
// it an inlier of (a, b, c, d), and the integers it adds to the sums.  planes.hip's kernels call it per lane; like
// hsk_reloc_point.h it is plain C++ with no HIP type in it, so that tests/plane_point_harness.cpp compiles the same text for the
// host and tests/test_planes_host.py compares it with the numpy twin (tests/planes_twin.py) bit for bit, without a GPU.
// One rounding per written operator: both builds forbid contraction.
#pragma once
#include <math.h>

#include "hsk_sample.h"

#define HSK_PLANE_REACH_M 64.0f      // |x|, |y|, |z| of a valid point
#define HSK_PLANE_Q_SCALE 4096.0f    // the moments' grid: q = rint(x 4096), |q| <= 2^18
#define HSK_PLANE_ABS_SCALE 65536.0f // sum_abs: rint(|s| 65536)

// all six numbers finite and the point within reach (a NaN fails every comparison)
HSK_HD bool plane_point_valid(float x, float y, float z, float nx, float ny, float nz) {
  const float big = 3.4028234663852886e38f;
  return (fabsf(x) <= HSK_PLANE_REACH_M) & (fabsf(y) <= HSK_PLANE_REACH_M) & (fabsf(z) <= HSK_PLANE_REACH_M) & (fabsf(nx) <= big) &
         (fabsf(ny) <= big) & (fabsf(nz) <= big);
}

// The inlier test of a point that is valid and unlabelled (`open`): |s| <= dist_m with s = ((a x + b y) + c z) + d, and
// g >= cos_min with g = (a nx + b ny) + c nz.  `as` takes |s|.  A plane with a NaN in it has no inlier.
HSK_HD bool plane_point_inlier(bool open, float a, float b, float c, float d, float dist_m, float cos_min, float x, float y, float z, float nx,
                               float ny, float nz, float& as) {
  const float s = hsk_dot3(a, b, c, x, y, z) + d;
  const float g = hsk_dot3(a, b, c, nx, ny, nz);
  as = fabsf(s);
  return open & (as <= dist_m) & (g >= cos_min);
}

// a coordinate of a valid point on the moments' grid (the product is exact: a power of two)
HSK_HD int plane_q(float v) { return (int)rintf(v * HSK_PLANE_Q_SCALE); }
// what an inlier adds to its plane's sum_abs (|s| <= dist_m <= 1: at most 65536)
HSK_HD unsigned plane_abs_q(float as) { return (unsigned)rintf(as * HSK_PLANE_ABS_SCALE); }

// the hypothesis a seed point makes: its normal as stored, d = -((a x + b y) + c z)
HSK_HD void plane_of_point(float x, float y, float z, float nx, float ny, float nz, float abcd[4]) {
  abcd[0] = nx;
  abcd[1] = ny;
  abcd[2] = nz;
  abcd[3] = -hsk_dot3(nx, ny, nz, x, y, z);
}
