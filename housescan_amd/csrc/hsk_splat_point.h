// hsk_splat_point.h -- cloud import (include/hskinfu.h "Cloud import"; DESIGN.md 3.27 the kernels, 8u the rule): the work on ONE
// point of a cloud seen by a virtual depth camera -- world -> camera -> pixel in key_geometry's conventions (hsk_keytex_point.h:
// p_c = R^T (p - t), u = fx (x / z) + cx), the depth clip, the depth value in millimetres, the square footprint, and what the
// point offers a pixel of it: its own depth (DISC) or the depth at which the pixel's ray meets its tangent plane (SURFEL).  A
// pixel keeps the smallest offer, so the image does not depend on the order of the points.  splat.hip's kernel calls splat_point
// and splat_offer per lane; plain C++ with no HIP type in it, so that tests/splat_point_harness.cpp compiles the same text for
// the host and tests/test_splat_host.py compares it with the numpy twin byte for byte, without a GPU.  One rounding per written
// operator: both builds forbid contraction.
//
// point_size_m is a property of the CLOUD, not of the camera or the volume: the leaf size of a downsampled cloud, the spacing
// at which neighbouring points of one surface lie.  The footprint is the square of half-width half_m = 0.5 point_size_m cover
// around the point, projected; with cover >= sqrt(2) the squares of a regular grid of that spacing, in any in-plane rotation,
// leave no pixel uncovered.
#pragma once
#include "hsk_sample.h"

#define SPLAT_DISC 0
#define SPLAT_SURFEL 1
// what became of a point, in the order the rule asks: the first that holds
#define SPLAT_INVALID 0     // a coordinate is not finite
#define SPLAT_CLIPPED 1     // z outside [near_m, far_m] (a NaN z with it)
#define SPLAT_BACKFACING 2  // SURFEL: n . p_c >= 0
#define SPLAT_OUTSIDE 3     // the footprint holds no pixel of the image
#define SPLAT_DONE 4        // the footprint's pixels are offered a depth
#define SPLAT_CLASSES 5
#define SPLAT_EMPTY 0xffffffffu  // a z-buffer word nothing was offered to
#define SPLAT_MAX_HALF_PX 64.0f

struct SplatCam {
  int w, h;
  float fx, fy, cx, cy;
};
struct SplatPose {
  float R[9], t[3];  // camera -> world, row-major
};
struct SplatArgs {
  int mode;
  float half_m;  // (0.5f * point_size_m) * cover
  float min_half_px, max_half_px, near_m, far_m;
};

// a point that is offered: its pixels u_lo <= u <= u_hi, v_lo <= v <= v_hi (inside the image), its own depth, and -- surfel --
// its tangent plane in camera coordinates: n_c . r = pn for the points r of the plane, and the band the ray depth is kept to
struct SplatFoot {
  int u_lo, u_hi, v_lo, v_hi;
  unsigned z_mm;
  int surfel;
  float ncx, ncy, ncz, pn, z_lo, z_hi;
};

HSK_HD bool splat_finite(float x) { return fabsf(x) <= 3.4028234663852886e38f; }  // (a NaN fails the comparison)

// z metres as the depth image's millimetres: rounded as hsk_render_view's depth image rounds (hsk_shade.h), kept to 1 .. 65535
HSK_HD unsigned splat_mm(float z) {
  float d = rintf(z * 1000.0f);
  if (!(d >= 1.0f)) d = 1.0f;
  if (!(d <= 65535.0f)) d = 65535.0f;
  return (unsigned)(int)d;
}

// one axis of the footprint: the integer pixels c - r <= i <= c + r clipped to 0 .. n - 1; false: none (c not finite with it)
HSK_HD bool splat_span(float c, float r, int n, int& lo, int& hi) {
  float a = ceilf(c - r), b = floorf(c + r);
  const float last = (float)(n - 1);
  if (!(b >= 0.0f && a <= last)) return false;
  if (a < 0.0f) a = 0.0f;
  if (b > last) b = last;
  lo = (int)a;
  hi = (int)b;
  return lo <= hi;
}

// the point (x, y, z) with the normal (nx, ny, nz) -- has_n false: none -- under one pose -> SPLAT_*; SPLAT_DONE fills f
HSK_HD int splat_point(const SplatCam& c, const SplatPose& p, const SplatArgs& a, float x, float y, float z, bool has_n, float nx, float ny,
                       float nz, SplatFoot& f) {
  if (!(splat_finite(x) && splat_finite(y) && splat_finite(z))) return SPLAT_INVALID;
  const float dx = x - p.t[0], dy = y - p.t[1], dz = z - p.t[2];
  const float xc = hsk_dot3(dx, dy, dz, p.R[0], p.R[3], p.R[6]);
  const float yc = hsk_dot3(dx, dy, dz, p.R[1], p.R[4], p.R[7]);
  const float zc = hsk_dot3(dx, dy, dz, p.R[2], p.R[5], p.R[8]);
  if (!(zc >= a.near_m && zc <= a.far_m)) return SPLAT_CLIPPED;
  f.surfel = 0;
  if (a.mode == SPLAT_SURFEL && has_n && splat_finite(nx) && splat_finite(ny) && splat_finite(nz) && !(nx == 0.0f && ny == 0.0f && nz == 0.0f)) {
    f.ncx = hsk_dot3(nx, ny, nz, p.R[0], p.R[3], p.R[6]);
    f.ncy = hsk_dot3(nx, ny, nz, p.R[1], p.R[4], p.R[7]);
    f.ncz = hsk_dot3(nx, ny, nz, p.R[2], p.R[5], p.R[8]);
    f.pn = hsk_dot3(f.ncx, f.ncy, f.ncz, xc, yc, zc);
    if (!(f.pn < 0.0f)) return SPLAT_BACKFACING;
    f.surfel = 1;
    const float band = 2.0f * a.half_m;
    f.z_lo = zc - band;
    f.z_hi = zc + band;
  }
  const float u0 = c.fx * (xc / zc) + c.cx, v0 = c.fy * (yc / zc) + c.cy;
  float ru = (c.fx * a.half_m) / zc, rv = (c.fy * a.half_m) / zc;
  ru = fminf(fmaxf(ru, a.min_half_px), a.max_half_px);  // (zc >= near_m > 0: no NaN reaches the clamps)
  rv = fminf(fmaxf(rv, a.min_half_px), a.max_half_px);
  if (!splat_span(u0, ru, c.w, f.u_lo, f.u_hi)) return SPLAT_OUTSIDE;
  if (!splat_span(v0, rv, c.h, f.v_lo, f.v_hi)) return SPLAT_OUTSIDE;
  f.z_mm = splat_mm(zc);
  return SPLAT_DONE;
}

// what the point offers pixel (u, v) of its footprint, in millimetres
HSK_HD unsigned splat_offer(const SplatCam& c, const SplatFoot& f, int u, int v) {
  if (!f.surfel) return f.z_mm;
  const float rx = ((float)u - c.cx) / c.fx, ry = ((float)v - c.cy) / c.fy;
  float zs = f.pn / hsk_dot3(f.ncx, f.ncy, f.ncz, rx, ry, 1.0f);  // (a ray along the plane or away from it lands on a clamp)
  if (!(zs >= f.z_lo)) zs = f.z_lo;
  if (!(zs <= f.z_hi)) zs = f.z_hi;
  return splat_mm(zs);
}
