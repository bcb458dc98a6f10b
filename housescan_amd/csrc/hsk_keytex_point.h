// hsk_keytex_point.h -- textures baked from keyframes (include/hskinfu.h "Keyframe textures"; DESIGN.md 3.26 the kernel, 8t the
// rule): the keyframe store's layout and the work on ONE texel -- its point and normal (hsk_texture_point.h: tex_point, tex_normal),
// then every keyframe in ascending index: camera coordinates, view angle, pixel, the four-tap occlusion test, the bilinear value
// and the weight, and the rule that says which photograph wins.  keytex.hip's kernel calls key_texel per lane; like
// hsk_texture_point.h it is plain C++ over hsk_sample.h with no HIP type in it, so that tests/keytex_point_harness.cpp compiles the
// same text for the host and tests/test_keytex_host.py compares it with the numpy twin byte for byte, without a GPU.  One rounding
// per written operator: both builds forbid contraction.
#pragma once
#include "hsk_texture_point.h"

#define TEX_KEYFRAME 32u  // mask bit: the texel's colour comes from a keyframe (HSK_TEXEL_KEYFRAME)
#define KEY_BEST 0
#define KEY_BLEND 1
#define KEY_NONE 255  // source plane: no keyframe
#define KEY_MAX_CAP 255
#define KEY_MAX_SIDE 4096

// a keyframe's record in the store: camera-to-world rotation (row-major) and translation, then fx fy cx cy
struct KeyRecord {
  float R[9], t[3];
  float fx, fy, cx, cy;
};
static_assert(sizeof(KeyRecord) == 64, "a keyframe record is 64 bytes");

// The store is one allocation of `cap` slots, `stride` bytes apart: a slot is its record, then w x h colour words
// (R | G << 8 | B << 16), then w x h depth values in millimetres (0: invalid).
static inline size_t key_slot_bytes(int w, int h) { return ((size_t)64 + (size_t)6 * (size_t)w * (size_t)h + 255) & ~(size_t)255; }
struct KeyStore {
  const unsigned char* base;
  size_t stride;
  int n, w, h;
};
HSK_HD const KeyRecord& key_record(const KeyStore& ks, int k) { return *(const KeyRecord*)(ks.base + (size_t)k * ks.stride); }
HSK_HD const unsigned* key_colour(const KeyStore& ks, int k) { return (const unsigned*)(ks.base + (size_t)k * ks.stride + 64); }
HSK_HD const unsigned short* key_depth(const KeyStore& ks, int k) {
  return (const unsigned short*)(ks.base + (size_t)k * ks.stride + 64 + (size_t)4 * (size_t)ks.w * (size_t)ks.h);
}

struct KeyArgs {
  int mode;  // KEY_BEST, KEY_BLEND
  float z_min, z_max, cos_min, border, occlusion_tol, blend_floor;
  int fallback;  // a texel no keyframe passes takes the colour volume's colour, where there is one
};

struct KeyTexelOut {
  unsigned mask;  // TEX_* and TEX_KEYFRAME
  unsigned rgb[3], nrm[3];
  unsigned source;  // the keyframe of the largest weight, KEY_NONE without one
  unsigned seen, occluded;  // the keyframes that reached the occlusion test for this texel; of them, those that failed it
  float p[3];
};

// steps 1 to 3 for the point q with the unit normal n: does keyframe r see it, at which pixel and with which weight
struct KeyGeo {
  float zc, weight;
  int iu, iv;
  float a, b;
};
HSK_HD bool key_geometry(const KeyRecord& r, const KeyArgs& ka, int w, int h, const float q[3], const float n[3], KeyGeo& g) {
  const float dx = q[0] - r.t[0], dy = q[1] - r.t[1], dz = q[2] - r.t[2];
  const float xc = hsk_dot3(dx, dy, dz, r.R[0], r.R[3], r.R[6]);
  const float yc = hsk_dot3(dx, dy, dz, r.R[1], r.R[4], r.R[7]);
  const float zc = hsk_dot3(dx, dy, dz, r.R[2], r.R[5], r.R[8]);
  if (!(zc >= ka.z_min && zc <= ka.z_max)) return false;
  const float r2 = hsk_dot3(dx, dy, dz, dx, dy, dz);
  const float c = -hsk_dot3(n[0], n[1], n[2], dx, dy, dz) / sqrtf(r2);
  if (!(c >= ka.cos_min)) return false;
  const float u = r.fx * (xc / zc) + r.cx, v = r.fy * (yc / zc) + r.cy;
  if (!(u >= ka.border && u <= (float)(w - 1) - ka.border)) return false;
  if (!(v >= ka.border && v <= (float)(h - 1) - ka.border)) return false;
  g.zc = zc;
  g.weight = c / r2;
  g.iu = hsk_min_i((int)u, w - 2);  // (0 <= u <= w - 1: border is not negative)
  g.iv = hsk_min_i((int)v, h - 2);
  g.a = u - (float)g.iu;
  g.b = v - (float)g.iv;
  return true;
}

// steps 4 and 5: the four taps of keyframe k around the pixel; false: one of them has no depth or another depth than the texel
HSK_HD bool key_taps(const KeyStore& ks, int k, const KeyArgs& ka, const KeyGeo& g, float val[3]) {
  const size_t at = (size_t)g.iv * (size_t)ks.w + (size_t)g.iu;
  const unsigned short* dp = key_depth(ks, k) + at;
  const unsigned d00 = dp[0], d10 = dp[1], d01 = dp[ks.w], d11 = dp[ks.w + 1];
  const unsigned dd[4] = {d00, d10, d01, d11};
  bool ok = true;
  HSK_UNROLL
  for (int i = 0; i < 4; ++i) ok = ok && dd[i] != 0u && fabsf(g.zc - (float)dd[i] * 0.001f) <= ka.occlusion_tol;
  if (!ok) return false;
  const unsigned* cp = key_colour(ks, k) + at;
  const unsigned c00 = cp[0], c10 = cp[1], c01 = cp[ks.w], c11 = cp[ks.w + 1];
  HSK_UNROLL
  for (int ch = 0; ch < 3; ++ch) {
    const int sh = 8 * ch;
    const float f00 = (float)((c00 >> sh) & 255u), f10 = (float)((c10 >> sh) & 255u), f01 = (float)((c01 >> sh) & 255u),
                f11 = (float)((c11 >> sh) & 255u);
    const float top = f00 + g.a * (f10 - f00), bot = f01 + g.a * (f11 - f01);
    val[ch] = top + g.b * (bot - top);
  }
  return true;
}

// The colour of a texel from the keyframes.  `active`: the texel has a point and a unit normal n (mask bit TEX_NORMAL); every
// caller of a group that votes together runs the loop, active or not.  any(x): whether x holds for any caller of the group -- the
// host's group is one texel, the kernel's the 64 texels of a wave (a ballot), which skips a keyframe's gathers when none of them
// passes steps 1 to 3.  Per texel the keyframes are visited in ascending index, so the sums of KEY_BLEND are in that order.
// -> true: keyed (rgb, source set); seen and occluded are counted either way.
template <class Any>
HSK_HD bool key_lookup(const KeyStore& ks, const KeyArgs& ka, bool active, const float q[3], const float n[3], Any any, unsigned rgb[3],
                       unsigned& source, unsigned& seen, unsigned& occluded) {
  int best = -1;
  float wmax = 0.0f, bval[3] = {0.0f, 0.0f, 0.0f};
  for (int k = 0; k < ks.n; ++k) {
    KeyGeo g;
    const bool pass = active && key_geometry(key_record(ks, k), ka, ks.w, ks.h, q, n, g);
    if (!any(pass)) continue;  // (the same for every caller of the group)
    if (pass) {
      seen += 1u;
      float val[3];
      if (!key_taps(ks, k, ka, g, val)) {
        occluded += 1u;
      } else if (best < 0 || g.weight > wmax) {  // (the lowest index on a tie)
        best = k;
        wmax = g.weight;
        bval[0] = val[0], bval[1] = val[1], bval[2] = val[2];
      }
    }
  }
  if (ka.mode == KEY_BLEND) {
    // the keyframes within blend_floor of the best, again in ascending index (every caller runs this loop, too: the votes)
    const float floor_w = ka.blend_floor * wmax;
    float sw = 0.0f, s[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < ks.n; ++k) {
      KeyGeo g;
      const bool pass = best >= 0 && key_geometry(key_record(ks, k), ka, ks.w, ks.h, q, n, g);
      if (!any(pass)) continue;
      float val[3];
      if (pass && key_taps(ks, k, ka, g, val) && g.weight >= floor_w) {
        sw = sw + g.weight;
        s[0] = s[0] + g.weight * val[0];
        s[1] = s[1] + g.weight * val[1];
        s[2] = s[2] + g.weight * val[2];
      }
    }
    if (sw > 0.0f) bval[0] = s[0] / sw, bval[1] = s[1] / sw, bval[2] = s[2] / sw;  // (sw = 0: every weight is 0, the best alone)
  }
  if (best < 0) return false;
  rgb[0] = (unsigned)hsk_min_i(255, (int)(bval[0] + 0.5f));
  rgb[1] = (unsigned)hsk_min_i(255, (int)(bval[1] + 0.5f));
  rgb[2] = (unsigned)hsk_min_i(255, (int)(bval[2] + 0.5f));
  source = (unsigned)best;
  return true;
}

// Texel (px, py) of the atlas with its colour from the keyframes; colv = the colour volume (null: none), asked only where no
// keyframe passes and ka.fallback is set.  The rest is tex_texel's.
template <class Any>
HSK_HD void key_texel(const unsigned* vol, const unsigned* colv, const SampleVol& v, const TexArgs& ta, const unsigned* tiles, const TexBlock* blocks,
                      const int* faces, const float* vertices, const KeyStore& ks, const KeyArgs& ka, int px, int py, Any any, KeyTexelOut& o) {
  o.rgb[0] = o.rgb[1] = o.rgb[2] = 0u;
  o.nrm[0] = o.nrm[1] = o.nrm[2] = 0u;
  o.source = KEY_NONE;
  o.seen = o.occluded = 0u;
  TexPoint tp;
  tex_point(vol, v, ta, tiles, blocks, faces, vertices, px, py, tp);
  o.mask = tp.mask;
  o.p[0] = tp.p[0], o.p[1] = tp.p[1], o.p[2] = tp.p[2];
  float n[3] = {0.0f, 0.0f, 0.0f};
  const bool owned = (tp.mask & TEX_OWNED) != 0u;
  const bool has_n = owned && tex_normal(tp.sm, v, n, o.nrm);
  if (has_n) o.mask |= TEX_NORMAL;
  if (key_lookup(ks, ka, has_n, tp.p, n, any, o.rgb, o.source, o.seen, o.occluded))
    o.mask |= TEX_KEYFRAME;
  else if (owned && ka.fallback && colv && tex_colour(colv, v, tp.sm.sc, o.rgb))
    o.mask |= TEX_COLORED;
}

// the host's group of one
struct KeyAnyOne {
  bool operator()(bool x) const { return x; }
};
