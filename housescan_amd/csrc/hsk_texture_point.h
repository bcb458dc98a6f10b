// hsk_texture_point.h -- baked textures (include/hskinfu.h "Baked textures"; DESIGN.md 3.25 the kernel, 8s the rule): the atlas
// layout of a triangle mesh and the work on ONE texel -- its tile, block, half and face, its point on the face, the projection
// onto the TSDF's zero level set, the colour and the normal there.  texture.hip's kernel calls tex_texel per lane; like
// hsk_align_point.h it is plain C++ over hsk_sample.h with no HIP type in it, so that tests/texture_point_harness.cpp compiles the
// same text for the host and tests/test_texture_host.py compares it with the numpy twin bit for bit, without a GPU.  One rounding
// per written operator: both builds forbid contraction.  The layout is integers and binary64 in a fixed order, host only.
#pragma once
#include <stdint.h>

#include <vector>

#include "hsk_sample.h"
#ifndef HSK_UNROLL
#if defined(__HIPCC__)
#define HSK_UNROLL _Pragma("unroll")
#else
#define HSK_UNROLL
#endif
#endif

#define TEX_EMPTY 0xffffffffu  // a tile of no block
#define TEX_MAX_SIDE 16384
#define TEX_MAX_ITER 16
// mask bits (HSK_TEXEL_* of the ABI)
#define TEX_OWNED 1u
#define TEX_INSIDE 2u
#define TEX_PROJECTED 4u
#define TEX_COLORED 8u
#define TEX_NORMAL 16u

// one block of s x s texels at (x0, y0): the faces of its halves (-1: none) and their rotations
struct TexBlock {
  int x0, y0, s;
  int face[2];
  int rot[2];
  int pad;
};
static_assert(sizeof(TexBlock) == 32, "a block record is 32 bytes");

// a face's record as the ABI hands it out (hsk_texture_chart): all -1 for a skipped face
struct TexChart {
  int x0, y0, s, half_rot;  // half | rotation << 8
};

struct TexLayout {
  long long W = 0, H = 0;  // H: the height the mesh needs, whether or not an atlas may be that high
  unsigned long long n_charted = 0, n_skipped = 0, n_blocks[4] = {0, 0, 0, 0};  // blocks of side 8, 16, 32, 64
  std::vector<TexBlock> blocks;
  std::vector<unsigned> tiles;  // (W / 8) x (H / 8) words, row-major: the tile's block, or TEX_EMPTY; empty when H > TEX_MAX_SIDE
  std::vector<TexChart> charts;
};

// the x (even bits) and y (odd bits) of a 6-bit Morton code
static inline void tex_morton6(unsigned m, int& x, int& y) {
  x = (int)((m & 1u) | ((m >> 1) & 2u) | ((m >> 2) & 4u));
  y = (int)(((m >> 1) & 1u) | ((m >> 2) & 2u) | ((m >> 3) & 4u));
}

static inline bool tex_finite(float v) { return v - v == 0.0f; }

// A face's block side (0: the face is skipped) and rotation r: chart corner j holds face corner (j + r) mod 3, r the corner
// opposite the longest edge -- it sits at the chart's right angle.
static inline int tex_face_side(const float* vertices, size_t n_vertices, const int32_t* f, double tpm, int* rot) {
  for (int c = 0; c < 3; ++c)
    if (f[c] < 0 || (size_t)f[c] >= n_vertices) return 0;
  if (f[0] == f[1] || f[1] == f[2] || f[0] == f[2]) return 0;
  const float* p[3] = {vertices + 3 * (size_t)f[0], vertices + 3 * (size_t)f[1], vertices + 3 * (size_t)f[2]};
  for (int c = 0; c < 3; ++c)
    for (int a = 0; a < 3; ++a)
      if (!tex_finite(p[c][a])) return 0;
  double L2 = -1.0;
  int kmax = 0;
  for (int k = 0; k < 3; ++k) {  // edge k joins corners k and k + 1 mod 3
    const float *a = p[k], *b = p[(k + 1) % 3];
    const double dx = (double)b[0] - (double)a[0], dy = (double)b[1] - (double)a[1], dz = (double)b[2] - (double)a[2];
    const double e2 = (dx * dx + dy * dy) + dz * dz;
    if (e2 > L2) L2 = e2, kmax = k;
  }
  if (!(L2 > 0.0)) return 0;
  *rot = (kmax + 2) % 3;
  const double T = L2 * (tpm * tpm);
  for (int s = 8; s <= 64; s *= 2)
    if ((double)((s - 5) * (s - 5)) >= T) return s;
  return 64;
}

// The layout of a mesh at tpm texels per metre in an atlas W wide (a multiple of 64 in 64 .. TEX_MAX_SIDE): the blocks, largest
// size first and in ascending face order within a size, two faces to a block; the tile table (only while H <= TEX_MAX_SIDE); a
// chart per face.  uv (may be null; only while 0 < H <= TEX_MAX_SIDE): 6 floats per face in the face's corner order.
static inline void tex_layout(const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces, double tpm, int W, TexLayout& L,
                              float* uv) {
  L = TexLayout();
  L.W = W;
  std::vector<unsigned char> side(n_faces), rot(n_faces);
  for (size_t i = 0; i < n_faces; ++i) {
    int r = 0;
    side[i] = (unsigned char)tex_face_side(vertices, n_vertices, faces + 3 * i, tpm, &r);
    rot[i] = (unsigned char)r;
    if (side[i]) L.n_charted += 1; else L.n_skipped += 1;
  }
  L.charts.assign(n_faces, TexChart{-1, -1, -1, -1});
  const int cols = W / 64;
  unsigned long long off = 0;  // in 8 x 8 tiles
  for (int s = 64, q = 3; s >= 8; s /= 2, --q) {
    const unsigned long long per = (unsigned long long)((s / 8) * (s / 8));
    int half = 0;
    for (size_t i = 0; i < n_faces; ++i) {
      if (side[i] != s) continue;
      if (half == 0) {
        const unsigned long long st = off >> 6;
        int tx, ty;
        tex_morton6((unsigned)(off & 63u), tx, ty);
        TexBlock b;
        b.x0 = 64 * (int)(st % (unsigned long long)cols) + 8 * tx;
        b.y0 = (int)(64 * (st / (unsigned long long)cols)) + 8 * ty;  // (callers keep H within int: n_faces * 64 tiles at most)
        b.s = s;
        b.face[0] = b.face[1] = -1;
        b.rot[0] = b.rot[1] = 0;
        b.pad = 0;
        L.blocks.push_back(b);
        L.n_blocks[q] += 1;
        off += per;
      }
      TexBlock& b = L.blocks.back();
      b.face[half] = (int)i;
      b.rot[half] = rot[i];
      L.charts[i] = TexChart{b.x0, b.y0, s, half | ((int)rot[i] << 8)};
      half ^= 1;
    }
  }
  const unsigned long long supers = (off + 63) >> 6;
  L.H = (long long)(64 * ((supers + (unsigned long long)cols - 1) / (unsigned long long)cols));
  if (L.H > TEX_MAX_SIDE) return;
  const int tw = W / 8;
  L.tiles.assign((size_t)tw * (size_t)(L.H / 8), TEX_EMPTY);
  for (size_t bi = 0; bi < L.blocks.size(); ++bi) {
    const TexBlock& b = L.blocks[bi];
    for (int ty = 0; ty < b.s / 8; ++ty)
      for (int tx = 0; tx < b.s / 8; ++tx) L.tiles[(size_t)(b.y0 / 8 + ty) * tw + (size_t)(b.x0 / 8 + tx)] = (unsigned)bi;
  }
  if (!uv) return;
  for (size_t i = 0; i < n_faces; ++i) {
    float* o = uv + 6 * i;
    for (int c = 0; c < 6; ++c) o[c] = 0.0f;
    const TexChart& ch = L.charts[i];
    if (ch.s < 0) continue;
    const int s = ch.s, half = ch.half_rot & 255, r = ch.half_rot >> 8;
    const int cx[3] = {1, s - 4, 1}, cy[3] = {1, 1, s - 4};
    for (int j = 0; j < 3; ++j) {
      const int x = ch.x0 + (half ? s - cx[j] : cx[j]), y = ch.y0 + (half ? s - cy[j] : cy[j]);
      const int c = (j + r) % 3;
      o[2 * c] = (float)((double)x / (double)L.W);
      o[2 * c + 1] = (float)(1.0 - (double)y / (double)L.H);
    }
  }
}

// ---- one texel ------------------------------------------------------------------------------------------------------------------
struct TexArgs {
  int W, H;            // the atlas, in texels
  int n_iter;          // projection steps, 0 .. TEX_MAX_ITER
  float f_tol;         // |F| up to this is on the surface (F in units of tau)
  float max_offset2;   // the projection may move a point by up to the root of this, in metres
};

struct TexelOut {
  unsigned mask;
  unsigned rgb[3], nrm[3];
  float p[3];  // the final point (the harness and the tests look at it; the kernel does not store it)
};

struct TexSample {
  SampleCell sc;
  float f[8];
  bool valid;  // inside the shell of samples and no tap never observed
};
HSK_HD void tex_sample(const unsigned* vol, const SampleVol& v, float px, float py, float pz, TexSample& s) {
  unsigned w[8];
  s.sc = hsk_sample_cell(v, px, py, pz);
  hsk_sample_words(vol, v, s.sc, w);
  s.valid = s.sc.in && hsk_sample_min_weight(w) > 0;
  hsk_sample_values(w, s.f);
}

// What a texel's colour and normal are taken at: its final point (the projection's, or P0 where that failed), the sample there and
// the mask's OWNED, INSIDE and PROJECTED bits (0: an unowned texel, nothing else set).  tex_texel is this, then tex_colour and
// tex_normal; the keyframe bake (hsk_keytex_point.h) takes the same point and asks its keyframes for the colour.
struct TexPoint {
  unsigned mask;
  float p[3];
  TexSample sm;
};

// Texel (px, py) of the atlas: vol = the TSDF in the device's block layout.  tiles, blocks, faces and vertices are the layout's and
// the mesh's.
HSK_HD void tex_point(const unsigned* vol, const SampleVol& v, const TexArgs& ta, const unsigned* tiles, const TexBlock* blocks, const int* faces,
                      const float* vertices, int px, int py, TexPoint& tp) {
  tp.mask = 0u;
  tp.p[0] = tp.p[1] = tp.p[2] = 0.0f;
  TexSample& sm = tp.sm;
  sm.valid = false;
  const unsigned tile = tiles[(size_t)(py >> 3) * (size_t)(ta.W >> 3) + (size_t)(px >> 3)];
  if (tile == TEX_EMPTY) return;
  const TexBlock& b = blocks[tile];
  const int s = b.s, i = px - b.x0, j = py - b.y0;
  const int half = (i + j <= s - 2) ? 0 : 1;
  const int face = b.face[half];
  if (face < 0) return;
  const int r = b.rot[half];
  // the point on the face: barycentrics by the chart's affine inverse, half B mirrored first
  float x = (float)i + 0.5f, y = (float)j + 0.5f;
  if (half) {
    x = (float)s - x;
    y = (float)s - y;
  }
  const float d = (float)(s - 5);
  const float bu = (x - 1.0f) / d, bv = (y - 1.0f) / d;
  const float bw = (1.0f - bu) - bv;
  const int* fc = faces + 3 * (size_t)face;
  const int i1 = r == 2 ? 0 : r + 1, i2 = r == 0 ? 2 : r - 1;  // (r + 1) mod 3, (r + 2) mod 3
  const float* c0 = vertices + 3 * (size_t)fc[r];
  const float* c1 = vertices + 3 * (size_t)fc[i1];
  const float* c2 = vertices + 3 * (size_t)fc[i2];
  const float p0x = (c0[0] + bu * (c1[0] - c0[0])) + bv * (c2[0] - c0[0]);
  const float p0y = (c0[1] + bu * (c1[1] - c0[1])) + bv * (c2[1] - c0[1]);
  const float p0z = (c0[2] + bu * (c1[2] - c0[2])) + bv * (c2[2] - c0[2]);
  unsigned mask = TEX_OWNED | ((bu >= 0.0f && bv >= 0.0f && bw >= 0.0f) ? TEX_INSIDE : 0u);
  // the projection onto the zero level set: Newton steps along the gradient, from P0
  float qx = p0x, qy = p0y, qz = p0z;
  bool projected = false;
  for (int it = 0;; ++it) {
    tex_sample(vol, v, qx, qy, qz, sm);
    if (!sm.valid) break;
    const float F = hsk_sample_blend(sm.f, sm.sc.a, sm.sc.b, sm.sc.c);
    if (fabsf(F) <= ta.f_tol) {
      projected = true;
      break;
    }
    if (it >= ta.n_iter) break;
    float gx, gy, gz;
    hsk_sample_gradient(sm.f, sm.sc.a, sm.sc.b, sm.sc.c, v.icell, gx, gy, gz);
    const float gg = hsk_dot3(gx, gy, gz, gx, gy, gz);
    if (!(gg > 0.0f)) break;
    const float t = F / gg;
    qx = qx - t * gx;
    qy = qy - t * gy;
    qz = qz - t * gz;
    const float ex = qx - p0x, ey = qy - p0y, ez = qz - p0z;
    if (!(hsk_dot3(ex, ey, ez, ex, ey, ez) <= ta.max_offset2)) break;
  }
  if (projected) {
    mask |= TEX_PROJECTED;
  } else {  // the texel uses P0
    qx = p0x, qy = p0y, qz = p0z;
    tex_sample(vol, v, qx, qy, qz, sm);
  }
  tp.p[0] = qx, tp.p[1] = qy, tp.p[2] = qz;
  tp.mask = mask;
}

// the colour at a sample's cell: the eight taps' trilinear mean over the taps that have a colour, in the blend's term order.
// colv = the colour volume, row-major.  false: the point is outside the shell or no tap has a colour (rgb untouched)
HSK_HD bool tex_colour(const unsigned* colv, const SampleVol& v, const SampleCell& sc, unsigned rgb[3]) {
  if (!sc.in) return false;
  const float a0 = 1.0f - sc.a, b0 = 1.0f - sc.b, e0 = 1.0f - sc.c;
  const float wt[8] = {a0 * b0 * e0, a0 * b0 * sc.c, a0 * sc.b * e0, a0 * sc.b * sc.c, sc.a * b0 * e0, sc.a * b0 * sc.c, sc.a * sc.b * e0,
                       sc.a * sc.b * sc.c};
  const int order[8] = {0, 4, 2, 6, 1, 5, 3, 7};  // dx + 2 dy + 4 dz of each term
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
  HSK_UNROLL
  for (int k = 0; k < 8; ++k) {
    const int t = order[k];
    const unsigned cw = colv[((size_t)(sc.z + (t >> 2)) * (size_t)v.Y + (size_t)(sc.y + ((t >> 1) & 1))) * (size_t)v.X + (size_t)(sc.x + (t & 1))];
    const float w = (cw >> 24) ? wt[k] : 0.0f;
    sw = sw + w;
    sr = sr + w * (float)(cw & 255u);
    sg = sg + w * (float)((cw >> 8) & 255u);
    sb = sb + w * (float)((cw >> 16) & 255u);
  }
  if (!(sw > 0.0f)) return false;
  rgb[0] = (unsigned)hsk_min_i(255, (int)(sr / sw + 0.5f));
  rgb[1] = (unsigned)hsk_min_i(255, (int)(sg / sw + 0.5f));
  rgb[2] = (unsigned)hsk_min_i(255, (int)(sb / sw + 0.5f));
  return true;
}

// the normal at a sample: its gradient to length 1, n, and as colour levels, nrm.  false: no valid sample or no gradient (both
// untouched)
HSK_HD bool tex_normal(const TexSample& sm, const SampleVol& v, float n[3], unsigned nrm[3]) {
  if (!sm.valid) return false;
  float gx, gy, gz;
  hsk_sample_gradient(sm.f, sm.sc.a, sm.sc.b, sm.sc.c, v.icell, gx, gy, gz);
  const float gg = hsk_dot3(gx, gy, gz, gx, gy, gz);
  if (!(gg > 0.0f)) return false;
  const float len = sqrtf(gg);
  n[0] = gx / len, n[1] = gy / len, n[2] = gz / len;
  nrm[0] = hsk_normal_level(n[0]);
  nrm[1] = hsk_normal_level(n[1]);
  nrm[2] = hsk_normal_level(n[2]);
  return true;
}

// Texel (px, py) of the atlas with its colour from the colour volume colv, row-major (null: no colour)
HSK_HD void tex_texel(const unsigned* vol, const unsigned* colv, const SampleVol& v, const TexArgs& ta, const unsigned* tiles,
                      const TexBlock* blocks, const int* faces, const float* vertices, int px, int py, TexelOut& o) {
  o.rgb[0] = o.rgb[1] = o.rgb[2] = 0u;
  o.nrm[0] = o.nrm[1] = o.nrm[2] = 0u;
  TexPoint tp;
  tex_point(vol, v, ta, tiles, blocks, faces, vertices, px, py, tp);
  o.mask = tp.mask;
  o.p[0] = tp.p[0], o.p[1] = tp.p[1], o.p[2] = tp.p[2];
  if (!(tp.mask & TEX_OWNED)) return;
  if (colv && tex_colour(colv, v, tp.sm.sc, o.rgb)) o.mask |= TEX_COLORED;
  float n[3];
  if (tex_normal(tp.sm, v, n, o.nrm)) o.mask |= TEX_NORMAL;
}
