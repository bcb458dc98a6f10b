// hsk_sample.h -- the trilinear TSDF sample at a point, once, for every kernel that takes one: the
// raycast and the views (hsk_march.h: trilinear), the normals of the cloud and the indexed mesh (extract.hip), fusion (fuse.hip)
// and alignment (hsk_align_point.h).  Plain C++ with no HIP type in it: tests/sample_harness.cpp compiles the same text for the
// host and tests/test_sample_host.py compares it with the numpy twins bit for bit, without a GPU.  One rounding per written
// operator (every build forbids contraction); the expression trees are the specification's: do not re-associate them.
//
// A caller composes what it uses: hsk_sample_cell locates the point; hsk_sample_taps gives the eight words of a whole volume
// (the march forms its own 64-bit terms: it knows slabs); hsk_sample_blend, hsk_sample_gradient and hsk_sample_min_weight work
// on the eight values.  Eight values are always in memory order, x fastest: index dx + 2 dy + 4 dz.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define HSK_HD static __host__ __device__ __forceinline__
#else
#define HSK_HD static inline
#endif

// (float)raw / 32767.0f of the specification, for an integer raw in [-32768, 32767], without the ~10-instruction
// correctly-rounded f32 division: the product with the binary64 reciprocal, rounded to binary32, equals the binary32
// quotient for EVERY such raw (checked exhaustively in tests/test_host_logic.py).
HSK_HD float hsk_tsdf_unpack(int raw) { return (float)((double)raw * (1.0 / 32767.0)); }

// x / c of the specification for a fixed binary32 divisor c, as a binary64 product with the correctly rounded binary64
// reciprocal rc: a binary32 quotient of two binary32 numbers is either exact or at least 2^-48 (relative) away from a
// rounding boundary (ties need c to be a power of two, where rc is exact), and the product is within 2^-52 of it.
HSK_HD float hsk_div_by_const(float x, double rc) { return (float)((double)x * rc); }

HSK_HD float hsk_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// a unit normal's component as a colour level (HSK_VIEW_NORMALS; the baked normal map of 8s)
HSK_HD unsigned hsk_normal_level(float n) { return (unsigned)(int)rintf((n * 0.5f + 0.5f) * 255.0f); }

HSK_HD int hsk_min_i(int a, int b) { return a < b ? a : b; }
HSK_HD int hsk_max_i(int a, int b) { return a > b ? a : b; }

// voxel index from the quotient q = p / cell: floor, with the specification's range guards (the oracle's vox_of; NaN: -1)
HSK_HD int hsk_vox_of_q(float quot) {
  const float q = floorf(quot);
  if (!(q >= 0.0f)) return -1;
  if (q > 1.0e6f) return 1000000;
  return (int)q;
}

// the halves of a voxel's 32-bit pair word
HSK_HD int hsk_pair_raw(unsigned w) { return (int)(short)(w & 0xffffu); }
HSK_HD int hsk_pair_wgt(unsigned w) { return (int)(short)(w >> 16); }

// what a sampler needs of a volume's geometry (VolParams carries three times as much, and fusion's scalar registers are full);
// the functions below take either: they are templates over anything with these members
struct SampleVol {
  int X, Y, Z;
  float cell[3];
  double icell[3];  // correctly rounded binary64 reciprocals of cell[]
};

// the voxel that contains p: floor(p / cell), clamped into the grid (a voxel whatever p is, a NaN included)
template <class Vol>
HSK_HD void hsk_voxel_at(const Vol& v, float px, float py, float pz, int& x, int& y, int& z) {
  x = hsk_min_i(hsk_max_i(hsk_vox_of_q(hsk_div_by_const(px, v.icell[0])), 0), v.X - 1);
  y = hsk_min_i(hsk_max_i(hsk_vox_of_q(hsk_div_by_const(py, v.icell[1])), 0), v.Y - 1);
  z = hsk_min_i(hsk_max_i(hsk_vox_of_q(hsk_div_by_const(pz, v.icell[2])), 0), v.Z - 1);
}

// Where a point lies among the voxel centres.  Branch-free: the cell is clamped for the loads (every tap lies inside the volume
// whatever the point is) and `in` -- false: the sample is the NaN of the outer shell -- is selected behind them, so the taps of
// several samples can be in flight together.
struct SampleCell {
  bool in;         // the containing voxel lies in [1, dims - 2] on every axis
  int cx, cy, cz;  // the containing voxel, clamped to that range (fusion's colour rule)
  int x, y, z;     // the lower corner of the eight taps: in [0, dims - 2]
  float a, b, c;   // the point's offset from the lower corner's centre, in cells
};
template <class Vol>
HSK_HD SampleCell hsk_sample_cell(const Vol& v, float px, float py, float pz) {
  SampleCell s;
  // floor(p / cell) and the fractions below are the spec's f32 quotients, obtained as binary64 products (hsk_div_by_const): 3
  // instructions each instead of a ~10-instruction correctly rounded division
  int gx = hsk_vox_of_q(hsk_div_by_const(px, v.icell[0])), gy = hsk_vox_of_q(hsk_div_by_const(py, v.icell[1])),
      gz = hsk_vox_of_q(hsk_div_by_const(pz, v.icell[2]));
  s.in = gx > 0 && gx < v.X - 1 && gy > 0 && gy < v.Y - 1 && gz > 0 && gz < v.Z - 1;
  s.cx = gx = hsk_min_i(hsk_max_i(gx, 1), v.X - 2);
  s.cy = gy = hsk_min_i(hsk_max_i(gy, 1), v.Y - 2);
  s.cz = gz = hsk_min_i(hsk_max_i(gz, 1), v.Z - 2);
  if (px < ((float)gx + 0.5f) * v.cell[0]) gx -= 1;
  if (py < ((float)gy + 0.5f) * v.cell[1]) gy -= 1;
  if (pz < ((float)gz + 0.5f) * v.cell[2]) gz -= 1;
  s.x = gx;
  s.y = gy;
  s.z = gz;
  s.a = hsk_div_by_const(px - ((float)gx + 0.5f) * v.cell[0], v.icell[0]);
  s.b = hsk_div_by_const(py - ((float)gy + 0.5f) * v.cell[1], v.icell[1]);
  s.c = hsk_div_by_const(pz - ((float)gz + 0.5f) * v.cell[2], v.icell[2]);
  return s;
}

// The eight taps' word indices in a whole volume's 64-B block layout (hsk_dev.h: hsk_vox_index; a volume holds fewer than 2^32
// words: hsk_create): one term per axis, the upper neighbours by steps -- +1 word in x (or into the next block: +13), one row
// pitch in y, +4 words in z (or into the next group of planes: the plane-group pitch - 12).
template <class Vol>
HSK_HD void hsk_sample_taps(const Vol& v, const SampleCell& s, unsigned t[8]) {
  const unsigned pitch = (unsigned)((v.X >> 2) << 4);
  const unsigned tx0 = (((unsigned)s.x >> 2) << 4) + ((unsigned)s.x & 3u), tx1 = tx0 + ((s.x & 3) == 3 ? 13u : 1u);
  const unsigned ty0 = (unsigned)s.y * pitch, ty1 = ty0 + pitch;
  const unsigned tz0 = ((unsigned)s.z >> 2) * (unsigned)v.Y * pitch + (((unsigned)s.z & 3u) << 2);
  const unsigned tz1 = tz0 + ((s.z & 3) == 3 ? (unsigned)v.Y * pitch - 12u : 4u);
  t[0] = tz0 + ty0 + tx0;
  t[1] = tz0 + ty0 + tx1;
  t[2] = tz0 + ty1 + tx0;
  t[3] = tz0 + ty1 + tx1;
  t[4] = tz1 + ty0 + tx0;
  t[5] = tz1 + ty0 + tx1;
  t[6] = tz1 + ty1 + tx0;
  t[7] = tz1 + ty1 + tx1;
}
// ... and the pair words there
template <class Vol>
HSK_HD void hsk_sample_words(const unsigned* vol, const Vol& v, const SampleCell& s, unsigned w[8]) {
  unsigned t[8];
  hsk_sample_taps(v, s, t);
  w[0] = vol[t[0]], w[1] = vol[t[1]], w[2] = vol[t[2]], w[3] = vol[t[3]];
  w[4] = vol[t[4]], w[5] = vol[t[5]], w[6] = vol[t[6]], w[7] = vol[t[7]];
}
HSK_HD void hsk_sample_values(const unsigned w[8], float f[8]) {
  f[0] = hsk_tsdf_unpack(hsk_pair_raw(w[0])), f[1] = hsk_tsdf_unpack(hsk_pair_raw(w[1]));
  f[2] = hsk_tsdf_unpack(hsk_pair_raw(w[2])), f[3] = hsk_tsdf_unpack(hsk_pair_raw(w[3]));
  f[4] = hsk_tsdf_unpack(hsk_pair_raw(w[4])), f[5] = hsk_tsdf_unpack(hsk_pair_raw(w[5]));
  f[6] = hsk_tsdf_unpack(hsk_pair_raw(w[6])), f[7] = hsk_tsdf_unpack(hsk_pair_raw(w[7]));
}

// the eight-term sum, in the specification's order (z fastest) and association
HSK_HD float hsk_sample_blend(const float f[8], float a, float b, float c) {
  float res = f[0] * (1.0f - a) * (1.0f - b) * (1.0f - c);
  res = res + f[4] * (1.0f - a) * (1.0f - b) * c;
  res = res + f[2] * (1.0f - a) * b * (1.0f - c);
  res = res + f[6] * (1.0f - a) * b * c;
  res = res + f[1] * a * (1.0f - b) * (1.0f - c);
  res = res + f[5] * a * (1.0f - b) * c;
  res = res + f[3] * a * b * (1.0f - c);
  res = res + f[7] * a * b * c;
  return res;
}

// the gradient of the same trilinear form from the same eight values, divided by the cells
HSK_HD void hsk_sample_gradient(const float f[8], float a1, float b1, float c1, const double icell[3], float& gx, float& gy, float& gz) {
  const float a0 = 1.0f - a1, b0 = 1.0f - b1, c0 = 1.0f - c1;
  const float sx = ((((f[1] - f[0]) * b0 * c0 + (f[5] - f[4]) * b0 * c1) + (f[3] - f[2]) * b1 * c0) + (f[7] - f[6]) * b1 * c1);
  const float sy = ((((f[2] - f[0]) * a0 * c0 + (f[6] - f[4]) * a0 * c1) + (f[3] - f[1]) * a1 * c0) + (f[7] - f[5]) * a1 * c1);
  const float sz = ((((f[4] - f[0]) * a0 * b0 + (f[6] - f[2]) * a0 * b1) + (f[5] - f[1]) * a1 * b0) + (f[7] - f[3]) * a1 * b1);
  gx = hsk_div_by_const(sx, icell[0]);
  gy = hsk_div_by_const(sy, icell[1]);
  gz = hsk_div_by_const(sz, icell[2]);
}

// the smallest weight of the eight taps (0: one of them was never observed)
HSK_HD int hsk_sample_min_weight(const unsigned w[8]) {
  return hsk_min_i(hsk_min_i(hsk_min_i(hsk_pair_wgt(w[0]), hsk_pair_wgt(w[1])), hsk_min_i(hsk_pair_wgt(w[2]), hsk_pair_wgt(w[3]))),
                   hsk_min_i(hsk_min_i(hsk_pair_wgt(w[4]), hsk_pair_wgt(w[5])), hsk_min_i(hsk_pair_wgt(w[6]), hsk_pair_wgt(w[7]))));
}
