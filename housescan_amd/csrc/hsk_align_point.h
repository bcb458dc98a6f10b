// hsk_align_point.h -- volume alignment, the work on ONE point: the probes along the normal, the
// choice among them, the row and its 28 quantised products.  align.hip's kernel calls it per lane; it is plain C++ with no HIP
// type in it, so that tests/align_point_harness.cpp compiles the same text for the host and tests/test_align_host.py compares
// it with the numpy twin bit for bit, without a GPU.  One rounding per written operator: both builds forbid contraction.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define HSK_ALIGN_HD static __host__ __device__ __forceinline__
#define HSK_ALIGN_UNROLL _Pragma("unroll")
#else
#define HSK_ALIGN_HD static inline
#define HSK_ALIGN_UNROLL
#endif

#define ALIGN_SCALE 67108864.0  // 2^26

// what the kernel needs of the destination's geometry
struct AlignVol {
  int X, Y, Z;
  float cell[3];
  double icell[3];
};
struct AlignArgs {
  float R[9], t[3];  // source -> destination
  float c[3];        // the destination's centre
  float tau, cos_gate;
  int J;             // probes to either side
  unsigned n, pitch; // points; floats between two planes of the cloud
};

// hsk_dev.h's hsk_tsdf_unpack, hsk_div_by_const and hsk_dot3, restated for both sides (those are device functions)
HSK_ALIGN_HD float align_tsdf_unpack(int raw) { return (float)((double)raw * (1.0 / 32767.0)); }
HSK_ALIGN_HD float align_div_by_const(float x, double rc) { return (float)((double)x * rc); }
HSK_ALIGN_HD float align_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
HSK_ALIGN_HD int align_min(int a, int b) { return a < b ? a : b; }
HSK_ALIGN_HD int align_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// floor of a quotient with the specification's range guards (the oracle's vox_of)
HSK_ALIGN_HD int align_vox_of_q(float quot) {
  const float q = floorf(quot);
  if (!(q >= 0.0f)) return -1;
  if (q > 1.0e6f) return 1000000;
  return (int)q;
}
HSK_ALIGN_HD int align_raw(unsigned w) { return (int)(short)(w & 0xffffu); }
HSK_ALIGN_HD int align_wgt(unsigned w) { return (int)(short)(w >> 16); }

// One probe at (px, py, pz): the sample F, the gradient (gx, gy, gz) and `ok`: not the NaN of the outer shell and no tap never
// observed.  Branch-free: the indices are clamped for the loads (every tap lies inside the volume whatever the point is, a
// NaN included) and the verdict is selected behind them.
HSK_ALIGN_HD bool align_probe(const unsigned* vol, const AlignVol& dv, float px, float py, float pz, float& F, float& gx, float& gy,
                              float& gz) {
  int ix = align_vox_of_q(align_div_by_const(px, dv.icell[0])), iy = align_vox_of_q(align_div_by_const(py, dv.icell[1])),
      iz = align_vox_of_q(align_div_by_const(pz, dv.icell[2]));
  const bool in = ix > 0 && ix < dv.X - 1 && iy > 0 && iy < dv.Y - 1 && iz > 0 && iz < dv.Z - 1;
  ix = align_clamp(ix, 1, dv.X - 2);
  iy = align_clamp(iy, 1, dv.Y - 2);
  iz = align_clamp(iz, 1, dv.Z - 2);
  if (px < ((float)ix + 0.5f) * dv.cell[0]) ix -= 1;
  if (py < ((float)iy + 0.5f) * dv.cell[1]) iy -= 1;
  if (pz < ((float)iz + 0.5f) * dv.cell[2]) iz -= 1;
  const float a1 = align_div_by_const(px - ((float)ix + 0.5f) * dv.cell[0], dv.icell[0]);
  const float b1 = align_div_by_const(py - ((float)iy + 0.5f) * dv.cell[1], dv.icell[1]);
  const float c1 = align_div_by_const(pz - ((float)iz + 0.5f) * dv.cell[2], dv.icell[2]);
  const float a0 = 1.0f - a1, b0 = 1.0f - b1, c0 = 1.0f - c1;
  // word indices (a volume holds fewer than 2^32 words: hsk_create): one term per axis, the upper neighbours by steps -- +1
  // word in x (or into the next block: +13), one row pitch in y, +4 words in z (or into the next group of planes)
  const unsigned pitch = (unsigned)((dv.X >> 2) << 4);
  const unsigned tx0 = (((unsigned)ix >> 2) << 4) + ((unsigned)ix & 3u), tx1 = tx0 + ((ix & 3) == 3 ? 13u : 1u);
  const unsigned ty0 = (unsigned)iy * pitch, ty1 = ty0 + pitch;
  const unsigned tz0 = ((unsigned)iz >> 2) * (unsigned)dv.Y * pitch + (((unsigned)iz & 3u) << 2);
  const unsigned tz1 = tz0 + ((iz & 3) == 3 ? (unsigned)dv.Y * pitch - 12u : 4u);
  const unsigned w000 = vol[tz0 + ty0 + tx0], w100 = vol[tz0 + ty0 + tx1], w010 = vol[tz0 + ty1 + tx0], w110 = vol[tz0 + ty1 + tx1];
  const unsigned w001 = vol[tz1 + ty0 + tx0], w101 = vol[tz1 + ty0 + tx1], w011 = vol[tz1 + ty1 + tx0], w111 = vol[tz1 + ty1 + tx1];
  const int Ws = align_min(align_min(align_min(align_wgt(w000), align_wgt(w100)), align_min(align_wgt(w010), align_wgt(w110))),
                           align_min(align_min(align_wgt(w001), align_wgt(w101)), align_min(align_wgt(w011), align_wgt(w111))));
  const float f000 = align_tsdf_unpack(align_raw(w000)), f100 = align_tsdf_unpack(align_raw(w100));
  const float f010 = align_tsdf_unpack(align_raw(w010)), f110 = align_tsdf_unpack(align_raw(w110));
  const float f001 = align_tsdf_unpack(align_raw(w001)), f101 = align_tsdf_unpack(align_raw(w101));
  const float f011 = align_tsdf_unpack(align_raw(w011)), f111 = align_tsdf_unpack(align_raw(w111));
  float res = f000 * a0 * b0 * c0;
  res = res + f001 * a0 * b0 * c1;
  res = res + f010 * a0 * b1 * c0;
  res = res + f011 * a0 * b1 * c1;
  res = res + f100 * a1 * b0 * c0;
  res = res + f101 * a1 * b0 * c1;
  res = res + f110 * a1 * b1 * c0;
  res = res + f111 * a1 * b1 * c1;
  F = res;
  // the gradient of the same trilinear form, from the same eight registers
  const float sx = ((((f100 - f000) * b0 * c0 + (f101 - f001) * b0 * c1) + (f110 - f010) * b1 * c0) + (f111 - f011) * b1 * c1);
  const float sy = ((((f010 - f000) * a0 * c0 + (f011 - f001) * a0 * c1) + (f110 - f100) * a1 * c0) + (f111 - f101) * a1 * c1);
  const float sz = ((((f001 - f000) * a0 * b0 + (f011 - f010) * a0 * b1) + (f101 - f100) * a1 * b0) + (f111 - f110) * a1 * b1);
  gx = align_div_by_const(sx, dv.icell[0]);
  gy = align_div_by_const(sy, dv.icell[1]);
  gz = align_div_by_const(sz, dv.icell[2]);
  return in && Ws > 0;
}

// One point (x, y, z) with normal (nx, ny, nz) in source coordinates: adds its 28 terms (integers, in units of 2^-26) to acc and
// returns true, or returns false when no probe is valid.
HSK_ALIGN_HD bool align_point(const unsigned* vol, const AlignVol& dv, const AlignArgs& aa, float x, float y, float z, float nx, float ny,
                              float nz, double* acc) {
  const float p0 = ((aa.R[0] * x + aa.R[1] * y) + aa.R[2] * z) + aa.t[0];
  const float p1 = ((aa.R[3] * x + aa.R[4] * y) + aa.R[5] * z) + aa.t[1];
  const float p2 = ((aa.R[6] * x + aa.R[7] * y) + aa.R[8] * z) + aa.t[2];
  const float n0 = (aa.R[0] * nx + aa.R[1] * ny) + aa.R[2] * nz;
  const float n1 = (aa.R[3] * nx + aa.R[4] * ny) + aa.R[5] * nz;
  const float n2 = (aa.R[6] * nx + aa.R[7] * ny) + aa.R[8] * nz;
  // the running best: |F| (2: none yet -- a valid probe has |F| < 1), F, nd, c_j, s_j
  float best = 2.0f, bF = 0.0f, bd0 = 0.0f, bd1 = 0.0f, bd2 = 0.0f, bc = 0.0f, bs = 0.0f;
  for (int jj = 0; jj <= 2 * aa.J; ++jj) {  // j = 0, +1, -1, +2, -2, ..
    const int h = (jj + 1) >> 1;
    const float sj = (float)((jj & 1) ? h : -h) * aa.tau;
    float F, gx, gy, gz;
    const bool ok = align_probe(vol, dv, p0 + sj * n0, p1 + sj * n1, p2 + sj * n2, F, gx, gy, gz);
    const float gg = align_dot3(gx, gy, gz, gx, gy, gz);
    const float len = sqrtf(gg);
    const float d0 = gx / len, d1 = gy / len, d2 = gz / len;
    const float cj = align_dot3(n0, n1, n2, d0, d1, d2);
    const float aF = fabsf(F);
    const bool take = ok & (aF < 1.0f) & (gg > 0.0f) & (cj >= aa.cos_gate) & (aF < best);
    best = take ? aF : best;
    bF = take ? F : bF;
    bd0 = take ? d0 : bd0;
    bd1 = take ? d1 : bd1;
    bd2 = take ? d2 : bd2;
    bc = take ? cj : bc;
    bs = take ? sj : bs;
  }
  if (best < 2.0f) {
    const float q0 = p0 - aa.c[0], q1 = p1 - aa.c[1], q2 = p2 - aa.c[2];
    const float row[7] = {q1 * bd2 - q2 * bd1, q2 * bd0 - q0 * bd2, q0 * bd1 - q1 * bd0, bd0, bd1, bd2, bs * bc - bF * aa.tau};
    double rd[7], rs[7];
    HSK_ALIGN_UNROLL
    for (int a = 0; a < 7; ++a) {
      rd[a] = (double)row[a];
      rs[a] = rd[a] * ALIGN_SCALE;
    }
    int k = 0;  // (unrolled: acc stays in registers)
    HSK_ALIGN_UNROLL
    for (int a = 0; a < 6; ++a)
      HSK_ALIGN_UNROLL
      for (int b = a; b < 7; ++b) {
        acc[k] = acc[k] + rint(rs[a] * rd[b]);
        ++k;
      }
    acc[27] = acc[27] + rint(rs[6] * rd[6]);
    return true;
  }
  return false;
}
