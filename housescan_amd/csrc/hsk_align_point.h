// hsk_align_point.h -- volume alignment, the work on ONE point: the probes along the normal, the
// choice among them, the row and its 28 quantised products.  align.hip's kernel calls it per lane; like hsk_sample.h, whose
// sample a probe is, it is plain C++ with no HIP type in it, so that tests/align_point_harness.cpp compiles the same text for
// the host and tests/test_align_host.py compares it with the numpy twin bit for bit, without a GPU.  One rounding per written
// operator: both builds forbid contraction.
#pragma once
#include "hsk_sample.h"
#ifndef HSK_UNROLL
#if defined(__HIPCC__)
#define HSK_UNROLL _Pragma("unroll")
#else
#define HSK_UNROLL
#endif
#endif

#define ALIGN_SCALE 67108864.0  // 2^26

typedef SampleVol AlignVol;  // the destination's geometry, under the name this header's callers fill it by

struct AlignArgs {
  float R[9], t[3];  // source -> destination
  float c[3];        // the destination's centre
  float tau, cos_gate;
  int J;             // probes to either side
  unsigned n, pitch; // points; floats between two planes of the cloud
};

// One probe at (px, py, pz): the sample F, the gradient (gx, gy, gz) and `ok`: not the NaN of the outer shell and no tap never
// observed.  Branch-free (hsk_sample.h): every tap lies inside the volume whatever the point is, a NaN included, and the verdict
// is selected behind the loads.
HSK_HD bool align_probe(const unsigned* vol, const SampleVol& dv, float px, float py, float pz, float& F, float& gx, float& gy, float& gz) {
  const SampleCell sc = hsk_sample_cell(dv, px, py, pz);
  unsigned w[8];
  float f[8];
  hsk_sample_words(vol, dv, sc, w);
  const int Ws = hsk_sample_min_weight(w);
  hsk_sample_values(w, f);
  F = hsk_sample_blend(f, sc.a, sc.b, sc.c);
  hsk_sample_gradient(f, sc.a, sc.b, sc.c, dv.icell, gx, gy, gz);
  return sc.in && Ws > 0;
}

// One point (x, y, z) with normal (nx, ny, nz) in source coordinates: adds its 28 terms (integers, in units of 2^-26) to acc and
// returns true, or returns false when no probe is valid.
HSK_HD bool align_point(const unsigned* vol, const SampleVol& dv, const AlignArgs& aa, float x, float y, float z, float nx, float ny,
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
    const float gg = hsk_dot3(gx, gy, gz, gx, gy, gz);
    const float len = sqrtf(gg);
    const float d0 = gx / len, d1 = gy / len, d2 = gz / len;
    const float cj = hsk_dot3(n0, n1, n2, d0, d1, d2);
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
    HSK_UNROLL
    for (int a = 0; a < 7; ++a) {
      rd[a] = (double)row[a];
      rs[a] = rd[a] * ALIGN_SCALE;
    }
    int k = 0;  // (unrolled: acc stays in registers)
    HSK_UNROLL
    for (int a = 0; a < 6; ++a)
      HSK_UNROLL
      for (int b = a; b < 7; ++b) {
        acc[k] = acc[k] + rint(rs[a] * rd[b]);
        ++k;
      }
    acc[27] = acc[27] + rint(rs[6] * rd[6]);
    return true;
  }
  return false;
}
