// level_point_harness.cpp -- the upright-frame estimate's work on one point (housescan_amd/csrc/hsk_level_point.h) and the host's
// steps between the device stages (hsk_level_solve.h), compiled for the host: the three device questions are answered by plain
// loops over the point functions, and level_estimate asks them in its order.  tests/test_level_host.py feeds it a cloud and
// compares every answer and every field of the result with the numpy twin.  Input file: n (uint32), the parameters (36 bytes),
// three cell weights (float), six planes of n floats (x, y, z, nx, ny, nz).  Output: one line per question -- "hist" and its 1536
// counts; "sums" and the 12 + 3 sums; "extents", the box's six words, then for every non-empty height bin "class bin count sum" --
// then "result": the 32 words of hsk_upright.
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_level_solve.h"
#include "harness_io.h"

struct HostStages {
  const float *X, *Y, *Z, *NX, *NY, *NZ;
  unsigned n;
  float w[3];
  double cone2, wall2;

  LevelPoint at(unsigned i) const { return level_point(X[i], Y[i], Z[i], NX[i], NY[i], NZ[i], w[0], w[1], w[2]); }
  static long long len2(const int32_t a[3]) { return level_dot(a, a); }

  int hist(uint32_t* h, uint64_t* n_valid) {
    for (int b = 0; b < HSK_LEVEL_HIST_BINS; ++b) h[b] = 0;
    *n_valid = 0;
    for (unsigned i = 0; i < n; ++i) {
      const LevelPoint q = at(i);
      if (!q.valid) continue;
      h[level_hist_bin(q.N)] += 1;
      *n_valid += 1;
    }
    printf("hist");
    for (int b = 0; b < HSK_LEVEL_HIST_BINS; ++b) printf(" %u", h[b]);
    printf("\n");
    return 0;
  }
  int sums(const int32_t A[3][3], int n_axes, int64_t s12[12], const int32_t W[3][3], int64_t w3[3]) {
    for (int v = 0; v < 12; ++v) s12[v] = 0;
    for (int v = 0; v < 3; ++v) w3[v] = 0;
    for (unsigned i = 0; i < n; ++i) {
      const LevelPoint q = at(i);
      if (!q.valid) continue;
      for (int a = 0; a < n_axes; ++a) {
        long long dot;
        if (!level_cone(q.N, A[a], len2(A[a]), cone2, true, dot)) continue;
        const long long sg = dot < 0 ? -1 : 1;
        s12[4 * a] += 1;
        for (int c = 0; c < 3; ++c) s12[4 * a + 1 + c] += sg * q.N[c];
      }
      if (W) {
        long long dot, re, im;
        if (!level_cone(q.N, W[0], len2(W[0]), wall2, false, dot)) continue;
        level_yaw_terms(q.N, W[1], W[2], re, im);
        w3[0] += 1, w3[1] += re, w3[2] += im;
      }
    }
    printf("sums");
    for (int v = 0; v < 12; ++v) printf(" %lld", (long long)s12[v]);
    for (int v = 0; v < 3; ++v) printf(" %lld", (long long)w3[v]);
    printf("\n");
    return 0;
  }
  int extents(const int32_t R[3][3], bool classes, int32_t box[6], uint32_t* cnt, int64_t* sum) {
    bool any = false;
    for (int v = 0; v < 6; ++v) box[v] = 0;
    for (size_t b = 0; b < (size_t)2 * HSK_LEVEL_H_BINS; ++b) cnt[b] = 0, sum[b] = 0;
    for (unsigned i = 0; i < n; ++i) {
      const LevelPoint q = at(i);
      if (!q.valid) continue;
      int t[3];
      for (int k = 0; k < 3; ++k) {
        t[k] = level_t(q.P, R[k]);
        box[k] = !any || t[k] < box[k] ? t[k] : box[k];
        box[3 + k] = !any || t[k] > box[3 + k] ? t[k] : box[3 + k];
      }
      any = true;
      long long dot;
      if (!classes || !level_cone(q.N, R[1], len2(R[1]), cone2, true, dot) || dot == 0) continue;
      const size_t key = (size_t)(dot > 0 ? HSK_LEVEL_H_BINS : 0) + (size_t)level_height_bin(t[1]);
      cnt[key] += 1, sum[key] += t[1];
    }
    printf("extents %d %d %d %d %d %d", box[0], box[1], box[2], box[3], box[4], box[5]);
    for (size_t b = 0; b < (size_t)2 * HSK_LEVEL_H_BINS; ++b)
      if (cnt[b]) printf(" %zu %zu %u %lld", b / HSK_LEVEL_H_BINS, b % HSK_LEVEL_H_BINS, cnt[b], (long long)sum[b]);
    printf("\n");
    return 0;
  }
};

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 1);
  unsigned n;
  hsk_upright_params p;
  HostStages st;
  if (!(in.get(&n, 1) && in.get(&p, 1) && in.get(st.w, 3))) return 2;
  std::vector<float> soa((size_t)n * 6);
  if (!in.get(soa)) return 2;
  st.n = n;
  st.X = soa.data(), st.Y = st.X + n, st.Z = st.Y + n, st.NX = st.Z + n, st.NY = st.NX + n, st.NZ = st.NY + n;
  st.cone2 = (double)p.cone_cos * (double)p.cone_cos;
  st.wall2 = (double)p.wall_sin * (double)p.wall_sin;
  std::vector<uint32_t> hist(HSK_LEVEL_HIST_BINS), cnt((size_t)2 * HSK_LEVEL_H_BINS);
  std::vector<int64_t> sum((size_t)2 * HSK_LEVEL_H_BINS);
  hsk_upright out;
  level_clear(&out, n);
  if (n > 0 && level_estimate(st, n, p, &out, hist.data(), cnt.data(), sum.data()) != 0) return 3;
  uint32_t words[sizeof(out) / 4];
  memcpy(words, &out, sizeof(out));
  printf("result");
  for (size_t v = 0; v < sizeof(out) / 4; ++v) printf(" %u", words[v]);
  printf("\n");
  return 0;
}
