// level.hip -- the upright-frame estimate for gfx950 (hsk_estimate_upright, hsk_estimate_upright_oriented, hsk_upright_sums;
// DESIGN.md 3.21 the kernels, 8o the rule): three streaming kernels over the n points of the alignment's six planes.  Each reads
// 24 bytes a point once and is bound by that; the host waits between them and solves in between (hsk_level_solve.h).
//
// The rule is per point in hsk_level_point.h.  Everything summed here is an integer, so any order of addition gives the same bits
// and no result depends on the launch shape; there is no floating-point atomic.
//
// k_level_hist: the cube-map histogram of the normals and the count of valid points.  A block counts in its own LDS -- the lanes of a
// wave that share a bin (neighbours on one face do) through one add -- and adds its non-zero bins to the zeroed result with integer
// atomics.
// k_level_sums: for up to three integer axes the count of supporters and the three signed sums, and for one up axis the wall
// points' count and their two fourth-power sums: 15 64-bit sums a lane, added over the wave by shuffles, over the block in LDS,
// stored per block and added by k_cloud_fold (planes.hip).
// k_level_extents: the min and max of the three levelled coordinates (per block, folded by k_cloud_fold as a box) and the two height
// histograms.  2 x 16384 bins of a count and a 64-bit sum do not fit LDS; they are global integer atomics, which only the
// up-facing and down-facing points reach, and a wave's lanes of one bin -- a floor is a few bins thick -- send one add of their
// count and one of their sum.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_cloud_dev.h"
#include "hsk_launch.h"
#include "hsk_level_point.h"

static __device__ __forceinline__ LevelPoint level_load(const float* __restrict__ soa, unsigned i, unsigned pitch, const LevelWeights& w) {
  const CloudPoint q = hsk_cloud_point(soa, i, pitch);
  return level_point(q.x, q.y, q.z, q.nx, q.ny, q.nz, w.w[0], w.w[1], w.w[2]);
}

// Every lane of the wave arrives.  The live lanes are grouped by `key`; each group's first lane gets *count = the group's size and
// *sum = the group's sum of v (SUM) and returns true, every other lane false.
template <bool SUM>
static __device__ __forceinline__ bool level_wave_groups(bool live, int key, long long v, unsigned* count, long long* sum) {
  const unsigned lane = threadIdx.x & 63u;
  unsigned long long todo = __ballot(live);
  bool lead = false;
  while (todo != 0ull) {  // (uniform over the wave)
    const int first = __ffsll((long long)todo) - 1;
    const int kf = __shfl(key, first, 64);
    const bool mine = live & (key == kf);
    const unsigned long long same = __ballot(mine);
    const long long s = SUM ? hsk_wave_sum(mine ? v : 0ll) : 0ll;
    if (lane == (unsigned)first) lead = true, *count = (unsigned)__popcll(same), *sum = s;
    todo &= ~same;
  }
  return lead;
}

__global__ __launch_bounds__(256) void k_level_hist(const float* __restrict__ soa, unsigned n, unsigned pitch, LevelWeights w,
                                                    unsigned* __restrict__ hist) {
  __shared__ unsigned acc[HSK_LEVEL_HIST_BINS + 1];  // the bins, then the valid points
  for (unsigned j = threadIdx.x; j <= (unsigned)HSK_LEVEL_HIST_BINS; j += 256u) acc[j] = 0u;
  __syncthreads();
  unsigned n_valid = 0u;  // (the wave's, in its lane 0)
  const unsigned rounds = (n + gridDim.x * 256u - 1u) / (gridDim.x * 256u);  // (uniform: every lane of a wave takes every round)
  for (unsigned r = 0; r < rounds; ++r) {
    const unsigned i = (r * gridDim.x + blockIdx.x) * 256u + threadIdx.x;  // (n <= 2^24: no wrap)
    const bool act = i < n;
    const LevelPoint q = level_load(soa, hsk_cloud_at(act, i, n), pitch, w);
    const bool live = act & q.valid;
    unsigned cnt;
    long long unused;
    if (level_wave_groups<false>(live, level_hist_bin(q.N), 0ll, &cnt, &unused)) atomicAdd(&acc[level_hist_bin(q.N)], cnt);
    n_valid += (unsigned)__popcll(__ballot(live));
  }
  if ((threadIdx.x & 63u) == 0u && n_valid != 0u) atomicAdd(&acc[HSK_LEVEL_HIST_BINS], n_valid);
  __syncthreads();
  for (unsigned j = threadIdx.x; j <= (unsigned)HSK_LEVEL_HIST_BINS; j += 256u)
    if (acc[j] != 0u) atomicAdd(&hist[j], acc[j]);
}

__global__ __launch_bounds__(256) void k_level_sums(const float* __restrict__ soa, unsigned n, unsigned pitch, LevelWeights w, LevelAxes ax,
                                                    unsigned long long* __restrict__ partial) {
  long long s[15];
#pragma unroll
  for (int v = 0; v < 15; ++v) s[v] = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const LevelPoint q = level_load(soa, i, pitch, w);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a >= ax.n_axes) break;  // (uniform)
      long long dot;
      const bool sup = q.valid & level_cone(q.N, ax.A[a], ax.aa[a], ax.cone2, true, dot);
      const long long sg = sup ? (dot < 0 ? -1 : 1) : 0;
      s[4 * a] += sup ? 1 : 0;
      s[4 * a + 1] += sg * q.N[0], s[4 * a + 2] += sg * q.N[1], s[4 * a + 3] += sg * q.N[2];
    }
    if (ax.wall) {
      long long dot, re, im;
      const bool wall = q.valid & level_cone(q.N, ax.W[0], ax.waa, ax.wall2, false, dot);
      level_yaw_terms(q.N, ax.W[1], ax.W[2], re, im);
      s[12] += wall ? 1 : 0;
      s[13] += wall ? re : 0, s[14] += wall ? im : 0;
    }
  }
  hsk_cloud_block_store<HskSum>(s, partial);
}

__global__ __launch_bounds__(256) void k_level_extents(const float* __restrict__ soa, unsigned n, unsigned pitch, LevelWeights w, LevelFrame fr,
                                                       unsigned long long* __restrict__ partial, unsigned* __restrict__ h_count,
                                                       unsigned long long* __restrict__ h_sum) {
  long long s[6];
#pragma unroll
  for (int v = 0; v < 6; ++v) s[v] = v < 3 ? 0x7fffffffll : -0x80000000ll;
  const unsigned rounds = (n + gridDim.x * 256u - 1u) / (gridDim.x * 256u);  // (uniform: every lane of a wave takes every round)
  for (unsigned r = 0; r < rounds; ++r) {
    const unsigned i = (r * gridDim.x + blockIdx.x) * 256u + threadIdx.x;
    const bool act = i < n;
    const LevelPoint q = level_load(soa, hsk_cloud_at(act, i, n), pitch, w);
    const bool live = act & q.valid;
    int t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t[k] = level_t(q.P, fr.R[k]);
      s[k] = live && t[k] < s[k] ? t[k] : s[k];
      s[3 + k] = live && t[k] > s[3 + k] ? t[k] : s[3 + k];
    }
    if (fr.classes) {  // (uniform)
      long long dot;
      const bool sup = live & level_cone(q.N, fr.R[1], fr.raa, fr.cone2, true, dot) & (dot != 0);
      const int key = (dot > 0 ? HSK_LEVEL_H_BINS : 0) + level_height_bin(t[1]);  // the floor class, then the ceiling class
      unsigned cnt;
      long long sum;
      if (level_wave_groups<true>(sup, key, (long long)t[1], &cnt, &sum)) {
        atomicAdd(&h_count[key], cnt);
        atomicAdd(&h_sum[key], (unsigned long long)sum);  // (two's complement: the sums are signed)
      }
    }
  }
  hsk_cloud_block_store<HskBox>(s, partial);
}

void launch_level_hist(hipStream_t s, const float* soa, unsigned n, unsigned pitch, const LevelWeights& w, unsigned* hist) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_level_hist, dim3(cloud_sweep_blocks(n)), dim3(256), 0, s, soa, n, pitch, w, hist);
}

void launch_level_sums(hipStream_t s, const float* soa, unsigned n, unsigned pitch, const LevelWeights& w, const LevelAxes& ax,
                       unsigned long long* partial, unsigned long long* sums15) {
  if (n == 0) return;
  const unsigned nb = cloud_sweep_blocks(n);
  hipLaunchKernelGGL(k_level_sums, dim3(nb), dim3(256), 0, s, soa, n, pitch, w, ax, partial);
  launch_cloud_fold(s, partial, nb, 15u, false, sums15);
}

void launch_level_extents(hipStream_t s, const float* soa, unsigned n, unsigned pitch, const LevelWeights& w, const LevelFrame& fr,
                          unsigned long long* partial, unsigned long long* box6, unsigned* h_count, unsigned long long* h_sum) {
  if (n == 0) return;
  const unsigned nb = cloud_sweep_blocks(n);
  hipLaunchKernelGGL(k_level_extents, dim3(nb), dim3(256), 0, s, soa, n, pitch, w, fr, partial, h_count, h_sum);
  launch_cloud_fold(s, partial, nb, 6u, true, box6);
}

int level_warm() {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, (const void*)k_level_hist);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_level_sums);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_level_extents);
  return (int)e;
}
