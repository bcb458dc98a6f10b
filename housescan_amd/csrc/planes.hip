// planes.hip -- oriented plane detection for gfx950 (hsk_detect_planes_oriented, hsk_detect_planes_volume, hsk_score_planes;
// DESIGN.md 3.14 the kernels, 8h the rule): with a normal at every point, one point is a plane hypothesis; a round scores
// hundreds of them against every point, refits the best on its inliers' integer moments and labels them.
//
// The rule (tests/planes_twin.py restates it in numpy) is per point in hsk_plane_point.h.  Everything summed here
// is an integer, so any order of addition gives the same bits and no result depends on the launch shape; the only atomics are
// integer adds in a block's own LDS.  Every sum is stored per block and added by k_cloud_fold / k_plane_count_sum.
//
// k_plane_seed: a lane per hypothesis -- its seed point's normal and d, or four NaNs (no inlier) when the point is invalid or
// labelled.
// k_plane_score: a block takes a tile of 1024 points into registers -- a lane four of them, with one "open" flag each (valid
// and unlabelled) -- and loops over the hypotheses, which are uniform: four floats by scalar loads.  Per hypothesis and wave,
// four ballots and population counts; the count goes to the lane whose number the hypothesis has (mod 64), and after every 64
// hypotheses the wave adds its 64 counts to the block's table in LDS.  So the cloud is read once per round, not once per
// hypothesis.  A wave whose tile has no open point skips the loop.  The block's table goes to partial[block][hypothesis].
// k_plane_moments: the count, the three sums of q and the six of q_a q_b over the inliers of one plane (64-bit integers).
// k_plane_label: labels the inliers of one plane, counts them and adds rint(|s| 65536).
// k_plane_unlabel: takes one plane's labels back (a refit that lost its support).
// k_plane_gather: a cloud with normals as two arrays of packed triples -> the alignment's six planes.
// k_cloud_fold: the blocks' partial[block][16] folded to 16 words, for every 256-point sweep over a cloud (level.hip's too).
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_cloud_dev.h"
#include "hsk_launch.h"
#include "hsk_plane_point.h"

#define PLANE_TILE 1024u  // points of a block's tile: four per lane

__global__ __launch_bounds__(256) void k_plane_seed(const float* __restrict__ soa, const int* __restrict__ labels,
                                                    const unsigned* __restrict__ seeds, unsigned n_hyp, unsigned pitch,
                                                    float* __restrict__ hyp) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n_hyp) return;
  const unsigned i = seeds[j];  // (< n: the host's next() % n)
  const CloudPoint q = hsk_cloud_point(soa, i, pitch);
  float abcd[4];
  plane_of_point(q.x, q.y, q.z, q.nx, q.ny, q.nz, abcd);
  const bool open = plane_point_valid(q.x, q.y, q.z, q.nx, q.ny, q.nz) & (labels[i] < 0);
  const float nan = __int_as_float(0x7fc00000);
#pragma unroll
  for (int c = 0; c < 4; ++c) hyp[4 * (size_t)j + c] = open ? abcd[c] : nan;
}

__global__ __launch_bounds__(256) void k_plane_score(const float* __restrict__ soa, const int* __restrict__ labels,
                                                     const float* __restrict__ hyp, unsigned n, unsigned pitch, unsigned n_hyp,
                                                     float dist_m, float cos_min, unsigned* __restrict__ partial) {
  __shared__ unsigned acc[HSK_PLANE_MAX_HYP];
  for (unsigned j = threadIdx.x; j < n_hyp; j += 256u) acc[j] = 0u;
  __syncthreads();
  const unsigned lane = threadIdx.x & 63u;
  for (unsigned base = blockIdx.x * PLANE_TILE; base < n; base += gridDim.x * PLANE_TILE) {  // (n <= 2^24, the grid <= 1024: no wrap)
    CloudPoint q[4];
    bool open[4];
    bool any = false;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned i = base + (unsigned)p * 256u + threadIdx.x;
      const bool act = i < n;
      const unsigned at = hsk_cloud_at(act, i, n);
      q[p] = hsk_cloud_point(soa, at, pitch);
      const bool free_ = labels ? labels[at] < 0 : true;
      open[p] = act & free_ & plane_point_valid(q[p].x, q[p].y, q[p].z, q[p].nx, q[p].ny, q[p].nz);
      any |= open[p];
    }
    if (__ballot(any) == 0ull) continue;  // (uniform over the wave; the barriers stand outside this loop)
    for (unsigned j0 = 0; j0 < n_hyp; j0 += 64u) {
      const unsigned jn = n_hyp - j0 < 64u ? n_hyp - j0 : 64u;
      unsigned mine = 0u;
      for (unsigned jj = 0; jj < jn; ++jj) {
        const float* __restrict__ h = hyp + 4 * (size_t)(j0 + jj);  // uniform over the block: scalar loads
        const float a = h[0], b = h[1], c = h[2], d = h[3];
        unsigned cnt = 0u;  // the wave's (uniform)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          float as;
          cnt += (unsigned)__popcll(__ballot(plane_point_inlier(open[p], a, b, c, d, dist_m, cos_min, q[p].x, q[p].y, q[p].z, q[p].nx, q[p].ny, q[p].nz, as)));
        }
        mine = lane == jj ? cnt : mine;
      }
      if (lane < jn && mine != 0u) atomicAdd(&acc[j0 + lane], mine);  // (integers in the block's LDS)
    }
  }
  __syncthreads();
  for (unsigned j = threadIdx.x; j < n_hyp; j += 256u) partial[(size_t)blockIdx.x * n_hyp + j] = acc[j];
}

// counts[j] = the sum over the blocks of partial[block][j]: a workgroup takes 64 hypotheses, each of its four waves every fourth
// block's row (coalesced, the loads of a wave independent of one another), and the waves meet in LDS
__global__ __launch_bounds__(256) void k_plane_count_sum(const unsigned* __restrict__ partial, unsigned n_blocks, unsigned n_hyp,
                                                         unsigned* __restrict__ counts) {
  __shared__ unsigned sh[4][64];
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6, j = blockIdx.x * 64u + lane;
  unsigned v = 0u;
  if (j < n_hyp) {
#pragma unroll 8
    for (unsigned b = w; b < n_blocks; b += 4u) v += partial[(size_t)b * n_hyp + j];
  }
  sh[w][lane] = v;
  __syncthreads();
  if (w == 0u && j < n_hyp) counts[j] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

struct PlaneEq {
  float a, b, c, d;
};

__global__ __launch_bounds__(256) void k_plane_moments(const float* __restrict__ soa, const int* __restrict__ labels, PlaneEq e, unsigned n,
                                                       unsigned pitch, float dist_m, float cos_min, unsigned long long* __restrict__ partial) {
  long long s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const CloudPoint q = hsk_cloud_point(soa, i, pitch);
    const bool open = plane_point_valid(q.x, q.y, q.z, q.nx, q.ny, q.nz) & (labels[i] < 0);
    float as;
    const bool inl = plane_point_inlier(open, e.a, e.b, e.c, e.d, dist_m, cos_min, q.x, q.y, q.z, q.nx, q.ny, q.nz, as);
    const long long qx = plane_q(inl ? q.x : 0.0f), qy = plane_q(inl ? q.y : 0.0f), qz = plane_q(inl ? q.z : 0.0f);
    s[0] += inl ? 1 : 0;
    s[1] += qx, s[2] += qy, s[3] += qz;
    s[4] += qx * qx, s[5] += qx * qy, s[6] += qx * qz;
    s[7] += qy * qy, s[8] += qy * qz, s[9] += qz * qz;
  }
  hsk_cloud_block_store<HskSum>(s, partial);
}

__global__ __launch_bounds__(256) void k_plane_label(const float* __restrict__ soa, int* __restrict__ labels, PlaneEq e, int index, unsigned n,
                                                     unsigned pitch, float dist_m, float cos_min, unsigned long long* __restrict__ partial) {
  long long s[2] = {0, 0};
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const CloudPoint q = hsk_cloud_point(soa, i, pitch);
    const bool open = plane_point_valid(q.x, q.y, q.z, q.nx, q.ny, q.nz) & (labels[i] < 0);
    float as;
    const bool inl = plane_point_inlier(open, e.a, e.b, e.c, e.d, dist_m, cos_min, q.x, q.y, q.z, q.nx, q.ny, q.nz, as);
    if (inl) labels[i] = index;
    s[0] += inl ? 1 : 0;
    s[1] += (long long)plane_abs_q(inl ? as : 0.0f);
  }
  hsk_cloud_block_store<HskSum>(s, partial);
}

// out[v] = the blocks' partial[block][v] folded: a workgroup per word v, a lane every 256th block.  box: the words are signed, v < 3
// the smallest and the others the largest; else their sum.
template <class Op>
static __device__ __forceinline__ void cloud_fold(const unsigned long long* __restrict__ partial, unsigned n_blocks, long long from,
                                                  unsigned long long* __restrict__ out) {
  long long v[1] = {from};
  for (unsigned b = threadIdx.x; b < n_blocks; b += 256u) v[0] = Op::of(0, v[0], (long long)partial[(size_t)b * 16u + blockIdx.x]);
  v[0] = hsk_wave_fold<Op>(v[0]);
  const long long r = hsk_block_meet<Op>(v);
  if (threadIdx.x == 0u) out[blockIdx.x] = (unsigned long long)r;
}
__global__ __launch_bounds__(256) void k_cloud_fold(const unsigned long long* __restrict__ partial, unsigned n_blocks, int box,
                                                    unsigned long long* __restrict__ out) {
  if (!box) cloud_fold<HskSum>(partial, n_blocks, 0ll, out);  // (uniform over the block)
  else if (blockIdx.x < 3u) cloud_fold<HskMin>(partial, n_blocks, 0x7fffffffll, out);
  else cloud_fold<HskMax>(partial, n_blocks, -0x80000000ll, out);
}

__global__ __launch_bounds__(256) void k_plane_unlabel(int* __restrict__ labels, int index, unsigned n) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n && labels[i] == index) labels[i] = -1;
}

__global__ __launch_bounds__(256) void k_plane_gather(const float* __restrict__ xyz, const float* __restrict__ normals, unsigned n,
                                                      unsigned pitch, float* __restrict__ soa) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    soa[(size_t)c * pitch + i] = xyz[3 * (size_t)i + c];
    soa[(size_t)(3 + c) * pitch + i] = normals[3 * (size_t)i + c];
  }
}

unsigned plane_score_blocks(unsigned n) {
  const unsigned b = (n + PLANE_TILE - 1u) / PLANE_TILE;
  return b < (unsigned)HSK_PLANE_MAX_BLOCKS ? (b ? b : 1u) : (unsigned)HSK_PLANE_MAX_BLOCKS;
}
unsigned cloud_sweep_blocks(unsigned n) {
  const unsigned b = (n + 255u) / 256u;
  return b < (unsigned)HSK_CLOUD_MAX_BLOCKS ? (b ? b : 1u) : (unsigned)HSK_CLOUD_MAX_BLOCKS;
}
void launch_cloud_fold(hipStream_t s, const unsigned long long* partial, unsigned n_blocks, unsigned n_words, bool box, unsigned long long* out) {
  hipLaunchKernelGGL(k_cloud_fold, dim3(n_words), dim3(256), 0, s, partial, n_blocks, box ? 1 : 0, out);
}

void launch_plane_seed(hipStream_t s, const float* soa, const int* labels, const unsigned* seeds, unsigned n_hyp, unsigned pitch, float* hyp) {
  if (n_hyp == 0) return;
  hipLaunchKernelGGL(k_plane_seed, dim3((n_hyp + 255u) / 256u), dim3(256), 0, s, soa, labels, seeds, n_hyp, pitch, hyp);
}

void launch_plane_score(hipStream_t s, const float* soa, const int* labels, const float* hyp, unsigned n, unsigned pitch, unsigned n_hyp,
                        float dist_m, float cos_min, unsigned* partial, unsigned* counts) {
  if (n == 0 || n_hyp == 0) return;
  const unsigned nb = plane_score_blocks(n);
  hipLaunchKernelGGL(k_plane_score, dim3(nb), dim3(256), 0, s, soa, labels, hyp, n, pitch, n_hyp, dist_m, cos_min, partial);
  hipLaunchKernelGGL(k_plane_count_sum, dim3((n_hyp + 63u) / 64u), dim3(256), 0, s, partial, nb, n_hyp, counts);
}

void launch_plane_moments(hipStream_t s, const float* soa, const int* labels, const float abcd[4], unsigned n, unsigned pitch, float dist_m,
                          float cos_min, unsigned long long* partial, unsigned long long* sums10) {
  if (n == 0) return;
  const unsigned nb = cloud_sweep_blocks(n);
  const PlaneEq e = {abcd[0], abcd[1], abcd[2], abcd[3]};
  hipLaunchKernelGGL(k_plane_moments, dim3(nb), dim3(256), 0, s, soa, labels, e, n, pitch, dist_m, cos_min, partial);
  launch_cloud_fold(s, partial, nb, 10u, false, sums10);
}

void launch_plane_label(hipStream_t s, const float* soa, int* labels, const float abcd[4], int index, unsigned n, unsigned pitch, float dist_m,
                        float cos_min, unsigned long long* partial, unsigned long long* out2) {
  if (n == 0) return;
  const unsigned nb = cloud_sweep_blocks(n);
  const PlaneEq e = {abcd[0], abcd[1], abcd[2], abcd[3]};
  hipLaunchKernelGGL(k_plane_label, dim3(nb), dim3(256), 0, s, soa, labels, e, index, n, pitch, dist_m, cos_min, partial);
  launch_cloud_fold(s, partial, nb, 2u, false, out2);
}

void launch_plane_unlabel(hipStream_t s, int* labels, int index, unsigned n) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_plane_unlabel, dim3((n + 255u) / 256u), dim3(256), 0, s, labels, index, n);
}

void launch_plane_gather(hipStream_t s, const float* xyz, const float* normals, unsigned n, unsigned pitch, float* soa) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_plane_gather, dim3((n + 255u) / 256u), dim3(256), 0, s, xyz, normals, n, pitch, soa);
}
