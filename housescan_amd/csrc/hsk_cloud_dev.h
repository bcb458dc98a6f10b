// hsk_cloud_dev.h -- a point of the cloud in the alignment's scratch (api_align.hip: align_scratch), for every kernel that strides
// over it (align.hip, reloc.hip, planes.hip, level.hip): the cloud lies as six planes `pitch` floats apart -- x, y, z, then the
// normal's nx, ny, nz -- of n <= 2^24 points each, so plane + point never wraps.
// A 256-point sweep keeps W <= 16 integer words a lane; its blocks leave theirs in partial[block][16], which k_cloud_fold
// (planes.hip: launch_cloud_fold) folds over the cloud_sweep_blocks(n) blocks.
#pragma once
#include "hsk_dev.h"

struct CloudPos {
  float x, y, z;
};
struct CloudPoint {
  float x, y, z, nx, ny, nz;
};

// point i's word in one of the planes
static __device__ __forceinline__ float hsk_cloud_word(const float* __restrict__ soa, unsigned plane, unsigned i, unsigned pitch) {
  return (soa + plane * (size_t)pitch)[i];
}
// point i: its position alone (three planes), or with its normal
static __device__ __forceinline__ CloudPos hsk_cloud_pos(const float* __restrict__ soa, unsigned i, unsigned pitch) {
  return {hsk_cloud_word(soa, 0u, i, pitch), hsk_cloud_word(soa, 1u, i, pitch), hsk_cloud_word(soa, 2u, i, pitch)};
}
static __device__ __forceinline__ CloudPoint hsk_cloud_point(const float* __restrict__ soa, unsigned i, unsigned pitch) {
  return {hsk_cloud_word(soa, 0u, i, pitch), hsk_cloud_word(soa, 1u, i, pitch), hsk_cloud_word(soa, 2u, i, pitch),
          hsk_cloud_word(soa, 3u, i, pitch), hsk_cloud_word(soa, 4u, i, pitch), hsk_cloud_word(soa, 5u, i, pitch)};
}
// the point a lane of a full-wave trip reads (n > 0): its own, or -- past the end -- the last one, which it then counts for nothing
static __device__ __forceinline__ unsigned hsk_cloud_at(bool act, unsigned i, unsigned n) { return act ? i : n - 1u; }

// the block's W words, a lane's each, folded by Op (hsk_dev.h) into partial[block][16]; every thread of the block arrives
template <class Op, int W>
static __device__ __forceinline__ void hsk_cloud_block_store(long long (&s)[W], unsigned long long* __restrict__ partial) {
  static_assert(W <= 16, "a block's row of partial holds 16 words");
#pragma unroll
  for (int v = 0; v < W; ++v) s[v] = hsk_wave_fold<Op>(s[v], v);
  const long long r = hsk_block_meet<Op>(s);
  if (threadIdx.x < (unsigned)W) partial[(size_t)blockIdx.x * 16u + threadIdx.x] = (unsigned long long)r;
}
