// pack.hip -- the sparse volume image for gfx950 (hsk_pack_volume / hsk_unpack_volume; DESIGN.md 3.11 the kernels, 8e the
// format; tests/pack_twin.py restates the format in numpy).
//
// A brick is 8 x 8 x 8 voxels.  In the block layout of the TSDF volume (hsk_dev.h: hsk_vox_index) it is 16 segments of 128
// contiguous bytes: for each of its 2 plane groups and 8 rows the 8 16-B vectors of 2 x-adjacent lane-blocks.  Vector c of a
// row (c in [0, X)) holds plane (c & 3) of the group and the voxels x = 4 (c >> 2) .. + 3, so the 8 vectors of a segment are
// c = 8 bx .. 8 bx + 7.  A record keeps the voxels in (z, y, x) order: record vector i = ((z * 8 + y) * 2 + xh), xh the half
// of the row.  The colour volume is row-major: a colour brick is 64 rows of 32 B.
//
//   classify  one streaming sweep in k_fuse_bricks' shape: a thread owns a column of vectors through a brick layer (16
//             independent loads), eight consecutive lanes hold a brick; each lane reduces OR and XOR-against-the-first-word,
//             the eight lanes combine by ballot, one lane writes the class byte and the record's size in words
//   scan      exclusive scan of the sizes (three small launches), the class counts and the payload's length with it
//   gather    a wave per brick: a ZERO brick leaves at once; 128 16-B loads land as the 2 KiB record (SPLIT: 512 weight bytes)
//   scatter   the inverse, behind a memset of the volume: ZERO bricks and the padding planes stay zero
// Records are 4-byte aligned only (a UNIFORM record is one word): the 16-B accesses of a record are declared so.
#include "hsk_dev.h"
#include "hsk_launch.h"

#define HSK_PK_ZERO 0
#define HSK_PK_UNIFORM 1
#define HSK_PK_SPLIT 2
#define HSK_PK_RAW 3

// a record's vector: dword aligned (one 16-B access all the same: global memory asks for no more)
static __device__ __forceinline__ uint4 pk_load_a4(const unsigned* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}
static __device__ __forceinline__ void pk_store_a4(unsigned* p, const uint4& v) { __builtin_memcpy(p, &v, 16); }

// size of a class's record in 4-byte words
static __device__ __forceinline__ unsigned pk_words(unsigned cls) {
  return cls == HSK_PK_RAW ? 512u : cls == HSK_PK_SPLIT ? 129u : cls == HSK_PK_UNIFORM ? 1u : 0u;
}

// ---- classify (TSDF): t -> (vector column c, brick row by, brick layer bz), as k_fuse_bricks
__global__ __launch_bounds__(256) void k_pack_classify(const uint4* __restrict__ vol, unsigned n_threads, int X, int Y, int nzs, int nbx,
                                                       int nby, unsigned char* __restrict__ cls, unsigned* __restrict__ size) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  const unsigned c = t % (unsigned)X, r = t / (unsigned)X;
  const unsigned by = r % (unsigned)nby, bz = r / (unsigned)nby;
  const int lane = threadIdx.x & 63;
  uint4 v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = make_uint4(0u, 0u, 0u, 0u);
  if (t < n_threads) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const unsigned z = 8u * bz + 4u * (unsigned)g + (c & 3u);  // this lane's stored plane in group g
      if (z < (unsigned)nzs) {  // (planes beyond the stored ones count as word 0)
        const uint4* __restrict__ p = vol + ((size_t)(2u * bz + (unsigned)g) * (unsigned)Y + 8u * by) * (unsigned)X + c;
#pragma unroll
        for (int y = 0; y < 8; ++y) v[g * 8 + y] = p[(size_t)y * (unsigned)X];
      }
    }
  }
  const unsigned first = (unsigned)__shfl((int)v[0].x, lane & ~7, 64);  // voxel (0, 0, 0) of the brick
  unsigned any = 0u, diff = 0u;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    any |= v[i].x | v[i].y | v[i].z | v[i].w;
    diff |= (v[i].x ^ first) | (v[i].y ^ first) | (v[i].z ^ first) | (v[i].w ^ first);
  }
  const unsigned long long b_any = __ballot(any != 0u);
  const unsigned long long b_diff = __ballot(diff != 0u);
  const unsigned long long b_raw = __ballot((diff & 0xffffu) != 0u || (any >> 24) != 0u);  // a tsdf differs, or a weight is not a byte
  if ((lane & 7) != 0 || t >= n_threads) return;
  const unsigned m_any = (unsigned)(b_any >> lane) & 0xffu, m_diff = (unsigned)(b_diff >> lane) & 0xffu, m_raw = (unsigned)(b_raw >> lane) & 0xffu;
  const unsigned k = m_any == 0u ? HSK_PK_ZERO : m_diff == 0u ? HSK_PK_UNIFORM : m_raw == 0u ? HSK_PK_SPLIT : HSK_PK_RAW;
  const unsigned brick = (bz * (unsigned)nby + by) * (unsigned)nbx + (c >> 3);
  cls[brick] = (unsigned char)k;
  size[brick] = pk_words(k);
}

// ---- classify (colour, row-major words): a thread owns a column of 16-B vectors (4 voxels) through a brick layer, two
// consecutive lanes hold a brick
__global__ __launch_bounds__(256) void k_pack_classify_color(const uint4* __restrict__ col, unsigned n_threads, int X4, int Y, int nzs,
                                                             int nby, unsigned char* __restrict__ cls, unsigned* __restrict__ size) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  const unsigned c = t % (unsigned)X4, r = t / (unsigned)X4;
  const unsigned by = r % (unsigned)nby, bz = r / (unsigned)nby;
  unsigned any = 0u;
  if (t < n_threads) {
    for (unsigned z = 8u * bz; z < 8u * bz + 8u && z < (unsigned)nzs; ++z) {
      const uint4* __restrict__ p = col + ((size_t)z * (unsigned)Y + 8u * by) * (unsigned)X4 + c;
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        const uint4 v = p[(size_t)y * (unsigned)X4];
        any |= v.x | v.y | v.z | v.w;
      }
    }
  }
  any |= (unsigned)__shfl_xor((int)any, 1, 64);
  if ((threadIdx.x & 1u) != 0u || t >= n_threads) return;
  const unsigned brick = (bz * (unsigned)nby + by) * (unsigned)(X4 >> 1) + (c >> 1);
  cls[brick] = any ? HSK_PK_RAW : HSK_PK_ZERO;
  size[brick] = any ? 512u : 0u;
}

// the sizes from a class table that came from outside (unpack); the host has validated every byte
__global__ __launch_bounds__(256) void k_pack_sizes(const unsigned char* __restrict__ cls, unsigned n, unsigned* __restrict__ size) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) size[i] = pk_words(cls[i]);
}

// ---- exclusive scan of n sizes in place (size -> offset, both in words): block sums of 1024 entries, their scan, the rest.
// counts: [0..3] bricks per class (told apart by their size), [4] the total in words -- zeroed by the launcher
static __device__ __forceinline__ unsigned pk_wave_incl(unsigned v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = (unsigned)__shfl_up((int)v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
// exclusive prefix of v over the block's threads (nw waves); *total: the block's sum.  s_w: 17 words of LDS
static __device__ __forceinline__ unsigned pk_block_excl(unsigned v, unsigned* s_w, int nw, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned inc = pk_wave_incl(v, lane);
  __syncthreads();  // (s_w may still be read from the previous round)
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  unsigned base = 0u, sum = 0u;
  for (int i = 0; i < nw; ++i) {
    const unsigned x = s_w[i];
    if (i < w) base += x;
    sum += x;
  }
  *total = sum;
  return base + inc - v;
}

__global__ __launch_bounds__(256) void k_pack_scan_sums(const unsigned* __restrict__ size, unsigned n, unsigned* __restrict__ bsum,
                                                        unsigned* __restrict__ counts) {
  __shared__ unsigned s_w[17];
  const unsigned i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  unsigned s = 0u, n1 = 0u, n2 = 0u, n3 = 0u, n0 = 0u;
#pragma unroll
  for (unsigned j = 0; j < 4u; ++j) {
    if (i0 + j < n) {
      const unsigned v = size[i0 + j];
      s += v;
      n0 += v == 0u;
      n1 += v == 1u;
      n2 += v == 129u;
      n3 += v == 512u;
    }
  }
  unsigned tot;
  (void)pk_block_excl(s, s_w, 4, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
  // the class counts: packed into one word per pair (a block holds at most 1024 bricks), one block reduction each
  unsigned t01, t23;
  (void)pk_block_excl(n0 | (n1 << 16), s_w, 4, &t01);
  (void)pk_block_excl(n2 | (n3 << 16), s_w, 4, &t23);
  if (threadIdx.x == 0) {
    if (t01 & 0xffffu) atomicAdd(&counts[0], t01 & 0xffffu);
    if (t01 >> 16) atomicAdd(&counts[1], t01 >> 16);
    if (t23 & 0xffffu) atomicAdd(&counts[2], t23 & 0xffffu);
    if (t23 >> 16) atomicAdd(&counts[3], t23 >> 16);
  }
}
__global__ __launch_bounds__(1024) void k_pack_scan_blocks(unsigned* __restrict__ bsum, unsigned nblk, unsigned* __restrict__ counts) {
  __shared__ unsigned s_w[17];
  unsigned carry = 0u;
  for (unsigned base = 0; base < nblk; base += 1024u) {
    const unsigned i = base + threadIdx.x;
    const unsigned v = i < nblk ? bsum[i] : 0u;
    unsigned tot;
    const unsigned e = pk_block_excl(v, s_w, 16, &tot);
    if (i < nblk) bsum[i] = carry + e;
    carry += tot;
  }
  if (threadIdx.x == 0) counts[4] = carry;
}
__global__ __launch_bounds__(256) void k_pack_scan_final(unsigned* __restrict__ size, unsigned n, const unsigned* __restrict__ bsum) {
  __shared__ unsigned s_w[17];
  const unsigned i0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  unsigned v[4], s = 0u;
#pragma unroll
  for (unsigned j = 0; j < 4u; ++j) {
    v[j] = i0 + j < n ? size[i0 + j] : 0u;
    s += v[j];
  }
  unsigned tot;
  unsigned e = pk_block_excl(s, s_w, 4, &tot) + bsum[blockIdx.x];
#pragma unroll
  for (unsigned j = 0; j < 4u; ++j) {
    if (i0 + j < n) size[i0 + j] = e;
    e += v[j];
  }
}

// ---- a record's vector i (0..127) <-> the volume: xh = i & 1, y = (i >> 1) & 7, z = i >> 4
struct PackGeom {
  int X, Y, nzs, nbx, nby;
};
static __device__ __forceinline__ void pk_brick_of(const PackGeom& g, unsigned brick, unsigned& bx, unsigned& by, unsigned& bz) {
  bx = brick % (unsigned)g.nbx;
  const unsigned r = brick / (unsigned)g.nbx;
  by = r % (unsigned)g.nby;
  bz = r / (unsigned)g.nby;
}
// index of the TSDF volume's vector for record vector i; false: beyond the stored planes
static __device__ __forceinline__ bool pk_tsdf_vec(const PackGeom& g, unsigned bx, unsigned by, unsigned bz, unsigned i, size_t& idx) {
  const unsigned xh = i & 1u, y = (i >> 1) & 7u, z = 8u * bz + (i >> 4);
  idx = ((size_t)(z >> 2) * (unsigned)g.Y + 8u * by + y) * (unsigned)g.X + 8u * bx + 4u * xh + (z & 3u);
  return z < (unsigned)g.nzs;
}
static __device__ __forceinline__ bool pk_color_vec(const PackGeom& g, unsigned bx, unsigned by, unsigned bz, unsigned i, size_t& idx) {
  const unsigned xh = i & 1u, y = (i >> 1) & 7u, z = 8u * bz + (i >> 4);
  idx = ((size_t)z * (unsigned)g.Y + 8u * by + y) * (unsigned)(g.X >> 2) + 2u * bx + xh;
  return z < (unsigned)g.nzs;
}

// a wave per brick; COLOR: the row-major colour volume (classes ZERO and RAW only)
template <bool COLOR>
__global__ __launch_bounds__(256) void k_pack_gather(const uint4* __restrict__ vol, PackGeom g, unsigned n_bricks,
                                                     const unsigned char* __restrict__ cls, const unsigned* __restrict__ off,
                                                     unsigned* __restrict__ out) {
  const unsigned brick = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (brick >= n_bricks) return;
  const unsigned k = (unsigned)__builtin_amdgcn_readfirstlane((int)cls[brick]);
  if (k == HSK_PK_ZERO) return;
  unsigned* __restrict__ rec = out + (size_t)__builtin_amdgcn_readfirstlane((int)off[brick]);
  const unsigned lane = threadIdx.x & 63u;
  unsigned bx, by, bz;
  pk_brick_of(g, brick, bx, by, bz);
  uint4 v[2];
#pragma unroll
  for (unsigned h = 0; h < 2u; ++h) {
    size_t idx;
    const bool in = COLOR ? pk_color_vec(g, bx, by, bz, lane + 64u * h, idx) : pk_tsdf_vec(g, bx, by, bz, lane + 64u * h, idx);
    v[h] = in ? vol[idx] : make_uint4(0u, 0u, 0u, 0u);
  }
  if (COLOR || k == HSK_PK_RAW) {
#pragma unroll
    for (unsigned h = 0; h < 2u; ++h) pk_store_a4(rec + 4u * (lane + 64u * h), v[h]);
  } else if (k == HSK_PK_SPLIT) {
    if (lane == 0u) rec[0] = v[0].x & 0xffffu;  // int16 tsdf, uint16 0
#pragma unroll
    for (unsigned h = 0; h < 2u; ++h)
      rec[1u + lane + 64u * h] = ((v[h].x >> 16) & 0xffu) | (((v[h].y >> 16) & 0xffu) << 8) | (((v[h].z >> 16) & 0xffu) << 16) | ((v[h].w >> 16) << 24);
  } else {
    if (lane == 0u) rec[0] = v[0].x;
  }
}

template <bool COLOR>
__global__ __launch_bounds__(256) void k_pack_scatter(uint4* __restrict__ vol, PackGeom g, unsigned n_bricks,
                                                      const unsigned char* __restrict__ cls, const unsigned* __restrict__ off,
                                                      const unsigned* __restrict__ in) {
  const unsigned brick = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (brick >= n_bricks) return;
  const unsigned k = (unsigned)__builtin_amdgcn_readfirstlane((int)cls[brick]);
  if (k == HSK_PK_ZERO) return;  // (the volume was zeroed in front)
  const unsigned* __restrict__ rec = in + (size_t)__builtin_amdgcn_readfirstlane((int)off[brick]);
  const unsigned lane = threadIdx.x & 63u;
  unsigned bx, by, bz;
  pk_brick_of(g, brick, bx, by, bz);
  const unsigned head = (COLOR || k == HSK_PK_RAW) ? 0u : rec[0];
#pragma unroll
  for (unsigned h = 0; h < 2u; ++h) {
    const unsigned i = lane + 64u * h;
    uint4 v;
    if (COLOR || k == HSK_PK_RAW) {
      v = pk_load_a4(rec + 4u * i);
    } else if (k == HSK_PK_SPLIT) {
      const unsigned w = rec[1u + i], t = head & 0xffffu;
      v = make_uint4(t | ((w & 0xffu) << 16), t | (((w >> 8) & 0xffu) << 16), t | (((w >> 16) & 0xffu) << 16), t | ((w >> 24) << 16));
    } else {
      v = make_uint4(head, head, head, head);
    }
    size_t idx;
    const bool in_vol = COLOR ? pk_color_vec(g, bx, by, bz, i, idx) : pk_tsdf_vec(g, bx, by, bz, i, idx);
    if (in_vol) vol[idx] = v;  // (planes beyond the stored ones are dropped: the padding stays zero)
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
static PackGeom pack_geom(const VolParams& vp) {
  PackGeom g;
  g.X = vp.X;
  g.Y = vp.Y;
  g.nzs = vp.nzs;
  g.nbx = vp.X >> 3;
  g.nby = vp.Y >> 3;
  return g;
}
size_t pack_bricks(const VolParams& vp) { return (size_t)(vp.X >> 3) * (size_t)(vp.Y >> 3) * (size_t)((vp.nzs + 7) >> 3); }
size_t pack_scan_blocks(size_t n_bricks) { return (n_bricks + 1023) / 1024; }

void launch_pack_classify(hipStream_t s, const void* vol, const VolParams& vp, unsigned char* cls, unsigned* size) {
  const unsigned n_threads = (unsigned)vp.X * (unsigned)(vp.Y >> 3) * (unsigned)((vp.nzs + 7) >> 3);
  hipLaunchKernelGGL(k_pack_classify, dim3((n_threads + 255u) / 256u), dim3(256), 0, s, (const uint4*)vol, n_threads, vp.X, vp.Y, vp.nzs,
                     vp.X >> 3, vp.Y >> 3, cls, size);
}
void launch_pack_classify_color(hipStream_t s, const unsigned* col, const VolParams& vp, unsigned char* cls, unsigned* size) {
  const unsigned n_threads = (unsigned)(vp.X >> 2) * (unsigned)(vp.Y >> 3) * (unsigned)((vp.nzs + 7) >> 3);
  hipLaunchKernelGGL(k_pack_classify_color, dim3((n_threads + 255u) / 256u), dim3(256), 0, s, (const uint4*)col, n_threads, vp.X >> 2, vp.Y,
                     vp.nzs, vp.Y >> 3, cls, size);
}
void launch_pack_sizes(hipStream_t s, const unsigned char* cls, size_t n_bricks, unsigned* size) {
  hipLaunchKernelGGL(k_pack_sizes, dim3((unsigned)((n_bricks + 255) / 256)), dim3(256), 0, s, cls, (unsigned)n_bricks, size);
}
void launch_pack_scan(hipStream_t s, unsigned* size, size_t n_bricks, unsigned* bsum, unsigned* counts) {
  const unsigned nblk = (unsigned)pack_scan_blocks(n_bricks);
  (void)hipMemsetAsync(counts, 0, 8 * sizeof(unsigned), s);
  hipLaunchKernelGGL(k_pack_scan_sums, dim3(nblk), dim3(256), 0, s, size, (unsigned)n_bricks, bsum, counts);
  hipLaunchKernelGGL(k_pack_scan_blocks, dim3(1), dim3(1024), 0, s, bsum, nblk, counts);
  hipLaunchKernelGGL(k_pack_scan_final, dim3(nblk), dim3(256), 0, s, size, (unsigned)n_bricks, bsum);
}
void launch_pack_gather(hipStream_t s, const void* vol, bool color, const VolParams& vp, const unsigned char* cls, const unsigned* off,
                        void* payload) {
  const unsigned n = (unsigned)pack_bricks(vp);
  if (color)
    hipLaunchKernelGGL((k_pack_gather<true>), dim3((n + 3u) / 4u), dim3(256), 0, s, (const uint4*)vol, pack_geom(vp), n, cls, off, (unsigned*)payload);
  else
    hipLaunchKernelGGL((k_pack_gather<false>), dim3((n + 3u) / 4u), dim3(256), 0, s, (const uint4*)vol, pack_geom(vp), n, cls, off, (unsigned*)payload);
}
void launch_pack_scatter(hipStream_t s, void* vol, bool color, const VolParams& vp, const unsigned char* cls, const unsigned* off,
                         const void* payload) {
  const unsigned n = (unsigned)pack_bricks(vp);
  if (color)
    hipLaunchKernelGGL((k_pack_scatter<true>), dim3((n + 3u) / 4u), dim3(256), 0, s, (uint4*)vol, pack_geom(vp), n, cls, off, (const unsigned*)payload);
  else
    hipLaunchKernelGGL((k_pack_scatter<false>), dim3((n + 3u) / 4u), dim3(256), 0, s, (uint4*)vol, pack_geom(vp), n, cls, off, (const unsigned*)payload);
}
