// keytex.hip -- the bake of a colour atlas from keyframes (include/hskinfu.h "Keyframe textures"; DESIGN.md 3.26 the kernel, 8t
// the rule) for gfx950.  The rule of a texel is hsk_keytex_point.h's key_texel, the text the host harness runs; this file is the
// shape around it.
//
// k_bake_texture's shape (texture.hip): one wave per 8 x 8-texel tile of the atlas, four waves to a workgroup, the tile word, the
// block record and the face vertices through wave-uniform addresses.  A texel's point and normal are found once; then the wave
// walks the keyframes in ascending index.  A keyframe's record lies at a wave-uniform address (64 bytes: scalar loads), and
// steps 1 to 3 of the rule -- camera coordinates, view angle, pixel -- are arithmetic on it.  The 64 texels are neighbours on the
// surface and pass or fail them together almost always, so a ballot of the three steps decides for the wave whether the
// keyframe's eight gathers per texel (four depth, four colour taps) are issued at all: a keyframe that looks elsewhere costs a
// wave its record and some forty VALU instructions.  Per texel the keyframes stay in ascending index in one thread, so the
// float sums of HSK_KEYTEX_BLEND are the twin's.
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_keytex_point.h"

#ifndef KEYTEX_WAVES
#define KEYTEX_WAVES 4  // per workgroup, as k_bake_texture
#endif

struct KeyAnyWave {
  __device__ bool operator()(bool x) const { return __ballot(x) != 0ull; }
};

__device__ __forceinline__ unsigned key_wave_sum(unsigned x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += (unsigned)__shfl_xor((int)x, off);
  return x;
}

__global__ __launch_bounds__(64 * KEYTEX_WAVES) void k_bake_keytex(const unsigned* __restrict__ vol, const unsigned* __restrict__ colv, SampleVol v,
                                                                   TexArgs ta, KeyStore ks, KeyArgs ka, const unsigned* __restrict__ tiles,
                                                                   const TexBlock* __restrict__ blocks, const int* __restrict__ faces,
                                                                   const float* __restrict__ vertices, unsigned n_tiles,
                                                                   unsigned char* __restrict__ rgb, unsigned char* __restrict__ nrm,
                                                                   unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                                   unsigned long long* __restrict__ counts) {
  const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KEYTEX_WAVES + (threadIdx.x >> 6)));
  if (tile >= n_tiles) return;
  if (tiles[tile] == TEX_EMPTY) return;  // (wave-uniform: the whole wave leaves, so every ballot below has all 64 lanes)
  const int lane = threadIdx.x & 63;
  const unsigned tw = (unsigned)ta.W >> 3;
  const int px = (int)((tile % tw) << 3) + (lane & 7), py = (int)((tile / tw) << 3) + (lane >> 3);
  KeyTexelOut o;
  key_texel(vol, colv, v, ta, tiles, blocks, faces, vertices, ks, ka, px, py, KeyAnyWave(), o);
  const size_t i = (size_t)py * (size_t)ta.W + (size_t)px;
  if (rgb) {
    unsigned char* p = rgb + 3 * i;
    p[0] = (unsigned char)o.rgb[0];
    p[1] = (unsigned char)o.rgb[1];
    p[2] = (unsigned char)o.rgb[2];
  }
  if (nrm) {
    unsigned char* p = nrm + 3 * i;
    p[0] = (unsigned char)o.nrm[0];
    p[1] = (unsigned char)o.nrm[1];
    p[2] = (unsigned char)o.nrm[2];
  }
  if (mask) mask[i] = (unsigned char)o.mask;
  if (source) source[i] = (unsigned char)o.source;
  // the wave's texels by mask bit (words 0 .. 5) and its pairs seen and occluded (6, 7): one atomic add per wave and counter, into
  // one of HSK_VIEW_COUNT_SLOTS slots by tile
  unsigned n[8];
#pragma unroll
  for (int k = 0; k < 6; ++k) n[k] = (unsigned)__popcll(__ballot((o.mask >> k) & 1u));
  n[6] = key_wave_sum(o.seen);
  n[7] = key_wave_sum(o.occluded);
  if (lane == 0) {
    unsigned long long* c = counts + (tile % HSK_VIEW_COUNT_SLOTS) * 16u;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (n[k]) atomicAdd(c + k, (unsigned long long)n[k]);
  }
}

void launch_bake_keytex(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const TexArgs& ta, const KeyStore& ks,
                        const KeyArgs& ka, const unsigned* tiles, const TexBlock* blocks, const int* faces, const float* vertices,
                        unsigned char* rgb, unsigned char* nrm, unsigned char* mask, unsigned char* source, unsigned long long* counts) {
  const unsigned n_tiles = (unsigned)(ta.W >> 3) * (unsigned)(ta.H >> 3);
  if (!n_tiles) return;
  hipLaunchKernelGGL(k_bake_keytex, dim3((n_tiles + KEYTEX_WAVES - 1) / KEYTEX_WAVES), dim3(64 * KEYTEX_WAVES), 0, s, (const unsigned*)vol, colv,
                     hsk_sample_vol(vp), ta, ks, ka, tiles, blocks, faces, vertices, n_tiles, rgb, nrm, mask, source, counts);
}

int keytex_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_bake_keytex);
}
