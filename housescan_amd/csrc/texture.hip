// texture.hip -- the bake of a colour atlas (include/hskinfu.h "Baked textures"; DESIGN.md 3.25 the kernel, 8s the rule) for
// gfx950.  The rule of a texel is hsk_texture_point.h's tex_texel, the text the host harness runs; this file is the shape around it.
//
// One wave per 8 x 8-texel tile of the atlas, four waves to a workgroup.  The layout aligns every block to 8 texels, so the 64
// texels of a wave share one tile word, one block record and the vertices of at most two faces: all of them are loaded through
// wave-uniform addresses (scalar loads), and a wave whose tile belongs to no block ends after one of them -- the outputs were
// cleared on the stream before the launch.  The 64 texels are neighbours on the surface, so the eight taps of their samples share
// cache lines; what a texel costs is the chain of dependent gathers of its projection (one per Newton step, four at most by
// default, most texels of a mesh that lies near the surface need one or two).
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_texture_point.h"

#ifndef TEX_WAVES
#define TEX_WAVES 4  // per workgroup (1 and 2 measure the same, 8 is 4 % slower: profiles/r29/texture_notes.md)
#endif

__global__ __launch_bounds__(64 * TEX_WAVES) void k_bake_texture(const unsigned* __restrict__ vol, const unsigned* __restrict__ colv, SampleVol v,
                                                                 TexArgs ta, const unsigned* __restrict__ tiles,
                                                                 const TexBlock* __restrict__ blocks, const int* __restrict__ faces,
                                                                 const float* __restrict__ vertices, unsigned n_tiles,
                                                                 unsigned char* __restrict__ rgb, unsigned char* __restrict__ nrm,
                                                                 unsigned char* __restrict__ mask, unsigned long long* __restrict__ counts) {
  const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * TEX_WAVES + (threadIdx.x >> 6)));
  if (tile >= n_tiles) return;
  if (tiles[tile] == TEX_EMPTY) return;
  const int lane = threadIdx.x & 63;
  const unsigned tw = (unsigned)ta.W >> 3;
  const int px = (int)((tile % tw) << 3) + (lane & 7), py = (int)((tile / tw) << 3) + (lane >> 3);
  TexelOut o;
  tex_texel(vol, colv, v, ta, tiles, blocks, faces, vertices, px, py, o);
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
  // the wave's texels by mask bit: one atomic add per wave and counter, into one of HSK_VIEW_COUNT_SLOTS slots by tile
  unsigned n[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) n[k] = (unsigned)__popcll(__ballot((o.mask >> k) & 1u));
  if (lane == 0) {
    unsigned long long* c = counts + (tile % HSK_VIEW_COUNT_SLOTS) * 16u;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (n[k]) atomicAdd(c + k, (unsigned long long)n[k]);
  }
}

void launch_bake_texture(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const TexArgs& ta, const unsigned* tiles,
                         const TexBlock* blocks, const int* faces, const float* vertices, unsigned char* rgb, unsigned char* nrm,
                         unsigned char* mask, unsigned long long* counts) {
  const unsigned n_tiles = (unsigned)(ta.W >> 3) * (unsigned)(ta.H >> 3);
  if (!n_tiles) return;
  hipLaunchKernelGGL(k_bake_texture, dim3((n_tiles + TEX_WAVES - 1) / TEX_WAVES), dim3(64 * TEX_WAVES), 0, s, (const unsigned*)vol, colv,
                     hsk_sample_vol(vp), ta, tiles, blocks, faces, vertices, n_tiles, rgb, nrm, mask, counts);
}

int texture_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_bake_texture);
}
