// hsk_shade.h -- the tail of an image kernel (view.hip: k_render_view; section.hip: k_render_section), once: what becomes of a
// ray's hit behind the march -- depth in millimetres, the colour by shading mode, the four optional
// outputs, the counters -- and the part of the argument block that both kernels read for it.
#pragma once
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"

// `follow` hands a kernel the TrackState as its camera: the pose must sit where a ViewCam has it
static_assert(offsetof(TrackState, R) == offsetof(ViewCam, R) && offsetof(TrackState, t) == offsetof(ViewCam, t),
              "a TrackState must begin like a ViewCam");

// what a kernel needs only after the march, read through the kernarg segment pointer behind the loop (raycast.hip: RcTail)
struct ShadeTail {
  unsigned char* rgb;        // 3 P bytes, or null
  unsigned short* depth;     // P, or null
  float* vmap;               // 3 P SoA, or null
  float* nmap;
  unsigned long long* counts;  // HSK_VIEW_COUNT_SLOTS x 16 words: a kernel's counters first, the rest unused (cleared on the stream before the launch)
  const unsigned* colv;      // the colour volume, (r, g, b, w) words, row-major (null without colour)
  float light[3];
  int light_in_camera;
  int mode;
  unsigned background;       // r | g << 8 | b << 16
};
static inline unsigned shade_pack_rgb(const unsigned char c[3]) { return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16); }
static inline void shade_fill_tail(ShadeTail& t, const unsigned* colv, int mode, const float light[3], int light_in_camera,
                                   const unsigned char background[3], unsigned char* rgb, unsigned short* depth, float* vmap, float* nmap,
                                   unsigned long long* counts) {
  t.rgb = rgb;
  t.depth = depth;
  t.vmap = vmap;
  t.nmap = nmap;
  t.counts = counts;
  t.colv = colv;
  for (int c = 0; c < 3; ++c) t.light[c] = light[c];
  t.light_in_camera = light_in_camera;
  t.mode = mode;
  t.background = shade_pack_rgb(background);
}

// what the march itself reads: an image kernel's argument block begins with it (the first 16 dwords arrive in SGPRs with the wave)
struct MarchHead {
  const unsigned* flags;
  int flag_words;
  int W, H;
  const ViewCam* cam;   // `follow` hands a kernel the TrackState here
  const short2* vol;
  Intr in;
  VolParams vp;
};
// ... filled; returns the LDS bytes of the launch
static inline size_t shade_fill_head(MarchHead& h, const void* vol, const ViewCam* cam, const VolParams& vp, int W, int H, Intr in,
                                     const unsigned* flags) {
  h.flags = flags;
  h.flag_words = hsk_flag_words(vp);
  h.W = W;
  h.H = H;
  h.cam = cam;
  h.vol = (const short2*)vol;
  h.in = in;
  h.vp = vp;
  return (size_t)(h.flag_words + HSK_SUPER_WORDS) * 4;
}

// a member of a kernel's argument block, read through the kernarg segment pointer (never by name: the block need not live
// in registers through the march)
#define HSK_KARG(Args, type, member) (*(const type*)(hsk_kernarg() + offsetof(Args, member)))
static __device__ __forceinline__ const char* hsk_kernarg() {
  const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  return ka;
}

// depth along the optical axis from the origin o, in the sensor's unit (0: none, or outside 1 .. 65535)
static __device__ __forceinline__ unsigned shade_depth_mm(const ViewCam* __restrict__ cam, float px, float py, float pz, float ox, float oy,
                                                          float oz) {
  const float zc = (cam->R[2] * (px - ox) + cam->R[5] * (py - oy)) + cam->R[8] * (pz - oz);
  const float d = rintf(zc * 1000.0f);
  return (d >= 1.0f && d <= 65535.0f) ? (unsigned)(int)d : 0u;
}

// the Lambert term of a hit: ambient 50, diffuse 205, no specular; a point light, or -- where a
// kernel knows them (DIRECTIONAL; a kernel that does not carries no test) -- a direction towards the light that is the same
// for every vertex
template <bool DIRECTIONAL>
static __device__ __forceinline__ int shade_brightness(const ViewCam* __restrict__ st, const ShadeTail& tl, float vx, float vy, float vz,
                                                       float nx, float ny, float nz, int light_directional) {
  float l0 = tl.light[0], l1 = tl.light[1], l2 = tl.light[2];
  float L0, L1, L2;
  if (DIRECTIONAL && light_directional) {
    L0 = l0;
    L1 = l1;
    L2 = l2;
    if (tl.light_in_camera) {
      L0 = (st->R[0] * l0 + st->R[1] * l1) + st->R[2] * l2;
      L1 = (st->R[3] * l0 + st->R[4] * l1) + st->R[5] * l2;
      L2 = (st->R[6] * l0 + st->R[7] * l1) + st->R[8] * l2;
    }
  } else {
    if (tl.light_in_camera) {
      const float w0 = ((st->R[0] * l0 + st->R[1] * l1) + st->R[2] * l2) + st->t[0];
      const float w1 = ((st->R[3] * l0 + st->R[4] * l1) + st->R[5] * l2) + st->t[1];
      const float w2 = ((st->R[6] * l0 + st->R[7] * l1) + st->R[8] * l2) + st->t[2];
      l0 = w0;
      l1 = w1;
      l2 = w2;
    }
    L0 = l0 - vx;
    L1 = l1 - vy;
    L2 = l2 - vz;
  }
  const float s = hsk_dot3(L0, L1, L2, L0, L1, L2);
  float w = 0.0f;
  if (s != 0.0f && !hsk_isnan(nx)) {
    w = hsk_dot3(L0, L1, L2, nx, ny, nz) * (1.0f / sqrtf(s));
    w = w > 0.0f ? w : 0.0f;   // (NaN: 0)
  }
  return min(255, 50 + (int)(205.0f * w));
}

static __device__ __forceinline__ bool shade_mode_has_colour(int mode) { return mode == HSK_VIEW_COLOR || mode == HSK_VIEW_COLOR_LIT; }

// The colour (c0, c1, c2) of a hit at vertex v with normal n by tl.mode: Lambert, normals (left as they are where the normal is
// NaN), colour or lit colour.  Returns `uncolored`: a colour mode found no colour in the voxel that contains the vertex.
template <bool DIRECTIONAL>
static __device__ __forceinline__ bool shade_hit(const ViewCam* __restrict__ cam, const ShadeTail& tl, const VolParams& vp, float vx, float vy,
                                                 float vz, float nx, float ny, float nz, unsigned& c0, unsigned& c1, unsigned& c2,
                                                 int light_directional = 0) {
  bool uncolored = false;
  int br = 0;
  if (tl.mode == HSK_VIEW_LAMBERT || tl.mode == HSK_VIEW_COLOR_LIT)
    br = shade_brightness<DIRECTIONAL>(cam, tl, vx, vy, vz, nx, ny, nz, light_directional);
  if (tl.mode == HSK_VIEW_LAMBERT) {
    c0 = c1 = c2 = (unsigned)br;
  } else if (tl.mode == HSK_VIEW_NORMALS) {
    if (!hsk_isnan(nx)) {
      c0 = hsk_normal_level(nx);
      c1 = hsk_normal_level(ny);
      c2 = hsk_normal_level(nz);
    }
  } else {
    int gx, gy, gz;
    hsk_voxel_at(vp, vx, vy, vz, gx, gy, gz);
    const unsigned cw = tl.colv[((size_t)gz * vp.Y + gy) * vp.X + gx];
    uncolored = (cw >> 24) == 0u;
    c0 = uncolored ? 0u : (cw & 255u);
    c1 = uncolored ? 0u : ((cw >> 8) & 255u);
    c2 = uncolored ? 0u : ((cw >> 16) & 255u);
    if (tl.mode == HSK_VIEW_COLOR_LIT) {
      c0 = (c0 * (unsigned)br + 127u) / 255u;
      c1 = (c1 * (unsigned)br + 127u) / 255u;
      c2 = (c2 * (unsigned)br + 127u) / 255u;
    }
  }
  return uncolored;
}

// the outputs of pixel i (of P): each may be null
static __device__ __forceinline__ void shade_write(const ShadeTail& tl, size_t i, size_t P, unsigned c0, unsigned c1, unsigned c2, unsigned dmm,
                                                   float vx, float vy, float vz, float nx, float ny, float nz) {
  if (tl.rgb) {
    unsigned char* p = tl.rgb + 3 * i;
    p[0] = (unsigned char)c0;
    p[1] = (unsigned char)c1;
    p[2] = (unsigned char)c2;
  }
  if (tl.depth) tl.depth[i] = (unsigned short)dmm;
  if (tl.vmap) {
    tl.vmap[i] = vx;
    tl.vmap[P + i] = vy;
    tl.vmap[2 * P + i] = vz;
  }
  if (tl.nmap) {
    tl.nmap[i] = nx;
    tl.nmap[P + i] = ny;
    tl.nmap[2 * P + i] = nz;
  }
}

// The wave's pixels of N classes, counted: one atomic add per wave and counter (every lane of the wave must arrive here), into
// one of HSK_VIEW_COUNT_SLOTS slots, 128 B apart, by tile: the waves of a launch end together, and thousands of atomic adds to
// ONE address queue up behind each other in its L2 channel; the host adds the slots up.
template <int N>
static __device__ __forceinline__ void shade_count(unsigned long long* counts, int tile, int lane, const bool (&is)[N]) {
  unsigned n[N];
#pragma unroll
  for (int k = 0; k < N; ++k) n[k] = (unsigned)__popcll(__ballot(is[k]));
  if (lane == 0) {
    unsigned long long* c = counts + ((unsigned)tile % HSK_VIEW_COUNT_SLOTS) * 16u;
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (n[k]) atomicAdd(c + k, (unsigned long long)n[k]);
  }
}
