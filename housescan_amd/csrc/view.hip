// view.hip -- scene views for gfx950 (hsk_render_view): the TSDF marched from a virtual pinhole camera of
// any pose, size and intrinsics, the hits shaded on the device.  The march is k_raycast's own text (hsk_march.h); what differs
// is where the camera comes from (a ViewCam block, never a kernel argument: the TrackState itself in `follow` mode), whose
// tile grid it is, and the tail: 3 + 2 bytes per pixel instead of six floats, a pyramid and a ring report.  Writes nothing
// the tracker reads.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#undef HSK_RC_TIMING  // (the per-tile time stamps are k_raycast's instrumentation)
#include "hsk_march.h"
#define RC_STAMP(k) do { } while (0)

// `follow` hands the kernel the TrackState as its camera: the pose must sit where a ViewCam has it
static_assert(offsetof(TrackState, R) == offsetof(ViewCam, R) && offsetof(TrackState, t) == offsetof(ViewCam, t),
              "a TrackState must begin like a ViewCam");

// what the kernel needs only after the march, read through the kernarg segment pointer behind the loop (raycast.hip: RcTail)
struct ViewTail {
  unsigned char* rgb;        // 3 P bytes, or null
  unsigned short* depth;     // P, or null
  float* vmap;               // 3 P SoA, or null
  float* nmap;
  unsigned long long* counts;  // HSK_VIEW_COUNT_SLOTS x { hits, uncoloured hits, 14 words unused } (cleared on the stream before the launch)
  const unsigned* colv;      // the colour volume, (r, g, b, w) words, row-major (null without colour)
  float light[3];
  int light_in_camera;
  int mode;
  unsigned background;       // r | g << 8 | b << 16
};
struct ViewArgs {   // (the first 16 dwords arrive in SGPRs with the wave)
  const unsigned* flags;
  int flag_words;
  int W, H;
  const ViewCam* cam;
  const short2* vol;
  Intr in;
  VolParams vp;
  ViewTail tail;   // never touched by name inside the kernel
};
typedef const ViewCam* ViewCamPtr;
#define VW_ARG(type, member) (*(const type*)(vw_kernarg() + offsetof(ViewArgs, member)))
static __device__ __forceinline__ const char* vw_kernarg() {
  const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  return ka;
}

// the Lambert term of a hit: ambient 50, diffuse 205, one point light, no specular
static __device__ __forceinline__ int view_brightness(const ViewCam* __restrict__ st, const ViewTail& tl, float vx, float vy, float vz,
                                                      float nx, float ny, float nz) {
  float l0 = tl.light[0], l1 = tl.light[1], l2 = tl.light[2];
  if (tl.light_in_camera) {
    const float w0 = ((st->R[0] * l0 + st->R[1] * l1) + st->R[2] * l2) + st->t[0];
    const float w1 = ((st->R[3] * l0 + st->R[4] * l1) + st->R[5] * l2) + st->t[1];
    const float w2 = ((st->R[6] * l0 + st->R[7] * l1) + st->R[8] * l2) + st->t[2];
    l0 = w0;
    l1 = w1;
    l2 = w2;
  }
  const float L0 = l0 - vx, L1 = l1 - vy, L2 = l2 - vz;
  const float s = hsk_dot3(L0, L1, L2, L0, L1, L2);
  float w = 0.0f;
  if (s != 0.0f && !hsk_isnan(nx)) {
    w = hsk_dot3(L0, L1, L2, nx, ny, nz) * (1.0f / sqrtf(s));
    w = w > 0.0f ? w : 0.0f;   // (NaN: 0)
  }
  return min(255, 50 + (int)(205.0f * w));
}

// RC_TW: the wave's tile is RC_TW x (64 / RC_TW) pixels, as k_raycast's.  The mode is read with the tail: it only chooses
// among a few dozen instructions behind the march.
template <int RC_TW>
__global__ __launch_bounds__(RC_BLOCK, RC_WPE) void k_render_view(ViewArgs a) {
  constexpr bool SLAB = false;   // a view marches a whole volume (hsk_render_view refuses slabs)
  const short2* __restrict__ vol = a.vol;
  const ViewCam* __restrict__ st = a.cam;
  const VolParams& vp = a.vp;
  const int W = a.W, H = a.H;
  const Intr& in = a.in;
  const unsigned* __restrict__ flags = a.flags;
  const int flag_words = a.flag_words;
#include "hsk_march_stage.h"
  // (lanes outside the image stay in the wave as ended rays: hsk_march_rays.h)
  const bool in_img = x < W && y < H;
#include "hsk_march_rays.h"
#include "hsk_march_loop.h"
  (void)key;
  const ViewTail tl = VW_ARG(ViewTail, tail);
  const ViewCam* __restrict__ cam = VW_ARG(ViewCamPtr, cam);   // (fetched again: the pointer need not live through the march)
  const bool hit = in_img && !hsk_isnan(vx);
  const bool colour = tl.mode == HSK_VIEW_COLOR || tl.mode == HSK_VIEW_COLOR_LIT;
  unsigned c0 = tl.background & 255u, c1 = (tl.background >> 8) & 255u, c2 = (tl.background >> 16) & 255u;
  unsigned dmm = 0u;
  bool uncolored = false;
  if (hit) {
    // depth along the optical axis, in the sensor's unit
    const float zc = (cam->R[2] * (vx - t0) + cam->R[5] * (vy - t1)) + cam->R[8] * (vz - t2);
    const float d = rintf(zc * 1000.0f);
    if (d >= 1.0f && d <= 65535.0f) dmm = (unsigned)(int)d;
    int br = 0;
    if (tl.mode == HSK_VIEW_LAMBERT || tl.mode == HSK_VIEW_COLOR_LIT) br = view_brightness(cam, tl, vx, vy, vz, nx, ny, nz);
    if (tl.mode == HSK_VIEW_LAMBERT) {
      c0 = c1 = c2 = (unsigned)br;
    } else if (tl.mode == HSK_VIEW_NORMALS) {
      if (!hsk_isnan(nx)) {
        c0 = (unsigned)(int)rintf((nx * 0.5f + 0.5f) * 255.0f);
        c1 = (unsigned)(int)rintf((ny * 0.5f + 0.5f) * 255.0f);
        c2 = (unsigned)(int)rintf((nz * 0.5f + 0.5f) * 255.0f);
      }
    } else {
      // the voxel that contains the vertex: floor(v / cell), clamped into the grid
      const int gx = min(max(vox_of_q(hsk_div_by_const(vx, vp.icell[0])), 0), vp.X - 1);
      const int gy = min(max(vox_of_q(hsk_div_by_const(vy, vp.icell[1])), 0), vp.Y - 1);
      const int gz = min(max(vox_of_q(hsk_div_by_const(vz, vp.icell[2])), 0), vp.Z - 1);
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
  }
  if (in_img) {
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
  // one atomic add per wave and counter (every lane of the wave arrives here: none has returned)
  const unsigned n_hit = (unsigned)__popcll(__ballot(hit));
  const unsigned n_unc = (unsigned)__popcll(__ballot(hit && colour && uncolored));
  // (into one of HSK_VIEW_COUNT_SLOTS counter pairs, 128 B apart, by tile: the waves of a launch end together, and thousands of
  // atomic adds to ONE address queue up behind each other in its L2 channel; the host adds the slots up)
  if (lane == 0) {
    unsigned long long* c = tl.counts + ((unsigned)tile % HSK_VIEW_COUNT_SLOTS) * 16u;
    if (n_hit) atomicAdd(c, (unsigned long long)n_hit);
    if (n_unc) atomicAdd(c + 1, (unsigned long long)n_unc);
  }
}

void launch_render_view(hipStream_t s, const void* vol, const unsigned* colv, const ViewCam* cam, const VolParams& vp, int W, int H,
                        Intr in, const unsigned* flags, int mode, const float light[3], int light_in_camera,
                        const unsigned char background[3], unsigned char* rgb, unsigned short* depth, float* vmap, float* nmap,
                        unsigned long long* counts) {
  // 16 x 4 tiles for the volumes launch_raycast gives them to; ragged tiles are fine in either shape (no pyramid here)
  const int tw_px = vp.stream_nt ? 16 : 8;
  const int tiles = ((W + tw_px - 1) / tw_px) * ((H + 64 / tw_px - 1) / (64 / tw_px));
  ViewArgs a;
  a.flags = flags;
  a.flag_words = hsk_flag_words(vp);
  a.W = W;
  a.H = H;
  a.cam = cam;
  a.vol = (const short2*)vol;
  a.in = in;
  a.vp = vp;
  a.tail.rgb = rgb;
  a.tail.depth = depth;
  a.tail.vmap = vmap;
  a.tail.nmap = nmap;
  a.tail.counts = counts;
  a.tail.colv = colv;
  for (int c = 0; c < 3; ++c) a.tail.light[c] = light[c];
  a.tail.light_in_camera = light_in_camera;
  a.tail.mode = mode;
  a.tail.background = (unsigned)background[0] | ((unsigned)background[1] << 8) | ((unsigned)background[2] << 16);
  const size_t lds = (size_t)(a.flag_words + HSK_SUPER_WORDS) * 4;
  if (tw_px == 16)
    hipLaunchKernelGGL((k_render_view<16>), dim3(tiles), dim3(RC_BLOCK), lds, s, a);
  else
    hipLaunchKernelGGL((k_render_view<8>), dim3(tiles), dim3(RC_BLOCK), lds, s, a);
}
// loads this file's code object (hsk_prepare_readout); a hipError_t
int view_warm() {
  hipFuncAttributes fa;
  return (int)hipFuncGetAttributes(&fa, (const void*)k_render_view<8>);
}
