// view.hip -- scene views for gfx950 (hsk_render_view): the TSDF marched from a virtual pinhole camera of
// any pose, size and intrinsics, the hits shaded on the device.  The march is k_raycast's own text (hsk_march.h); what differs
// is where the camera comes from (a ViewCam block, never a kernel argument: the TrackState itself in `follow` mode), whose
// tile grid it is, and the tail: 3 + 2 bytes per pixel instead of six floats, a pyramid and a ring report.  Writes nothing
// the tracker reads.
#pragma clang fp contract(off)
#include "hsk_shade.h"
#undef HSK_RC_TIMING  // (the per-tile time stamps are k_raycast's instrumentation)
#include "hsk_march.h"
#define RC_STAMP(k) do { } while (0)

struct ViewArgs {
  MarchHead head;
  ShadeTail tail;   // never touched by name inside the kernel; counts: { hits, uncoloured hits } per slot
};
typedef const ViewCam* ViewCamPtr;

// RC_TW: the wave's tile is RC_TW x (64 / RC_TW) pixels, as k_raycast's.  The mode is read with the tail: it only chooses
// among a few dozen instructions behind the march.
template <int RC_TW>
__global__ __launch_bounds__(RC_BLOCK, RC_WPE) void k_render_view(ViewArgs a) {
  constexpr bool SLAB = false;   // a view marches a whole volume (hsk_render_view refuses slabs)
  const short2* __restrict__ vol = a.head.vol;
  const ViewCam* __restrict__ st = a.head.cam;
  const VolParams& vp = a.head.vp;
  const int W = a.head.W, H = a.head.H;
  const Intr& in = a.head.in;
  const unsigned* __restrict__ flags = a.head.flags;
  const int flag_words = a.head.flag_words;
#include "hsk_march_stage.h"
  // (lanes outside the image stay in the wave as ended rays: hsk_march_rays.h)
  const bool in_img = x < W && y < H;
#include "hsk_march_rays.h"
#include "hsk_march_loop.h"
  (void)key;
  const ShadeTail tl = HSK_KARG(ViewArgs, ShadeTail, tail);
  const ViewCam* __restrict__ cam = HSK_KARG(ViewArgs, ViewCamPtr, head.cam);   // (fetched again: the pointer need not live through the march)
  const bool hit = in_img && !hsk_isnan(vx);
  unsigned c0 = tl.background & 255u, c1 = (tl.background >> 8) & 255u, c2 = (tl.background >> 16) & 255u;
  unsigned dmm = 0u;
  bool uncolored = false;
  if (hit) {
    dmm = shade_depth_mm(cam, vx, vy, vz, t0, t1, t2);
    uncolored = shade_hit<false>(cam, tl, vp, vx, vy, vz, nx, ny, nz, c0, c1, c2);   // (no directional light here)
  }
  if (in_img) shade_write(tl, i, P, c0, c1, c2, dmm, vx, vy, vz, nx, ny, nz);
  // (every lane of the wave arrives here: none has returned)
  const bool counted[2] = {hit, hit && shade_mode_has_colour(tl.mode) && uncolored};
  shade_count(tl.counts, tile, lane, counted);
}

void launch_render_view(hipStream_t s, const void* vol, const unsigned* colv, const ViewCam* cam, const VolParams& vp, int W, int H,
                        Intr in, const unsigned* flags, int mode, const float light[3], int light_in_camera,
                        const unsigned char background[3], unsigned char* rgb, unsigned short* depth, float* vmap, float* nmap,
                        unsigned long long* counts) {
  // 16 x 4 tiles for the volumes launch_raycast gives them to; ragged tiles are fine in either shape (no pyramid here)
  const int tw_px = vp.stream_nt ? 16 : 8;
  const int tiles = ((W + tw_px - 1) / tw_px) * ((H + 64 / tw_px - 1) / (64 / tw_px));
  ViewArgs a;
  const size_t lds = shade_fill_head(a.head, vol, cam, vp, W, H, in, flags);
  shade_fill_tail(a.tail, colv, mode, light, light_in_camera, background, rgb, depth, vmap, nmap, counts);
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
