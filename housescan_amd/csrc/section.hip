// section.hip -- section views for gfx950 (hsk_render_section): floor plans, elevations and dollhouse views.
// The third user of the march text (hsk_march.h): k_render_view's kernel with a ray piece of its own -- the rays may be parallel
// (an orthographic camera: the origin is then a per-lane value) and start on clip planes inside the volume -- and a tail that
// knows a third class of pixel beside hit and background: CUT, where a clip plane runs through a negative TSDF.  Projection,
// planes, light kind and cut colour are run-time values of the argument block, read in the prelude and again in the tail.
// Writes nothing the tracker reads.
#pragma clang fp contract(off)
#include "hsk_shade.h"
#undef HSK_RC_TIMING  // (the per-tile time stamps are k_raycast's instrumentation)
#include "hsk_march.h"
#define RC_STAMP(k) do { } while (0)

struct SectionTail {
  ShadeTail sh;   // counts: { hits, uncoloured hits, cut pixels } per slot
  int light_directional;
  unsigned cut;   // cut_rgb, packed like the background
};
struct SectionArgs {
  MarchHead head;
  SectionClip clip;   // read by name in the prelude, through the kernarg pointer in the tail
  SectionTail tail;   // never touched by name inside the kernel
};
typedef const ViewCam* SectionCamPtr;

// RC_TW: the wave's tile is RC_TW x (64 / RC_TW) pixels, as k_render_view's.
template <int RC_TW>
__global__ __launch_bounds__(RC_BLOCK, RC_WPE) void k_render_section(SectionArgs a) {
  constexpr bool SLAB = false;   // a section marches a whole volume (hsk_render_section refuses slabs)
  const short2* __restrict__ vol = a.head.vol;
  const ViewCam* __restrict__ st = a.head.cam;
  const VolParams& vp = a.head.vp;
  const int W = a.head.W, H = a.head.H;
  const Intr& in = a.head.in;
  const unsigned* __restrict__ flags = a.head.flags;
  const int flag_words = a.head.flag_words;
#include "hsk_march_stage.h"
  // ---- the ray piece, in hsk_march_rays.h's place ----
  const bool in_px = x < W && y < H;   // (lanes outside the image stay in the wave as ended rays)
  const size_t P = (size_t)W * H;
  float vx = HSK_NANF, vy = HSK_NANF, vz = HSK_NANF, nx = HSK_NANF, ny = HSK_NANF, nz = HSK_NANF;
  int key = HSK_KEY_NONE_I;
  const bool ortho = a.clip.projection == HSK_PROJ_ORTHO;
  const float rx = ((float)x - in.cx) / in.fx, ry = ((float)y - in.cy) / in.fy;
  // step 1: pinhole o = t, d = (R0 rx + R1 ry) + R2 * 1.0f (R2 * 1.0f is R2); ortho o = (R0 rx + R1 ry) + t, d = R2
  const float a0_ = st->R[0] * rx + st->R[1] * ry, a1_ = st->R[3] * rx + st->R[4] * ry, a2_ = st->R[6] * rx + st->R[7] * ry;
  const float t0 = ortho ? a0_ + st->t[0] : st->t[0];
  const float t1 = ortho ? a1_ + st->t[1] : st->t[1];
  const float t2 = ortho ? a2_ + st->t[2] : st->t[2];
  float d0 = ortho ? st->R[2] : a0_ + st->R[2];
  float d1 = ortho ? st->R[5] : a1_ + st->R[5];
  float d2 = ortho ? st->R[8] : a2_ + st->R[8];
  const float inv = 1.0f / sqrtf(hsk_dot3(d0, d1, d2, d0, d1, d2));
  d0 = d0 * inv;
  d1 = d1 * inv;
  d2 = d2 * inv;
  if (d0 == 0.0f) d0 = 1e-15f;
  if (d1 == 0.0f) d1 = 1e-15f;
  if (d2 == 0.0f) d2 = 1e-15f;
  // step 2
  const float tmin0 = ((d0 > 0.0f ? 0.0f : vp.size[0]) - t0) / d0, tmax0 = ((d0 > 0.0f ? vp.size[0] : 0.0f) - t0) / d0;
  const float tmin1 = ((d1 > 0.0f ? 0.0f : vp.size[1]) - t1) / d1, tmax1 = ((d1 > 0.0f ? vp.size[1] : 0.0f) - t1) / d1;
  const float tmin2 = ((d2 > 0.0f ? 0.0f : vp.size[2]) - t2) / d2, tmax2 = ((d2 > 0.0f ? vp.size[2] : 0.0f) - t2) / d2;
  const float t_box = fmaxf(fmaxf(fmaxf(tmin0, tmin1), tmin2), 0.0f);
  float t_exit = fminf(fminf(tmax0, tmax1), tmax2);
  // step 3
  float t_start = t_box;
  bool alive = true;
#pragma unroll
  for (int c = 0; c < HSK_MAX_CLIP; ++c) {
    if (c < a.clip.n_clip) {   // (wave-uniform)
      const float pa = a.clip.plane[c].a, pb = a.clip.plane[c].b, pc = a.clip.plane[c].c, pd = a.clip.plane[c].d;
      const float s0 = ((pa * t0 + pb * t1) + pc * t2) + pd;
      const float sd = (pa * d0 + pb * d1) + pc * d2;
      const float tp = (-s0) / sd;
      t_start = sd > 0.0f ? fmaxf(t_start, tp) : t_start;
      t_exit = sd < 0.0f ? fminf(t_exit, tp) : t_exit;
      alive = alive && !(sd == 0.0f && s0 < 0.0f);
    }
  }
  // step 4: the ray marches iff ...
  const bool in_img = in_px && alive && t_start < t_exit;
  // step 6: one gather per ray, on its way while the bitfield is put into LDS.  The voxel is clamped into the grid, so the
  // address is a voxel's whatever the lane's numbers are.
  const float t_sec = t_start;
  bool cut = false;
  if (in_img && t_start > t_box) {
    int gx, gy, gz;
    hsk_voxel_at(vp, t0 + d0 * t_start, t1 + d1 * t_start, t2 + d2 * t_start, gx, gy, gz);
    cut = raw_at(vol, vp, gx, gy, gz) < 0;
  }
#include "hsk_march_loop.h"
  (void)key;
  // ---- the tail (8c steps 5-9) ----
  const SectionTail tl = HSK_KARG(SectionArgs, SectionTail, tail);
  const ViewCam* __restrict__ cam = HSK_KARG(SectionArgs, SectionCamPtr, head.cam);   // (fetched again: the pointer need not live through the march)
  bool hit = in_px && !cut && !hsk_isnan(vx);
  {
    const int n_clip = HSK_KARG(SectionArgs, int, clip.n_clip);
#pragma unroll
    for (int c = 0; c < HSK_MAX_CLIP; ++c) {
      if (c < n_clip) {
        const SectionPlane pl = *(const SectionPlane*)(hsk_kernarg() + offsetof(SectionArgs, clip.plane) + sizeof(SectionPlane) * c);
        hit = hit && (((pl.a * vx + pl.b * vy) + pl.c * vz) + pl.d >= 0.0f);
      }
    }
  }
  if (!hit) vx = vy = vz = nx = ny = nz = HSK_NANF;
  unsigned c0 = tl.sh.background & 255u, c1 = (tl.sh.background >> 8) & 255u, c2 = (tl.sh.background >> 16) & 255u;
  unsigned dmm = 0u;
  bool uncolored = false;
  if (hit || cut) {
    // depth from the camera's t: of the vertex, or of the ray's start on the plane
    const float px_ = cut ? t0 + d0 * t_sec : vx, py_ = cut ? t1 + d1 * t_sec : vy, pz_ = cut ? t2 + d2 * t_sec : vz;
    dmm = shade_depth_mm(cam, px_, py_, pz_, cam->t[0], cam->t[1], cam->t[2]);
  }
  if (cut) {
    c0 = tl.cut & 255u;
    c1 = (tl.cut >> 8) & 255u;
    c2 = (tl.cut >> 16) & 255u;
  }
  if (hit) uncolored = shade_hit<true>(cam, tl.sh, vp, vx, vy, vz, nx, ny, nz, c0, c1, c2, tl.light_directional);
  if (in_px) {
    // (the pixel's index is formed again here, from the thread's number as the stage text forms it: behind the empty asm it is not
    // the prelude's value, which then need not live through the march and the refinement -- two VGPRs where every one counts)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int tile_ = blockIdx.x * (blockDim.x >> 6) + (tid >> 6), lane_ = tid & 63;
    const int ty_lin_ = tile_ / tiles_x;
    const int ty_ = (ty_lin_ & 1) ? (tiles_y - 1 - (ty_lin_ >> 1)) : (ty_lin_ >> 1);
    const size_t i = (size_t)(ty_ * RC_TH + (lane_ / RC_TW)) * W + ((tile_ % tiles_x) * RC_TW + (lane_ % RC_TW));
    shade_write(tl.sh, i, P, c0, c1, c2, dmm, vx, vy, vz, nx, ny, nz);
  }
  // (every lane of the wave arrives here: none has returned)
  const bool counted[3] = {hit, hit && shade_mode_has_colour(tl.sh.mode) && uncolored, cut};
  shade_count(tl.sh.counts, tile, lane, counted);
}

void launch_render_section(hipStream_t s, const void* vol, const unsigned* colv, const ViewCam* cam, const VolParams& vp, int W, int H,
                           Intr in, const unsigned* flags, int mode, const float light[3], int light_in_camera, int light_directional,
                           const unsigned char background[3], const unsigned char cut_rgb[3], const SectionClip& clip,
                           unsigned char* rgb, unsigned short* depth, float* vmap, float* nmap, unsigned long long* counts) {
  // the tile shapes of launch_render_view
  const int tw_px = vp.stream_nt ? 16 : 8;
  const int tiles = ((W + tw_px - 1) / tw_px) * ((H + 64 / tw_px - 1) / (64 / tw_px));
  SectionArgs a;
  const size_t lds = shade_fill_head(a.head, vol, cam, vp, W, H, in, flags);
  shade_fill_tail(a.tail.sh, colv, mode, light, light_in_camera, background, rgb, depth, vmap, nmap, counts);
  a.clip = clip;
  a.tail.light_directional = light_directional;
  a.tail.cut = shade_pack_rgb(cut_rgb);
  if (tw_px == 16)
    hipLaunchKernelGGL((k_render_section<16>), dim3(tiles), dim3(RC_BLOCK), lds, s, a);
  else
    hipLaunchKernelGGL((k_render_section<8>), dim3(tiles), dim3(RC_BLOCK), lds, s, a);
}
// loads this file's code object (hsk_prepare_readout); a hipError_t
int section_warm() {
  hipFuncAttributes fa;
  return (int)hipFuncGetAttributes(&fa, (const void*)k_render_section<8>);
}
