// section.hip -- section views for gfx950 (hsk_render_section): floor plans, elevations and dollhouse views.
// The third user of the march text (hsk_march.h): k_render_view's kernel with a ray piece of its own -- the rays may be parallel
// (an orthographic camera: the origin is then a per-lane value) and start on clip planes inside the volume -- and a tail that
// knows a third class of pixel beside hit and background: CUT, where a clip plane runs through a negative TSDF.  Projection,
// planes, light kind and cut colour are run-time values of the argument block, read in the prelude and again in the tail.
// Writes nothing the tracker reads.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#undef HSK_RC_TIMING  // (the per-tile time stamps are k_raycast's instrumentation)
#include "hsk_march.h"
#define RC_STAMP(k) do { } while (0)

static_assert(offsetof(TrackState, R) == offsetof(ViewCam, R) && offsetof(TrackState, t) == offsetof(ViewCam, t),
              "a TrackState must begin like a ViewCam");

// what the kernel needs only after the march, read through the kernarg segment pointer behind the loop (view.hip: ViewTail)
struct SectionTail {
  unsigned char* rgb;        // 3 P bytes, or null
  unsigned short* depth;     // P, or null
  float* vmap;               // 3 P SoA, or null
  float* nmap;
  unsigned long long* counts;  // HSK_VIEW_COUNT_SLOTS x { hits, uncoloured hits, cut pixels, 13 words unused } (cleared before the launch)
  const unsigned* colv;      // the colour volume, (r, g, b, w) words, row-major (null without colour)
  float light[3];
  int light_in_camera;
  int light_directional;
  int mode;
  unsigned background;       // r | g << 8 | b << 16
  unsigned cut;              // the same of cut_rgb
};
struct SectionArgs {   // (the first 16 dwords arrive in SGPRs with the wave)
  const unsigned* flags;
  int flag_words;
  int W, H;
  const ViewCam* cam;
  const short2* vol;
  Intr in;
  VolParams vp;
  SectionClip clip;   // read by name in the prelude, through the kernarg pointer in the tail
  SectionTail tail;   // never touched by name inside the kernel
};
typedef const ViewCam* SectionCamPtr;
#define SC_ARG(type, member) (*(const type*)(sc_kernarg() + offsetof(SectionArgs, member)))
static __device__ __forceinline__ const char* sc_kernarg() {
  const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  return ka;
}

// the Lambert term of a hit: ambient 50, diffuse 205, no specular; a point light, or a
// direction towards the light that is the same for every vertex
static __device__ __forceinline__ int section_brightness(const ViewCam* __restrict__ st, const SectionTail& tl, float vx, float vy, float vz,
                                                         float nx, float ny, float nz) {
  float l0 = tl.light[0], l1 = tl.light[1], l2 = tl.light[2];
  float L0, L1, L2;
  if (tl.light_directional) {
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

// RC_TW: the wave's tile is RC_TW x (64 / RC_TW) pixels, as k_render_view's.
template <int RC_TW>
__global__ __launch_bounds__(RC_BLOCK, RC_WPE) void k_render_section(SectionArgs a) {
  constexpr bool SLAB = false;   // a section marches a whole volume (hsk_render_section refuses slabs)
  const short2* __restrict__ vol = a.vol;
  const ViewCam* __restrict__ st = a.cam;
  const VolParams& vp = a.vp;
  const int W = a.W, H = a.H;
  const Intr& in = a.in;
  const unsigned* __restrict__ flags = a.flags;
  const int flag_words = a.flag_words;
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
    const int gx = min(max(vox_of_q(hsk_div_by_const(t0 + d0 * t_start, vp.icell[0])), 0), vp.X - 1);
    const int gy = min(max(vox_of_q(hsk_div_by_const(t1 + d1 * t_start, vp.icell[1])), 0), vp.Y - 1);
    const int gz = min(max(vox_of_q(hsk_div_by_const(t2 + d2 * t_start, vp.icell[2])), 0), vp.Z - 1);
    cut = raw_at(vol, vp, gx, gy, gz) < 0;
  }
#include "hsk_march_loop.h"
  (void)key;
  // ---- the tail (8c steps 5-9) ----
  const SectionTail tl = SC_ARG(SectionTail, tail);
  const ViewCam* __restrict__ cam = SC_ARG(SectionCamPtr, cam);   // (fetched again: the pointer need not live through the march)
  bool hit = in_px && !cut && !hsk_isnan(vx);
  {
    const int n_clip = SC_ARG(int, clip.n_clip);
#pragma unroll
    for (int c = 0; c < HSK_MAX_CLIP; ++c) {
      if (c < n_clip) {
        const SectionPlane pl = *(const SectionPlane*)(sc_kernarg() + offsetof(SectionArgs, clip.plane) + sizeof(SectionPlane) * c);
        hit = hit && (((pl.a * vx + pl.b * vy) + pl.c * vz) + pl.d >= 0.0f);
      }
    }
  }
  if (!hit) vx = vy = vz = nx = ny = nz = HSK_NANF;
  const bool colour = tl.mode == HSK_VIEW_COLOR || tl.mode == HSK_VIEW_COLOR_LIT;
  unsigned c0 = tl.background & 255u, c1 = (tl.background >> 8) & 255u, c2 = (tl.background >> 16) & 255u;
  unsigned dmm = 0u;
  bool uncolored = false;
  if (hit || cut) {
    // depth along the optical axis from the camera's t, in the sensor's unit: of the vertex, or of the ray's start on the plane
    const float px_ = cut ? t0 + d0 * t_sec : vx, py_ = cut ? t1 + d1 * t_sec : vy, pz_ = cut ? t2 + d2 * t_sec : vz;
    const float zc = (cam->R[2] * (px_ - cam->t[0]) + cam->R[5] * (py_ - cam->t[1])) + cam->R[8] * (pz_ - cam->t[2]);
    const float d = rintf(zc * 1000.0f);
    if (d >= 1.0f && d <= 65535.0f) dmm = (unsigned)(int)d;
  }
  if (cut) {
    c0 = tl.cut & 255u;
    c1 = (tl.cut >> 8) & 255u;
    c2 = (tl.cut >> 16) & 255u;
  }
  if (hit) {
    int br = 0;
    if (tl.mode == HSK_VIEW_LAMBERT || tl.mode == HSK_VIEW_COLOR_LIT) br = section_brightness(cam, tl, vx, vy, vz, nx, ny, nz);
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
  if (in_px) {
    // (the pixel's index is formed again here, from the thread's number as the stage text forms it: behind the empty asm it is not
    // the prelude's value, which then need not live through the march and the refinement -- two VGPRs where every one counts)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int tile_ = blockIdx.x * (blockDim.x >> 6) + (tid >> 6), lane_ = tid & 63;
    const int ty_lin_ = tile_ / tiles_x;
    const int ty_ = (ty_lin_ & 1) ? (tiles_y - 1 - (ty_lin_ >> 1)) : (ty_lin_ >> 1);
    const size_t i = (size_t)(ty_ * RC_TH + (lane_ / RC_TW)) * W + ((tile_ % tiles_x) * RC_TW + (lane_ % RC_TW));
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
  // one atomic add per wave and counter (every lane of the wave arrives here: none has returned), into the tile's slot of
  // HSK_VIEW_COUNT_SLOTS (view.hip: why slots)
  const unsigned n_hit = (unsigned)__popcll(__ballot(hit));
  const unsigned n_unc = (unsigned)__popcll(__ballot(hit && colour && uncolored));
  const unsigned n_cut = (unsigned)__popcll(__ballot(cut));
  if (lane == 0) {
    unsigned long long* c = tl.counts + ((unsigned)tile % HSK_VIEW_COUNT_SLOTS) * 16u;
    if (n_hit) atomicAdd(c, (unsigned long long)n_hit);
    if (n_unc) atomicAdd(c + 1, (unsigned long long)n_unc);
    if (n_cut) atomicAdd(c + 2, (unsigned long long)n_cut);
  }
}

void launch_render_section(hipStream_t s, const void* vol, const unsigned* colv, const ViewCam* cam, const VolParams& vp, int W, int H,
                           Intr in, const unsigned* flags, int mode, const float light[3], int light_in_camera, int light_directional,
                           const unsigned char background[3], const unsigned char cut_rgb[3], const SectionClip& clip,
                           unsigned char* rgb, unsigned short* depth, float* vmap, float* nmap, unsigned long long* counts) {
  // the tile shapes of launch_render_view
  const int tw_px = vp.stream_nt ? 16 : 8;
  const int tiles = ((W + tw_px - 1) / tw_px) * ((H + 64 / tw_px - 1) / (64 / tw_px));
  SectionArgs a;
  a.flags = flags;
  a.flag_words = hsk_flag_words(vp);
  a.W = W;
  a.H = H;
  a.cam = cam;
  a.vol = (const short2*)vol;
  a.in = in;
  a.vp = vp;
  a.clip = clip;
  a.tail.rgb = rgb;
  a.tail.depth = depth;
  a.tail.vmap = vmap;
  a.tail.nmap = nmap;
  a.tail.counts = counts;
  a.tail.colv = colv;
  for (int c = 0; c < 3; ++c) a.tail.light[c] = light[c];
  a.tail.light_in_camera = light_in_camera;
  a.tail.light_directional = light_directional;
  a.tail.mode = mode;
  a.tail.background = (unsigned)background[0] | ((unsigned)background[1] << 8) | ((unsigned)background[2] << 16);
  a.tail.cut = (unsigned)cut_rgb[0] | ((unsigned)cut_rgb[1] << 8) | ((unsigned)cut_rgb[2] << 16);
  const size_t lds = (size_t)(a.flag_words + HSK_SUPER_WORDS) * 4;
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
