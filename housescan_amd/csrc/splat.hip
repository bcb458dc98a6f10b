// splat.hip -- cloud import for gfx950 (hsk_splat_cloud, hsk_import_cloud; DESIGN.md 3.27 the kernels, 8u the rule): a cloud in the
// alignment scratch's planes (hsk_cloud_dev.h) rendered into the depth image of a virtual camera.  k_splat_points: a lane a point
// (hsk_splat_point.h), its footprint's pixels offered to a z-buffer of 32-bit words by atomicMin -- an integer minimum, so the
// image is the same bits whatever the order; k_splat_resolve: the z-buffer as the 16-bit frame the integrate stage takes, and the
// z-buffer armed again for the next view; k_splat_pose: the view's pose into the tracker state, where the integrate reads it.
#pragma clang fp contract(off)
#include "hsk_cloud_dev.h"
#include "hsk_launch.h"
#include "hsk_splat_point.h"

#define SPLAT_GRID_MAX 1024u  // blocks of a launch: a cloud beyond 262144 points takes further passes of the same grid

// counts: SPLAT_COUNT_WORDS words of the view -- the points by SPLAT_* class, then (k_splat_resolve) the pixels with a depth --
// zeroed by the caller
__global__ __launch_bounds__(256) void k_splat_points(const float* __restrict__ soa, unsigned n, unsigned pitch, int with_normals, SplatCam cam,
                                                      SplatPose pose, SplatArgs args, unsigned* __restrict__ zbuf, unsigned* __restrict__ counts) {
  unsigned c[SPLAT_CLASSES] = {0u, 0u, 0u, 0u, 0u};
  for (unsigned base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {  // (the same trips for every thread of the block)
    const unsigned i = base + threadIdx.x;
    const bool act = i < n;
    const unsigned at = hsk_cloud_at(act, i, n);
    const CloudPos p = hsk_cloud_pos(soa, at, pitch);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (with_normals) {
      nx = hsk_cloud_word(soa, 3u, at, pitch);
      ny = hsk_cloud_word(soa, 4u, at, pitch);
      nz = hsk_cloud_word(soa, 5u, at, pitch);
    }
    SplatFoot f;
    const int cls = act ? splat_point(cam, pose, args, p.x, p.y, p.z, with_normals != 0, nx, ny, nz, f) : -1;
#pragma unroll
    for (int k = 0; k < SPLAT_CLASSES; ++k) c[k] += cls == k ? 1u : 0u;
    const bool draws = cls == SPLAT_DONE;
    if (__ballot(draws) == 0ull) continue;  // none of the wave's points survives: the wave moves on whole
    if (draws) {
      for (int v = f.v_lo; v <= f.v_hi; ++v) {
        unsigned* __restrict__ row = zbuf + (size_t)v * (size_t)cam.w;  // (0 <= v < h, 0 <= u < w: splat_span clips to the image)
        for (int u = f.u_lo; u <= f.u_hi; ++u) {
          const unsigned offer = splat_offer(cam, f, u, v);
          // the word only ever falls: a stale read costs an atomic, never a pixel
          if (__hip_atomic_load(row + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > offer) atomicMin(row + u, offer);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < SPLAT_CLASSES; ++k) c[k] = hsk_wave_fold<HskSum>(c[k], k);
  const unsigned r = hsk_block_meet<HskSum>(c);
  if (threadIdx.x < (unsigned)SPLAT_CLASSES && r != 0u) atomicAdd(counts + threadIdx.x, r);
}

__global__ __launch_bounds__(256) void k_splat_resolve(unsigned* __restrict__ zbuf, unsigned n_pixels, unsigned short* __restrict__ frame,
                                                       unsigned* __restrict__ counts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned z = SPLAT_EMPTY;
  if (i < n_pixels) {
    z = zbuf[i];
    zbuf[i] = SPLAT_EMPTY;
    frame[i] = z == SPLAT_EMPTY ? (unsigned short)0 : (unsigned short)z;  // (an offer is 1 .. 65535)
  }
  unsigned c[1] = {(unsigned)__popcll(__ballot(z != SPLAT_EMPTY))};
  const unsigned r = hsk_block_meet<HskSum>(c);
  if (threadIdx.x == 0u && r != 0u) atomicAdd(counts + SPLAT_CLASSES, r);
}

// what hsk_set_pose does to the tracker state, without the host in between
__global__ void k_splat_pose(TrackState* __restrict__ st, SplatPose pose) {
  if (threadIdx.x < 9u) st->R[threadIdx.x] = pose.R[threadIdx.x];
  if (threadIdx.x < 3u) st->t[threadIdx.x] = pose.t[threadIdx.x];
  if (threadIdx.x == 0u) st->lost = 0;
}

void launch_splat_points(hipStream_t s, const float* soa, unsigned n, unsigned pitch, bool with_normals, const SplatCam& cam, const SplatPose& pose,
                         const SplatArgs& args, unsigned* zbuf, unsigned* counts) {
  if (n == 0u) return;
  const unsigned blocks = (n + 255u) / 256u;
  k_splat_points<<<blocks < SPLAT_GRID_MAX ? blocks : SPLAT_GRID_MAX, 256, 0, s>>>(soa, n, pitch, with_normals ? 1 : 0, cam, pose, args, zbuf, counts);
}
void launch_splat_resolve(hipStream_t s, unsigned* zbuf, unsigned n_pixels, unsigned short* frame, unsigned* counts) {
  k_splat_resolve<<<(n_pixels + 255u) / 256u, 256, 0, s>>>(zbuf, n_pixels, frame, counts);
}
void launch_splat_pose(hipStream_t s, TrackState* st, const SplatPose& pose) { k_splat_pose<<<1, 64, 0, s>>>(st, pose); }

// loads this file's code object (hsk_prepare_readout); a hipError_t
int splat_warm() {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, (const void*)k_splat_points);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_splat_resolve);
  return (int)e;
}
