// raycast.hip -- TSDF raycast for gfx950: the synthetic model frame, its step keys and levels 1 and 2 of
// the model maps.  (Split out of kernels_volume.hip in round 5; no behaviour change.)
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_march.h"

// one level of the map pyramid inside a wave that holds an 8x8 pixel tile (lane = y * 8 + x): the lane at the top
// left of each 2x2 group (dx, dy = lane distance to its right / lower neighbour at this level) forms the mean of the
// vertex taps and the renormalised mean of the normal taps, NaN when any tap is NaN; other lanes' results are unused.
// (The rule is hsk_mean2x2's, hsk_dev.h, written out once more: calling it here changes k_raycast's listing.)
static __device__ __forceinline__ void pyramid_step(const float* m, int dx, int dy, float* out) {
  float t1[6], t2[6], t3[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    t1[c] = __shfl_down(m[c], dx, 64);
    t2[c] = __shfl_down(m[c], dy, 64);
    t3[c] = __shfl_down(m[c], dx + dy, 64);
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int b = 3 * h;
    float a0 = HSK_NANF, a1 = HSK_NANF, a2 = HSK_NANF;
    if (!(hsk_isnan(m[b]) || hsk_isnan(t1[b]) || hsk_isnan(t2[b]) || hsk_isnan(t3[b]))) {
      a0 = (((m[b] + t1[b]) + t2[b]) + t3[b]) / 4.0f;
      a1 = (((m[b + 1] + t1[b + 1]) + t2[b + 1]) + t3[b + 1]) / 4.0f;
      a2 = (((m[b + 2] + t1[b + 2]) + t2[b + 2]) + t3[b + 2]) / 4.0f;
      if (h == 1) {
        const float inv = 1.0f / sqrtf(hsk_dot3(a0, a1, a2, a0, a1, a2));
        a0 = a0 * inv;
        a1 = a1 * inv;
        a2 = a2 * inv;
      }
    }
    out[b] = a0;
    out[b + 1] = a1;
    out[b + 2] = a2;
  }
}

#ifdef HSK_RC_TIMING
__device__ unsigned long long g_rc_times[8192 * 8];  // per tile: 4 stamps, march trips, trips in which a lane gathered
extern "C" int hsk_debug_rc_times(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rc_times), (size_t)n * 8);
}
#define RC_STAMP(k) do { if (lane == 0 && tile_id < 8192) g_rc_times[tile_id * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define RC_STAMP(k) do { } while (0)
#endif

// What the kernel needs only AFTER the march (the maps it writes, the pyramid levels): kept out of the march loop's
// scalar registers.  The compiler loads every kernel argument it uses in the entry block and keeps it there; the march
// loop already needs ~100 SGPRs (uniform volume constants plus a saved lane mask per level of divergent control flow),
// so the 16 that these pointers took were spilled into VGPR lanes (v_writelane / v_readlane inside the loop, and any
// further scalar state cost VGPRs the same way: what rounds 2 and 3 took for a wall at 80 VGPRs).  They are therefore
// the LAST member of the argument block and read through the kernarg segment pointer after the loop.
struct RcTail {
  float* vmap;
  float* nmap;
  int* keys;
  MapPyramid pyr;
  int W, H;
};
struct RcArgs {   // (what the kernel needs first comes first: the first 16 dwords arrive in SGPRs with the wave)
  const unsigned* flags;
  int flag_words;
  int W, H;
  const TrackState* st;
  const short2* vol;
  RingOut ring;
  Intr in;
  VolParams vp;
  RcTail tail;   // never touched by name inside the kernel
};
// a member of the argument block fetched where it is used (see RcTail)
#define RC_ARG(type, member) (*(const type*)(rc_kernarg() + offsetof(RcArgs, member)))
static __device__ __forceinline__ const char* rc_kernarg() {
  const char* ka = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(ka));
  return ka;
}
// SLAB: this context stores / owns only part of the z range (multi-GPU).
template <bool SLAB, int RC_TW>
__global__ __launch_bounds__(RC_BLOCK, RC_WPE) void k_raycast(RcArgs a) {
  const short2* __restrict__ vol = a.vol;
  const TrackState* __restrict__ st = a.st;
  const VolParams& vp = a.vp;
  const int W = a.W, H = a.H;
  const Intr& in = a.in;
  const unsigned* __restrict__ flags = a.flags;
  const int flag_words = a.flag_words;
  const RingOut& ring = a.ring;
#include "hsk_march_stage.h"
  if (!SLAB && ring.slots && blockIdx.x == 0 && threadIdx.x == 0) {
    // the tracker state is final once the ICP has ended (nothing after it writes it): report it to the host now, also
    // for a lost or dropped frame, which returns just below
    const unsigned n = *ring.seq;
    *ring.seq = n + 1u;
    TrackState* dst = ring.slots + ring.slot_fifo[n % HSK_RING_FIFO];
    const int* src_w = (const int*)st;
    int* dst_w = (int*)dst;
    for (unsigned i = 0; i < (unsigned)(offsetof(TrackState, ring_mark) / 4); ++i) dst_w[i] = src_w[i];
    __threadfence_system();     // the state words reach the host before the marks that announce them
    // (pose_mark: already there when the integrate's first kernel reported early; set here for the frames it did not)
    __hip_atomic_store(&dst->pose_mark, (n + 1u) | 0x80000000u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&dst->ring_mark, (n + 1u) | 0x80000000u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // Lanes outside the image (a ragged last tile) and lanes whose ray misses the volume stay in the wave as rays that have
  // ended: every lane is then active at the top of the march loop, which lets its wave-wide decisions use DPP
  // reductions read from a fixed lane, and takes one level of divergent control flow out of the loop.
  const bool in_img = x < W && y < H;
  if (st->lost) return;
#include "hsk_march_rays.h"
#include "hsk_march_loop.h"
  // the tail of the argument block, fetched now (the empty asm hides where the pointer comes from, so the loads cannot
  // be moved up across the march)
  const RcTail tl = RC_ARG(RcTail, tail);
  float* __restrict__ vmap = tl.vmap;
  float* __restrict__ nmap = tl.nmap;
  int* __restrict__ keys = tl.keys;
  const MapPyramid pyr = tl.pyr;
  if (in_img) {
    vmap[i] = vx;
    vmap[P + i] = vy;
    vmap[2 * P + i] = vz;
    nmap[i] = nx;
    nmap[P + i] = ny;
    nmap[2 * P + i] = nz;
    if (keys) keys[i] = key;
  }
  RC_STAMP(3);
  if (!SLAB && pyr.v1) {
    // Model pyramid (resizeVMap / resizeNMap, A.3) from the wave's own 8x8 tile: level 1 is the 2x2 mean held by
    // the even-even lanes, level 2 the 2x2 mean of those -- the arithmetic and its order are hsk_mean2x2's (what
    // k_resize_maps2 computes), the taps arrive by lane shuffles instead of a second launch reading the maps back.
    float m[6] = {vx, vy, vz, nx, ny, nz};
    float l1[6], l2[6];
    pyramid_step(m, 1, RC_TW, l1);
    pyramid_step(l1, 2, 2 * RC_TW, l2);
    const int w1 = W >> 1, w2 = W >> 2;
    const size_t P1 = (size_t)w1 * (H >> 1), P2 = (size_t)w2 * (H >> 2);
    if (((x | y) & 1) == 0) {
      const size_t o = (size_t)(y >> 1) * w1 + (x >> 1);
      pyr.v1[o] = l1[0]; pyr.v1[P1 + o] = l1[1]; pyr.v1[2 * P1 + o] = l1[2];
      pyr.n1[o] = l1[3]; pyr.n1[P1 + o] = l1[4]; pyr.n1[2 * P1 + o] = l1[5];
    }
    if (((x | y) & 3) == 0) {
      const size_t o = (size_t)(y >> 2) * w2 + (x >> 2);
      pyr.v2[o] = l2[0]; pyr.v2[P2 + o] = l2[1]; pyr.v2[2 * P2 + o] = l2[2];
      pyr.n2[o] = l2[3]; pyr.n2[P2 + o] = l2[4]; pyr.n2[2 * P2 + o] = l2[5];
    }
  }
}

void launch_raycast(hipStream_t s, const void* vol, const TrackState* st, const VolParams& vp, int W, int H, Intr in,
                    float* vmap, float* nmap, int* keys, const unsigned* flags, const MapPyramid* pyramid, const RingOut* ring) {
  // (the wide tile wants whole tiles: the fused pyramid's shuffles assume them)
  const int tw_px = (vp.stream_nt && (W % 16) == 0 && (H % 4) == 0) ? 16 : 8;
  const int tiles = ((W + tw_px - 1) / tw_px) * ((H + 64 / tw_px - 1) / (64 / tw_px));
  dim3 block(RC_BLOCK);
  dim3 grid((tiles + RC_BLOCK / 64 - 1) / (RC_BLOCK / 64));
  const int words = hsk_flag_words(vp);
  const bool slab = vp.zs0 != 0 || vp.nzs != vp.Z || vp.zo0 != 0 || vp.zo1 != vp.Z;
  const MapPyramid none = {nullptr, nullptr, nullptr, nullptr};
  const RingOut quiet = {nullptr, nullptr, nullptr};
  RcArgs a;
  a.vol = (const short2*)vol;
  a.st = st;
  a.vp = vp;
  a.W = W;
  a.H = H;
  a.in = in;
  a.flags = flags;
  a.flag_words = words;
  a.ring = (!slab && ring) ? *ring : quiet;
  a.tail.vmap = vmap;
  a.tail.nmap = nmap;
  a.tail.keys = keys;
  a.tail.pyr = (!slab && pyramid) ? *pyramid : none;
  a.tail.W = W;
  a.tail.H = H;
  const size_t lds = (size_t)(words + HSK_SUPER_WORDS) * 4;
  if (slab && tw_px == 16)
    hipLaunchKernelGGL((k_raycast<true, 16>), grid, block, lds, s, a);
  else if (slab)
    hipLaunchKernelGGL((k_raycast<true, 8>), grid, block, lds, s, a);
  else if (tw_px == 16)
    hipLaunchKernelGGL((k_raycast<false, 16>), grid, block, lds, s, a);
  else
    hipLaunchKernelGGL((k_raycast<false, 8>), grid, block, lds, s, a);
}
// the fused pyramid needs complete 8x8 tiles and a single-device volume
bool raycast_can_fuse_pyramid(const VolParams& vp, int W, int H) {
  const bool slab = vp.zs0 != 0 || vp.nzs != vp.Z || vp.zo0 != 0 || vp.zo1 != vp.Z;
  return !slab && (W % 8) == 0 && (H % 8) == 0;
}
