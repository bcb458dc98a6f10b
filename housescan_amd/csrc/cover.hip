// cover.hip -- scan coverage for gfx950 (hsk_coverage_census, hsk_score_views, hsk_render_coverage; DESIGN.md 3.15 the kernels,
// 8i the rule; tests/cover_twin.py restates the rule in numpy): what a volume has never observed, and how much of it a camera
// at each of many candidate poses would reveal.
//
// k_cover_rays: a wave is one 8 x 8 tile of a probe's rays (lane = 8 row + column: neighbouring rays read neighbouring voxels)
// under one pose; a block is four tiles, the grid tiles x poses (a block strides over the poses when there are more than the grid's
// second dimension holds).  The pose's 12 floats are uniform: scalar loads.  A ray is hsk_cover_point.h's: per trip the 4-byte
// gathers of COVER_GROUP samples are issued together -- their addresses hang on the pose and the pixel alone -- and the state
// machine then takes them in order; a lane whose ray has ended gathers nothing more, and a wave whose rays have all ended leaves
// the loop (ballot).  The class counts are the wave's (a ballot and a population count per class), the gain one butterfly; lane 0
// adds the wave's non-zero values to the pose's record with integer atomics (the records are zeroed in front): integers, so any
// order gives the same bits, and no scratch grows with tiles x poses.  The image form also stores each pixel's class, depth and gain.
// k_cover_census: one sweep in k_pack_classify's shape, clipped to the lane-blocks the box touches: a thread owns a column of 16-B
// vectors through a brick layer (16 independent loads) and keeps two bit masks of its 64 voxels, UNSEEN and FREE.  The six
// neighbours' UNSEEN masks are shifts of its own (x inside a vector, y inside its rows), its workgroup's masks in LDS (x: the
// thread 4 to either side -- a workgroup's first and last four threads only publish theirs, the workgroups overlap by that
// much; z: the thread 1 or 3 to either side, a lane-block being 4 vectors deep) and, at the rim of what the thread owns, vectors
// read again (one row below and above per plane group; the plane next to the brick layer for the threads of planes 0 and 3):
// lines other threads stream anyway, and issued together with the thread's own loads, so a workgroup waits for memory once.
// Ten workgroup sums go to [10][workgroup]; k_cover_census_sum adds them, a workgroup per value.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_cover_point.h"

template <bool IMAGE>
__global__ __launch_bounds__(256) void k_cover_rays(const unsigned* __restrict__ vol, const float* __restrict__ poses, SampleVol dv, CoverProbe pr,
                                                    unsigned n_poses, unsigned tiles_x, unsigned n_tiles, hsk_view_score* __restrict__ scores,
                                                    unsigned char* __restrict__ cls_out, unsigned short* __restrict__ depth_out,
                                                    unsigned short* __restrict__ gain_out) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (tile >= n_tiles) return;
  const int pu = (int)((tile % tiles_x) * 8u + (lane & 7u)), pv = (int)((tile / tiles_x) * 8u + (lane >> 3));
  const bool live = pu < pr.W && pv < pr.H;  // (a ragged tile's other lanes walk no ray and store nothing)
  const float dx = cover_dir(pu, pr.cx, pr.fx), dy = cover_dir(pv, pr.cy, pr.fy);
  for (unsigned pose = blockIdx.y; pose < n_poses; pose += gridDim.y) {
    const float* __restrict__ P = poses + (size_t)pose * 12u;  // uniform over the block: scalar loads
    float R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = P[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = P[9 + i];
    CoverRay r = cover_ray_begin(live);
    for (int i0 = 0; i0 < pr.n; i0 += COVER_GROUP) {
      const bool run = cover_running(r.rs);
      if (__ballot(run) == 0ull) break;
      if (run) cover_ray_group(vol, dv, pr, R, t, dx, dy, i0, r);
    }
    const int cls = live ? cover_class(r.rs) : -1;
    unsigned cnt[COVER_CLASSES];
#pragma unroll
    for (int c = 0; c < COVER_CLASSES; ++c) cnt[c] = (unsigned)__popcll(__ballot(cls == c));
    const unsigned gain = hsk_wave_sum(live ? r.gain : 0u);
    hsk_view_score* __restrict__ sc = scores + pose;
    if (tile == 0u) {
      const int eye = cover_eye_state(vol, dv, t);
      if (lane == 0u) sc->eye_state = (unsigned)eye;
    }
    if (lane == 0u) {
      if (cnt[COVER_HIT]) atomicAdd(&sc->n_hit, cnt[COVER_HIT]);
      if (cnt[COVER_FRONTIER]) atomicAdd(&sc->n_frontier, cnt[COVER_FRONTIER]);
      if (cnt[COVER_OPEN]) atomicAdd(&sc->n_open, cnt[COVER_OPEN]);
      if (cnt[COVER_BLIND]) atomicAdd(&sc->n_blind, cnt[COVER_BLIND]);
      if (cnt[COVER_OUTSIDE]) atomicAdd(&sc->n_outside, cnt[COVER_OUTSIDE]);
      if (gain) atomicAdd((unsigned long long*)&sc->gain, (unsigned long long)gain);
    }
    if (IMAGE && live) {
      const size_t at = (size_t)pv * (unsigned)pr.W + (unsigned)pu;
      if (cls_out) cls_out[at] = (unsigned char)cls;
      if (depth_out) depth_out[at] = (unsigned short)(r.decided >= 0 ? cover_depth_mm(cover_depth(pr, r.decided)) : 0u);
      if (gain_out) gain_out[at] = (unsigned short)(r.gain < 65535u ? r.gain : 65535u);
    }
  }
}

void launch_cover_rays(hipStream_t s, const void* vol, const VolParams& vp, const CoverProbe& pr, const float* poses12, unsigned n_poses,
                       hsk_view_score* scores, unsigned char* cls, unsigned short* depth, unsigned short* gain) {
  if (n_poses == 0) return;
  const unsigned tiles_x = ((unsigned)pr.W + 7u) / 8u, n_tiles = tiles_x * (((unsigned)pr.H + 7u) / 8u);
  const unsigned gx = (n_tiles + 3u) / 4u;
  // (at most 2^22 blocks in one launch: a block takes every gy-th pose)
  unsigned gy = n_poses < 65535u ? n_poses : 65535u;
  const unsigned room = (1u << 22) / gx;
  gy = gy < room ? gy : (room ? room : 1u);
  const bool image = cls || depth || gain;
  if (image)
    hipLaunchKernelGGL((k_cover_rays<true>), dim3(gx, gy), dim3(256), 0, s, (const unsigned*)vol, poses12, hsk_sample_vol(vp), pr, n_poses, tiles_x,
                       n_tiles, scores, cls, depth, gain);
  else
    hipLaunchKernelGGL((k_cover_rays<false>), dim3(gx, gy), dim3(256), 0, s, (const unsigned*)vol, poses12, hsk_sample_vol(vp), pr, n_poses, tiles_x,
                       n_tiles, scores, cls, depth, gain);
}

// ---- census ---------------------------------------------------------------------------------------------------------------
// A thread's 64 voxels as bits: nibble i = 8 g + y' is the vector of plane group g (0, 1) and row y' (0..7) of its brick layer,
// bit j of the nibble the voxel x = 4 (c >> 2) + j.
#define CZ_NIB_LO 0x1111111111111111ull  // bit 0 of every nibble
#define CZ_ROW0 0x0000000f0000000full    // the first row of both plane groups
#define CZ_ROW7 0xf0000000f0000000ull    // ... and the last

static __device__ __forceinline__ unsigned cz_unseen4(const uint4& v) {
  return (unsigned)((v.x >> 16) == 0u) | ((unsigned)((v.y >> 16) == 0u) << 1) | ((unsigned)((v.z >> 16) == 0u) << 2) | ((unsigned)((v.w >> 16) == 0u) << 3);
}
static __device__ __forceinline__ unsigned cz_free4(const uint4& v) {
  return (unsigned)(cover_state(v.x) == COVER_FREE) | ((unsigned)(cover_state(v.y) == COVER_FREE) << 1) |
         ((unsigned)(cover_state(v.z) == COVER_FREE) << 2) | ((unsigned)(cover_state(v.w) == COVER_FREE) << 3);
}
// the UNSEEN bits of vector c of row y in plane group G, read again; 0 where that lies outside the grid (the padding planes too)
static __device__ __forceinline__ unsigned cz_unseen_at(const uint4* __restrict__ vol, const CoverSweep& g, int G, int y, int c) {
  if (G < 0 || y < 0 || y >= g.Y || c < 0 || c >= g.X || 4 * G + (c & 3) >= g.Z) return 0u;
  return cz_unseen4(vol[((size_t)G * (unsigned)g.Y + (unsigned)y) * (unsigned)g.X + (unsigned)c]);
}
// ... of all 16 vectors of the thread's shape at column c (a block's rim in x)
static __device__ __forceinline__ unsigned long long cz_unseen_column(const uint4* __restrict__ vol, const CoverSweep& g, int bz, int by, int c) {
  unsigned long long m = 0ull;
#pragma unroll
  for (int i = 0; i < 16; ++i) m |= (unsigned long long)cz_unseen_at(vol, g, 2 * bz + (i >> 3), 8 * by + (i & 7), c) << (4 * i);
  return m;
}

// threads of a workgroup that count: the four at either end only publish their masks, so that every counting thread finds the
// masks 4 threads to either side in LDS
#define CZ_OWN 248u

__global__ __launch_bounds__(256) void k_cover_census(const uint4* __restrict__ vol, CoverSweep g, unsigned n_threads, unsigned n_blocks,
                                                      unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long s_u[256];
  const unsigned tid = threadIdx.x;
  const long long ts = (long long)blockIdx.x * CZ_OWN + tid - 4;  // (a workgroup overlaps its neighbours by four threads at either end)
  const bool act = ts >= 0 && ts < (long long)n_threads;
  const bool own = act && tid >= 4u && tid < 4u + CZ_OWN;
  const unsigned t = act ? (unsigned)ts : 0u;
  const unsigned cc = t % (unsigned)g.ncols, r = t / (unsigned)g.ncols;
  const int c = g.c0 + (int)cc, by = g.by0 + (int)(r % (unsigned)g.nby), bz = g.bz0 + (int)(r / (unsigned)g.nby);
  const int pl = c & 3;  // this thread's plane within a group (tid & 3 as well: every offset above is a multiple of 4)
  // every load of the thread is issued before the first is used: its own 16 vectors, one row below and above per plane group,
  // and for the threads of planes 0 and 3 the eight vectors of the plane next to the brick layer
  uint4 v[16], hy[4], hz[8];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int i = 0; i < 4; ++i) hy[i] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int i = 0; i < 8; ++i) hz[i] = make_uint4(0u, 0u, 0u, 0u);
  unsigned long long have = 0ull;  // the nibbles whose vector exists (a plane below Z)
  unsigned have_y = 0u;            // bit 2 g + s: the row below (s = 0) / above (s = 1) of plane group g exists
  bool have_z = false;
  const size_t row = (unsigned)g.X, grp = (size_t)(unsigned)g.Y * (unsigned)g.X;
  if (act) {
#pragma unroll
    for (int gg = 0; gg < 2; ++gg) {
      if (8 * bz + 4 * gg + pl < g.Z) {
        const uint4* __restrict__ p = vol + (size_t)(unsigned)(2 * bz + gg) * grp + (size_t)(unsigned)(8 * by) * row + (unsigned)c;
#pragma unroll
        for (int y = 0; y < 8; ++y) v[gg * 8 + y] = p[(size_t)y * row];
        have |= 0xffffffffull << (32 * gg);
        if (own && by > 0) {
          hy[2 * gg] = *(p - row);
          have_y |= 1u << (2 * gg);
        }
        if (own && 8 * by + 8 < g.Y) {
          hy[2 * gg + 1] = p[8 * row];
          have_y |= 2u << (2 * gg);
        }
      }
    }
    // (the plane before plane 0 is plane 3 of the group before: column c + 3; the plane behind plane 3 is plane 0 of the group
    // behind: column c - 3)
    const int zg = pl == 0 ? 2 * bz - 1 : 2 * bz + 2, zc = pl == 0 ? c + 3 : c - 3;
    have_z = own && (pl == 0 || pl == 3) && zg >= 0 && 4 * zg + (zc & 3) < g.Z;
    if (have_z) {
      const uint4* __restrict__ p = vol + (size_t)(unsigned)zg * grp + (size_t)(unsigned)(8 * by) * row + (unsigned)zc;
#pragma unroll
      for (int y = 0; y < 8; ++y) hz[y] = p[(size_t)y * row];
    }
  }
  unsigned long long U = 0ull, F = 0ull;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    U |= (unsigned long long)cz_unseen4(v[i]) << (4 * i);
    F |= (unsigned long long)cz_free4(v[i]) << (4 * i);
  }
  U &= have;  // (a vector that does not exist is no voxel: not UNSEEN)
  s_u[tid] = U;
  // the box: bits of the voxels lo <= (x, y, z) < hi
  unsigned long long B = 0ull;
  {
    unsigned xn = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = 4 * (c >> 2) + j;
      xn |= (unsigned)(x >= g.lo[0] && x < g.hi[0]) << j;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int z = 8 * bz + 4 * (i >> 3) + pl, y = 8 * by + (i & 7);
      const bool in = z >= g.lo[2] && z < g.hi[2] && y >= g.lo[1] && y < g.hi[1];
      B |= (unsigned long long)(in ? xn : 0u) << (4 * i);
    }
    B = own ? B : 0ull;
  }
  // y: inside the thread's rows, and the rows read above; z at the brick layer's rim: the planes read above
  unsigned long long n_ym = (U << 4) & ~CZ_ROW0, n_yp = (U >> 4) & ~CZ_ROW7, z_rim = 0ull;
#pragma unroll
  for (int gg = 0; gg < 2; ++gg) {
    n_ym |= (unsigned long long)((have_y >> (2 * gg)) & 1u ? cz_unseen4(hy[2 * gg]) : 0u) << (32 * gg);
    n_yp |= (unsigned long long)((have_y >> (2 * gg + 1)) & 1u ? cz_unseen4(hy[2 * gg + 1]) : 0u) << (32 * gg + 28);
  }
#pragma unroll
  for (int y = 0; y < 8; ++y) z_rim |= (unsigned long long)cz_unseen4(hz[y]) << (4 * y);
  z_rim = have_z ? z_rim : 0ull;
  __syncthreads();
  unsigned long long n_xm = 0ull, n_xp = 0ull, n_zm = 0ull, n_zp = 0ull;
  if (own) {
    // x: inside a vector, and the vector 4 columns to either side (the same plane of the next lane-block): 4 threads away, or,
    // where a box's sweep ends inside the grid, read now
    unsigned long long left = 0ull, right = 0ull;
    if (cc >= 4u) left = s_u[tid - 4u];
    else if (c >= 4) left = cz_unseen_column(vol, g, bz, by, c - 4);
    if (cc + 4u < (unsigned)g.ncols) right = s_u[tid + 4u];
    else if (c + 4 < g.X) right = cz_unseen_column(vol, g, bz, by, c + 4);
    n_xm = ((U << 1) & ~CZ_NIB_LO) | ((left >> 3) & CZ_NIB_LO);
    n_xp = ((U >> 1) & ~(CZ_NIB_LO << 3)) | ((right & CZ_NIB_LO) << 3);
    // z: the plane before is the thread before, or -- plane 0 -- the other plane group of the thread 3 on and the rim; the plane
    // behind likewise
    n_zm = pl > 0 ? s_u[tid - 1u] : ((s_u[tid + 3u] & 0xffffffffull) << 32) | z_rim;
    n_zp = pl < 3 ? s_u[tid + 1u] : (s_u[tid - 3u] >> 32) | (z_rim << 32);
  }
  const unsigned long long FB = F & B;
  unsigned val[10];
  val[0] = (unsigned)__popcll(U & B);
  val[1] = (unsigned)__popcll(FB);
  val[2] = (unsigned)__popcll(B) - val[0] - val[1];
  val[3] = (unsigned)__popcll(FB & (((n_xm | n_xp) | (n_ym | n_yp)) | (n_zm | n_zp)));
  val[4] = (unsigned)__popcll(FB & n_xm);
  val[5] = (unsigned)__popcll(FB & n_xp);
  val[6] = (unsigned)__popcll(FB & n_ym);
  val[7] = (unsigned)__popcll(FB & n_yp);
  val[8] = (unsigned)__popcll(FB & n_zm);
  val[9] = (unsigned)__popcll(FB & n_zp);
#pragma unroll
  for (int i = 0; i < 10; ++i) val[i] = hsk_wave_sum(val[i]);
  const unsigned sum = hsk_block_meet<HskSum>(val);
  if (tid < 10u) partial[(size_t)tid * n_blocks + blockIdx.x] = (unsigned long long)sum;
}

// workgroup v adds the workgroups' sums of value v (partial[v][n_blocks]) -> out[v]: hsk_coverage's words
__global__ __launch_bounds__(256) void k_cover_census_sum(const unsigned long long* __restrict__ partial, unsigned n_blocks,
                                                          unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_sum[4];
  const unsigned long long* __restrict__ p = partial + (size_t)blockIdx.x * n_blocks;
  unsigned long long v = 0ull;
  for (unsigned b0 = threadIdx.x; b0 < n_blocks; b0 += 2048u) {  // (eight independent loads a trip: a lane walking its rows one
    unsigned long long x[8];                                      // dependent load after the other took 13 us for 8192 rows)
#pragma unroll
    for (unsigned k = 0; k < 8u; ++k) x[k] = b0 + 256u * k < n_blocks ? p[b0 + 256u * k] : 0ull;
#pragma unroll
    for (unsigned k = 0; k < 8u; ++k) v += x[k];
  }
  v = hsk_wave_sum(v);
  if ((threadIdx.x & 63u) == 0u) s_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0u) out[blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
}

// the sweep of a box lo <= v < hi (inside the grid, not empty): the lane-blocks, brick rows and brick layers it touches
CoverSweep cover_sweep(const VolParams& vp, const int lo[3], const int hi[3]) {
  CoverSweep g;
  g.X = vp.X;
  g.Y = vp.Y;
  g.Z = vp.Z;
  for (int i = 0; i < 3; ++i) {
    g.lo[i] = lo[i];
    g.hi[i] = hi[i];
  }
  g.c0 = (lo[0] >> 2) * 4;
  g.ncols = ((hi[0] + 3) >> 2) * 4 - g.c0;
  g.by0 = lo[1] >> 3;
  g.nby = ((hi[1] + 7) >> 3) - g.by0;
  g.bz0 = lo[2] >> 3;
  g.nbz = ((hi[2] + 7) >> 3) - g.bz0;
  return g;
}
unsigned cover_census_blocks(const CoverSweep& g) { return ((unsigned)g.ncols * (unsigned)g.nby * (unsigned)g.nbz + CZ_OWN - 1u) / CZ_OWN; }

void launch_cover_census(hipStream_t s, const void* vol, const CoverSweep& g, unsigned long long* partial, unsigned long long* out10) {
  const unsigned n_threads = (unsigned)g.ncols * (unsigned)g.nby * (unsigned)g.nbz, n_blocks = cover_census_blocks(g);
  hipLaunchKernelGGL(k_cover_census, dim3(n_blocks), dim3(256), 0, s, (const uint4*)vol, g, n_threads, n_blocks, partial);
  hipLaunchKernelGGL(k_cover_census_sum, dim3(10), dim3(256), 0, s, partial, n_blocks, out10);
}

int cover_warm() {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, (const void*)k_cover_rays<false>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_cover_rays<true>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_cover_census);
  return (int)e;
}
