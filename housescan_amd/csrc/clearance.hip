// clearance.hip -- the clearance field for gfx950 (hsk_build_clearance, hsk_download_clearance, hsk_clearance_at,
// hsk_clearance_floor; DESIGN.md 3.18 the kernels, 8l the rule; tests/clearance_twin.py restates the rule in numpy): the exact
// squared distance, under integer axis weights, from every voxel to the nearest obstacle, as three separable passes.  Every value
// is an integer and every pass a minimum: no schedule can change a bit.  No kernel here waits for another workgroup, wave or lane;
// every loop is bounded by the reach (at most 255) or by the grid, and says so.
//
// k_clear_rows, the x pass and the only kernel that reads the block layout: a wave takes one (y, plane group).  A row of a plane
// group is X 16-B vectors in a piece (vector i: lane-block i >> 2, plane i & 3, four x-adjacent voxels), so the lanes' loads cover
// whole sectors.  The obstacle bits of the four planes' rows are collected as 64-bit masks in LDS (an integer OR per vector);
// then, lanes along x, each voxel finds the nearest set bit on either side by counting leading / trailing zeros over the mask
// words (hsk_clear_point.h) and writes the distance as uint16 to a row-major array.  The wave's obstacles are counted from the
// masks and added once.
// k_clear_axis<AXIS>, y then z: lanes along x, so every load and store of a wave is one contiguous piece (128 B of
// uint16, 256 B of uint32); a wave makes CLEAR_AXIS_SEG consecutive outputs along the axis and reads its window straight from
// memory (the windows of neighbouring outputs overlap in all but one row: they are served by the caches).  It is the one form
// that serves every legal reach: a tile of 64 lanes with its halo fits 64 KiB of LDS only up to a reach of 96, short of the 170 of
// a 512^3 volume's default metre; DESIGN.md 3.18 has both forms measured (tools/clearance_axis_forms.hip) where the tile fits.
// The z pass writes the field and adds n_far and max_d2_seen, wave-reduced first.
// k_clear_project, k_clear_axis_plain, k_clear_gather: the floor map's column test and its two passes over a 2-D array, the
// lookup of n points.  A thread an item; speed does not matter there.  (A box of the field: volume_sweep.hip's k_box_rows.)
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_clear_point.h"

// ---- the x pass ---------------------------------------------------------------------------------------------------------------
// dynamic LDS: per wave 4 planes x nw mask words of 64 bits
__global__ __launch_bounds__(256) void k_clear_rows(const uint4* __restrict__ vol, unsigned short* __restrict__ dx, ClearGeom q,
                                                    unsigned long long* __restrict__ stats) {
  extern __shared__ unsigned long long s_mask_all[];
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned row = blockIdx.x * 4u + wave;  // (y, plane group)
  unsigned long long* s_mask = s_mask_all + (size_t)wave * 4u * q.nw;
  const bool live = row < q.Y * q.Zg;  // (wave-uniform; a dead wave still meets the barriers below)
  const unsigned y = row % q.Y, zg = row / q.Y;
  for (unsigned i = lane; i < 4u * q.nw; i += 64u) s_mask[i] = 0ull;  // (ends: i grows by 64)
  __syncthreads();
  if (live) {
    const uint4* __restrict__ src = vol + ((size_t)zg * q.Y + y) * q.X;  // (X vectors a row: X / 4 lane-blocks of four)
    for (unsigned i0 = 0u; i0 < q.X; i0 += 64u) {  // (ends: i0 grows by 64; a wave-uniform trip count)
      const unsigned i = i0 + lane, pl = i & 3u, x0 = (i >> 2) << 2;
      if (i < q.X && 4u * zg + pl < q.Z) {  // (a padding plane is no voxel: not read, no obstacle)
        const uint4 v = src[i];
        const unsigned bits = (clear_obstacle(v.x, q.flags) ? 1u : 0u) | (clear_obstacle(v.y, q.flags) ? 2u : 0u) |
                              (clear_obstacle(v.z, q.flags) ? 4u : 0u) | (clear_obstacle(v.w, q.flags) ? 8u : 0u);
        // (x0 is a multiple of 4: the four bits lie in one 32-bit half of their mask word)
        if (bits) atomicOr((unsigned*)(s_mask + (size_t)pl * q.nw) + (x0 >> 5), bits << (x0 & 31u));
      }
    }
  }
  __syncthreads();
  if (!live) return;  // (the whole wave, behind the last barrier)
  unsigned n_obst = 0u;
  for (unsigned i = lane; i < 4u * q.nw; i += 64u) n_obst += (unsigned)__popcll(s_mask[i]);  // (ends: i grows by 64)
  n_obst = hsk_wave_sum(n_obst);
  if (lane == 0u && n_obst) atomicAdd(&stats[0], (unsigned long long)n_obst);
#pragma unroll 1
  for (unsigned pl = 0u; pl < 4u; ++pl) {
    const unsigned z = 4u * zg + pl;
    if (z >= q.Z) break;  // (wave-uniform)
    unsigned short* __restrict__ dst = dx + ((size_t)z * q.Y + y) * q.X;
    for (unsigned x0 = 0u; x0 < q.X; x0 += 64u) {  // (ends: x0 grows by 64)
      const unsigned x = x0 + lane;
      if (x < q.X) dst[x] = (unsigned short)clear_row_dx(s_mask + (size_t)pl * q.nw, q.nw, x, q.X, q.R[0], q.flags);
    }
  }
}

// ---- the y and z passes -------------------------------------------------------------------------------------------------------
// the loads of a pass: position i along the axis, `stride` elements apart, from the voxel's base
struct ClearLoadDx {
  const unsigned short* p;
  size_t stride;
  unsigned wx;
  __device__ __forceinline__ unsigned operator()(unsigned i) const { return clear_dx_value(p[(size_t)i * stride], wx); }
};
struct ClearLoadU32 {
  const unsigned* p;
  size_t stride;
  __device__ __forceinline__ unsigned operator()(unsigned i) const { return p[(size_t)i * stride]; }
};

// AXIS 1: the y pass, uint16 distances in, capped sums out (CLEAR_INF above max_d2).  AXIS 2: the z pass, those in, the field out
// (CLEAR_FAR above max_d2) and the counts.  Grid: x segments of 64 x segments of the axis x the third axis; a wave a segment.
template <int AXIS>
__global__ __launch_bounds__(256) void k_clear_axis(const void* __restrict__ in, unsigned* __restrict__ out, ClearGeom q,
                                                    unsigned long long* __restrict__ stats) {
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned n = AXIS == 1 ? q.Y : q.Z, other = AXIS == 1 ? q.Z : q.Y;
  const unsigned nxs = (q.X + 63u) >> 6, nseg = (n + CLEAR_AXIS_SEG - 1u) / CLEAR_AXIS_SEG;
  const unsigned id = blockIdx.x * 4u + wave;  // ((o nseg) + seg) nxs + xs
  const unsigned xs = id % nxs, t = id / nxs, seg = t % nseg, o = t / nseg;
  const unsigned x = 64u * xs + lane;
  const bool live = o < other && x < q.X;  // (o < other: wave-uniform)
  const size_t stride = AXIS == 1 ? (size_t)q.X : (size_t)q.X * q.Y;
  const size_t base = AXIS == 1 ? (size_t)o * q.Y * q.X + x : (size_t)o * q.X + x;
  unsigned n_far = 0u, seen = 0u;
  if (live) {
    const unsigned i1 = (seg + 1u) * CLEAR_AXIS_SEG < n ? (seg + 1u) * CLEAR_AXIS_SEG : n;
    for (unsigned i = seg * CLEAR_AXIS_SEG; i < i1; ++i) {  // (at most CLEAR_AXIS_SEG trips)
      unsigned v;
      if (AXIS == 1) {
        const ClearLoadDx ld{(const unsigned short*)in + base, stride, q.w[0]};
        v = clear_cap(clear_window_min(ld, i, n, q.w[1], q.R[1], q.flags), q.max_d2, CLEAR_INF);
      } else {
        const ClearLoadU32 ld{(const unsigned*)in + base, stride};
        v = clear_cap(clear_window_min(ld, i, n, q.w[2], q.R[2], q.flags), q.max_d2, CLEAR_FAR);
        n_far += v == CLEAR_FAR ? 1u : 0u;
        seen = (v != CLEAR_FAR && v > seen) ? v : seen;
      }
      out[base + (size_t)i * stride] = v;
    }
  }
  if (AXIS == 2) {  // (every lane of the wave arrives here: nothing above returns)
    n_far = hsk_wave_sum(n_far);
    seen = hsk_wave_max(seen);
    if (lane == 0u) {
      if (n_far) atomicAdd(&stats[1], (unsigned long long)n_far);
      if (seen) atomicMax(&stats[2], (unsigned long long)seen);
    }
  }
}

// ---- the floor map, the point lookup ------------------------------------------------------------------------------------------
// a column of the band lo <= p < hi along `axis` is an obstacle when any voxel of it is; u: the lower-numbered remaining axis
__global__ __launch_bounds__(256) void k_clear_project(const unsigned* __restrict__ vol, VolParams vp, unsigned flags, int axis, int lo, int hi,
                                                       unsigned nu, unsigned nv, unsigned* __restrict__ map) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= nu * nv) return;
  const int u = (int)(e % nu), v = (int)(e / nu);
  bool hit = false;
  for (int p = lo; p < hi; ++p) {  // (ends: the band lies inside the axis)
    const int x = axis == 0 ? p : u, y = axis == 0 ? u : axis == 1 ? p : v, z = axis == 2 ? p : v;
    hit = hit || clear_obstacle(vol[hsk_vox_index(vp, x, y, z)], flags);
  }
  map[e] = hit ? 0u : CLEAR_INF;
}

// one pass over a 2-D (or any strided) array of n_total elements: element e lies at position (e / stride) % len of its row
__global__ __launch_bounds__(256) void k_clear_axis_plain(const unsigned* __restrict__ in, unsigned* __restrict__ out, unsigned n_total,
                                                          unsigned len, unsigned stride, unsigned w, unsigned R, unsigned flags, unsigned max_d2,
                                                          unsigned far) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n_total) return;
  const unsigned i = (e / stride) % len;
  const ClearLoadU32 ld{in + (e - i * stride), (size_t)stride};
  out[e] = clear_cap(clear_window_min(ld, i, len, w, R, flags), max_d2, far);
}

__global__ __launch_bounds__(256) void k_clear_gather(const unsigned* __restrict__ field, SampleVol sv, const float* __restrict__ xyz, unsigned n,
                                                      unsigned* __restrict__ out) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  unsigned x, y, z;
  bool inside;
  clear_point_voxel(sv, xyz[3u * e], xyz[3u * e + 1u], xyz[3u * e + 2u], x, y, z, inside);
  const unsigned v = field[((size_t)z * (unsigned)sv.Y + y) * (unsigned)sv.X + x];  // (the clamped voxel: a legal load whatever the point is)
  out[e] = inside ? v : CLEAR_OUTSIDE;
}

// ---- the launchers ------------------------------------------------------------------------------------------------------------
size_t clear_layout(const VolParams& vp, void* base, ClearBufs* b) {
  const size_t n = (size_t)vp.X * vp.Y * vp.Z;
  ScratchCarve c{base};
  ClearBufs out;
  out.stats = (unsigned long long*)c.take(64);
  out.field = (unsigned*)c.take(n * 4);
  out.tmp = (unsigned*)c.take(n * 4);
  out.dx = (unsigned short*)c.take(n * 2);
  if (b) *b = out;
  return c.bytes;
}

void launch_clear_build(hipStream_t s, const void* vol, const ClearGeom& q, const ClearBufs& b) {
  (void)hipMemsetAsync(b.stats, 0, 64, s);
  const unsigned rows = q.Y * q.Zg;
  hipLaunchKernelGGL(k_clear_rows, dim3((rows + 3u) / 4u), dim3(256), (size_t)4 * 4 * q.nw * 8, s, (const uint4*)vol, b.dx, q, b.stats);
  const unsigned nxs = (q.X + 63u) >> 6;
  const unsigned wy = nxs * ((q.Y + CLEAR_AXIS_SEG - 1u) / CLEAR_AXIS_SEG) * q.Z, wz = nxs * ((q.Z + CLEAR_AXIS_SEG - 1u) / CLEAR_AXIS_SEG) * q.Y;
  hipLaunchKernelGGL((k_clear_axis<1>), dim3((wy + 3u) / 4u), dim3(256), 0, s, (const void*)b.dx, b.tmp, q, b.stats);
  hipLaunchKernelGGL((k_clear_axis<2>), dim3((wz + 3u) / 4u), dim3(256), 0, s, (const void*)b.tmp, b.field, q, b.stats);
}

void launch_clear_floor(hipStream_t s, const void* vol, const VolParams& vp, const ClearGeom& q, int axis, int lo, int hi, unsigned* a, unsigned* b) {
  const int au = axis == 0 ? 1 : 0, av = axis == 2 ? 1 : 2;
  const unsigned dims[3] = {q.X, q.Y, q.Z};
  const unsigned nu = dims[au], nv = dims[av], n = nu * nv, blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_clear_project, dim3(blocks), dim3(256), 0, s, (const unsigned*)vol, vp, q.flags, axis, lo, hi, nu, nv, a);
  hipLaunchKernelGGL(k_clear_axis_plain, dim3(blocks), dim3(256), 0, s, (const unsigned*)a, b, n, nu, 1u, q.w[au], q.R[au], q.flags, q.max_d2,
                     CLEAR_INF);
  hipLaunchKernelGGL(k_clear_axis_plain, dim3(blocks), dim3(256), 0, s, (const unsigned*)b, a, n, nv, nu, q.w[av], q.R[av], q.flags, q.max_d2,
                     CLEAR_FAR);
}

void launch_clear_gather(hipStream_t s, const unsigned* field, const VolParams& vp, const float* xyz, unsigned n, unsigned* out) {
  hipLaunchKernelGGL(k_clear_gather, dim3((n + 255u) / 256u), dim3(256), 0, s, field, hsk_sample_vol(vp), xyz, n, out);
}
