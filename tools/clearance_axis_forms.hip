// clearance_axis_forms.hip -- a stand-alone measurement (its own main; not part of the library): one axis pass of the clearance
// field (housescan_amd/csrc/hsk_clear_point.h: clear_window_min) over a 512^3 array along z, in the two forms DESIGN.md 3.18
// weighs -- the window read straight from memory (what clearance.hip ships) and the segment plus its halo staged in LDS --
// at a reach whose tile fits 64 KiB (R = 85: max_d2 = 7282, the half-metre of a 512^3 volume over 3 m; at the default metre,
// R = 170, no tile of 64 lanes fits).  Inputs: 0 at a hashed fraction of the voxels, CLEAR_INF elsewhere -- a dense field
// (every loop short) and a sparse one (most loops run the whole window).  Both forms must give the same array; prints ms.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/clearance_axis_forms.hip -o clearance_axis_forms && ./clearance_axis_forms
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_clear_point.h"

#define CHECK(call)                                                                      \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "%s failed: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

#define SEG_DIRECT 16u  // CLEAR_AXIS_SEG
#define SEG_LDS 64u     // outputs along the axis a workgroup of the LDS form makes

struct Geom {
  unsigned X, Y, Z, w, R, max_d2, flags;
};
struct LoadU32 {
  const unsigned* p;
  size_t stride;
  __device__ __forceinline__ unsigned operator()(unsigned i) const { return p[(size_t)i * stride]; }
};

__global__ __launch_bounds__(256) void k_fill(unsigned* __restrict__ a, size_t n, unsigned per_million) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  unsigned h = (unsigned)i * 2654435761u;
  h ^= h >> 15;
  h *= 2246822519u;
  h ^= h >> 13;
  a[i] = (h % 1000000u) < per_million ? 0u : CLEAR_INF;
}

// the shipped form: a wave makes SEG_DIRECT consecutive outputs along z for 64 x, every load from memory
__global__ __launch_bounds__(256) void k_direct(const unsigned* __restrict__ in, unsigned* __restrict__ out, Geom q) {
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned nxs = (q.X + 63u) >> 6, nseg = (q.Z + SEG_DIRECT - 1u) / SEG_DIRECT;
  const unsigned id = blockIdx.x * 4u + wave;
  const unsigned xs = id % nxs, t = id / nxs, seg = t % nseg, y = t / nseg;
  const unsigned x = 64u * xs + lane;
  if (y >= q.Y || x >= q.X) return;
  const size_t stride = (size_t)q.X * q.Y, base = (size_t)y * q.X + x;
  const LoadU32 ld{in + base, stride};
  const unsigned i1 = (seg + 1u) * SEG_DIRECT < q.Z ? (seg + 1u) * SEG_DIRECT : q.Z;
  for (unsigned i = seg * SEG_DIRECT; i < i1; ++i) out[base + (size_t)i * stride] = clear_cap(clear_window_min(ld, i, q.Z, q.w, q.R, q.flags), q.max_d2, CLEAR_FAR);
}

// the LDS form: a workgroup stages rows [s0 - R, s0 + SEG_LDS + R) of 64 x (those inside the axis) and makes SEG_LDS outputs from the tile
struct LoadTile {
  const unsigned* tile;  // row r of the axis at tile[(r - r0) * 64 + lane]
  unsigned r0, lane;
  __device__ __forceinline__ unsigned operator()(unsigned i) const { return tile[(i - r0) * 64u + lane]; }
};
__global__ __launch_bounds__(256) void k_lds(const unsigned* __restrict__ in, unsigned* __restrict__ out, Geom q) {
  extern __shared__ unsigned s_tile[];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned nxs = (q.X + 63u) >> 6, nseg = (q.Z + SEG_LDS - 1u) / SEG_LDS;
  const unsigned id = blockIdx.x;
  const unsigned xs = id % nxs, t = id / nxs, seg = t % nseg, y = t / nseg;  // (the grid is exactly nxs * nseg * Y blocks)
  const unsigned x = 64u * xs + lane;
  const bool col = x < q.X;
  const size_t stride = (size_t)q.X * q.Y, base = (size_t)y * q.X + x;
  const unsigned s0 = seg * SEG_LDS, s1 = s0 + SEG_LDS < q.Z ? s0 + SEG_LDS : q.Z;
  const unsigned r0 = s0 > q.R ? s0 - q.R : 0u, r1 = s1 + q.R < q.Z ? s1 + q.R : q.Z;  // (r1 - r0 <= SEG_LDS + 2 R rows: the launch's LDS)
  for (unsigned r = r0 + wave; r < r1; r += 4u) s_tile[(r - r0) * 64u + lane] = col ? in[base + (size_t)r * stride] : CLEAR_INF;
  __syncthreads();
  if (!col) return;
  // clear_window_min never asks for a row outside [max(i - R, 0), min(i + R, Z - 1)], which lies in [r0, r1) for s0 <= i < s1
  const LoadTile ld{s_tile, r0, lane};
  for (unsigned i = s0 + wave; i < s1; i += 4u) out[base + (size_t)i * stride] = clear_cap(clear_window_min(ld, i, q.Z, q.w, q.R, q.flags), q.max_d2, CLEAR_FAR);
}

int main() {
  const unsigned N = 512u;
  Geom q{N, N, N, 1u, 0u, 7282u, CLEAR_FLAG_UNKNOWN};
  q.R = clear_reach(q.max_d2, q.w);
  const size_t n = (size_t)N * N * N, lds = (size_t)(SEG_LDS + 2u * q.R) * 256u;
  if (q.R > CLEAR_MAX_REACH || lds > 65536u) {
    fprintf(stderr, "the tile does not fit: R %u, %zu bytes\n", q.R, lds);
    return 1;
  }
  unsigned *in = nullptr, *a = nullptr, *b = nullptr;
  CHECK(hipMalloc(&in, n * 4));
  CHECK(hipMalloc(&a, n * 4));
  CHECK(hipMalloc(&b, n * 4));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const unsigned nxs = (N + 63u) >> 6;
  const unsigned grid_d = (nxs * ((N + SEG_DIRECT - 1u) / SEG_DIRECT) * N + 3u) / 4u, grid_l = nxs * ((N + SEG_LDS - 1u) / SEG_LDS) * N;
  printf("512^3, z pass, w 1, max_d2 %u, R %u, LDS tile %zu B, direct %u blocks, lds %u blocks\n", q.max_d2, q.R, lds, grid_d, grid_l);
  std::vector<unsigned> ha(1u << 20), hb(1u << 20);
  const unsigned densities[3] = {200000u, 1000u, 10u};  // obstacles per million voxels
  for (int flags = 1; flags >= 0; --flags) {
    q.flags = (unsigned)flags;
    for (int d = 0; d < 3; ++d) {
      hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, in, n, densities[d]);
      CHECK(hipGetLastError());
      float ms_d[6], ms_l[6];
      for (int rep = 0; rep < 6; ++rep) {
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_direct, dim3(grid_d), dim3(256), 0, 0, (const unsigned*)in, a, q);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventElapsedTime(&ms_d[rep], e0, e1));
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_lds, dim3(grid_l), dim3(256), lds, 0, (const unsigned*)in, b, q);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipGetLastError());
        CHECK(hipEventElapsedTime(&ms_l[rep], e0, e1));
      }
      // the two forms agree: a 4 MiB piece from the start, the middle and the end
      size_t differ = 0, far = 0;
      const size_t at[3] = {0, n / 2, n - ha.size()};
      for (int p = 0; p < 3; ++p) {
        CHECK(hipMemcpy(ha.data(), a + at[p], ha.size() * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(hb.data(), b + at[p], hb.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ha.size(); ++i) {
          differ += ha[i] != hb[i];
          far += ha[i] == CLEAR_FAR;
        }
      }
      float best_d = ms_d[1], best_l = ms_l[1];
      for (int rep = 2; rep < 6; ++rep) {
        best_d = ms_d[rep] < best_d ? ms_d[rep] : best_d;
        best_l = ms_l[rep] < best_l ? ms_l[rep] : best_l;
      }
      printf("flags %d, %6u obstacles per million: direct %.3f ms (first %.3f), lds %.3f ms (first %.3f); %zu of 3 Mi values differ, %zu FAR\n", flags, densities[d],
             best_d, ms_d[0], best_l, ms_l[0], differ, far);
      if (differ) return 2;
    }
  }
  CHECK(hipFree(in));
  CHECK(hipFree(a));
  CHECK(hipFree(b));
  return 0;
}
