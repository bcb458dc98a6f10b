// reach.hip -- the reach field for gfx950 (hsk_build_reach, hsk_reach_floor, hsk_reach_path; DESIGN.md 3.19 the kernels, 8m the
// rule; tests/reach_twin.py restates the rule in numpy): for every voxel the length of the shortest chain of allowed moves from a
// seed, as a label-correcting relaxation over tiles held in LDS with a compacted worklist of active tiles.  Every value is an
// integer and the field the least fixpoint of a monotone relaxation: no schedule can change a bit.  No workgroup, wave or lane
// waits for another; every loop is bounded and says by what.
//
// k_reach_init: one sweep over the clearance field writes BLOCKED / UNREACHED and counts the passable voxels.
// k_reach_seed: a thread a seed voxel: 0 into a passable one, its tile onto the first worklist.
// k_reach_round (its body is hsk_relax_dev.h's hsk_relax_round, which k_part_round runs on 64-bit keys): a workgroup takes one
// tile of the current worklist, loads it with a one-voxel halo into LDS, relaxes the interior
// to a local fixpoint (the halo is read only), stores what fell, and puts the neighbouring tiles that can see a fallen voxel -- up
// to 26 -- onto the next worklist.  A tile is appended by whoever sets its flag first, so a list holds a tile once and a round's
// work is the active tiles' alone.  A halo value another workgroup lowers meanwhile is read as the old or the new one: both are
// upper bounds, and whoever lowered it has marked this tile for the next round.
// k_reach_stats, k_reach_path: the counts of the finished field; one wave walks a path back from a goal.
#pragma clang fp contract(off)
#include <algorithm>

#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_relax_dev.h"

static_assert(REACH_TILE_X * REACH_TILE_Y == 256, "k_reach_round: a thread per (x, y) of the tile");

// grid-stride: a thread sums its voxels, a wave adds once -- at 512^3 a wave a 64 voxels was two million atomics on one word
__global__ __launch_bounds__(256) void k_reach_init(const unsigned* __restrict__ d2, unsigned* __restrict__ g, unsigned long long n, unsigned min_d2,
                                                    unsigned long long* __restrict__ counters) {
  const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
  unsigned pass = 0u;
  for (unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x; e < n; e += stride) {  // (ends: e grows by the grid)
    const bool p = reach_passable(d2[e], min_d2);
    g[e] = p ? REACH_UNREACHED : REACH_BLOCKED;
    pass += p ? 1u : 0u;
  }
  pass = hsk_wave_sum(pass);  // (every lane of the wave arrives here; a thread takes at most n / stride + 1 < 2^32 voxels)
  if ((threadIdx.x & 63u) == 0u && pass) atomicAdd(&counters[0], (unsigned long long)pass);
}

__global__ __launch_bounds__(256) void k_reach_seed(unsigned* __restrict__ g, ReachGeom q, const unsigned* __restrict__ seeds, unsigned n_seeds,
                                                    unsigned* __restrict__ flags, unsigned* __restrict__ list, unsigned long long* __restrict__ counters,
                                                    unsigned long long* __restrict__ count) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n_seeds) return;
  const unsigned v = seeds[e];  // (a voxel of the grid: the host mapped the point and dropped what fell outside)
  if (g[v] == REACH_BLOCKED) return;  // (a duplicate finds 0 or UNREACHED here: it is counted as well)
  g[v] = 0u;
  atomicAdd(&counters[3], 1ull);
  // Placing a seed lowers a value like a tile's store does: every tile that holds the voxel in its cells or halo is marked, the
  // seed's own and up to 7 neighbours.  (Its own tile alone would not do: the seed does not fall in that tile's relaxation, so a
  // seed on a tile face whose in-tile neighbours do not fall on that face would never reach the tile across it.)
  const unsigned x = v % q.X, y = (v / q.X) % q.Y, z = v / (q.X * q.Y);
  const unsigned tx = x / REACH_TILE_X, ty = y / REACH_TILE_Y, tz = z / REACH_TILE_Z;
  const unsigned seen_by = reach_seen_by((int)(x % REACH_TILE_X), (int)(y % REACH_TILE_Y), (int)(z % REACH_TILE_Z));
  for (int m = 0; m < REACH_MOVES; ++m)  // (27 trips; the centre bit is the seed's own tile)
    if ((seen_by >> m) & 1u) hsk_relax_mark_around(q, tx, ty, tz, m, flags, list, count);
}

// the field's global accesses are plain: a 32-bit word is never torn
struct ReachLoad {
  const unsigned* p;
  __device__ __forceinline__ unsigned operator()(size_t i) const { return p[i]; }
};
struct ReachStore {
  unsigned* p;
  __device__ __forceinline__ void operator()(size_t i, unsigned v) const { p[i] = v; }
};

// grid: the tiles of list_cur, a workgroup each (hsk_relax_dev.h: hsk_relax_round)
__global__ __launch_bounds__(256) void k_reach_round(unsigned* g, ReachGeom q, const unsigned* __restrict__ list_cur, unsigned* __restrict__ flags_cur,
                                                     unsigned* __restrict__ flags_next, unsigned* __restrict__ list_next,
                                                     unsigned long long* __restrict__ count_next) {
  __shared__ unsigned s_cells[REACH_HALO_CELLS];
  __shared__ unsigned s_moves[REACH_TILE_VOXELS];
  __shared__ unsigned s_seen[REACH_MOVES];
  hsk_relax_round<ReachValue>(s_cells, s_moves, s_seen, ReachLoad{g}, ReachStore{g}, q, list_cur, flags_cur, flags_next, list_next, count_next);
}

__global__ __launch_bounds__(256) void k_reach_stats(const unsigned* __restrict__ g, unsigned long long n, unsigned long long* __restrict__ counters) {
  const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
  unsigned reached = 0u, top = 0u;
  for (unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x; e < n; e += stride) {  // (ends: e grows by the grid)
    const unsigned v = g[e];
    if (reach_is_value(v)) {
      reached += 1u;
      top = v > top ? v : top;
    }
  }
  reached = hsk_wave_sum(reached);
  top = hsk_wave_max(top);
  if ((threadIdx.x & 63u) == 0u && reached) {
    atomicAdd(&counters[1], (unsigned long long)reached);
    atomicMin(&counters[2], (unsigned long long)(~top));  // (the largest value as the least complement; the word starts as all ones)
  }
}

// One wave, one workgroup.  From the goal voxel back to a seed: lane m tests move m, a ballot picks the smallest.  out: the voxels
// from the goal on, x y z each, the first `cap` of them; result[0]: the path's length (0: the goal holds no value), result[1]: 1
// when a voxel of the walk had no such move (never at a fixpoint).  Bounded: the value falls by a cost >= 1 per step, and the loop
// takes at most `limit` (the grid's voxels) steps in any case.
__global__ __launch_bounds__(64) void k_reach_path(const unsigned* __restrict__ g, ReachGeom q, unsigned goal, unsigned long long cap,
                                                   unsigned long long limit, int* __restrict__ out, unsigned long long* __restrict__ result) {
  const int lane = (int)threadIdx.x;
  unsigned x = goal % q.X, y = (goal / q.X) % q.Y, z = goal / (q.X * q.Y);
  unsigned gv = g[goal];
  unsigned long long n = 0ull, broken = 0ull;
  if (reach_is_value(gv)) {
    const ReachLoad ld{g};
    unsigned cost_m = 0u;  // this lane's move's cost (constant indices: the table stays in the kernel's arguments)
#pragma unroll
    for (int m = 0; m < REACH_MOVES; ++m) cost_m = lane == m ? q.cost[m] : cost_m;
#pragma unroll 1
    for (unsigned long long step = 0ull; step < limit; ++step) {
      if (lane == 0 && n < cap) {
        out[3ull * n] = (int)x;
        out[3ull * n + 1ull] = (int)y;
        out[3ull * n + 2ull] = (int)z;
      }
      n += 1ull;
      if (gv == 0u) break;
      const bool ok = reach_trace_ok(ld, q.X, q.Y, q.Z, x, y, z, lane, cost_m, gv);  // (false for the centre and the lanes past 26)
      const unsigned long long votes = __ballot(ok);
      if (!votes) {
        broken = 1ull;
        break;
      }
      const int m = __ffsll((long long)votes) - 1;  // (wave-uniform)
      x = (unsigned)((int)x + reach_dx(m));
      y = (unsigned)((int)y + reach_dy(m));
      z = (unsigned)((int)z + reach_dz(m));
      gv -= (unsigned)__shfl((int)cost_m, m, 64);
    }
  }
  if (lane == 0) {
    result[0] = n;
    result[1] = broken;
  }
}

// ---- the launchers ------------------------------------------------------------------------------------------------------------
void reach_geom(unsigned X, unsigned Y, unsigned Z, const unsigned w[3], unsigned min_d2, unsigned max_cost, ReachGeom* q) {
  hsk_relax_geom(X, Y, Z, w, q);
  q->min_d2 = min_d2;
  q->max_cost = max_cost;
}

size_t reach_layout(const ReachGeom& q, void* base, ReachBufs* b) {
  RelaxCarve c{base};
  ReachBufs out;
  out.counters = (unsigned long long*)c.take(64);
  out.field = (unsigned*)c.take((size_t)q.X * q.Y * q.Z * 4);
  c.worklists((size_t)q.ntx * q.nty * q.ntz, out.flags, out.list);
  if (b) *b = out;
  return c.bytes;
}

hipError_t launch_reach_init(hipStream_t s, const unsigned* d2, const ReachGeom& q, const ReachBufs& b) {
  const unsigned long long n = (unsigned long long)q.X * q.Y * q.Z, tiles = (unsigned long long)q.ntx * q.nty * q.ntz;
  hipError_t e = hipMemsetAsync(b.counters, 0, 64, s);
  if (e == hipSuccess) e = hipMemsetAsync(b.counters + 2, 0xff, 8, s);  // (k_reach_stats keeps the largest value as the least complement)
  if (e == hipSuccess) e = hipMemsetAsync(b.flags[0], 0, tiles * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(b.flags[1], 0, tiles * 4, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_reach_init, dim3(hsk_sweep_blocks(n)), dim3(256), 0, s, d2, b.field, n, q.min_d2, b.counters);
  return hipGetLastError();
}

void launch_reach_seed(hipStream_t s, const ReachGeom& q, const ReachBufs& b, const unsigned* seeds, unsigned n_seeds) {
  hipLaunchKernelGGL(k_reach_seed, dim3((n_seeds + 255u) / 256u), dim3(256), 0, s, b.field, q, seeds, n_seeds, b.flags[0], b.list[0], b.counters,
                     b.counters + 4);
}

hipError_t launch_reach_round(hipStream_t s, const ReachGeom& q, const ReachBufs& b, int cur, unsigned n_active) {
  const int next = cur ^ 1;
  const hipError_t e = hipMemsetAsync(b.counters + 4 + next, 0, 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_reach_round, dim3(n_active), dim3(256), 0, s, b.field, q, (const unsigned*)b.list[cur], b.flags[cur], b.flags[next], b.list[next],
                     b.counters + 4 + next);
  return hipGetLastError();
}

void launch_reach_stats(hipStream_t s, const ReachGeom& q, const ReachBufs& b) {
  const unsigned long long n = (unsigned long long)q.X * q.Y * q.Z;
  hipLaunchKernelGGL(k_reach_stats, dim3(hsk_sweep_blocks(n)), dim3(256), 0, s, (const unsigned*)b.field, n, b.counters);
}

void launch_reach_path(hipStream_t s, const unsigned* field, const ReachGeom& q, unsigned goal, unsigned long long cap, int* out,
                       unsigned long long* result) {
  hipLaunchKernelGGL(k_reach_path, dim3(1), dim3(64), 0, s, field, q, goal, cap, (unsigned long long)q.X * q.Y * q.Z, out, result);
}
