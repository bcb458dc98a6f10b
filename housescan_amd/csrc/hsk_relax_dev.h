// hsk_relax_dev.h -- the device side of hsk_reach_point.h's tile relaxation, shared by reach.hip (k_reach_round, 32-bit costs) and
// partition.hip (k_part_round, 64-bit keys): the marking of a tile for a worklist, a tile in LDS as the shared text takes it, and
// the body of a round's workgroup.  What differs between the two fields arrives as template arguments: the value policy
// (ReachValue, PartValue), the geometry block and the global load and store.  DESIGN.md 3.19 describes the round.  At the end, what
// the two files' launchers share on the host: the sweeps' grid, the tile grid of a geometry block, the carving of the scratch.
#pragma once
#include <algorithm>

#include "hsk_dev.h"
#include "hsk_reach_point.h"

// marks a tile for the list `list` (its length in *count): the flag counts the marks of a round, and whoever finds it 0 appends the
// tile, so the list holds it once and its length never exceeds the number of tiles (a round adds at most 26 marks a tile and the
// seeds at most 4096: the count cannot wrap before the tile's relaxation clears it)
static __device__ __forceinline__ void hsk_relax_mark(unsigned tile, unsigned* __restrict__ flags, unsigned* __restrict__ list,
                                                      unsigned long long* __restrict__ count) {
  if (atomicAdd(&flags[tile], 1u) == 0u) list[atomicAdd(count, 1ull)] = tile;
}

// marks the tile at offset m (indexed as the moves) from tile (tx, ty, tz), where the grid of q.ntx q.nty q.ntz tiles has one
template <class Geom>
static __device__ __forceinline__ void hsk_relax_mark_around(const Geom& q, unsigned tx, unsigned ty, unsigned tz, int m, unsigned* flags, unsigned* list,
                                                             unsigned long long* count) {
  const int nx = (int)tx + reach_dx(m), ny = (int)ty + reach_dy(m), nz = (int)tz + reach_dz(m);
  if (nx >= 0 && nx < (int)q.ntx && ny >= 0 && ny < (int)q.nty && nz >= 0 && nz < (int)q.ntz)
    hsk_relax_mark(((unsigned)nz * q.nty + (unsigned)ny) * q.ntx + (unsigned)nx, flags, list, count);
}

// A tile in LDS, as the shared text takes it.  A 32-bit cell is read and written by a plain access.  A 64-bit cell is read and
// written WHOLE, by one relaxed atomic at workgroup scope: a torn key (new G, old L) can lie below the fixpoint, and then the result
// is wrong, not merely late (hsk_part_point.h).
template <class T>
struct RelaxTile {
  T* cells;
  unsigned* mv;
  __device__ __forceinline__ T at(int x, int y, int z) const {
    if constexpr (sizeof(T) == 8) return __hip_atomic_load(cells + reach_halo_index(x, y, z), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return cells[reach_halo_index(x, y, z)];
  }
  __device__ __forceinline__ void set(int x, int y, int z, T v) const {
    if constexpr (sizeof(T) == 8) __hip_atomic_store(cells + reach_halo_index(x, y, z), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else cells[reach_halo_index(x, y, z)] = v;
  }
  __device__ __forceinline__ unsigned moves(unsigned i) const { return mv[i]; }
  __device__ __forceinline__ void set_moves(unsigned i, unsigned v) const { mv[i] = v; }
};

// One workgroup of a round (grid: the tiles of list_cur, 256 threads each): it takes its tile of the current worklist, loads it with
// a one-voxel halo into LDS, relaxes the interior to a local fixpoint (the halo is read only), stores what fell, and puts the
// neighbouring tiles that can see a fallen voxel -- up to 26 -- onto the next worklist.  A halo value another workgroup lowers
// meanwhile is read as the old or the new one: both are upper bounds, and whoever lowered it has marked this tile for the next
// round.  s_cells: REACH_HALO_CELLS cells, s_moves: REACH_TILE_VOXELS words, s_seen: REACH_MOVES words, all in LDS.
template <class V, class Geom, class Load, class Store>
static __device__ __forceinline__ void hsk_relax_round(typename V::T* s_cells, unsigned* s_moves, unsigned* s_seen, const Load& ld, const Store& st,
                                                       const Geom& q, const unsigned* list_cur, unsigned* flags_cur, unsigned* flags_next,
                                                       unsigned* list_next, unsigned long long* count_next) {
  const unsigned tid = threadIdx.x;
  const unsigned tile = list_cur[blockIdx.x];
  const unsigned tx = tile % q.ntx, ty = (tile / q.ntx) % q.nty, tz = tile / (q.ntx * q.nty);
  const unsigned ox = tx * REACH_TILE_X, oy = ty * REACH_TILE_Y, oz = tz * REACH_TILE_Z;
  if (tid == 0u) flags_cur[tile] = 0u;  // (this round reads this set and clears it; marks go to the other)
  if (tid < (unsigned)REACH_MOVES) s_seen[tid] = 0u;  // per tile offset: a voxel that tile can see fell (plain stores of 1)
  RelaxTile<typename V::T> s{s_cells, s_moves};
  reach_tile_load<V>(s, ld, ox, oy, oz, q.X, q.Y, q.Z, tid, 256u);
  __syncthreads();
  reach_tile_moves<V>(s, tid, 256u);
  __syncthreads();
  // The local fixpoint, Bellman-Ford in place: after sweep k every voxel holds at most the length of its best chain of at most k
  // moves inside the tile from the halo or the values loaded, and such a chain visits no voxel twice (the costs are positive), so
  // at most REACH_TILE_VOXELS sweeps change anything.  The loop ends at the first sweep in which no thread lowered a value -- every
  // read of that sweep then saw the cells as they stay -- and after REACH_TILE_VOXELS sweeps in any case.
#pragma unroll 1
  for (unsigned sweep = 0u; sweep < (unsigned)REACH_TILE_VOXELS; ++sweep) {
    const bool fell = reach_tile_sweep<V>(s, tid, 256u, q.cost, q.max_cost);
    if (!__syncthreads_or(fell ? 1 : 0)) break;  // (block-uniform)
  }
  const unsigned seen_by = reach_tile_store<V>(s, ld, st, ox, oy, oz, q.X, q.Y, q.Z, tid, 256u);
  if (seen_by) {  // (rare: a thread whose voxels fell; several threads may store the same 1)
    for (int m = 0; m < REACH_MOVES; ++m)  // (27 trips)
      if ((seen_by >> m) & 1u) s_seen[m] = 1u;
  }
  __syncthreads();
  if (tid < (unsigned)REACH_MOVES && tid != (unsigned)REACH_CENTRE && s_seen[tid]) hsk_relax_mark_around(q, tx, ty, tz, (int)tid, flags_next, list_next, count_next);
}

// ---- what the two files' launchers share (host) -------------------------------------------------------------------------------
// the grid of a sweep over the field: a block a 256 voxels, at most 4096 blocks (16 a CU), the rest by the kernel's grid-stride loop
static inline unsigned hsk_sweep_blocks(unsigned long long n) { return (unsigned)std::min<unsigned long long>((n + 255u) / 256u, 4096ull); }

// the grid, its tiles and the 27 move costs into a geometry block (ReachGeom, PartGeom)
template <class Geom>
static inline void hsk_relax_geom(unsigned X, unsigned Y, unsigned Z, const unsigned w[3], Geom* q) {
  q->X = X, q->Y = Y, q->Z = Z;
  q->ntx = (X + REACH_TILE_X - 1u) / REACH_TILE_X;
  q->nty = (Y + REACH_TILE_Y - 1u) / REACH_TILE_Y;
  q->ntz = (Z + REACH_TILE_Z - 1u) / REACH_TILE_Z;
  reach_cost_table(w, q->cost);
}

// one device buffer carved into arrays, each 256-byte aligned: take() -> the next array (null while only the size is asked for)
struct RelaxCarve {
  void* base;
  size_t bytes = 0;
  char* take(size_t k) {
    char* p = base ? (char*)base + bytes : nullptr;
    bytes += (k + 255) & ~(size_t)255;
    return p;
  }
  // per tile two flag words and two worklist words
  void worklists(size_t tiles, unsigned* flags[2], unsigned* list[2]) {
    for (int i = 0; i < 2; ++i) flags[i] = (unsigned*)take(tiles * 4);
    for (int i = 0; i < 2; ++i) list[i] = (unsigned*)take(tiles * 4);
  }
};
