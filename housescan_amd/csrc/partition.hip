// partition.hip -- the room partition for gfx950 (hsk_build_partition, hsk_partition_floor, hsk_partition_at; DESIGN.md 3.20 the
// kernels, 8n the rule; tests/partition_twin.py restates the rule in numpy): the free space is split into rooms by spreading the
// labels of its wide places -- the CORES, the 6-connected components of the voxels whose clearance is at least core_d2 -- through
// everything passable, each voxel going to the core that is nearest along the reach field's moves.  Every value is an integer,
// the labelling a union-find whose entries only ever fall and the field the least fixpoint of a monotone relaxation on 64-bit
// keys: no schedule can change a bit.  No workgroup, wave or lane waits for another; every loop is bounded and says by what.
//
// k_part_label_tile: a workgroup labels the core voxels of one 32 x 8 x 8 tile in LDS and writes every voxel's parent: the smallest
// lin of its piece of the core inside the tile.  k_part_label_faces: the core voxels on a tile's lower faces are united with their
// neighbours across them by atomic minima in global memory.  k_part_flatten_count: parent = root, and the root's slot of the key
// array -- idle until the init -- counts the core's voxels.  k_part_roots: the cores are counted and those of min_core voxels kept.
// k_part_init: (0, label), UNASSIGNED or BLOCKED per voxel; the tiles that hold an UNASSIGNED voxel make the first worklist.
// k_part_round: the reach field's tile relaxation (hsk_relax_dev.h: hsk_relax_round, k_reach_round's body too) on 64-bit keys.
// k_part_records, k_part_doors: one sweep each, integer atomics only.  k_part_box, k_part_gather: the reads.
#pragma clang fp contract(off)
#include <algorithm>

#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_clear_point.h"
#include "hsk_part_point.h"
#include "hsk_relax_dev.h"

static_assert(REACH_TILE_X * REACH_TILE_Y == 256, "the tile kernels: a thread per (x, y) of the tile");
static_assert(REACH_TILE_X == 32 && REACH_TILE_Y == 8 && REACH_TILE_Z == 8, "k_part_label_faces tests a voxel's place in its tile with these");
static_assert(PART_MAX_ROOMS == 1024 && PART_REC_WORDS == 16 && PART_DOOR_WORDS == 8, "the tables in LDS and the sums' layout");
static_assert(32 * PART_DOOR_WORDS == 256, "k_part_doors clears its slots a thread a word");

// ---- the core labelling -------------------------------------------------------------------------------------------------------
// grid: the tiles.  Thread (x, y) of the tile takes its 8 voxels along z.  The local label of a voxel is its index in the tile,
// (z 8 + y) 32 + x, whose order is lin's: the smallest local label of a piece is its smallest lin.
__global__ __launch_bounds__(256) void k_part_label_tile(const unsigned* __restrict__ d2, unsigned* __restrict__ parent,
                                                         unsigned long long* __restrict__ keys, PartGeom q) {
  __shared__ unsigned s_par[REACH_TILE_VOXELS];
  const unsigned tid = threadIdx.x, lx = tid % REACH_TILE_X, ly = tid / REACH_TILE_X;
  const unsigned tile = blockIdx.x;
  const unsigned tx = tile % q.ntx, ty = (tile / q.ntx) % q.nty, tz = tile / (q.ntx * q.nty);
  const unsigned gx = tx * REACH_TILE_X + lx, gy = ty * REACH_TILE_Y + ly, oz = tz * REACH_TILE_Z;
  const bool in_xy = gx < q.X && gy < q.Y;
#pragma unroll
  for (unsigned z = 0u; z < (unsigned)REACH_TILE_Z; ++z) {  // (8 trips)
    const unsigned i = z * 256u + tid;
    const bool in = in_xy && oz + z < q.Z;
    const bool core = in && part_core(d2[((size_t)(oz + z) * q.Y + gy) * q.X + gx], q.core_d2);
    s_par[i] = core ? i : COMP_NONE;
  }
  __syncthreads();
  const CompDirect map;
  // (whether an entry is COMP_NONE never changes; comp_unite ends by hsk_comp_point.h's invariant: an entry only ever falls)
#pragma unroll 1
  for (unsigned z = 0u; z < (unsigned)REACH_TILE_Z; ++z) {  // (8 trips)
    const unsigned i = z * 256u + tid;
    if (CompLdsOps::load(s_par + i) == COMP_NONE) continue;
    if (lx > 0u && CompLdsOps::load(s_par + i - 1u) != COMP_NONE) comp_unite<CompLdsOps>(s_par, map, i, i - 1u);
    if (ly > 0u && CompLdsOps::load(s_par + i - REACH_TILE_X) != COMP_NONE) comp_unite<CompLdsOps>(s_par, map, i, i - REACH_TILE_X);
    if (z > 0u && CompLdsOps::load(s_par + i - 256u) != COMP_NONE) comp_unite<CompLdsOps>(s_par, map, i, i - 256u);
  }
  __syncthreads();
#pragma unroll 1
  for (unsigned z = 0u; z < (unsigned)REACH_TILE_Z; ++z) {  // (8 trips; nothing lowers an entry any more)
    const unsigned i = z * 256u + tid;
    if (!(in_xy && oz + z < q.Z)) continue;
    const size_t at = ((size_t)(oz + z) * q.Y + gy) * q.X + gx;
    if (s_par[i] == COMP_NONE) {
      parent[at] = COMP_NONE;
      continue;
    }
    const unsigned r = comp_find<CompLdsOps>(s_par, map, i);
    const unsigned rx = r % REACH_TILE_X, ry = (r / REACH_TILE_X) % REACH_TILE_Y, rz = r / 256u;
    parent[at] = ((oz + rz) * q.Y + (ty * REACH_TILE_Y + ry)) * q.X + (tx * REACH_TILE_X + rx);
    if (r == i) keys[at] = 0ull;  // (the slot that counts the core's voxels, should this voxel stay a root)
  }
}

// a thread a voxel: a core voxel at local 0 of its tile on an axis is united with the core voxel below it on that axis, across the
// tile's face.  Every walk is strictly decreasing (hsk_comp_point.h).
__global__ __launch_bounds__(256) void k_part_label_faces(unsigned* parent, PartGeom q, unsigned n) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  const unsigned row = e / q.X, x = e - row * q.X, z = row / q.Y, y = row - z * q.Y;
  const bool fx = x > 0u && (x % REACH_TILE_X) == 0u, fy = y > 0u && (y % REACH_TILE_Y) == 0u, fz = z > 0u && (z % REACH_TILE_Z) == 0u;
  if (!(fx || fy || fz)) return;
  if (CompGlobalOps::load(parent + e) == COMP_NONE) return;
  const CompDirect map;
  if (fx && CompGlobalOps::load(parent + e - 1u) != COMP_NONE) comp_unite<CompGlobalOps>(parent, map, e, e - 1u);
  if (fy && CompGlobalOps::load(parent + e - q.X) != COMP_NONE) comp_unite<CompGlobalOps>(parent, map, e, e - q.X);
  if (fz && CompGlobalOps::load(parent + e - q.X * q.Y) != COMP_NONE) comp_unite<CompGlobalOps>(parent, map, e, e - q.X * q.Y);
}

// a thread a voxel: parent = root (an entry only falls, so a walk through it meanwhile stays a walk to the same root), and the
// root's slot counts.  A wave whose core voxels all have one root adds once.
__global__ __launch_bounds__(256) void k_part_flatten_count(unsigned* parent, unsigned long long* __restrict__ keys, unsigned n) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  const bool member = e < n && CompGlobalOps::load(parent + e) != COMP_NONE;
  unsigned r = COMP_NONE;
  if (member) {
    r = comp_find<CompGlobalOps>(parent, CompDirect(), e);
    __hip_atomic_store(parent + e, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const unsigned long long mask = __ballot(member);  // (every lane of the wave arrives here)
  if (!mask) return;
  const int first = __ffsll((long long)mask) - 1;
  const unsigned r0 = (unsigned)__shfl((int)r, first, 64);
  if (__all(!member || r == r0)) {
    if ((int)(threadIdx.x & 63u) == first) atomicAdd(&keys[r0], (unsigned long long)__popcll(mask));
  } else if (member) {
    atomicAdd(&keys[r], 1ull);
  }
}

// a thread a voxel: a root is a core; one of at least min_core voxels is kept -- the first PART_MAX_ROOMS of them are written, all
// are counted
__global__ __launch_bounds__(256) void k_part_roots(const unsigned* __restrict__ parent, const unsigned long long* __restrict__ keys, unsigned n,
                                                    unsigned min_core, unsigned* __restrict__ roots_found, unsigned long long* __restrict__ counters) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  const bool root = e < n && parent[e] == e;
  const unsigned long long roots = __ballot(root);  // (every lane of the wave arrives here)
  if ((threadIdx.x & 63u) == 0u && roots) atomicAdd(&counters[1], (unsigned long long)__popcll(roots));
  if (root && keys[e] >= (unsigned long long)min_core) {
    const unsigned long long at = atomicAdd(&counters[2], 1ull);
    if (at < (unsigned long long)PART_MAX_ROOMS) roots_found[at] = e;
  }
}

// the ascending roots (and the ranks) into LDS; the caller synchronises
static __device__ __forceinline__ void part_load_table(unsigned* s_tab, const unsigned* __restrict__ tab, unsigned n_kept) {
  for (unsigned i = threadIdx.x; i < n_kept; i += 256u) s_tab[i] = tab[i];  // (ends: i grows by 256; n_kept <= 1024)
}

// grid: the tiles, as k_part_label_tile
__global__ __launch_bounds__(256) void k_part_init(const unsigned* __restrict__ d2, const unsigned* __restrict__ parent, unsigned long long* __restrict__ keys,
                                                   PartGeom q, const unsigned* __restrict__ roots, unsigned n_kept, unsigned* __restrict__ flags,
                                                   unsigned* __restrict__ list, unsigned long long* __restrict__ counters) {
  __shared__ unsigned s_roots[PART_MAX_ROOMS];
  const unsigned tid = threadIdx.x, lx = tid % REACH_TILE_X, ly = tid / REACH_TILE_X;
  const unsigned tile = blockIdx.x;
  const unsigned tx = tile % q.ntx, ty = (tile / q.ntx) % q.nty, tz = tile / (q.ntx * q.nty);
  const unsigned gx = tx * REACH_TILE_X + lx, gy = ty * REACH_TILE_Y + ly, oz = tz * REACH_TILE_Z;
  const bool in_xy = gx < q.X && gy < q.Y;
  part_load_table(s_roots, roots, n_kept);
  __syncthreads();
  unsigned pass = 0u;
  bool open = false;
#pragma unroll 1
  for (unsigned z = 0u; z < (unsigned)REACH_TILE_Z; ++z) {  // (8 trips)
    if (!(in_xy && oz + z < q.Z)) continue;
    const size_t at = ((size_t)(oz + z) * q.Y + gy) * q.X + gx;
    const unsigned label = parent[at];
    const bool p = reach_passable(d2[at], q.min_d2);
    const bool kept = label != COMP_NONE && comp_search(s_roots, n_kept, label) < n_kept;  // (a core voxel is passable: min_d2 <= core_d2)
    keys[at] = kept ? part_key_of(0u, label) : p ? PART_KEY_UNASSIGNED : PART_KEY_BLOCKED;
    pass += p ? 1u : 0u;
    open = open || (p && !kept);
  }
  pass = hsk_wave_sum(pass);  // (every lane of the wave arrives here)
  if ((tid & 63u) == 0u && pass) atomicAdd(&counters[0], (unsigned long long)pass);
  // only the tile that holds a voxel can lower it, and only an UNASSIGNED voxel can fall (a cost is positive, so nothing falls
  // below (0, label)): the tiles that hold one are all the first round can need
  if (__syncthreads_or(open ? 1 : 0) && tid == 0u) hsk_relax_mark(tile, flags, list, &counters[4]);  // (the flags start as zeros: a tile once)
}

// ---- the relaxation -----------------------------------------------------------------------------------------------------------
// EVERY global read and write of a key that another workgroup may touch is ONE 64-bit relaxed atomic at agent scope: a halo cell
// another tile's workgroup stores meanwhile is read as the old or the new key, never as half of each (in LDS likewise, at workgroup
// scope: hsk_relax_dev.h's RelaxTile)
struct PartLoad {
  const unsigned long long* p;
  __device__ __forceinline__ part_key operator()(size_t i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
struct PartStore {
  unsigned long long* p;
  __device__ __forceinline__ void operator()(size_t i, part_key v) const { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// grid: the tiles of list_cur, a workgroup each (hsk_relax_dev.h: hsk_relax_round).  LDS: 34 x 10 x 10 keys = 27.2 KB and 8 KB of moves.
__global__ __launch_bounds__(256) void k_part_round(unsigned long long* keys, PartGeom q, const unsigned* __restrict__ list_cur, unsigned* __restrict__ flags_cur,
                                                    unsigned* __restrict__ flags_next, unsigned* __restrict__ list_next,
                                                    unsigned long long* __restrict__ count_next) {
  __shared__ unsigned long long s_cells[REACH_HALO_CELLS];
  __shared__ unsigned s_moves[REACH_TILE_VOXELS];
  __shared__ unsigned s_seen[REACH_MOVES];
  hsk_relax_round<PartValue>(s_cells, s_moves, s_seen, PartLoad{keys}, PartStore{keys}, q, list_cur, flags_cur, flags_next, list_next, count_next);
}

// ---- records and doors ----------------------------------------------------------------------------------------------------------
// the index of a key's label among the ascending roots, n_kept when the key holds no room (bisection: comp_search)
static __device__ __forceinline__ unsigned part_index_of(part_key k, const unsigned* s_roots, unsigned n_kept) {
  return part_is_value(k) ? comp_search(s_roots, n_kept, part_label(k)) : n_kept;
}
// the room id a voxel reports
static __device__ __forceinline__ unsigned part_id_of(part_key k, const unsigned* s_roots, const unsigned* s_rank, unsigned n_kept) {
  if (!part_is_value(k)) return part_g(k) == REACH_BLOCKED ? PART_ROOM_BLOCKED : PART_ROOM_UNASSIGNED;
  const unsigned i = comp_search(s_roots, n_kept, part_label(k));
  return i < n_kept ? s_rank[i] : PART_ROOM_UNASSIGNED;  // (i == n_kept cannot be: every label in the field is a kept root)
}

// The two sweeps add into a few words per room (per pair of rooms): at 1024 x 512 x 512 four million waves adding into the words of
// six rooms took a second in global atomics.  A block therefore adds in LDS first: PART_SLOTS slots of sums, a slot claimed by
// the first room (pair) that hashes to it -- another room that meets it taken adds to global memory directly --, flushed with one
// set of global atomics when the block's grid-stride loop ends.  Integer sums and maxima: the bits do not depend on the route.
#define PART_SLOTS 32
#define PART_SLOT_FREE 0xffffffffu

// slot tag % PART_SLOTS when `tag` owns it (claimed here if free), else PART_SLOTS
static __device__ __forceinline__ unsigned part_slot(unsigned* s_tag, unsigned tag) {
  const unsigned slot = tag % PART_SLOTS;
  const unsigned old = atomicCAS(&s_tag[slot], PART_SLOT_FREE, tag);
  return (old == PART_SLOT_FREE || old == tag) ? slot : (unsigned)PART_SLOTS;
}

// one room's sums (PART_REC_WORDS words; LDS or global): words 0..4 are added, 5..12 are maxima
static __device__ __forceinline__ void part_rec_add(unsigned long long* r, unsigned long long n_vox, unsigned long long n_core, unsigned long long sx,
                                                    unsigned long long sy, unsigned long long sz, const unsigned top[8]) {
  atomicAdd(r + 0, n_vox);
  if (n_core) atomicAdd(r + 1, n_core);
  atomicAdd(r + 2, sx);
  atomicAdd(r + 3, sy);
  atomicAdd(r + 4, sz);
#pragma unroll
  for (int i = 0; i < 8; ++i) atomicMax(r + 5 + i, (unsigned long long)top[i]);
}

// Grid-stride, a block 256 consecutive voxels a trip.  recs[i], the room of roots[i]: PART_REC_WORDS sums, integer atomics only, so
// any order gives the same bits; the lower corner is kept as the largest complement, so that the table starts as zeros.  A wave
// whose voxels all belong to one room reduces first and adds once.
__global__ __launch_bounds__(256) void k_part_records(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ d2, PartGeom q,
                                                      unsigned long long n, const unsigned* __restrict__ roots, unsigned n_kept,
                                                      unsigned long long* __restrict__ recs) {
  __shared__ unsigned s_roots[PART_MAX_ROOMS];
  __shared__ unsigned s_tag[PART_SLOTS];
  __shared__ unsigned long long s_acc[PART_SLOTS * PART_REC_WORDS];
  part_load_table(s_roots, roots, n_kept);
  if (threadIdx.x < (unsigned)PART_SLOTS) s_tag[threadIdx.x] = PART_SLOT_FREE;
  for (unsigned i = threadIdx.x; i < (unsigned)(PART_SLOTS * PART_REC_WORDS); i += 256u) s_acc[i] = 0ull;  // (ends: i grows by 256)
  __syncthreads();
  const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
  const unsigned lane = threadIdx.x & 63u;
  for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < n; base += stride) {  // (ends: base grows by the grid; block-uniform)
    const unsigned long long e = base + threadIdx.x;
    const part_key k = e < n ? keys[e] : PART_KEY_BLOCKED;
    const unsigned idx = part_index_of(k, s_roots, n_kept);
    const bool has = idx < n_kept;
    const unsigned long long mask = __ballot(has);  // (every lane of the wave arrives here)
    if (!mask) continue;
    const unsigned row = (unsigned)(e / q.X), x = (unsigned)(e - (unsigned long long)row * q.X), z = row / q.Y, y = row - z * q.Y;
    const unsigned g = part_g(k), d = has ? d2[e] : 0u;
    const int first = __ffsll((long long)mask) - 1;
    const unsigned idx0 = (unsigned)__shfl((int)idx, first, 64);
    if (__all(!has || idx == idx0)) {
      const unsigned long long cores = __ballot(has && g == 0u);
      const unsigned long long sx = hsk_wave_sum<unsigned long long>(has ? x : 0u), sy = hsk_wave_sum<unsigned long long>(has ? y : 0u),
                               sz = hsk_wave_sum<unsigned long long>(has ? z : 0u);
      const unsigned top[8] = {hsk_wave_max(has ? ~x : 0u), hsk_wave_max(has ? ~y : 0u), hsk_wave_max(has ? ~z : 0u), hsk_wave_max(has ? x : 0u),
                               hsk_wave_max(has ? y : 0u),  hsk_wave_max(has ? z : 0u),  hsk_wave_max(d),             hsk_wave_max(has ? g : 0u)};
      if ((int)lane == first) {
        const unsigned slot = part_slot(s_tag, idx0);
        const unsigned long long n_vox = (unsigned long long)__popcll(mask), n_core = (unsigned long long)__popcll(cores);
        if (slot < (unsigned)PART_SLOTS) part_rec_add(s_acc + slot * PART_REC_WORDS, n_vox, n_core, sx, sy, sz, top);
        else part_rec_add(recs + (size_t)idx0 * PART_REC_WORDS, n_vox, n_core, sx, sy, sz, top);
      }
    } else if (has) {
      const unsigned top[8] = {~x, ~y, ~z, x, y, z, d, g};
      const unsigned slot = part_slot(s_tag, idx);
      if (slot < (unsigned)PART_SLOTS) part_rec_add(s_acc + slot * PART_REC_WORDS, 1ull, g == 0u ? 1ull : 0ull, x, y, z, top);
      else part_rec_add(recs + (size_t)idx * PART_REC_WORDS, 1ull, g == 0u ? 1ull : 0ull, x, y, z, top);
    }
  }
  __syncthreads();
  // the flush: a thread a word of a claimed slot (words 13..15 are not used)
  for (unsigned i = threadIdx.x; i < (unsigned)(PART_SLOTS * PART_REC_WORDS); i += 256u) {  // (ends: i grows by 256)
    const unsigned slot = i / PART_REC_WORDS, w = i % PART_REC_WORDS, tag = s_tag[slot];
    const unsigned long long v = s_acc[i];
    if (tag == PART_SLOT_FREE || w > 12u || v == 0ull) continue;  // (a zero adds nothing and is below every maximum)
    unsigned long long* r = recs + (size_t)tag * PART_REC_WORDS + w;
    if (w < 5u) atomicAdd(r, v);
    else atomicMax(r, v);
  }
}

// one pair's sums (PART_DOOR_WORDS words; LDS or global) take one face: the lower voxel (x, y, z), the axis crossed, min(D, D')
static __device__ __forceinline__ void part_door_add(unsigned long long* t, unsigned x, unsigned y, unsigned z, int a, unsigned width) {
  unsigned* t32 = (unsigned*)(t + 3);
  atomicAdd(t + 0, (unsigned long long)(2u * x + (a == 0 ? 1u : 0u)));
  atomicAdd(t + 1, (unsigned long long)(2u * y + (a == 1 ? 1u : 0u)));
  atomicAdd(t + 2, (unsigned long long)(2u * z + (a == 2 ? 1u : 0u)));
  atomicAdd(t32 + a, 1u);
  atomicMax(t32 + 3, ~x);
  atomicMax(t32 + 4, ~y);
  atomicMax(t32 + 5, ~z);
  atomicMax(t32 + 6, x);
  atomicMax(t32 + 7, y);
  atomicMax(t32 + 8, z);
  atomicMax(t32 + 9, width);
}

// Grid-stride as k_part_records.  A voxel looks at its three upper neighbours; a FACE is a pair that holds two different rooms.
// table[a n_kept + b], a < b the room ids: PART_DOOR_WORDS words, integer atomics only.  A wave without a face leaves by a ballot.
__global__ __launch_bounds__(256) void k_part_doors(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ d2, PartGeom q,
                                                    unsigned long long n, const unsigned* __restrict__ roots, const unsigned* __restrict__ rank,
                                                    unsigned n_kept, unsigned long long* __restrict__ table) {
  __shared__ unsigned s_roots[PART_MAX_ROOMS];
  __shared__ unsigned s_rank[PART_MAX_ROOMS];
  __shared__ unsigned s_tag[PART_SLOTS];
  __shared__ unsigned long long s_acc[PART_SLOTS * PART_DOOR_WORDS];
  part_load_table(s_roots, roots, n_kept);
  part_load_table(s_rank, rank, n_kept);
  if (threadIdx.x < (unsigned)PART_SLOTS) s_tag[threadIdx.x] = PART_SLOT_FREE;
  s_acc[threadIdx.x] = 0ull;  // (PART_SLOTS * PART_DOOR_WORDS == 256)
  __syncthreads();
  const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
  const unsigned long long step[3] = {1ull, (unsigned long long)q.X, (unsigned long long)q.X * q.Y};
  for (unsigned long long base = (unsigned long long)blockIdx.x * 256u; base < n; base += stride) {  // (ends: base grows by the grid; block-uniform)
    const unsigned long long e = base + threadIdx.x;
    const part_key k = e < n ? keys[e] : PART_KEY_BLOCKED;
    const bool has = part_is_value(k);
    if (!__ballot(has)) continue;  // (every lane of the wave arrives here)
    const unsigned row = (unsigned)(e / q.X), x = (unsigned)(e - (unsigned long long)row * q.X), z = row / q.Y, y = row - z * q.Y;
    const unsigned at[3] = {x, y, z}, dims[3] = {q.X, q.Y, q.Z};
    unsigned other[3] = {PART_ROOM_NONE, PART_ROOM_NONE, PART_ROOM_NONE};
    unsigned own = PART_ROOM_NONE;
    bool face = false;
    if (has) {
      own = part_id_of(k, s_roots, s_rank, n_kept);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (at[a] + 1u >= dims[a]) continue;  // (the neighbour lies in the grid: e + step[a] < n)
        const part_key kn = keys[e + step[a]];
        if (!part_is_value(kn)) continue;
        const unsigned id = part_id_of(kn, s_roots, s_rank, n_kept);
        if (id == own || id >= n_kept || own >= n_kept) continue;
        other[a] = id;
        face = true;
      }
    }
    if (!__ballot(face)) continue;  // (every lane of the wave arrives here)
    if (!face) continue;
    const unsigned du = d2[e];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (other[a] == PART_ROOM_NONE) continue;
      const unsigned lo_id = own < other[a] ? own : other[a], hi_id = own < other[a] ? other[a] : own;
      const unsigned pair = lo_id * n_kept + hi_id;  // (below 2^20)
      const unsigned dn = d2[e + step[a]];
      const unsigned slot = part_slot(s_tag, pair);
      if (slot < (unsigned)PART_SLOTS) part_door_add(s_acc + slot * PART_DOOR_WORDS, x, y, z, a, du < dn ? du : dn);
      else part_door_add(table + (size_t)pair * PART_DOOR_WORDS, x, y, z, a, du < dn ? du : dn);
    }
  }
  __syncthreads();
  // the flush: a thread a slot
  if (threadIdx.x < (unsigned)PART_SLOTS && s_tag[threadIdx.x] != PART_SLOT_FREE) {
    const unsigned long long* v = s_acc + (size_t)threadIdx.x * PART_DOOR_WORDS;
    const unsigned* v32 = (const unsigned*)(v + 3);
    unsigned long long* t = table + (size_t)s_tag[threadIdx.x] * PART_DOOR_WORDS;
    unsigned* t32 = (unsigned*)(t + 3);
    for (int i = 0; i < 3; ++i) {  // (3 trips)
      atomicAdd(t + i, v[i]);
      atomicAdd(t32 + i, v32[i]);
    }
    for (int i = 3; i < 10; ++i) atomicMax(t32 + i, v32[i]);  // (7 trips)
  }
}

// ---- the reads ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_part_box(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ roots,
                                                  const unsigned* __restrict__ rank, unsigned n_kept, unsigned X, unsigned Y, int x0, int y0, int z0, unsigned bx,
                                                  unsigned by, unsigned long long n, int cost, unsigned* __restrict__ out) {
  __shared__ unsigned s_roots[PART_MAX_ROOMS];
  __shared__ unsigned s_rank[PART_MAX_ROOMS];
  part_load_table(s_roots, roots, n_kept);
  part_load_table(s_rank, rank, n_kept);
  __syncthreads();
  const unsigned long long e = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  const unsigned x = (unsigned)(e % bx), t = (unsigned)(e / bx), y = t % by, z = t / by;
  const part_key k = keys[((size_t)((unsigned)z0 + z) * Y + ((unsigned)y0 + y)) * X + ((unsigned)x0 + x)];
  out[e] = cost ? part_g(k) : part_id_of(k, s_roots, s_rank, n_kept);
}

struct PartPlainLoad {
  const unsigned long long* p;
  __device__ __forceinline__ part_key operator()(size_t i) const { return p[i]; }
};

__global__ __launch_bounds__(256) void k_part_gather(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ roots,
                                                     const unsigned* __restrict__ rank, unsigned n_kept, PartGeom q, SampleVol sv, const float* __restrict__ xyz,
                                                     unsigned n, int radius, unsigned* __restrict__ out) {
  __shared__ unsigned s_roots[PART_MAX_ROOMS];
  __shared__ unsigned s_rank[PART_MAX_ROOMS];
  part_load_table(s_roots, roots, n_kept);
  part_load_table(s_rank, rank, n_kept);
  __syncthreads();
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  unsigned x, y, z;
  bool inside;
  clear_point_voxel(sv, xyz[3u * e], xyz[3u * e + 1u], xyz[3u * e + 2u], x, y, z, inside);
  if (!inside) {
    out[e] = PART_ROOM_OUTSIDE;
    return;
  }
  const part_key k = part_nearest(PartPlainLoad{keys}, q.X, q.Y, q.Z, x, y, z, radius, q.w);  // (at most 729 trips)
  out[e] = part_is_value(k) ? part_id_of(k, s_roots, s_rank, n_kept) : PART_ROOM_NONE;
}

// ---- the launchers ------------------------------------------------------------------------------------------------------------
void part_geom(unsigned X, unsigned Y, unsigned Z, const unsigned w[3], unsigned core_d2, unsigned min_d2, unsigned min_core, unsigned max_cost,
               PartGeom* q) {
  hsk_relax_geom(X, Y, Z, w, q);
  q->core_d2 = core_d2;
  q->min_d2 = min_d2;
  q->min_core = min_core;
  q->max_cost = max_cost;
  for (int i = 0; i < 3; ++i) q->w[i] = w[i];
}

size_t part_layout(const PartGeom& q, void* base, PartBufs* b) {
  const size_t n = (size_t)q.X * q.Y * q.Z;
  RelaxCarve c{base};
  PartBufs out;
  out.counters = (unsigned long long*)c.take(128);
  out.keys = (unsigned long long*)c.take(n * 8);
  out.parent = (unsigned*)c.take(n * 4);
  c.worklists((size_t)q.ntx * q.nty * q.ntz, out.flags, out.list);
  out.roots_found = (unsigned*)c.take((size_t)PART_MAX_ROOMS * 4);
  out.roots = (unsigned*)c.take((size_t)PART_MAX_ROOMS * 4);
  out.rank = (unsigned*)c.take((size_t)PART_MAX_ROOMS * 4);
  out.recs = (unsigned long long*)c.take((size_t)PART_MAX_ROOMS * PART_REC_WORDS * 8);
  if (b) *b = out;
  return c.bytes;
}

hipError_t launch_part_label(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b) {
  const unsigned n = (unsigned)((size_t)q.X * q.Y * q.Z), tiles = q.ntx * q.nty * q.ntz;  // (at most 2^31 voxels: the callers check)
  const hipError_t e = hipMemsetAsync(b.counters, 0, 128, s);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)(((unsigned long long)n + 255u) / 256u);
  hipLaunchKernelGGL(k_part_label_tile, dim3(tiles), dim3(256), 0, s, d2, b.parent, b.keys, q);
  hipLaunchKernelGGL(k_part_label_faces, dim3(blocks), dim3(256), 0, s, b.parent, q, n);
  hipLaunchKernelGGL(k_part_flatten_count, dim3(blocks), dim3(256), 0, s, b.parent, b.keys, n);
  hipLaunchKernelGGL(k_part_roots, dim3(blocks), dim3(256), 0, s, (const unsigned*)b.parent, (const unsigned long long*)b.keys, n, q.min_core, b.roots_found,
                     b.counters);
  return hipGetLastError();
}

hipError_t launch_part_init(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b, unsigned n_kept) {
  const size_t tiles = (size_t)q.ntx * q.nty * q.ntz;
  hipError_t e = hipMemsetAsync(b.flags[0], 0, tiles * 4, s);
  if (e == hipSuccess) e = hipMemsetAsync(b.flags[1], 0, tiles * 4, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_part_init, dim3((unsigned)tiles), dim3(256), 0, s, d2, (const unsigned*)b.parent, b.keys, q, (const unsigned*)b.roots, n_kept, b.flags[0],
                     b.list[0], b.counters);
  return hipGetLastError();
}

hipError_t launch_part_round(hipStream_t s, const PartGeom& q, const PartBufs& b, int cur, unsigned n_active) {
  const int next = cur ^ 1;
  const hipError_t e = hipMemsetAsync(b.counters + 4 + next, 0, 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_part_round, dim3(n_active), dim3(256), 0, s, b.keys, q, (const unsigned*)b.list[cur], b.flags[cur], b.flags[next], b.list[next],
                     b.counters + 4 + next);
  return hipGetLastError();
}

hipError_t launch_part_records(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b, unsigned n_kept) {
  const unsigned long long n = (unsigned long long)q.X * q.Y * q.Z;
  const hipError_t e = hipMemsetAsync(b.recs, 0, (size_t)PART_MAX_ROOMS * PART_REC_WORDS * 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_part_records, dim3(hsk_sweep_blocks(n)), dim3(256), 0, s, (const unsigned long long*)b.keys, d2, q, n, (const unsigned*)b.roots, n_kept,
                     b.recs);
  return hipGetLastError();
}

hipError_t launch_part_doors(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b, unsigned n_kept, unsigned long long* table) {
  const unsigned long long n = (unsigned long long)q.X * q.Y * q.Z;
  const hipError_t e = hipMemsetAsync(table, 0, (size_t)n_kept * n_kept * PART_DOOR_WORDS * 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_part_doors, dim3(hsk_sweep_blocks(n)), dim3(256), 0, s, (const unsigned long long*)b.keys, d2, q, n, (const unsigned*)b.roots,
                     (const unsigned*)b.rank, n_kept, table);
  return hipGetLastError();
}

void launch_part_box(hipStream_t s, const PartGeom& q, const PartBufs& b, unsigned n_kept, const int lo[3], const int hi[3], bool cost, unsigned* out) {
  const unsigned bx = (unsigned)(hi[0] - lo[0]), by = (unsigned)(hi[1] - lo[1]), bz = (unsigned)(hi[2] - lo[2]);
  const unsigned long long n = (unsigned long long)bx * by * bz;
  hipLaunchKernelGGL(k_part_box, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, s, (const unsigned long long*)b.keys, (const unsigned*)b.roots,
                     (const unsigned*)b.rank, n_kept, q.X, q.Y, lo[0], lo[1], lo[2], bx, by, n, cost ? 1 : 0, out);
}

void launch_part_gather(hipStream_t s, const PartGeom& q, const PartBufs& b, unsigned n_kept, const VolParams& vp, const float* xyz, unsigned n, int radius,
                        unsigned* out) {
  hipLaunchKernelGGL(k_part_gather, dim3((n + 255u) / 256u), dim3(256), 0, s, (const unsigned long long*)b.keys, (const unsigned*)b.roots,
                     (const unsigned*)b.rank, n_kept, q, hsk_sample_vol(vp), xyz, n, radius, out);
}
