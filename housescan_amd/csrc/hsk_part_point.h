// hsk_part_point.h -- the room partition (DESIGN.md 8n the rule, 3.20 the kernels): the 64-bit key (cost, label of the core the
// chain starts in) a voxel holds, one tile's relaxation on such keys -- templated on its load and store, as the reach field's is
// --, the order of the room records and the point lookup's search.  The moves, the box rule, the costs, the halo's index and the
// tiles a voxel is seen by are hsk_reach_point.h's, the union-find of the core labelling hsk_comp_point.h's: this file restates
// none of them.  Plain C++ with no HIP type in it, so that tests/part_point_harness.cpp compiles the same text for the host and
// tests/test_partition_host.py compares what it makes with the numpy twin (tests/partition_twin.py).  All integers.
//
// THE KEY is (G << 32) | L: G the sum of the costs of a chain of allowed moves, L the label of the kept core the chain starts in
// (the smallest lin among the core's voxels).  Keys are compared as 64-bit words, which is the lexicographic order of (G, L), and
// a move adds (c << 32): that preserves the order of keys, so the least fixpoint of K(v) = min(K(v), K(u) + (c << 32)) does not
// depend on the order of the work.  THE BOUND is the reach field's: G <= REACH_MAX_COST = 0xf0000000 where it is propagated and a
// cost is at most 887, so G + c stays below 2^32 and the addition never carries into nothing.
//
// A KEY MUST NEVER BE READ OR WRITTEN IN HALVES where another worker may touch it: a torn key (new G, old L) can lie BELOW the
// fixpoint -- the smaller cost of one core with the smaller label of another -- and a relaxation only ever lowers, so the result
// would be wrong, not merely late.  The load and the store are therefore template arguments; the kernels pass 64-bit atomics.
#pragma once
#include "hsk_comp_point.h"
#include "hsk_reach_point.h"

#define PART_MAX_ROOMS 1024
#define PART_MAX_RADIUS 4
#define PART_ROOM_UNASSIGNED 0xffffffffu  // passable, but no chain from a kept core within max_cost (HSK_ROOM_UNASSIGNED)
#define PART_ROOM_OUTSIDE 0xfffffffeu     // a point lookup outside the grid (HSK_ROOM_OUTSIDE)
#define PART_ROOM_BLOCKED 0xfffffffdu     // not passable (HSK_ROOM_BLOCKED)
#define PART_ROOM_NONE 0xfffffffcu        // a point lookup that finds no voxel of a room within its radius (HSK_ROOM_NONE)
// the two markers as keys: their G is the reach field's marker, so that G alone IS the reach field seeded at every kept core voxel
#define PART_KEY_UNASSIGNED 0xffffffffffffffffull
#define PART_KEY_BLOCKED 0xfffffffdffffffffull

typedef unsigned long long part_key;

HSK_HD part_key part_key_of(unsigned g, unsigned label) { return ((part_key)g << 32) | (part_key)label; }
HSK_HD unsigned part_g(part_key k) { return (unsigned)(k >> 32); }
HSK_HD unsigned part_label(part_key k) { return (unsigned)(k & 0xffffffffull); }
HSK_HD bool part_is_value(part_key k) { return reach_is_value(part_g(k)); }  // (holds a room: not one of the two markers)
HSK_HD bool part_core(unsigned d2, unsigned core_d2) { return d2 >= core_d2; }  // (CLEAR_FAR = 0xffffffff passes)

// ---- one tile in a local store --------------------------------------------------------------------------------------------------
// `Cells` is the reach field's tile with 64-bit cells: k(x, y, z) / set(x, y, z, v) with -1 <= x <= REACH_TILE_X (and so on; only
// interior cells are ever set), moves(i) / set_moves(i, m).  A cell outside the grid holds PART_KEY_BLOCKED.

template <class Cells, class Load>
HSK_HD void part_tile_load(Cells& s, const Load& ld, unsigned ox, unsigned oy, unsigned oz, unsigned X, unsigned Y, unsigned Z, unsigned lane,
                           unsigned nlanes) {
  for (unsigned i = lane; i < (unsigned)REACH_HALO_CELLS; i += nlanes) {  // (ends: i grows by nlanes)
    const int hx = (int)(i % REACH_HALO_X) - 1, hy = (int)((i / REACH_HALO_X) % REACH_HALO_Y) - 1, hz = (int)(i / (REACH_HALO_X * REACH_HALO_Y)) - 1;
    const long long gx = (long long)ox + hx, gy = (long long)oy + hy, gz = (long long)oz + hz;
    const bool in = gx >= 0 && gx < (long long)X && gy >= 0 && gy < (long long)Y && gz >= 0 && gz < (long long)Z;
    s.set(hx, hy, hz, in ? ld(((size_t)gz * Y + (size_t)gy) * X + (size_t)gx) : PART_KEY_BLOCKED);
  }
}

// the allowed moves of every interior voxel (hsk_reach_point.h: reach_moves_of), from the cells as loaded
template <class Cells>
HSK_HD void part_tile_moves(Cells& s, unsigned lane, unsigned nlanes) {
  for (unsigned i = lane; i < (unsigned)REACH_TILE_VOXELS; i += nlanes) {  // (ends: i grows by nlanes)
    const int x = (int)(i % REACH_TILE_X), y = (int)((i / REACH_TILE_X) % REACH_TILE_Y), z = (int)(i / (REACH_TILE_X * REACH_TILE_Y));
    unsigned pass = 0u;
REACH_UNROLL
    for (int c = 0; c < REACH_MOVES; ++c) pass |= s.k(x + reach_dx(c), y + reach_dy(c), z + reach_dz(c)) != PART_KEY_BLOCKED ? 1u << c : 0u;
    s.set_moves(i, reach_moves_of(pass));
  }
}

// one voxel: the least of its key and, over its allowed moves, the neighbour's key plus the move's cost, where that cost sum is at
// most max_cost.  A neighbour that holds no room offers nothing.
template <class Cells>
HSK_HD part_key part_relax_voxel(const Cells& s, int x, int y, int z, unsigned moves, const unsigned* cost, unsigned max_cost) {
  part_key best = s.k(x, y, z);
REACH_UNROLL
  for (int m = 0; m < REACH_MOVES; ++m) {
    if (m == REACH_CENTRE || !((moves >> m) & 1u)) continue;
    const part_key n = s.k(x + reach_dx(m), y + reach_dy(m), z + reach_dz(m));
    if (!part_is_value(n)) continue;
    const part_key cand = n + ((part_key)cost[m] << 32);  // (G + c < 2^32: the bound above)
    best = (part_g(cand) <= max_cost && cand < best) ? cand : best;
  }
  return best;
}

// one sweep of this worker's voxels, in place (a key read while another worker lowers it is the old or the new one, whole: both
// are upper bounds of the fixpoint) -> whether any of them fell
template <class Cells>
HSK_HD bool part_tile_sweep(Cells& s, unsigned lane, unsigned nlanes, const unsigned* cost, unsigned max_cost) {
  bool fell = false;
  for (unsigned i = lane; i < (unsigned)REACH_TILE_VOXELS; i += nlanes) {  // (ends: i grows by nlanes)
    const unsigned moves = s.moves(i);
    if (!moves) continue;
    const int x = (int)(i % REACH_TILE_X), y = (int)((i / REACH_TILE_X) % REACH_TILE_Y), z = (int)(i / (REACH_TILE_X * REACH_TILE_Y));
    const part_key v = part_relax_voxel(s, x, y, z, moves, cost, max_cost);
    if (v < s.k(x, y, z)) {
      s.set(x, y, z, v);
      fell = true;
    }
  }
  return fell;
}

// store: every interior voxel whose key fell below the field's goes back -> the tiles that can see a voxel that fell
// (hsk_reach_point.h: reach_seen_by), a bit per tile offset.  Only the worker of a tile ever stores its interior voxels.
template <class Cells, class Load, class Store>
HSK_HD unsigned part_tile_store(const Cells& s, const Load& ld, const Store& st, unsigned ox, unsigned oy, unsigned oz, unsigned X, unsigned Y, unsigned Z,
                                unsigned lane, unsigned nlanes) {
  unsigned seen_by = 0u;
  for (unsigned i = lane; i < (unsigned)REACH_TILE_VOXELS; i += nlanes) {  // (ends: i grows by nlanes)
    const int x = (int)(i % REACH_TILE_X), y = (int)((i / REACH_TILE_X) % REACH_TILE_Y), z = (int)(i / (REACH_TILE_X * REACH_TILE_Y));
    const unsigned gx = ox + (unsigned)x, gy = oy + (unsigned)y, gz = oz + (unsigned)z;
    if (gx >= X || gy >= Y || gz >= Z) continue;
    const size_t at = ((size_t)gz * Y + gy) * X + gx;
    const part_key v = s.k(x, y, z);
    if (v >= ld(at)) continue;
    st(at, v);
    seen_by |= reach_seen_by(x, y, z);
  }
  return seen_by;
}

// ---- the point lookup -----------------------------------------------------------------------------------------------------------
// Among the voxels within |dx|, |dy|, |dz| <= radius of (x, y, z) that lie in the grid and hold a room, the one that minimises
// (w_x dx^2 + w_y dy^2 + w_z dz^2, lin) -> its key, or PART_KEY_UNASSIGNED when there is none.  `key(linear index)` reads the
// field.  At most (2 * 4 + 1)^3 = 729 trips; a weight is at most 1024, so a distance is at most 3 * 1024 * 16.
template <class Load>
HSK_HD part_key part_nearest(const Load& key, unsigned X, unsigned Y, unsigned Z, unsigned x, unsigned y, unsigned z, int radius, const unsigned w[3]) {
  part_key found = PART_KEY_UNASSIGNED;
  unsigned long long best = ~0ull;  // (distance << 32 | lin: lin < 2^31)
  for (int dz = -radius; dz <= radius; ++dz)
    for (int dy = -radius; dy <= radius; ++dy)
      for (int dx = -radius; dx <= radius; ++dx) {
        const long long nx = (long long)x + dx, ny = (long long)y + dy, nz = (long long)z + dz;
        if (nx < 0 || nx >= (long long)X || ny < 0 || ny >= (long long)Y || nz < 0 || nz >= (long long)Z) continue;
        const size_t at = ((size_t)nz * Y + (size_t)ny) * X + (size_t)nx;
        const part_key k = key(at);
        if (!part_is_value(k)) continue;
        const unsigned long long d = (unsigned long long)(w[0] * (unsigned)(dx * dx) + w[1] * (unsigned)(dy * dy) + w[2] * (unsigned)(dz * dz));
        const unsigned long long rank = (d << 32) | (unsigned long long)at;
        if (rank < best) {
          best = rank;
          found = k;
        }
      }
  return found;
}

// the order of the room records is the components': more voxels first, ties to the smaller root (comp_record_before)
