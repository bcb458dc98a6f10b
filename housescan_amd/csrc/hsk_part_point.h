// hsk_part_point.h -- the room partition (DESIGN.md 8n the rule, 3.20 the kernels): the 64-bit key (cost, label of the core the
// chain starts in) a voxel holds, the value policy that makes the reach field's tile relaxation one on such keys, the order of the
// room records and the point lookup's search.  The moves, the box rule, the costs, the tile relaxation, the halo's index and the
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
// would be wrong, not merely late.  The relaxation's tile, load and store are therefore template arguments; the kernels pass 64-bit
// atomics.
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
// The tile relaxation is hsk_reach_point.h's (reach_tile_load / _moves / _sweep / _store) with this value policy: a cell is a key,
// a move adds (c << 32) -- G + c < 2^32 by THE BOUND, so nothing is carried out of the word -- and max_cost bounds G.
struct PartValue {
  typedef part_key T;
  HSK_HD T blocked() { return PART_KEY_BLOCKED; }
  HSK_HD bool is_value(T k) { return part_is_value(k); }
  HSK_HD T plus(T k, unsigned cost) { return k + ((part_key)cost << 32); }
  HSK_HD unsigned cost(T k) { return part_g(k); }
};

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
