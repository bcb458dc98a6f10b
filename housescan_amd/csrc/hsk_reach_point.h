// hsk_reach_point.h -- the reach field (DESIGN.md 8m the rule, 3.19 the kernels): which voxels a person can stand in, which of the
// 26 moves between them are allowed (the box rule), what a move costs, one tile's relaxation -- templated on the value a cell holds
// (the room partition relaxes its 64-bit keys with the same text: hsk_part_point.h) and on its load and store -- and the step of
// the path trace.  Plain C++ with no HIP type in it, so that tests/reach_point_harness.cpp compiles the same text
// for the host and tests/test_reach_host.py compares the field it makes with the numpy twin (tests/reach_twin.py).  All integers.
//
// THE METRIC is a 26-neighbour chamfer metric, NOT the Euclidean geodesic: a path is a chain of the 26 moves, each at its Euclidean
// length (times 16, rounded).  In open space, for unit weights, a straight segment of direction (a, b, c), a >= b >= c >= 0, is
// walked as c corner, b - c edge and a - b face moves: length a + (sqrt2 - 1) b + (sqrt3 - sqrt2) c against sqrt(a^2 + b^2 + c^2).
// The ratio is largest where the gradient of the first is parallel to the direction, (a, b, c) ~ (1, sqrt2 - 1, sqrt3 - sqrt2), and
// is there sqrt(1 + (sqrt2 - 1)^2 + (sqrt3 - sqrt2)^2) = 1.1280: the field overestimates a free straight walk by at most 12.8 %
// (8.24 % in a plane, the floor form) and never underestimates it beyond the rounding of the seven costs (half a unit in 16 or
// more: 3.2 %).
//
// THE BOUND every sum below rests on: a weight is at most 1024, so a cost is at most rint(16 sqrt(3 * 1024)) = 887; a value that is
// propagated is at most REACH_MAX_COST = 0xf0000000, so value + cost stays below 2^32: nothing wraps.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hsk_sample.h"

#define REACH_UNREACHED 0xffffffffu  // passable, but no path within max_cost (HSK_REACH_UNREACHED)
#define REACH_OUTSIDE 0xfffffffeu    // a point lookup outside the grid (HSK_REACH_OUTSIDE)
#define REACH_BLOCKED 0xfffffffdu    // not passable (HSK_REACH_BLOCKED); stored in the field itself
#define REACH_MAX_COST 0xf0000000u   // the largest max_cost; every value above it is one of the three markers
#define REACH_MAX_SEEDS 4096
#define REACH_MAX_ROUNDS 65536
// a tile: what one workgroup relaxes in LDS.  32 voxels along x make a row of the tile one 128-B piece of the field
#define REACH_TILE_X 32
#define REACH_TILE_Y 8
#define REACH_TILE_Z 8
#define REACH_TILE_VOXELS (REACH_TILE_X * REACH_TILE_Y * REACH_TILE_Z)
#define REACH_HALO_X (REACH_TILE_X + 2)
#define REACH_HALO_Y (REACH_TILE_Y + 2)
#define REACH_HALO_Z (REACH_TILE_Z + 2)
#define REACH_HALO_CELLS (REACH_HALO_X * REACH_HALO_Y * REACH_HALO_Z)
#define REACH_MOVES 27   // move index m = (dz + 1) 9 + (dy + 1) 3 + (dx + 1); m = 13 is the centre and no move
#define REACH_CENTRE 13

#if defined(__HIPCC__)
#define REACH_UNROLL _Pragma("unroll")
#else
#define REACH_UNROLL
#endif

HSK_HD bool reach_passable(unsigned d2, unsigned min_d2) { return d2 >= min_d2; }  // (CLEAR_FAR = 0xffffffff passes)
HSK_HD bool reach_is_value(unsigned g) { return g <= REACH_MAX_COST; }             // (not one of the three markers)

HSK_HD int reach_dx(int m) { return m % 3 - 1; }
HSK_HD int reach_dy(int m) { return (m / 3) % 3 - 1; }
HSK_HD int reach_dz(int m) { return m / 9 - 1; }

// the seven costs as a table over the move index: c(d) = rint(16 sqrt(w_x dx^2 + w_y dy^2 + w_z dz^2)) in binary64 (host only)
static inline void reach_cost_table(const unsigned w[3], unsigned cost[REACH_MOVES]) {
  for (int m = 0; m < REACH_MOVES; ++m) {
    const int dx = reach_dx(m), dy = reach_dy(m), dz = reach_dz(m);
    cost[m] = (unsigned)rint(16.0 * sqrt((double)w[0] * (dx * dx) + (double)w[1] * (dy * dy) + (double)w[2] * (dz * dz)));
  }
}

// The box rule.  Over the 27 cells around a voxel (cell index as the move index), the cells of the box spanned by the voxel and
// its neighbour m: the move is allowed when all of them (2, 4 or 8, the voxel itself among them) are passable.
HSK_HD unsigned reach_box_bits(int m) {
  const int dx = reach_dx(m), dy = reach_dy(m), dz = reach_dz(m);
  unsigned bits = 0u;
  for (int ez = 0; ez <= (dz != 0 ? 1 : 0); ++ez)
    for (int ey = 0; ey <= (dy != 0 ? 1 : 0); ++ey)
      for (int ex = 0; ex <= (dx != 0 ? 1 : 0); ++ex) bits |= 1u << ((ez * dz + 1) * 9 + (ey * dy + 1) * 3 + (ex * dx + 1));
  return bits;
}
// passable bits of the 27 cells -> the allowed moves, a bit per move index (0 when the voxel itself is not passable)
HSK_HD unsigned reach_moves_of(unsigned passable27) {
  unsigned moves = 0u;
REACH_UNROLL
  for (int m = 0; m < REACH_MOVES; ++m) {
    if (m == REACH_CENTRE) continue;
    const unsigned box = reach_box_bits(m);
    moves |= (passable27 & box) == box ? 1u << m : 0u;
  }
  return moves;
}

// ---- one tile in a local store --------------------------------------------------------------------------------------------------
// ONE relaxation text for every field over the free space, templated on a value policy `V`: V::T the cell's type, V::blocked() the
// marker of a cell that is not passable, V::is_value(v) whether a cell holds a value that can be propagated, V::plus(v, cost) the
// value one move of that cost further and V::cost(v) the cost sum it carries, which max_cost bounds.  plus must preserve the
// order of values and must not wrap (THE BOUND above); then the least fixpoint does not depend on the order of the work.
// ReachValue below is the reach field's policy, PartValue (hsk_part_point.h) the room partition's.
//
// `Cells` is a tile with its one-voxel halo and a word per interior voxel for its allowed moves: at(x, y, z) / set(x, y, z, v) with
// -1 <= x <= REACH_TILE_X (and so on; only interior cells are ever set), moves(i) / set_moves(i, m) with i the interior voxel's
// index (z REACH_TILE_Y + y) REACH_TILE_X + x.  A cell outside the grid holds V::blocked().  `lane` of `nlanes` workers takes the
// voxels i = lane, lane + nlanes, ...: the device runs 256 of them with a barrier between the steps, the host harness one.
struct ReachValue {
  typedef unsigned T;
  HSK_HD T blocked() { return REACH_BLOCKED; }
  HSK_HD bool is_value(T v) { return reach_is_value(v); }
  HSK_HD T plus(T v, unsigned cost) { return v + cost; }  // (below 2^32: THE BOUND)
  HSK_HD unsigned cost(T v) { return v; }
};

// the index into a halo array of REACH_HALO_CELLS words
HSK_HD unsigned reach_halo_index(int x, int y, int z) {
  return (unsigned)(((z + 1) * REACH_HALO_Y + (y + 1)) * REACH_HALO_X + (x + 1));
}

// load: the tile at voxel (ox, oy, oz) with its halo from the field `ld(linear index)` of an X Y Z grid
template <class V, class Cells, class Load>
HSK_HD void reach_tile_load(Cells& s, const Load& ld, unsigned ox, unsigned oy, unsigned oz, unsigned X, unsigned Y, unsigned Z, unsigned lane,
                            unsigned nlanes) {
  for (unsigned i = lane; i < (unsigned)REACH_HALO_CELLS; i += nlanes) {  // (ends: i grows by nlanes)
    const int hx = (int)(i % REACH_HALO_X) - 1, hy = (int)((i / REACH_HALO_X) % REACH_HALO_Y) - 1, hz = (int)(i / (REACH_HALO_X * REACH_HALO_Y)) - 1;
    const long long gx = (long long)ox + hx, gy = (long long)oy + hy, gz = (long long)oz + hz;
    const bool in = gx >= 0 && gx < (long long)X && gy >= 0 && gy < (long long)Y && gz >= 0 && gz < (long long)Z;
    s.set(hx, hy, hz, in ? ld(((size_t)gz * Y + (size_t)gy) * X + (size_t)gx) : V::blocked());
  }
}

// the allowed moves of every interior voxel, from the cells as loaded (whether a cell is blocked never changes afterwards)
template <class V, class Cells>
HSK_HD void reach_tile_moves(Cells& s, unsigned lane, unsigned nlanes) {
  for (unsigned i = lane; i < (unsigned)REACH_TILE_VOXELS; i += nlanes) {  // (ends: i grows by nlanes)
    const int x = (int)(i % REACH_TILE_X), y = (int)((i / REACH_TILE_X) % REACH_TILE_Y), z = (int)(i / (REACH_TILE_X * REACH_TILE_Y));
    unsigned pass = 0u;
REACH_UNROLL
    for (int c = 0; c < REACH_MOVES; ++c) pass |= s.at(x + reach_dx(c), y + reach_dy(c), z + reach_dz(c)) != V::blocked() ? 1u << c : 0u;
    s.set_moves(i, reach_moves_of(pass));
  }
}

// one voxel: the least of its value and, over its allowed moves, the neighbour's value plus the move's cost, where that cost sum
// is at most max_cost.  A neighbour that holds no value (UNREACHED, UNASSIGNED) offers nothing.
template <class V, class Cells>
HSK_HD typename V::T reach_relax_voxel(const Cells& s, int x, int y, int z, unsigned moves, const unsigned* cost, unsigned max_cost) {
  typename V::T best = s.at(x, y, z);
REACH_UNROLL
  for (int m = 0; m < REACH_MOVES; ++m) {
    if (m == REACH_CENTRE || !((moves >> m) & 1u)) continue;
    const typename V::T n = s.at(x + reach_dx(m), y + reach_dy(m), z + reach_dz(m));
    if (!V::is_value(n)) continue;
    const typename V::T cand = V::plus(n, cost[m]);
    best = (V::cost(cand) <= max_cost && cand < best) ? cand : best;
  }
  return best;
}

// one sweep of this worker's voxels, in place (a value read while another worker lowers it is the old or the new one, whole: both
// are upper bounds of the fixpoint) -> whether any of them fell
template <class V, class Cells>
HSK_HD bool reach_tile_sweep(Cells& s, unsigned lane, unsigned nlanes, const unsigned* cost, unsigned max_cost) {
  bool fell = false;
  for (unsigned i = lane; i < (unsigned)REACH_TILE_VOXELS; i += nlanes) {  // (ends: i grows by nlanes)
    const unsigned moves = s.moves(i);
    if (!moves) continue;
    const int x = (int)(i % REACH_TILE_X), y = (int)((i / REACH_TILE_X) % REACH_TILE_Y), z = (int)(i / (REACH_TILE_X * REACH_TILE_Y));
    const typename V::T v = reach_relax_voxel<V>(s, x, y, z, moves, cost, max_cost);
    if (v < s.at(x, y, z)) {
      s.set(x, y, z, v);
      fell = true;
    }
  }
  return fell;
}

// The tiles that hold the interior voxel (x, y, z) of a tile in their own cells or halo, a bit per tile offset (indexed as the
// moves; the centre bit is the tile itself): a voxel on a face of the tile is seen across that face, one on an edge or a corner
// across the two or three faces and the edge or corner itself -- a diagonal move crosses them.  Whoever lowers a voxel's value,
// a tile's store or the placing of a seed, owes a mark to every one of these tiles.
HSK_HD unsigned reach_seen_by(int x, int y, int z) {
  const int sx = x == 0 ? 0 : x == REACH_TILE_X - 1 ? 2 : 1, sy = y == 0 ? 0 : y == REACH_TILE_Y - 1 ? 2 : 1,
            sz = z == 0 ? 0 : z == REACH_TILE_Z - 1 ? 2 : 1;
  unsigned bits = 0u;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c) bits |= 1u << ((a ? sz : 1) * 9 + (b ? sy : 1) * 3 + (c ? sx : 1));
  return bits;
}

// store: every interior voxel whose value fell below the field's goes back -> the neighbouring tiles that can see a voxel that
// fell (reach_seen_by), a bit per tile offset (indexed as the moves; the centre bit says that anything fell at all).  Only the
// worker of a tile ever stores its interior voxels.
template <class V, class Cells, class Load, class Store>
HSK_HD unsigned reach_tile_store(const Cells& s, const Load& ld, const Store& st, unsigned ox, unsigned oy, unsigned oz, unsigned X, unsigned Y,
                                 unsigned Z, unsigned lane, unsigned nlanes) {
  unsigned seen_by = 0u;
  for (unsigned i = lane; i < (unsigned)REACH_TILE_VOXELS; i += nlanes) {  // (ends: i grows by nlanes)
    const int x = (int)(i % REACH_TILE_X), y = (int)((i / REACH_TILE_X) % REACH_TILE_Y), z = (int)(i / (REACH_TILE_X * REACH_TILE_Y));
    const unsigned gx = ox + (unsigned)x, gy = oy + (unsigned)y, gz = oz + (unsigned)z;
    if (gx >= X || gy >= Y || gz >= Z) continue;
    const size_t at = ((size_t)gz * Y + gy) * X + gx;
    const typename V::T v = s.at(x, y, z);
    if (v >= ld(at)) continue;
    st(at, v);
    seen_by |= reach_seen_by(x, y, z);
  }
  return seen_by;
}

// ---- the path trace ---------------------------------------------------------------------------------------------------------------
// whether the step from voxel (x, y, z), whose value is gv, along move m is one of the path rule's: the move is allowed and
// G(v + d) + c(d) == G(v), cost_m = c(d).  `g(linear index)` reads the field.  The path takes the smallest such m.
template <class Load>
HSK_HD bool reach_trace_ok(const Load& g, unsigned X, unsigned Y, unsigned Z, unsigned x, unsigned y, unsigned z, int m, unsigned cost_m,
                           unsigned gv) {
  if (m == REACH_CENTRE || m < 0 || m >= REACH_MOVES) return false;
  const int dx = reach_dx(m), dy = reach_dy(m), dz = reach_dz(m);
  const long long nx = (long long)x + dx, ny = (long long)y + dy, nz = (long long)z + dz;
  if (nx < 0 || nx >= (long long)X || ny < 0 || ny >= (long long)Y || nz < 0 || nz >= (long long)Z) return false;
  bool open = true;  // (the box's cells lie between the two voxels: all inside the grid)
  for (int ez = 0; ez <= (dz != 0 ? 1 : 0); ++ez)
    for (int ey = 0; ey <= (dy != 0 ? 1 : 0); ++ey)
      for (int ex = 0; ex <= (dx != 0 ? 1 : 0); ++ex)
        open = open && g(((size_t)((long long)z + ez * dz) * Y + (size_t)((long long)y + ey * dy)) * X + (size_t)((long long)x + ex * dx)) != REACH_BLOCKED;
  if (!open) return false;
  const unsigned n = g(((size_t)nz * Y + (size_t)ny) * X + (size_t)nx);
  return reach_is_value(n) && n + cost_m == gv;
}
