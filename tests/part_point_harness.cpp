// part_point_harness.cpp -- the partition kernels' shared text (housescan_amd/csrc/hsk_part_point.h: the 64-bit key, one tile's
// relaxation on keys, the point lookup's search; with it hsk_reach_point.h's moves and hsk_comp_point.h's union-find), compiled for
// the host: it labels the cores with comp_unite over the dense grid, drops the small ones, and makes the whole field the way
// partition.hip's rounds do -- the first worklist the tiles that hold an UNASSIGNED voxel, double-buffered flags, a tile loaded with
// its halo, relaxed to a local fixpoint, stored, its neighbours marked -- one tile after the other, in the worklist's order,
// reversed, or shuffled; tests/test_partition_host.py compares it with the numpy twin (tests/partition_twin.py).  Input file: dims
// (3 int32), weight (3 uint32), core_d2, min_d2, min_core_voxels, max_cost, the order (0 as listed, 1 reversed, 2 shuffled), the
// lookup's radius, the number of lookups (uint32 each), the lookups' voxels (linear indices, uint32 each), then the clearance field
// (X Y Z uint32, row-major, x fastest).  Output file: cores, kept cores, passable, rounds, tiles relaxed, tiles of the first worklist
// (6 uint64); with at most PART_MAX_ROOMS kept cores then the keys (X Y Z uint64), the kept roots ascending (uint32 each) and per
// lookup the key found (uint64).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_part_point.h"
#include "harness_io.h"

struct Tile {  // (exactly the cells of a tile and its halo: an access past them is the sanitizer's to find)
  std::vector<part_key> cells = std::vector<part_key>(REACH_HALO_CELLS);
  std::vector<unsigned> mv = std::vector<unsigned>(REACH_TILE_VOXELS);
  part_key at(int x, int y, int z) const { return cells[reach_halo_index(x, y, z)]; }
  void set(int x, int y, int z, part_key v) { cells[reach_halo_index(x, y, z)] = v; }
  unsigned moves(unsigned i) const { return mv[i]; }
  void set_moves(unsigned i, unsigned v) { mv[i] = v; }
};
struct Load {
  const std::vector<part_key>* p;
  part_key operator()(size_t i) const { return p->at(i); }
};
struct Store {
  std::vector<part_key>* p;
  void operator()(size_t i, part_key v) const { p->at(i) = v; }
};

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int dims[3];
  unsigned par[10];
  if (!(in.get(dims, 3) && in.get(par, 10))) return 2;
  const unsigned n_points = par[9];
  std::vector<unsigned> points(n_points);
  const unsigned X = (unsigned)dims[0], Y = (unsigned)dims[1], Z = (unsigned)dims[2];
  const unsigned w[3] = {par[0], par[1], par[2]}, core_d2 = par[3], min_d2 = par[4], min_core = par[5], max_cost = par[6], order = par[7];
  const int radius = (int)par[8];
  const size_t n = (size_t)X * Y * Z;
  std::vector<unsigned> d2(n);
  if (!(in.get(points) && in.get(d2)) || max_cost > REACH_MAX_COST || radius > PART_MAX_RADIUS || !(1u <= min_d2 && min_d2 <= core_d2)) return 2;
  unsigned cost[REACH_MOVES];
  reach_cost_table(w, cost);
  unsigned long long counts[6] = {0, 0, 0, 0, 0, 0};
  // the cores: the dense grid's union-find, every core voxel united with the core voxels below it on the three axes
  std::vector<unsigned> parent(n);
  const CompDirect map;
  for (size_t i = 0; i < n; ++i) parent[i] = part_core(d2[i], core_d2) ? (unsigned)i : COMP_NONE;
  for (size_t i = 0; i < n; ++i) {
    if (parent[i] == COMP_NONE) continue;
    const unsigned x = (unsigned)(i % X), y = (unsigned)((i / X) % Y), z = (unsigned)(i / ((size_t)X * Y));
    if (x > 0 && parent[i - 1] != COMP_NONE) comp_unite<CompPlainOps>(parent.data(), map, (unsigned)i, (unsigned)(i - 1));
    if (y > 0 && parent[i - X] != COMP_NONE) comp_unite<CompPlainOps>(parent.data(), map, (unsigned)i, (unsigned)(i - X));
    if (z > 0 && parent[i - (size_t)X * Y] != COMP_NONE) comp_unite<CompPlainOps>(parent.data(), map, (unsigned)i, (unsigned)(i - (size_t)X * Y));
  }
  std::vector<unsigned long long> size(n, 0ull);
  for (size_t i = 0; i < n; ++i)
    if (parent[i] != COMP_NONE) {
      parent[i] = comp_find<CompPlainOps>(parent.data(), map, (unsigned)i);
      size[parent[i]] += 1;
    }
  std::vector<unsigned> roots;
  for (size_t i = 0; i < n; ++i)
    if (parent[i] == (unsigned)i) {
      counts[0] += 1;
      if (size[i] >= min_core) roots.push_back((unsigned)i);  // (ascending)
    }
  counts[1] = roots.size();
  HarnessOut o(argv[2]);
  if (roots.size() > (size_t)PART_MAX_ROOMS) return o.put(counts, 6), o.finish();
  // the tiles, their flags and worklists; init
  const unsigned ntx = (X + REACH_TILE_X - 1u) / REACH_TILE_X, nty = (Y + REACH_TILE_Y - 1u) / REACH_TILE_Y, ntz = (Z + REACH_TILE_Z - 1u) / REACH_TILE_Z;
  const size_t tiles = (size_t)ntx * nty * ntz;
  std::vector<unsigned> flags[2] = {std::vector<unsigned>(tiles, 0u), std::vector<unsigned>(tiles, 0u)}, list[2];
  auto mark = [&](unsigned tile, int which) {
    if (flags[which].at(tile) == 0u) {
      flags[which][tile] = 1u;
      list[which].push_back(tile);
    }
  };
  std::vector<part_key> key(n);
  for (size_t i = 0; i < n; ++i) {
    const bool pass = reach_passable(d2[i], min_d2);
    const bool kept = parent[i] != COMP_NONE && comp_search(roots.data(), (unsigned)roots.size(), parent[i]) < roots.size();
    key[i] = kept ? part_key_of(0u, parent[i]) : pass ? PART_KEY_UNASSIGNED : PART_KEY_BLOCKED;
    counts[2] += pass ? 1 : 0;
    if (pass && !kept) {
      const unsigned x = (unsigned)(i % X), y = (unsigned)((i / X) % Y), z = (unsigned)(i / ((size_t)X * Y));
      mark(((z / REACH_TILE_Z) * nty + y / REACH_TILE_Y) * ntx + x / REACH_TILE_X, 0);
    }
  }
  counts[5] = list[0].size();
  if (roots.empty()) list[0].clear();
  // the rounds
  unsigned long long lcg = 12345;
  int cur = 0;
  Tile s;
  while (!list[cur].empty()) {
    if (counts[3] >= REACH_MAX_ROUNDS) return 5;
    std::vector<unsigned> work = list[cur];
    if (order == 1u) std::reverse(work.begin(), work.end());
    if (order == 2u)
      for (size_t i = work.size(); i > 1; --i) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(work[i - 1], work[(size_t)((lcg >> 33) % i)]);
      }
    list[cur ^ 1].clear();
    for (unsigned tile : work) {
      flags[cur].at(tile) = 0u;
      const unsigned tx = tile % ntx, ty = (tile / ntx) % nty, tz = tile / (ntx * nty);
      const unsigned ox = tx * REACH_TILE_X, oy = ty * REACH_TILE_Y, oz = tz * REACH_TILE_Z;
      const Load ld{&key};
      reach_tile_load<PartValue>(s, ld, ox, oy, oz, X, Y, Z, 0u, 1u);
      reach_tile_moves<PartValue>(s, 0u, 1u);
      // (bounded as on the device: at most REACH_TILE_VOXELS sweeps change anything)
      unsigned sweep = 0;
      for (; sweep < (unsigned)REACH_TILE_VOXELS; ++sweep)
        if (!reach_tile_sweep<PartValue>(s, 0u, 1u, cost, max_cost)) break;
      if (sweep == (unsigned)REACH_TILE_VOXELS) return 6;
      const unsigned seen_by = reach_tile_store<PartValue>(s, ld, Store{&key}, ox, oy, oz, X, Y, Z, 0u, 1u);
      for (int m = 0; m < REACH_MOVES; ++m) {
        if (m == REACH_CENTRE || !((seen_by >> m) & 1u)) continue;
        const int nx = (int)tx + reach_dx(m), ny = (int)ty + reach_dy(m), nz = (int)tz + reach_dz(m);
        if (nx >= 0 && nx < (int)ntx && ny >= 0 && ny < (int)nty && nz >= 0 && nz < (int)ntz) mark(((unsigned)nz * nty + (unsigned)ny) * ntx + (unsigned)nx, cur ^ 1);
      }
      counts[4] += 1;
    }
    counts[3] += 1;
    cur ^= 1;
  }
  o.put(counts, 6), o.put(key.data(), n), o.put(roots);
  const Load ld{&key};
  for (unsigned v : points) {
    if (v >= n) return 4;
    const part_key found = part_nearest(ld, X, Y, Z, v % X, (v / X) % Y, v / (X * Y), radius, w);
    o.put(&found, 1);
  }
  return o.finish();
}
