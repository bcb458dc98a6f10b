// reach_point_harness.cpp -- the reach kernels' shared text (housescan_amd/csrc/hsk_reach_point.h: passability, the box rule, the
// cost table, one tile's relaxation, the trace step), compiled for the host: it makes a whole field the way reach.hip's rounds do
// -- worklists of active tiles, double-buffered flags, a tile loaded with its halo, relaxed to a local fixpoint, stored, its
// neighbours marked -- one tile after the other, in the worklist's order, reversed, or shuffled; tests/test_reach_host.py compares
// it with the numpy twin (tests/reach_twin.py).  Input file: dims (3 int32), weight (3 uint32), min_d2, max_cost, the order (0 as
// listed, 1 reversed, 2 shuffled) (uint32 each), the number of seeds (uint32), the seeds' voxels (linear indices, uint32 each), the
// number of goals and the goals' voxels likewise, then the clearance field (X Y Z uint32, row-major, x fastest).  Output file: the
// field (X Y Z uint32), then passable, reached, the largest value, seeds used, rounds, tiles relaxed (6 uint64), then per goal the
// path's length (uint32) and its voxels from the seed to the goal (x, y, z int32 each).
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_reach_point.h"
#include "harness_io.h"

struct Tile {  // (exactly the cells of a tile and its halo: an access past them is the sanitizer's to find)
  std::vector<unsigned> cells = std::vector<unsigned>(REACH_HALO_CELLS), mv = std::vector<unsigned>(REACH_TILE_VOXELS);
  unsigned at(int x, int y, int z) const { return cells[reach_halo_index(x, y, z)]; }
  void set(int x, int y, int z, unsigned v) { cells[reach_halo_index(x, y, z)] = v; }
  unsigned moves(unsigned i) const { return mv[i]; }
  void set_moves(unsigned i, unsigned v) { mv[i] = v; }
};
struct Load {
  const std::vector<unsigned>* p;
  unsigned operator()(size_t i) const { return p->at(i); }
};
struct Store {
  std::vector<unsigned>* p;
  void operator()(size_t i, unsigned v) const { p->at(i) = v; }
};

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int dims[3];
  unsigned par[6], n_seeds, n_goals;
  if (!(in.get(dims, 3) && in.get(par, 6) && in.get(&n_seeds, 1))) return 2;
  std::vector<unsigned> seeds(n_seeds);
  if (!(in.get(seeds) && in.get(&n_goals, 1))) return 2;
  std::vector<unsigned> goals(n_goals);
  const unsigned X = (unsigned)dims[0], Y = (unsigned)dims[1], Z = (unsigned)dims[2];
  const unsigned w[3] = {par[0], par[1], par[2]}, min_d2 = par[3], max_cost = par[4], order = par[5];
  const size_t n = (size_t)X * Y * Z;
  std::vector<unsigned> d2(n);
  if (!(in.get(goals) && in.get(d2)) || n_seeds > REACH_MAX_SEEDS || max_cost > REACH_MAX_COST) return 2;
  unsigned cost[REACH_MOVES];
  reach_cost_table(w, cost);
  unsigned long long counts[6] = {0, 0, 0, 0, 0, 0};
  // init
  std::vector<unsigned> g(n);
  for (size_t i = 0; i < n; ++i) {
    const bool pass = reach_passable(d2[i], min_d2);
    g[i] = pass ? REACH_UNREACHED : REACH_BLOCKED;
    counts[0] += pass ? 1 : 0;
  }
  // the tiles, their flags and worklists
  const unsigned ntx = (X + REACH_TILE_X - 1u) / REACH_TILE_X, nty = (Y + REACH_TILE_Y - 1u) / REACH_TILE_Y, ntz = (Z + REACH_TILE_Z - 1u) / REACH_TILE_Z;
  const size_t tiles = (size_t)ntx * nty * ntz;
  std::vector<unsigned> flags[2] = {std::vector<unsigned>(tiles, 0u), std::vector<unsigned>(tiles, 0u)}, list[2];
  auto mark = [&](unsigned tile, int which) {
    if (flags[which].at(tile) == 0u) {
      flags[which][tile] = 1u;
      list[which].push_back(tile);
    }
  };
  for (unsigned v : seeds) {
    if (v >= n) return 4;
    if (g[v] == REACH_BLOCKED) continue;
    g[v] = 0u;
    counts[3] += 1;
    // (as k_reach_seed: every tile that holds the seed in its cells or halo is marked, not its own alone)
    const unsigned x = v % X, y = (v / X) % Y, z = v / (X * Y);
    const unsigned tx = x / REACH_TILE_X, ty = y / REACH_TILE_Y, tz = z / REACH_TILE_Z;
    const unsigned seen_by = reach_seen_by((int)(x % REACH_TILE_X), (int)(y % REACH_TILE_Y), (int)(z % REACH_TILE_Z));
    for (int m = 0; m < REACH_MOVES; ++m) {
      if (!((seen_by >> m) & 1u)) continue;
      const int nx = (int)tx + reach_dx(m), ny = (int)ty + reach_dy(m), nz = (int)tz + reach_dz(m);
      if (nx >= 0 && nx < (int)ntx && ny >= 0 && ny < (int)nty && nz >= 0 && nz < (int)ntz) mark(((unsigned)nz * nty + (unsigned)ny) * ntx + (unsigned)nx, 0);
    }
  }
  // the rounds
  unsigned long long lcg = 12345;
  int cur = 0;
  Tile s;
  while (!list[cur].empty()) {
    if (counts[4] >= REACH_MAX_ROUNDS) return 5;
    std::vector<unsigned> work = list[cur];
    if (order == 1u)
      for (size_t i = 0; i < work.size() / 2; ++i) std::swap(work[i], work[work.size() - 1 - i]);
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
      const Load ld{&g};
      reach_tile_load<ReachValue>(s, ld, ox, oy, oz, X, Y, Z, 0u, 1u);
      reach_tile_moves<ReachValue>(s, 0u, 1u);
      // (bounded as on the device: at most REACH_TILE_VOXELS sweeps change anything)
      unsigned sweep = 0;
      for (; sweep < (unsigned)REACH_TILE_VOXELS; ++sweep)
        if (!reach_tile_sweep<ReachValue>(s, 0u, 1u, cost, max_cost)) break;
      if (sweep == (unsigned)REACH_TILE_VOXELS) return 6;
      const unsigned seen_by = reach_tile_store<ReachValue>(s, ld, Store{&g}, ox, oy, oz, X, Y, Z, 0u, 1u);
      for (int m = 0; m < REACH_MOVES; ++m) {
        if (m == REACH_CENTRE || !((seen_by >> m) & 1u)) continue;
        const int nx = (int)tx + reach_dx(m), ny = (int)ty + reach_dy(m), nz = (int)tz + reach_dz(m);
        if (nx >= 0 && nx < (int)ntx && ny >= 0 && ny < (int)nty && nz >= 0 && nz < (int)ntz) mark(((unsigned)nz * nty + (unsigned)ny) * ntx + (unsigned)nx, cur ^ 1);
      }
      counts[5] += 1;
    }
    counts[4] += 1;
    cur ^= 1;
  }
  for (size_t i = 0; i < n; ++i)
    if (reach_is_value(g[i])) {
      counts[1] += 1;
      if (g[i] > counts[2]) counts[2] = g[i];
    }
  HarnessOut o(argv[2]);
  o.put(g.data(), n), o.put(counts, 6);
  // the paths
  const Load ld{&g};
  for (unsigned goal : goals) {
    if (goal >= n) return 4;
    std::vector<int> back;
    unsigned x = goal % X, y = (goal / X) % Y, z = goal / (X * Y), gv = g[goal];
    if (reach_is_value(gv))
      for (size_t step = 0; step < n; ++step) {  // (bounded: the value falls with every step)
        back.insert(back.end(), {(int)x, (int)y, (int)z});
        if (gv == 0u) break;
        int m = 0;
        while (m < REACH_MOVES && !reach_trace_ok(ld, X, Y, Z, x, y, z, m, cost[m], gv)) ++m;
        if (m == REACH_MOVES) return 7;  // (no move of the path rule: the field is no fixpoint)
        x = (unsigned)((int)x + reach_dx(m)), y = (unsigned)((int)y + reach_dy(m)), z = (unsigned)((int)z + reach_dz(m));
        gv -= cost[m];
      }
    const unsigned len = (unsigned)(back.size() / 3);
    o.put(&len, 1);
    for (unsigned i = len; i > 0; --i) o.put(&back[3 * (size_t)(i - 1)], 3);
  }
  return o.finish();
}
