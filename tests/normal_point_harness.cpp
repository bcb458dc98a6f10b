// normal_point_harness.cpp -- the cloud normals' work on one point (housescan_amd/csrc/hsk_normal_point.h), compiled for the host:
// tests/test_normals_host.py feeds it a cloud, viewpoints and parameters and compares every output with the numpy twin.  Input file:
// n, n_viewpoints, min_neighbours, max_neighbours (4 uint32); radius_m, line_rel (2 float); the points (3 floats each); the
// viewpoints likewise.  Output file: the normals (3 n float), the curvature (n float), the neighbour counts (n uint32), the classes
// (n uint8), then n_ok, n_invalid, n_sparse, n_crowded, n_degenerate, n_cells (uint32) and n_pairs (uint64).  The search is the
// device's in its plainest form: the valid points sorted by their cell's key, the 27 cells around a point found by bisection; a
// point stops counting once it has max_neighbours + 1 neighbours, as a lane does.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_normal_point.h"
#include "harness_io.h"

struct Entry {
  unsigned long long key;
  int q[3];
};

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  unsigned head[4];
  float pf[2];
  if (!(in.get(head, 4) && in.get(pf, 2))) return 2;
  const size_t n = head[0], nv = head[1];
  const unsigned min_nb = head[2], max_nb = head[3];
  std::vector<float> xyz(n * 3), view(nv * 3);
  if (!(in.get(xyz) && in.get(view))) return 2;
  const int r_q = normal_radius_q(pf[0]);
  if (r_q < NORMAL_MIN_RQ || r_q > NORMAL_MAX_RQ || min_nb < 3u || max_nb < min_nb || max_nb > (unsigned)NORMAL_MAX_NEIGHBOURS) return 3;
  const normal_i64 r2 = (normal_i64)r_q * r_q;
  std::vector<Entry> cells;
  for (size_t i = 0; i < n; ++i) {
    const float* p = &xyz[i * 3];
    if (!normal_point_valid(p[0], p[1], p[2])) continue;
    Entry e;
    for (int a = 0; a < 3; ++a) e.q[a] = plane_q(p[a]);
    e.key = normal_key(normal_cell(e.q[0], r_q), normal_cell(e.q[1], r_q), normal_cell(e.q[2], r_q));
    cells.push_back(e);
  }
  std::sort(cells.begin(), cells.end(), [](const Entry& a, const Entry& b) { return a.key < b.key; });
  std::vector<float> normals(n * 3, 0.0f), curv(n, 0.0f);
  std::vector<unsigned> counts(n, 0u);
  std::vector<unsigned char> cls(n, (unsigned char)NORMAL_INVALID);
  unsigned tally[NORMAL_CLASSES + 1] = {0u, 0u, 0u, 0u, 0u, 0u};
  uint64_t pairs = 0;
  for (size_t c = 0; c < cells.size(); ++c) tally[NORMAL_CLASSES] += (c == 0 || cells[c].key != cells[c - 1].key) ? 1u : 0u;
  const int c_max = (int)normal_cell_max(r_q);
  for (size_t i = 0; i < n; ++i) {
    const float* p = &xyz[i * 3];
    if (!normal_point_valid(p[0], p[1], p[2])) {
      tally[NORMAL_INVALID] += 1u;
      continue;
    }
    const int q[3] = {plane_q(p[0]), plane_q(p[1]), plane_q(p[2])};
    const int cc[3] = {(int)normal_cell(q[0], r_q), (int)normal_cell(q[1], r_q), (int)normal_cell(q[2], r_q)};
    normal_i64 s[NORMAL_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool full = false;
    for (int c = 0; c < 27 && !full; ++c) {
      const int nx = cc[0] + c % 3 - 1, ny = cc[1] + (c / 3) % 3 - 1, nz = cc[2] + c / 9 - 1;
      if (nx < 0 || ny < 0 || nz < 0 || nx > c_max || ny > c_max || nz > c_max) continue;
      const unsigned long long key = normal_key((unsigned)nx, (unsigned)ny, (unsigned)nz);
      auto it = std::lower_bound(cells.begin(), cells.end(), key, [](const Entry& e, unsigned long long k) { return e.key < k; });
      for (; it != cells.end() && it->key == key; ++it)
        if (normal_add(s, it->q[0] - q[0], it->q[1] - q[1], it->q[2] - q[2], r2) && s[0] > (normal_i64)max_nb) {
          full = true;
          break;
        }
    }
    int k = normal_count_class(s[0], min_nb, max_nb);
    if (k == NORMAL_OK) k = normal_solve(s, p[0], p[1], p[2], view.data(), nv, pf[1], &normals[i * 3], &curv[i]);
    counts[i] = (unsigned)s[0];
    cls[i] = (unsigned char)k;
    tally[k] += 1u;
    pairs += (uint64_t)s[0];
  }
  HarnessOut out(argv[2]);
  out.put(normals);
  out.put(curv);
  out.put(counts);
  out.put(cls);
  out.put(tally, NORMAL_CLASSES + 1);
  out.put(&pairs, 1);
  return out.finish();
}
