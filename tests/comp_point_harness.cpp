// comp_point_harness.cpp -- the component kernels' shared text (housescan_amd/csrc/hsk_comp_point.h: the class of a word, lin and
// the place of a voxel's parent, find and unite), compiled for the host with the plain minimum: it labels a volume sequentially
// and tests/test_components_host.py compares labels and records with the numpy twin (tests/components_twin.py).  Input file:
// dims (3 int32), then the volume's words in the device's block layout.  Output file: the labels (X Y Z uint32, row-major, x
// fastest), the number of components (uint32), the records (hsk_component, 48 bytes each) in their order.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../housescan_amd/csrc/hsk_comp_point.h"
#include "../include/hskinfu.h"
#include "harness_io.h"

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int dims[3];
  if (!in.get(dims, 3)) return 2;
  const CompGrid g{(unsigned)dims[0], (unsigned)dims[1], (unsigned)dims[2]};
  const size_t words = volume_words(g.X, g.Y, g.Z);
  std::vector<unsigned> vol(words), parent(words, COMP_NONE);
  if (!in.get(vol)) return 2;
  for (unsigned z = 0; z < g.Z; ++z)
    for (unsigned y = 0; y < g.Y; ++y)
      for (unsigned x = 0; x < g.X; ++x)
        if (comp_inside(vol[g.at_xyz(x, y, z)])) parent[g.at_xyz(x, y, z)] = g.lin(x, y, z);
  for (unsigned z = 0; z < g.Z; ++z)
    for (unsigned y = 0; y < g.Y; ++y)
      for (unsigned x = 0; x < g.X; ++x) {
        if (parent[g.at_xyz(x, y, z)] == COMP_NONE) continue;
        const unsigned l = g.lin(x, y, z);
        if (x > 0 && parent[g.at_xyz(x - 1, y, z)] != COMP_NONE) comp_unite<CompPlainOps>(parent.data(), g, l, g.lin(x - 1, y, z));
        if (y > 0 && parent[g.at_xyz(x, y - 1, z)] != COMP_NONE) comp_unite<CompPlainOps>(parent.data(), g, l, g.lin(x, y - 1, z));
        if (z > 0 && parent[g.at_xyz(x, y, z - 1)] != COMP_NONE) comp_unite<CompPlainOps>(parent.data(), g, l, g.lin(x, y, z - 1));
      }
  std::vector<unsigned> labels((size_t)g.X * g.Y * g.Z), roots;
  for (unsigned l = 0; l < labels.size(); ++l) {
    labels[l] = parent[g.at(l)] == COMP_NONE ? COMP_NONE : comp_find<CompPlainOps>(parent.data(), g, l);
    if (labels[l] == l) roots.push_back(l);  // (ascending)
  }
  // the device's table, eight words a root (count, lo, hi); the records and their order are the library's own text
  std::vector<unsigned> table(roots.size() * 8, 0u);
  for (size_t i = 0; i < roots.size(); ++i)
    for (int a = 0; a < 3; ++a) table[i * 8 + 1 + a] = 0x7fffffffu;
  for (unsigned l = 0; l < labels.size(); ++l) {
    if (labels[l] == COMP_NONE) continue;
    const unsigned at = comp_search(roots.data(), (unsigned)roots.size(), labels[l]);
    if (at >= roots.size()) return 3;
    unsigned p[3];
    g.xyz(l, p[0], p[1], p[2]);
    unsigned* t8 = &table[(size_t)at * 8];
    t8[0] += 1;
    for (int a = 0; a < 3; ++a) {
      t8[1 + a] = std::min(t8[1 + a], p[a]);
      t8[4 + a] = std::max(t8[4 + a], p[a] + 1);
    }
  }
  std::vector<hsk_component> recs;
  comp_region_records(g, roots.data(), table.data(), roots.size(), 0, &recs, [](hsk_component&, size_t) {});
  HarnessOut o(argv[2]);
  const unsigned n = (unsigned)recs.size();
  o.put(labels), o.put(&n, 1), o.put(recs);
  return o.finish();
}
