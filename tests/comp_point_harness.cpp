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
  std::vector<hsk_component> recs(roots.size());
  for (size_t i = 0; i < roots.size(); ++i) {
    unsigned x, y, z;
    g.xyz(roots[i], x, y, z);
    hsk_component c = {};
    c.root[0] = (int)x, c.root[1] = (int)y, c.root[2] = (int)z;
    for (int a = 0; a < 3; ++a) c.lo[a] = 0x7fffffff;
    recs[i] = c;
  }
  for (unsigned l = 0; l < labels.size(); ++l) {
    if (labels[l] == COMP_NONE) continue;
    const unsigned at = comp_search(roots.data(), (unsigned)roots.size(), labels[l]);
    if (at >= roots.size()) return 3;
    unsigned p[3];
    g.xyz(l, p[0], p[1], p[2]);
    hsk_component& c = recs[at];
    c.n_voxels += 1;
    for (int a = 0; a < 3; ++a) {
      c.lo[a] = std::min(c.lo[a], (int)p[a]);
      c.hi[a] = std::max(c.hi[a], (int)p[a] + 1);
    }
  }
  std::sort(recs.begin(), recs.end(), [&](const hsk_component& a, const hsk_component& b) {
    return comp_record_before(a.n_voxels, g.lin((unsigned)a.root[0], (unsigned)a.root[1], (unsigned)a.root[2]), b.n_voxels,
                              g.lin((unsigned)b.root[0], (unsigned)b.root[1], (unsigned)b.root[2]));
  });
  HarnessOut o(argv[2]);
  const unsigned n = (unsigned)recs.size();
  o.put(labels), o.put(&n, 1), o.put(recs);
  return o.finish();
}
