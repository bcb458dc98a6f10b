// diff_point_harness.cpp -- the diff kernels' shared text (housescan_amd/csrc/hsk_diff_point.h: the class of a word pair, the class
// word, the hsk_diff_at choice, membership of the adopt set; hsk_comp_point.h: the union-find and the record order), compiled for
// the host: it diffs two volumes sequentially the way the kernels do -- class words, a labelling of the words comp_inside accepts,
// the MINOR step as prune's FREE fill -- and adopts with a literal dilation; tests/test_diff_host.py compares everything with the
// numpy twin (tests/diff_twin.py).  Input file: 12 int32 -- dims (3), thresh, min_weight, min_voxels, which, halo, ref has colour,
// cur has colour, radius, the number of query voxels --, then ref's and cur's words in the device's block layout, then (where
// present) ref's and cur's colour words, row-major, then the query voxels (3 int32 each).  Output file: the class bytes and the
// labels (X Y Z each, row-major), 2 uint64 (kept regions, minor regions), the records (hsk_diff_region), per query voxel a class
// byte then a label (uint32), ref's words after the adopt (X Y Z uint32, row-major), its colour words (when it has colour), then
// 3 uint64: n_targets, n_adopted, n_colored.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../housescan_amd/csrc/hsk_diff_point.h"
#include "../include/hskinfu.h"
#include "harness_io.h"

struct ClassAt {
  const std::vector<unsigned>* words;
  CompGrid g;
  int operator()(unsigned x, unsigned y, unsigned z) const { return diff_word_class((*words)[g.at_xyz(x, y, z)]); }
};

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int h[12];
  if (!in.get(h, 12)) return 2;
  const CompGrid g{(unsigned)h[0], (unsigned)h[1], (unsigned)h[2]};
  const int thresh = h[3], min_weight = h[4], which = h[6], halo = h[7], radius = h[10];
  const unsigned min_voxels = (unsigned)h[5];
  const bool ref_col = h[8] != 0, cur_col = h[9] != 0;
  const size_t n_at = (size_t)h[11];
  const size_t words = volume_words(g.X, g.Y, g.Z), n = (size_t)g.X * g.Y * g.Z;
  std::vector<unsigned> ref(words), cur(words), ca(ref_col ? n : 0), cb(cur_col ? n : 0);
  std::vector<int> at(3 * n_at);
  if (!(in.get(ref) && in.get(cur) && in.get(ca) && in.get(cb) && in.get(at))) return 2;
  const unsigned X = g.X, Y = g.Y, Z = g.Z;
  // the class words and the labelling's initial parents
  std::vector<unsigned> cw(words, 0u), parent(words, COMP_NONE);
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z);
        cw[a] = diff_class_word(diff_class(ref[a], cur[a], thresh, min_weight));
        if (comp_inside(cw[a])) parent[a] = g.lin(x, y, z);
      }
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        if (!comp_inside(cw[g.at_xyz(x, y, z)])) continue;
        const unsigned l = g.lin(x, y, z);
        if (x > 0 && comp_inside(cw[g.at_xyz(x - 1, y, z)])) comp_unite<CompPlainOps>(parent.data(), g, l, g.lin(x - 1, y, z));
        if (y > 0 && comp_inside(cw[g.at_xyz(x, y - 1, z)])) comp_unite<CompPlainOps>(parent.data(), g, l, g.lin(x, y - 1, z));
        if (z > 0 && comp_inside(cw[g.at_xyz(x, y, z - 1)])) comp_unite<CompPlainOps>(parent.data(), g, l, g.lin(x, y, z - 1));
      }
  // flatten; the regions' records, indexed by root
  std::vector<unsigned> roots;
  std::vector<hsk_diff_region> all(n);
  memset(all.data(), 0, n * sizeof(hsk_diff_region));
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z);
        if (parent[a] == COMP_NONE) continue;
        const unsigned r = comp_find<CompPlainOps>(parent.data(), g, g.lin(x, y, z));
        parent[a] = r;
        hsk_diff_region& c = all[r];
        if (c.n_voxels == 0) {
          roots.push_back(r);
          unsigned rx, ry, rz;
          g.xyz(r, rx, ry, rz);
          c.root[0] = (int)rx, c.root[1] = (int)ry, c.root[2] = (int)rz;
          c.lo[0] = (int)X, c.lo[1] = (int)Y, c.lo[2] = (int)Z;
        }
        c.n_voxels += 1;
        (diff_word_class(cw[a]) == DIFF_APPEARED ? c.n_appeared : c.n_vanished) += 1;
        const int p[3] = {(int)x, (int)y, (int)z};
        for (int k = 0; k < 3; ++k) {
          c.lo[k] = std::min(c.lo[k], p[k]);
          c.hi[k] = std::max(c.hi[k], p[k] + 1);
        }
      }
  // the MINOR step: prune's FREE fill on the class words of the regions below min_voxels
  // (the records, the cut at min_voxels and their order are the library's own text)
  std::vector<hsk_diff_region> recs;
  const std::vector<unsigned> table = region_table(all, roots);
  const unsigned long long n_minor = comp_region_records(g, roots.data(), table.data(), roots.size(), min_voxels, &recs, [&](hsk_diff_region& c, size_t i) {
    c.n_appeared = all[roots[i]].n_appeared;
    c.n_vanished = all[roots[i]].n_vanished;
  });
  const unsigned long long n_kept = recs.size();
  std::vector<unsigned char> cls(n);
  std::vector<unsigned> region(n);
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z), l = g.lin(x, y, z);
        if (parent[a] != COMP_NONE && all[parent[a]].n_voxels < min_voxels) cw[a] = (cw[a] & 0xffff0000u) | 0x7fffu;
        const int c = diff_word_class(cw[a]);
        cls[l] = (unsigned char)c;
        region[l] = diff_changed(c) ? parent[a] : COMP_NONE;
      }
  // the point query, on voxels
  std::vector<unsigned char> at_cls(n_at);
  std::vector<unsigned> at_region(n_at);
  const ClassAt class_at{&cw, g};
  for (size_t e = 0; e < n_at; ++e) {
    int c = DIFF_UNSEEN;
    const unsigned l = diff_at_pick(g, (unsigned)at[3 * e], (unsigned)at[3 * e + 1], (unsigned)at[3 * e + 2], radius, class_at, &c);
    at_cls[e] = (unsigned char)c;
    at_region[e] = l == COMP_NONE ? COMP_NONE : parent[g.at(l)];
  }
  // adopt
  std::vector<unsigned char> target(n);
  unsigned long long st[3] = {0, 0, 0};
  for (size_t l = 0; l < n; ++l) {
    target[l] = diff_adopt_target(cls[l], which);
    st[0] += target[l];
  }
  std::vector<unsigned> out(n);
  const int iX = (int)X, iY = (int)Y, iZ = (int)Z;
  for (int z = 0; z < iZ; ++z)
    for (int y = 0; y < iY; ++y)
      for (int x = 0; x < iX; ++x) {
        const size_t a = g.at_xyz((unsigned)x, (unsigned)y, (unsigned)z), l = g.lin((unsigned)x, (unsigned)y, (unsigned)z);
        out[l] = ref[a];
        bool in_halo = false;
        for (int dz = -halo; dz <= halo && !in_halo; ++dz)
          for (int dy = -halo; dy <= halo && !in_halo; ++dy)
            for (int dx = -halo; dx <= halo && !in_halo; ++dx) {
              const int xx = x + dx, yy = y + dy, zz = z + dz;
              if (xx < 0 || yy < 0 || zz < 0 || xx >= iX || yy >= iY || zz >= iZ) continue;
              in_halo = target[g.lin((unsigned)xx, (unsigned)yy, (unsigned)zz)] != 0;
            }
        if (!diff_adopts(in_halo, cur[a])) continue;
        out[l] = cur[a];
        st[1] += 1;
        if (ref_col) ca[l] = cur_col ? cb[l] : 0u;
        st[2] += (ref_col && cur_col) ? 1 : 0;
      }
  HarnessOut o(argv[2]);
  const unsigned long long counts[2] = {n_kept, n_minor};
  o.put(cls.data(), n), o.put(region.data(), n), o.put(counts, 2), o.put(recs);
  o.put(at_cls.data(), n_at), o.put(at_region.data(), n_at), o.put(out.data(), n), o.put(ca), o.put(st, 3);
  return o.finish();
}
