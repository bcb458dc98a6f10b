// split_point_harness.cpp -- the split kernels' shared text (housescan_amd/csrc/hsk_split_point.h: the gradient, the distance to a
// plane, the NEAR and ALIGNED tests, the choice among the planes, the class word, the contacts, the hsk_split_at choice, the
// removal's rule and plane word; hsk_comp_point.h: the union-find and the record order), compiled for the host: it splits a volume
// sequentially the way the kernels do -- class words, a labelling of the words comp_inside accepts, the MINOR step as prune's FREE
// fill -- and removes with a literal dilation; tests/test_split_host.py compares everything with the numpy twin
// (tests/split_twin.py).  Input file: 12 int32 -- dims (3), the number of planes, min_voxels, mode, halo, fill_weight, has colour,
// radius, the number of query voxels, the number of roots (-1: all kept) --, then 7 int64 (front, back, tauq, w[3], the floor plane)
// and a double (cos2), then per plane 8 int64 (Q[3], Qd, N[3], kind), then the volume's words in the device's block layout, then
// (where present) its colour words, row-major, then the query voxels (3 int32 each), then the roots (uint32).  Output file: the
// class bytes, the plane bytes and the labels (X Y Z each, row-major), 4 uint64 (kept objects, minor objects, edge voxels, voxels
// with G = 0), the records (hsk_object), per query voxel a class byte, then a plane byte, then a label (uint32), the words after
// the removal (X Y Z uint32, row-major), the colour words (when there is colour), then 5 uint64: hsk_remove_stats.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../housescan_amd/csrc/hsk_split_point.h"
#include "../include/hskinfu.h"
#include "harness_io.h"

struct WordAt {
  const std::vector<unsigned>* words;
  CompGrid g;
  unsigned operator()(unsigned x, unsigned y, unsigned z) const { return (*words)[g.at_xyz(x, y, z)]; }
};

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int h[12];
  long long r7[7];
  double cos2;
  if (!(in.get(h, 12) && in.get(r7, 7) && in.get(&cos2, 1))) return 2;
  const CompGrid g{(unsigned)h[0], (unsigned)h[1], (unsigned)h[2]};
  const int n_planes = h[3], mode = h[5], halo = h[6], fill_weight = h[7], radius = h[9];
  const unsigned min_voxels = (unsigned)h[4];
  const bool has_col = h[8] != 0;
  const size_t n_at = (size_t)h[10];
  const int n_roots_in = h[11];
  if (n_planes < 0 || n_planes > SPLIT_MAX_PLANES) return 2;
  SplitRule rule;
  memset(&rule, 0, sizeof(rule));
  rule.front = r7[0], rule.back = r7[1], rule.tauq = r7[2];
  rule.w[0] = (int)r7[3], rule.w[1] = (int)r7[4], rule.w[2] = (int)r7[5];
  rule.floor_plane = (int)r7[6];
  rule.cos2 = cos2;
  rule.n_planes = n_planes;
  std::vector<SplitPlaneQ> planes((size_t)n_planes);
  for (int k = 0; k < n_planes; ++k) {
    long long p8[8];
    if (!in.get(p8, 8)) return 2;
    SplitPlaneQ& p = planes[(size_t)k];
    for (int j = 0; j < 3; ++j) p.Q[j] = p8[j], p.N[j] = (int)p8[4 + j];
    p.Qd = p8[3];
    p.kind = (int)p8[7];
  }
  const size_t words = volume_words(g.X, g.Y, g.Z), n = (size_t)g.X * g.Y * g.Z;
  std::vector<unsigned> vol(words), col(has_col ? n : 0), roots_in(n_roots_in > 0 ? (size_t)n_roots_in : 0);
  std::vector<int> at(3 * n_at);
  if (!(in.get(vol) && in.get(col) && in.get(at) && in.get(roots_in))) return 2;
  const unsigned X = g.X, Y = g.Y, Z = g.Z;
  const WordAt vol_at{&vol, g};
  // the class words and the labelling's initial parents
  std::vector<unsigned> cw(words, 0u), parent(words, COMP_NONE);
  unsigned long long n_edge = 0, n_flat = 0;
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z);
        const unsigned w = vol[a];
        if (!comp_inside(w)) continue;
        const int gr[3] = {split_grad(x > 0 ? vol_at(x - 1, y, z) : 0u, w, x + 1 < X ? vol_at(x + 1, y, z) : 0u),
                           split_grad(y > 0 ? vol_at(x, y - 1, z) : 0u, w, y + 1 < Y ? vol_at(x, y + 1, z) : 0u),
                           split_grad(z > 0 ? vol_at(x, y, z - 1) : 0u, w, z + 1 < Z ? vol_at(x, y, z + 1) : 0u)};
        unsigned plane;
        bool edge, flat;
        const int c = split_classify(planes.data(), rule, x, y, z, gr, &plane, &edge, &flat);
        cw[a] = split_class_word(c, plane);
        n_edge += edge ? 1 : 0;
        n_flat += flat ? 1 : 0;
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
  // flatten; count and box per root
  std::vector<unsigned> roots;
  std::vector<hsk_object> all(n);
  memset(all.data(), 0, n * sizeof(hsk_object));
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z);
        if (parent[a] == COMP_NONE) continue;
        const unsigned r = comp_find<CompPlainOps>(parent.data(), g, g.lin(x, y, z));
        parent[a] = r;
        hsk_object& c = all[r];
        if (c.n_voxels == 0) {
          roots.push_back(r);
          unsigned rx, ry, rz;
          g.xyz(r, rx, ry, rz);
          c.root[0] = (int)rx, c.root[1] = (int)ry, c.root[2] = (int)rz;
          c.lo[0] = (int)X, c.lo[1] = (int)Y, c.lo[2] = (int)Z;
        }
        c.n_voxels += 1;
        const int p[3] = {(int)x, (int)y, (int)z};
        for (int k = 0; k < 3; ++k) {
          c.lo[k] = std::min(c.lo[k], p[k]);
          c.hi[k] = std::max(c.hi[k], p[k] + 1);
        }
      }
  // the MINOR step: prune's FREE fill on the class words of the objects below min_voxels; then the kept objects' records
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z);
        if (parent[a] != COMP_NONE && all[parent[a]].n_voxels < min_voxels) cw[a] = (cw[a] & 0xffff0000u) | 0x7fffu;
      }
  const WordAt class_at{&cw, g};
  std::vector<unsigned char> first(n, 1);
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z);
        if (!comp_inside(cw[a])) continue;
        hsk_object& c = all[parent[a]];
        c.sum[0] += x, c.sum[1] += y, c.sum[2] += z;
        unsigned kinds;
        unsigned long long mask;
        split_contacts(g, x, y, z, class_at, &kinds, &mask);
        for (int k = 0; k < 4; ++k) c.contact[k] += (kinds >> k) & 1u;
        c.plane_mask |= mask;
        if (rule.floor_plane >= 0) {
          const int ht = split_height(planes[(size_t)rule.floor_plane], x, y, z);
          if (first[parent[a]]) c.height_lo = c.height_hi = ht;
          c.height_lo = std::min(c.height_lo, ht);
          c.height_hi = std::max(c.height_hi, ht);
          first[parent[a]] = 0;
        }
      }
  // (the records, the cut at min_voxels and their order are the library's own text)
  std::vector<hsk_object> recs;
  const std::vector<unsigned> table = region_table(all, roots);
  const unsigned long long n_minor = comp_region_records(g, roots.data(), table.data(), roots.size(), min_voxels, &recs, [&](hsk_object& c, size_t i) {
    const hsk_object& o = all[roots[i]];
    memcpy(c.sum, o.sum, sizeof(c.sum));
    memcpy(c.contact, o.contact, sizeof(c.contact));
    c.plane_mask = o.plane_mask;
    c.height_lo = o.height_lo;
    c.height_hi = o.height_hi;
  });
  std::vector<unsigned char> cls(n), pln(n);
  std::vector<unsigned> label(n);
  for (unsigned z = 0; z < Z; ++z)
    for (unsigned y = 0; y < Y; ++y)
      for (unsigned x = 0; x < X; ++x) {
        const size_t a = g.at_xyz(x, y, z), l = g.lin(x, y, z);
        cls[l] = (unsigned char)split_word_class(cw[a]);
        pln[l] = (unsigned char)split_word_plane(cw[a]);
        label[l] = comp_inside(cw[a]) ? parent[a] : COMP_NONE;
      }
  // the point query, on voxels
  std::vector<unsigned char> at_cls(n_at), at_pln(n_at);
  std::vector<unsigned> at_obj(n_at);
  for (size_t e = 0; e < n_at; ++e) {
    const unsigned l = split_at_pick(g, (unsigned)at[3 * e], (unsigned)at[3 * e + 1], (unsigned)at[3 * e + 2], radius, class_at);
    const unsigned w = l == COMP_NONE ? 0u : cw[g.at(l)];
    at_cls[e] = (unsigned char)split_word_class(w);
    at_pln[e] = (unsigned char)split_word_plane(w);
    at_obj[e] = (l != COMP_NONE && comp_inside(w)) ? parent[g.at(l)] : COMP_NONE;
  }
  // the removal
  std::vector<SplitSelected> sel;
  const int dims[3] = {(int)X, (int)Y, (int)Z};
  auto take = [&](const hsk_object& c) {
    SplitSelected e;
    memset(&e, 0, sizeof(e));
    e.plane_mask = c.plane_mask;
    e.root = g.lin((unsigned)c.root[0], (unsigned)c.root[1], (unsigned)c.root[2]);
    for (const SplitSelected& o : sel)
      if (o.root == e.root) return;
    for (int a = 0; a < 3; ++a) {
      e.lo[a] = std::max(c.lo[a] - halo, 0);
      e.hi[a] = std::min(c.hi[a] + halo, dims[a]);
    }
    sel.push_back(e);
  };
  if (n_roots_in < 0) {
    for (const hsk_object& c : recs) take(c);
  } else {
    for (unsigned r : roots_in) {
      if (r >= n || all[r].n_voxels < min_voxels || all[r].n_voxels == 0) return 3;
      take(all[r]);
    }
  }
  std::vector<unsigned char> target(n, 0);
  unsigned long long st[5] = {sel.size(), 0, 0, 0, 0};
  for (size_t l = 0; l < n; ++l) {
    if (label[l] == COMP_NONE) continue;
    for (const SplitSelected& o : sel) target[l] |= o.root == label[l] ? 1 : 0;
    st[1] += target[l];
  }
  std::vector<unsigned> out(n);
  const int iX = (int)X, iY = (int)Y, iZ = (int)Z;
  for (int z = 0; z < iZ; ++z)
    for (int y = 0; y < iY; ++y)
      for (int x = 0; x < iX; ++x) {
        const size_t a = g.at_xyz((unsigned)x, (unsigned)y, (unsigned)z), l = g.lin((unsigned)x, (unsigned)y, (unsigned)z);
        out[l] = vol[a];
        bool in_halo = false;
        for (int dz = -halo; dz <= halo && !in_halo; ++dz)
          for (int dy = -halo; dy <= halo && !in_halo; ++dy)
            for (int dx = -halo; dx <= halo && !in_halo; ++dx) {
              const int xx = x + dx, yy = y + dy, zz = z + dz;
              if (xx < 0 || yy < 0 || zz < 0 || xx >= iX || yy >= iY || zz >= iZ) continue;
              in_halo = target[g.lin((unsigned)xx, (unsigned)yy, (unsigned)zz)] != 0;
            }
        unsigned long long A = 0;
        const bool in_box = split_boxes_at(sel.data(), (unsigned)sel.size(), x, y, z, &A);
        const int act = split_remove_rule(mode, in_box, A, in_halo, target[l] != 0, vol[a]);
        if (act == 0) continue;
        out[l] = act == 1 ? split_plane_word(planes.data(), rule, A, (unsigned)x, (unsigned)y, (unsigned)z, fill_weight) : 0u;
        st[2] += 1;
        st[3] += out[l] != 0u ? 1 : 0;
        if (has_col) col[l] = 0u;
        st[4] += has_col ? 1 : 0;
      }
  HarnessOut o(argv[2]);
  const unsigned long long counts[4] = {recs.size(), n_minor, n_edge, n_flat};
  o.put(cls.data(), n), o.put(pln.data(), n), o.put(label.data(), n), o.put(counts, 4), o.put(recs);
  o.put(at_cls.data(), n_at), o.put(at_pln.data(), n_at), o.put(at_obj.data(), n_at), o.put(out.data(), n), o.put(col), o.put(st, 5);
  return o.finish();
}
