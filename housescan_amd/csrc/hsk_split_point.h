// hsk_split_point.h -- the scene split (DESIGN.md 8r the rule, 3.24 the kernels): a voxel's gradient, its signed distance to a
// plane, the NEAR and ALIGNED tests, the choice among the planes, the word that carries a class (and a plane) through the labelling
// of components.hip, an object voxel's contacts, the choice hsk_split_at makes among a point's neighbours, and the removal's
// decision and plane word.  Plain C++ with no HIP type in it: split.hip compiles this text for the device,
// tests/split_point_harness.cpp for the host, where it splits and removes sequentially and tests/test_split_host.py compares it
// with the numpy twin (tests/split_twin.py).  Integers, and the three binary64 products of the ALIGNED test (no contraction).
//
// THE BOUNDS nothing below wraps within: |a_j| <= 2 and |d| <= 64 (the call's checks), and Q_j (2 i + 1) = a_j times the centre's
// coordinate times 2^30, a volume's extent being far below 2^10 m: |s| < 2^43.  |g_j| <= 131068 < 2^17, w_j <= 4096, so
// |G_j| < 2^29; |N_j| <= 8192: |dot| < 2^44, |G|^2 < 2^60, |N|^2 < 2^28.
#pragma once
#include "hsk_comp_point.h"

// the classes (include/hskinfu.h: HSK_SPLIT_*; 1..4 are the kinds HSK_KIND_*; api_split.hip asserts that they agree)
#define SPLIT_NONE 0
#define SPLIT_FLOOR 1
#define SPLIT_CEILING 2
#define SPLIT_WALL 3
#define SPLIT_OTHER 4
#define SPLIT_OBJECT 5
#define SPLIT_MINOR 6
#define SPLIT_CLASSES 7
#define SPLIT_NO_PLANE 0xffu
#define SPLIT_MAX_PLANES 64
#define SPLIT_MAX_SELECTED 256
#define SPLIT_REMOVE_ERASE 0
#define SPLIT_REMOVE_RESTORE 1

// a plane as the host converted it: Q_j = rint(a_j c_j 2^29), Qd = rint(d 2^30), N_j = rint(a_j 4096)
struct SplitPlaneQ {
  long long Q[3], Qd;
  int N[3], kind;
};
// the rest of the rule's numbers: front = rint(dist_m 2^30), back = rint(back_m 2^30), tauq = rint(tau 2^30), cos2 = cos_min^2 in
// binary64, w_j = rint(4096 c_min / c_j); floor_plane: the first plane of kind FLOOR, -1 when there is none
struct SplitRule {
  long long front, back, tauq;
  double cos2;
  int w[3];
  int n_planes, floor_plane, pad;
};

// a word's value: its raw TSDF, a raw of -32768 counting as -32767
HSK_HD int split_value(unsigned word) {
  const int raw = hsk_pair_raw(word);
  return raw < -32767 ? -32767 : raw;
}
HSK_HD bool split_observed(unsigned word) { return hsk_pair_wgt(word) != 0; }

// the gradient along one axis from the voxel's word and its two neighbours' (a neighbour outside the grid: word 0, unobserved)
HSK_HD int split_grad(unsigned lo, unsigned mid, unsigned hi) {
  const bool ol = split_observed(lo), oh = split_observed(hi);
  const int rl = split_value(lo), rm = split_value(mid), rh = split_value(hi);
  return ol ? (oh ? rh - rl : 2 * (rm - rl)) : (oh ? 2 * (rh - rm) : 0);
}

// the signed distance of voxel (x, y, z)'s centre to a plane, in units of 2^-30 m
HSK_HD long long split_s(const SplitPlaneQ& p, unsigned x, unsigned y, unsigned z) {
  return p.Q[0] * (long long)(2u * x + 1u) + p.Q[1] * (long long)(2u * y + 1u) + p.Q[2] * (long long)(2u * z + 1u) + p.Qd;
}
HSK_HD long long split_abs(long long v) { return v < 0 ? -v : v; }
HSK_HD bool split_near(long long s, const SplitRule& r) { return s >= -r.back && s <= r.front; }
// G = (g_j w_j), G2 = |G|^2
HSK_HD bool split_aligned(const long long G[3], long long G2, const SplitPlaneQ& p, double cos2) {
  if (G2 == 0) return true;
  const long long dot = G[0] * (long long)p.N[0] + G[1] * (long long)p.N[1] + G[2] * (long long)p.N[2];
  if (dot <= 0) return false;
  const long long N2 = (long long)p.N[0] * p.N[0] + (long long)p.N[1] * p.N[1] + (long long)p.N[2] * p.N[2];
  const double lhs = (double)dot * (double)dot;
  const double gn = (double)G2 * (double)N2;
  const double rhs = cos2 * gn;
  return lhs >= rhs;
}

// the choice among the planes: fed every plane in ascending k, so that of equal |s| the lower index stays
struct SplitPick {
  long long q_abs, m_abs;
  int q_k, m_k, m;
};
HSK_HD SplitPick split_pick_none() { return SplitPick{0, 0, -1, -1, 0}; }
HSK_HD void split_pick_feed(SplitPick& c, int k, long long s, bool near, bool aligned) {
  if (!near) return;
  const long long a = split_abs(s);
  c.m += 1;
  if (c.m_k < 0 || a < c.m_abs) {
    c.m_abs = a;
    c.m_k = k;
  }
  if (aligned && (c.q_k < 0 || a < c.q_abs)) {
    c.q_abs = a;
    c.q_k = k;
  }
}
// -> the plane (SPLIT_NO_PLANE: an OBJECT voxel); *edge: the edge rule decided
HSK_HD unsigned split_pick_plane(const SplitPick& c, bool* edge) {
  *edge = c.q_k < 0 && c.m >= 2;
  return c.q_k >= 0 ? (unsigned)c.q_k : (c.m >= 2 ? (unsigned)c.m_k : SPLIT_NO_PLANE);
}

// The class of an INSIDE voxel (x, y, z) with the gradient g (before the weights): walks all planes.  *plane: its plane or
// SPLIT_NO_PLANE; *edge, *no_normal: the stats' conditions.  n_planes trips.
HSK_HD int split_classify(const SplitPlaneQ* planes, const SplitRule& r, unsigned x, unsigned y, unsigned z, const int g[3], unsigned* plane, bool* edge,
                          bool* no_normal) {
  const long long G[3] = {(long long)g[0] * r.w[0], (long long)g[1] * r.w[1], (long long)g[2] * r.w[2]};
  const long long G2 = G[0] * G[0] + G[1] * G[1] + G[2] * G[2];
  SplitPick c = split_pick_none();
  for (int k = 0; k < r.n_planes; ++k) {
    const long long s = split_s(planes[k], x, y, z);
    const bool near = split_near(s, r);
    split_pick_feed(c, k, s, near, near && split_aligned(G, G2, planes[k], r.cos2));
  }
  *no_normal = G2 == 0;
  *plane = split_pick_plane(c, edge);
  return *plane == SPLIT_NO_PLANE ? SPLIT_OBJECT : planes[*plane].kind;
}

// THE CLASS WORD.  The class volume is held as pair words in the volume's own layout, the class in the weight half, such that
// comp_inside(word) holds exactly for OBJECT voxels: they carry the raw -1; a structure voxel carries its plane's index (0..63, not
// negative) in the raw half; NONE is word 0.  components.hip then labels the objects as it labels a volume's pieces, and its prune
// with the FREE fill -- the weight kept, the raw 0x7fff -- turns the voxels of a small object into words that still say OBJECT in
// their weight half and are no members any more: MINOR.
HSK_HD unsigned split_class_word(int cls, unsigned plane) {
  return cls == SPLIT_NONE ? 0u : (((unsigned)cls << 16) | (cls == SPLIT_OBJECT ? 0xffffu : plane));
}
HSK_HD int split_word_class(unsigned word) {
  const int c = hsk_pair_wgt(word);
  return (c == SPLIT_OBJECT && hsk_pair_raw(word) >= 0) ? SPLIT_MINOR : c;
}
HSK_HD unsigned split_word_plane(unsigned word) {
  const int c = hsk_pair_wgt(word);
  return (c >= SPLIT_FLOOR && c <= SPLIT_OTHER) ? (word & 0xffu) : SPLIT_NO_PLANE;
}

// an object voxel's contacts from a 6-neighbour's class word: bit kind - 1 of *kinds, bit plane of *planes
HSK_HD void split_contact(unsigned word, unsigned* kinds, unsigned long long* planes) {
  const int c = hsk_pair_wgt(word);
  if (c < SPLIT_FLOOR || c > SPLIT_OTHER) return;
  *kinds |= 1u << (c - 1);
  *planes |= 1ull << (word & 63u);
}
// ... over the six neighbours inside the grid; word_at(x, y, z) gives a voxel's class word
template <class WordAt>
HSK_HD void split_contacts(const CompGrid& g, unsigned x, unsigned y, unsigned z, const WordAt& word_at, unsigned* kinds, unsigned long long* planes) {
  *kinds = 0u;
  *planes = 0ull;
  if (x > 0u) split_contact(word_at(x - 1u, y, z), kinds, planes);
  if (x + 1u < g.X) split_contact(word_at(x + 1u, y, z), kinds, planes);
  if (y > 0u) split_contact(word_at(x, y - 1u, z), kinds, planes);
  if (y + 1u < g.Y) split_contact(word_at(x, y + 1u, z), kinds, planes);
  if (z > 0u) split_contact(word_at(x, y, z - 1u), kinds, planes);
  if (z + 1u < g.Z) split_contact(word_at(x, y, z + 1u), kinds, planes);
}
// the height of a voxel above the floor plane f in units of 2^-16 m (an arithmetic shift: the floor of the quotient)
HSK_HD int split_height(const SplitPlaneQ& f, unsigned x, unsigned y, unsigned z) {
  return (int)(split_s(f, x, y, z) >> 14);
}

// The voxel hsk_split_at reports for a point whose voxel (x, y, z) lies in the grid: among the voxels within Chebyshev `radius`
// of it whose class is not NONE the one with the smallest (dx^2 + dy^2 + dz^2, lin); COMP_NONE with none.  word_at(x, y, z) gives
// a voxel's class word.  (2 radius + 1)^3 trips: radius is at most 4.
template <class WordAt>
HSK_HD unsigned split_at_pick(const CompGrid& g, unsigned x, unsigned y, unsigned z, int radius, const WordAt& word_at) {
  unsigned best_d2 = 0xffffffffu, best_lin = COMP_NONE;
  for (int dz = -radius; dz <= radius; ++dz)
    for (int dy = -radius; dy <= radius; ++dy)
      for (int dx = -radius; dx <= radius; ++dx) {
        const unsigned xx = x + (unsigned)dx, yy = y + (unsigned)dy, zz = z + (unsigned)dz;  // (below 0 wraps to a large number)
        if (xx >= g.X || yy >= g.Y || zz >= g.Z) continue;
        if (split_word_class(word_at(xx, yy, zz)) == SPLIT_NONE) continue;
        const unsigned d2 = (unsigned)(dx * dx + dy * dy + dz * dz), l = g.lin(xx, yy, zz);
        if (best_lin == COMP_NONE || (d2 != best_d2 ? d2 < best_d2 : l < best_lin)) {
          best_d2 = d2;
          best_lin = l;
        }
      }
  return best_lin;
}

// ---- the removal -------------------------------------------------------------------------------------------------------------------
// a selected object: its label, its box grown by the halo and clipped, its plane mask
struct SplitSelected {
  unsigned long long plane_mask;
  unsigned root;
  int lo[3], hi[3];
  int pad;
};
// A(v) and "v lies in some grown box" over the n selected objects.  n trips.
HSK_HD bool split_boxes_at(const SplitSelected* sel, unsigned n, int x, int y, int z, unsigned long long* A) {
  bool in = false;
  unsigned long long a = 0ull;
  for (unsigned o = 0u; o < n; ++o) {
    const SplitSelected& e = sel[o];
    if (x < e.lo[0] || x >= e.hi[0] || y < e.lo[1] || y >= e.hi[1] || z < e.lo[2] || z >= e.hi[2]) continue;
    in = true;
    a |= e.plane_mask;
  }
  *A = a;
  return in;
}
// what happens to a voxel: 0 it stays, 1 it becomes the plane word P(v), 2 it becomes word 0
HSK_HD int split_remove_rule(int mode, bool in_box, unsigned long long A, bool in_halo, bool target, unsigned word) {
  if (mode == SPLIT_REMOVE_RESTORE && A != 0ull && in_box && (in_halo || !split_observed(word))) return 1;
  if (target || (in_halo && split_observed(word) && !comp_inside(word))) return 2;
  return 0;
}
HSK_HD long long split_floor_div(long long a, long long b) {  // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
// P(v): what an ideal scan of the planes of A holds at voxel (x, y, z).  At most 64 trips.
HSK_HD unsigned split_plane_word(const SplitPlaneQ* planes, const SplitRule& r, unsigned long long A, unsigned x, unsigned y, unsigned z, int fill_weight) {
  bool any = false;
  long long s = 0;
  for (int k = 0; k < r.n_planes; ++k) {
    if (!((A >> k) & 1ull)) continue;
    const long long sk = split_s(planes[k], x, y, z);
    if (!any || sk < s) s = sk;
    any = true;
  }
  if (!any || s < -r.tauq) return 0u;
  const long long sc = s < r.tauq ? s : r.tauq;
  const long long raw = split_floor_div(65534ll * sc + r.tauq, 2ll * r.tauq);
  return ((unsigned)fill_weight << 16) | ((unsigned)raw & 0xffffu);
}
