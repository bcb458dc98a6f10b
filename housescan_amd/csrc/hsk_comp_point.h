// hsk_comp_point.h -- surface components (DESIGN.md 8j the rule, 3.16 the kernels): the class of a pair word, a voxel's number
// lin(x, y, z) = (z Y + y) X + x and where its parent lives, and the union-find every kernel of components.hip runs -- `find`
// and `unite` over an array of parents.  Plain C++ with no HIP type in it: the atomic minimum and the load are a template
// argument, so tests/comp_point_harness.cpp compiles the same text for the host with a plain minimum and labels a volume
// sequentially, and tests/test_components_host.py compares it with the numpy twin (tests/components_twin.py).  The kernels' two
// sets of atomic operations stand beside the sequential ones, for the device compiler alone.  Last comes the host's half of the
// records (comp_region_records): the library and the harnesses of the labelling, the diff and the split all run that one text.
//
// THE INVARIANT every loop below rests on: parent[v] <= v, always, for every v that is a member.  An entry starts as v, and is
// only ever lowered (an atomic minimum with a smaller member of the same component).  So a walk v -> parent[v] -> ... is
// strictly decreasing until it meets an entry that names itself, and it ends after at most v steps whatever other threads do
// meanwhile.  No thread ever waits for another.
#pragma once
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hsk_sample.h"
#if defined(__HIPCC__)
#define HSK_HD_MEMBER __host__ __device__ __forceinline__
#else
#define HSK_HD_MEMBER inline
#endif

#define COMP_NONE 0xffffffffu  // the label of a voxel that is no member

// INSIDE: observed, with a negative TSDF -- the voxels that can be the negative end of a zero crossing.  (Not 8i's SOLID, which
// also takes raw == 0.)
HSK_HD bool comp_inside(unsigned word) { return hsk_pair_wgt(word) != 0 && hsk_pair_raw(word) < 0; }

// the grid of a whole volume; Z = vol_z, the padding planes of the last plane group are no voxels
struct CompGrid {
  unsigned X, Y, Z;
  // where the parent of voxel `lin` lives: the voxel's own word index in the block layout (hsk_dev.h: hsk_vox_index)
  HSK_HD_MEMBER size_t at_xyz(unsigned x, unsigned y, unsigned z) const {
    const size_t pitch = (size_t)(X >> 2) << 4;
    return ((size_t)(z >> 2) * Y * pitch + ((size_t)(z & 3u) << 2)) + (size_t)y * pitch + (((size_t)(x >> 2) << 4) + (x & 3u));
  }
  HSK_HD_MEMBER unsigned lin(unsigned x, unsigned y, unsigned z) const { return (z * Y + y) * X + x; }
  HSK_HD_MEMBER void xyz(unsigned l, unsigned& x, unsigned& y, unsigned& z) const {
    const unsigned r = l / X;
    x = l - r * X;
    z = r / Y;
    y = r - z * Y;
  }
  HSK_HD_MEMBER size_t at(unsigned l) const {
    unsigned x, y, z;
    xyz(l, x, y, z);
    return at_xyz(x, y, z);
  }
};
// the voxels lo <= (x, y, z) < hi of such a grid
struct VoxBox {
  int lo[3], hi[3];
};
HSK_HD VoxBox vox_box(const int lo[3], const int hi[3]) { return VoxBox{{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}}; }
HSK_HD bool vox_in_box(const VoxBox& b, int x, int y, int z) {
  return x >= b.lo[0] && x < b.hi[0] && y >= b.lo[1] && y < b.hi[1] && z >= b.lo[2] && z < b.hi[2];
}
// a table indexed by the label itself (a tile's labels in LDS)
struct CompDirect {
  HSK_HD_MEMBER size_t at(unsigned l) const { return (size_t)l; }
};

// the sequential operations (the host harness; a kernel passes its own: an atomic load and an atomic minimum)
struct CompPlainOps {
  static inline unsigned load(const unsigned* p) { return *p; }
  static inline unsigned fetch_min(unsigned* p, unsigned v) {
    const unsigned old = *p;
    if (v < old) *p = v;
    return old;
  }
};
#if defined(__HIPCC__)
// the kernels' operations (components.hip, partition.hip): a relaxed load that other workgroups' atomics are seen by (it passes the
// CU's L1), and the hardware's integer minimum; in LDS the same at workgroup scope
struct CompGlobalOps {
  static __device__ __forceinline__ unsigned load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ unsigned fetch_min(unsigned* p, unsigned v) { return atomicMin(p, v); }
};
struct CompLdsOps {
  static __device__ __forceinline__ unsigned load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ unsigned fetch_min(unsigned* p, unsigned v) { return atomicMin(p, v); }
};
#endif

// the root of member v.  Terminates: parent[u] <= u (the invariant above), so u strictly decreases until parent[u] == u.
template <class Ops, class Map>
HSK_HD unsigned comp_find(const unsigned* parent, const Map& m, unsigned v) {
  for (;;) {
    const unsigned p = Ops::load(parent + m.at(v));
    if (p >= v) return v;  // (== v: a root.  > v cannot be; taking it as the end keeps the walk finite whatever the memory holds)
    v = p;
  }
}

// a and b, members, become one component.  Each trip finds both roots; when they differ the larger root's entry is lowered to
// the smaller by an atomic minimum.  The value the minimum returns says what the entry really held: the root itself -- linked,
// done -- or something smaller, another thread's link made meanwhile; then that value and the smaller root are still to be
// united (whether the minimum replaced it or not), and the trip is repeated with them.
// Terminates: with a > b the trip's roots, the next trip's are find(old) <= old < a and find(b) <= b < a: the larger of the
// pair strictly decreases from trip to trip, and every find inside ends by the invariant.  No trip waits for anyone.
template <class Ops, class Map>
HSK_HD void comp_unite(unsigned* parent, const Map& m, unsigned a, unsigned b) {
  for (;;) {
    a = comp_find<Ops>(parent, m, a);
    b = comp_find<Ops>(parent, m, b);
    if (a == b) return;
    if (a < b) {
      const unsigned t = a;
      a = b;
      b = t;
    }
    const unsigned old = Ops::fetch_min(parent + m.at(a), b);
    if (old == a) return;
    a = old;
  }
}

// the index of `root` in the ascending list roots[0, n), or n when it is not there.  Terminates: hi - lo at least halves a trip.
HSK_HD unsigned comp_search(const unsigned* roots, unsigned n, unsigned root) {
  unsigned lo = 0u, hi = n;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (roots[mid] < root) lo = mid + 1u;
    else hi = mid;
  }
  return (lo < n && roots[lo] == root) ? lo : n;
}

// the order of the records: more voxels first, ties to the smaller root
HSK_HD bool comp_record_before(unsigned long long n_a, unsigned root_a, unsigned long long n_b, unsigned root_b) {
  return n_a != n_b ? n_a > n_b : root_a < root_b;
}

// The ABI's records of n labelled regions (host only; hsk_component, hsk_diff_region and hsk_object all have root, n_voxels, lo
// and hi), from the ascending roots and the table's eight words a region (count, lo[3], hi[3], one unused): a zeroed record with
// those four members for every region of at least min_voxels, handed to extra(record, the region's index) for what else it
// holds, then all of them in comp_record_before's order.  Returns the regions below min_voxels.
template <class Rec, class Extra>
size_t comp_region_records(const CompGrid& g, const unsigned* roots, const unsigned* table, size_t n, unsigned long long min_voxels, std::vector<Rec>* recs,
                           Extra extra) {
  size_t n_below = 0;
  recs->clear();
  for (size_t i = 0; i < n; ++i) {
    const unsigned* t8 = table + i * 8;
    if ((unsigned long long)t8[0] < min_voxels) {
      n_below += 1;
      continue;
    }
    Rec c;
    memset(&c, 0, sizeof(c));
    unsigned p[3];
    g.xyz(roots[i], p[0], p[1], p[2]);
    c.n_voxels = t8[0];
    for (int a = 0; a < 3; ++a) {
      c.root[a] = (int)p[a];
      c.lo[a] = (int)t8[1 + a];
      c.hi[a] = (int)t8[4 + a];
    }
    extra(c, i);
    recs->push_back(c);
  }
  auto lin_of = [&](const Rec& c) { return g.lin((unsigned)c.root[0], (unsigned)c.root[1], (unsigned)c.root[2]); };
  std::sort(recs->begin(), recs->end(), [&](const Rec& a, const Rec& c) { return comp_record_before(a.n_voxels, lin_of(a), c.n_voxels, lin_of(c)); });
  return n_below;
}
