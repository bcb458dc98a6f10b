// hsk_diff_point.h -- volume differencing (DESIGN.md 8q the rule, 3.23 the kernels): the class of a pair of words, the word that
// carries a class through the labelling of components.hip, the order of the records (hsk_comp_point.h's), the choice hsk_diff_at
// makes among a point's neighbours and membership of the adopt set.  Plain C++ with no HIP type in it: diff.hip compiles this
// text for the device, tests/diff_point_harness.cpp for the host, where it diffs and adopts sequentially and
// tests/test_diff_host.py compares it with the numpy twin (tests/diff_twin.py).  All integers.
#pragma once
#include "hsk_comp_point.h"

// the classes (include/hskinfu.h: HSK_DIFF_*; api_diff.hip asserts that they agree)
#define DIFF_UNSEEN 0
#define DIFF_ONLY_REF 1
#define DIFF_ONLY_CUR 2
#define DIFF_SAME 3
#define DIFF_APPEARED 4
#define DIFF_VANISHED 5
#define DIFF_MINOR 6
#define DIFF_CLASSES 7
// hsk_adopt_params.which
#define DIFF_ADOPT_APPEARED 1
#define DIFF_ADOPT_VANISHED 2

// a word's value: its raw TSDF, a raw of -32768 counting as -32767 (so the difference of two values lies in -65534..65534)
HSK_HD int diff_value(unsigned word) {
  const int raw = hsk_pair_raw(word);
  return raw < -32767 ? -32767 : raw;
}
HSK_HD bool diff_observed(unsigned word, int min_weight) { return hsk_pair_wgt(word) >= min_weight; }

// the class of a voxel from ref's word a and cur's word b, before the MINOR step
HSK_HD int diff_class(unsigned a, unsigned b, int thresh, int min_weight) {
  const bool oa = diff_observed(a, min_weight), ob = diff_observed(b, min_weight);
  const int d = diff_value(b) - diff_value(a);
  const int both = d <= -thresh ? DIFF_APPEARED : (d >= thresh ? DIFF_VANISHED : DIFF_SAME);
  return oa ? (ob ? both : DIFF_ONLY_REF) : (ob ? DIFF_ONLY_CUR : DIFF_UNSEEN);
}
HSK_HD bool diff_changed(int cls) { return cls == DIFF_APPEARED || cls == DIFF_VANISHED; }

// THE CLASS WORD.  The class volume is held as pair words in the volume's own layout, the class in the weight half, such that
// comp_inside(word) holds exactly for the CHANGED classes: they carry the raw -1, every other observed class 0x7fff, UNSEEN is
// word 0.  components.hip then labels the regions as it labels a volume's pieces, and its prune with the FREE fill -- the weight
// kept, the raw 0x7fff -- turns the voxels of a small region into words that still say APPEARED or VANISHED in their weight half
// and are no members any more: MINOR.
HSK_HD unsigned diff_class_word(int cls) {
  return cls == DIFF_UNSEEN ? 0u : (((unsigned)cls << 16) | (diff_changed(cls) ? 0xffffu : 0x7fffu));
}
HSK_HD int diff_word_class(unsigned word) {
  const int c = hsk_pair_wgt(word);
  return (c >= DIFF_APPEARED && hsk_pair_raw(word) >= 0) ? DIFF_MINOR : c;
}

// hsk_diff_at: of two candidates (squared distance in voxels, lin) the one that is taken
HSK_HD bool diff_at_before(unsigned d2_a, unsigned lin_a, unsigned d2_b, unsigned lin_b) { return d2_a != d2_b ? d2_a < d2_b : lin_a < lin_b; }
// The voxel hsk_diff_at reports for a point whose voxel (x, y, z) lies in the grid: among the voxels within Chebyshev `radius` of
// it whose class is APPEARED or VANISHED the one with the smallest (dx^2 + dy^2 + dz^2, lin); with none, the voxel itself.
// class_at(x, y, z) gives a voxel's final class.  *cls: the reported class; returns the lin of the reported voxel when it is a
// candidate (its region is that voxel's label), COMP_NONE otherwise.  (2 radius + 1)^3 trips: radius is at most 4.
template <class ClassAt>
HSK_HD unsigned diff_at_pick(const CompGrid& g, unsigned x, unsigned y, unsigned z, int radius, const ClassAt& class_at, int* cls) {
  unsigned best_d2 = 0xffffffffu, best_lin = COMP_NONE;
  int best_cls = class_at(x, y, z);
  for (int dz = -radius; dz <= radius; ++dz)
    for (int dy = -radius; dy <= radius; ++dy)
      for (int dx = -radius; dx <= radius; ++dx) {
        const unsigned xx = x + (unsigned)dx, yy = y + (unsigned)dy, zz = z + (unsigned)dz;  // (below 0 wraps to a large number)
        if (xx >= g.X || yy >= g.Y || zz >= g.Z) continue;
        const int c = class_at(xx, yy, zz);
        if (!diff_changed(c)) continue;
        const unsigned d2 = (unsigned)(dx * dx + dy * dy + dz * dz), l = g.lin(xx, yy, zz);
        if (best_lin == COMP_NONE || diff_at_before(d2, l, best_d2, best_lin)) {
          best_d2 = d2;
          best_lin = l;
          best_cls = c;
        }
      }
  *cls = best_cls;
  return best_lin;
}

// the adopt set: a target is a voxel of a kept region (its final class is APPEARED or VANISHED) whose class `which` selects; a
// voxel within the halo of a target is adopted iff cur's word there has a weight other than 0
HSK_HD bool diff_adopt_target(int cls, int which) {
  return (cls == DIFF_APPEARED && (which & DIFF_ADOPT_APPEARED) != 0) || (cls == DIFF_VANISHED && (which & DIFF_ADOPT_VANISHED) != 0);
}
HSK_HD bool diff_adopts(bool in_halo, unsigned cur_word) { return in_halo && hsk_pair_wgt(cur_word) != 0; }
