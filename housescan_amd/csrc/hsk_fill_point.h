// hsk_fill_point.h -- hole filling by volumetric diffusion (DESIGN.md 8p the rule, 3.22 the kernels; after Davis, Marschner, Garr
// and Levoy, "Filling holes in complex surfaces using volumetric diffusion", 3DPVT 2002): a voxel's state, one Jacobi step of a
// voxel from its own state and its six face neighbours', the crossing test of the keep rule and the word that is written.  Plain
// C++ with no HIP type in it: fill.hip compiles this text for the device, tests/fill_point_harness.cpp for the host, where it
// fills a volume sequentially and tests/test_fill_host.py compares it with the numpy twin (tests/fill_twin.py).  All integers.
//
// A STATE is one int16: FILL_UNKNOWN (-32768) or a KNOWN voxel's value in -32767..32767.  A source's value is its raw TSDF, a
// raw of -32768 counting as -32767, so a value never collides with the mark; a filled value is a mean of values and lies in
// their range.
#pragma once
#include "hsk_sample.h"

#define FILL_UNKNOWN (-32768)

// a SOURCE: an observed voxel.  (A deferred weight is never zero in the volume's own copy: the test needs no flush, 8j.)
HSK_HD bool fill_is_source(unsigned word) { return hsk_pair_wgt(word) != 0; }
HSK_HD int fill_source_value(unsigned word) {
  const int raw = hsk_pair_raw(word);
  return raw < -32767 ? -32767 : raw;
}
// the state a voxel starts with
HSK_HD int fill_initial(unsigned word) { return fill_is_source(word) ? fill_source_value(word) : FILL_UNKNOWN; }

// One Jacobi step of a non-source voxel inside the box (a VoxBox, hsk_comp_point.h): s[0] its own state, s[1..6] its face neighbours'
// (FILL_UNKNOWN for one outside the grid), all of the previous iteration.  With K the KNOWN ones among the seven, n = |K| and U the sum of
// value + 32768 over K: FILL_UNKNOWN when n = 0, else (2 U + n) div (2 n) - 32768 -- the mean, half rounded up.  (U <= 7 * 65535:
// no overflow.  Every term lies in 1..65535, so does the mean: the result is never FILL_UNKNOWN.)
HSK_HD int fill_step(const int s[7]) {
  unsigned n = 0u, U = 0u;
  for (int i = 0; i < 7; ++i) {
    const bool known = s[i] != FILL_UNKNOWN;
    n += known ? 1u : 0u;
    U += known ? (unsigned)(s[i] + 32768) : 0u;
  }
  if (n == 0u) return FILL_UNKNOWN;
  return (int)((2u * U + n) / (2u * n)) - 32768;
}

// a crossing, in the words of the cloud read-out (A.7): two face-adjacent KNOWN voxels, neither at 32767, one value > 0 and the
// other < 0
HSK_HD bool fill_usable(int s) { return s != FILL_UNKNOWN && s != 32767; }
HSK_HD bool fill_crossing(int a, int b) { return fill_usable(a) && fill_usable(b) && ((a > 0 && b < 0) || (a < 0 && b > 0)); }
// s[0] a voxel's final state, s[1..6] its face neighbours': the voxel is a crossing voxel
HSK_HD bool fill_crossing_voxel(const int s[7]) {
  bool c = false;
  for (int i = 1; i < 7; ++i) c = c || fill_crossing(s[0], s[i]);
  return c;
}

// the word of a written voxel
HSK_HD unsigned fill_word(int fill_weight, int value) { return ((unsigned)fill_weight << 16) | ((unsigned)value & 0xffffu); }
