// fill_point_harness.cpp -- the fill kernels' shared text (housescan_amd/csrc/hsk_fill_point.h: a voxel's initial state, one Jacobi
// step, the crossing test, the written word), compiled for the host: it fills a volume sequentially, every iteration over every
// voxel with no skip logic, and tests/test_fill_host.py compares states, words, mask and stats with the numpy twin
// (tests/fill_twin.py).  Input file: 13 int32 -- dims (3), iterations, keep, band, fill_weight, the box's lo (3) and hi (3) --,
// then the volume's words in the device's block layout.  Output file: the final states (X Y Z int16, row-major, x fastest), the
// mask (X Y Z bytes), the volume's words after the fill (X Y Z uint32, row-major), then 5 uint64: n_unseen, n_reached, n_written,
// n_written_negative, iterations_run.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../housescan_amd/csrc/hsk_comp_point.h"
#include "../housescan_amd/csrc/hsk_fill_point.h"
#include "../include/hskinfu.h"
#include "harness_io.h"

int main(int argc, char** argv) {
  HarnessIn in(argc, argv, 2);
  int h[13];
  if (!in.get(h, 13)) return 2;
  const CompGrid g{(unsigned)h[0], (unsigned)h[1], (unsigned)h[2]};
  const int iterations = h[3], keep = h[4], band = h[5], fill_weight = h[6];
  VoxBox box;
  for (int a = 0; a < 3; ++a) box.lo[a] = h[7 + a], box.hi[a] = h[10 + a];
  const size_t n = (size_t)g.X * g.Y * g.Z;
  std::vector<unsigned> vol(volume_words(g.X, g.Y, g.Z));
  if (!in.get(vol)) return 2;
  const int X = (int)g.X, Y = (int)g.Y, Z = (int)g.Z;
  std::vector<short> cur(n), nxt(n);
  std::vector<unsigned char> fr(n), cross(n, 0), mask(n, 0);
  unsigned long long st[5] = {0, 0, 0, 0, 0};
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const unsigned w = vol[g.at_xyz((unsigned)x, (unsigned)y, (unsigned)z)];
        const size_t l = g.lin((unsigned)x, (unsigned)y, (unsigned)z);
        cur[l] = (short)fill_initial(w);
        fr[l] = !fill_is_source(w) && vox_in_box(box, x, y, z);
        st[0] += fr[l];
      }
  // a voxel's state and its six face neighbours', FILL_UNKNOWN outside the grid
  auto seven = [&](const std::vector<short>& s, int x, int y, int z, int out[7]) {
    auto at = [&](int xx, int yy, int zz) {
      return (xx < 0 || yy < 0 || zz < 0 || xx >= X || yy >= Y || zz >= Z) ? FILL_UNKNOWN : (int)s[g.lin((unsigned)xx, (unsigned)yy, (unsigned)zz)];
    };
    out[0] = at(x, y, z), out[1] = at(x - 1, y, z), out[2] = at(x + 1, y, z), out[3] = at(x, y - 1, z), out[4] = at(x, y + 1, z);
    out[5] = at(x, y, z - 1), out[6] = at(x, y, z + 1);
  };
  st[4] = (unsigned long long)iterations;
  bool settled = false;
  for (int it = 1; it <= iterations; ++it) {
    size_t changed = 0;
    for (int z = 0; z < Z; ++z)
      for (int y = 0; y < Y; ++y)
        for (int x = 0; x < X; ++x) {
          const size_t l = g.lin((unsigned)x, (unsigned)y, (unsigned)z);
          nxt[l] = cur[l];
          if (!fr[l]) continue;
          int s7[7];
          seven(cur, x, y, z, s7);
          nxt[l] = (short)fill_step(s7);
          changed += nxt[l] != cur[l];
        }
    cur.swap(nxt);
    if (changed == 0 && !settled) {
      settled = true;
      st[4] = (unsigned long long)it;
    }
  }
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        int s7[7];
        seven(cur, x, y, z, s7);
        cross[g.lin((unsigned)x, (unsigned)y, (unsigned)z)] = fill_crossing_voxel(s7);
      }
  std::vector<unsigned> out(n);
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const size_t l = g.lin((unsigned)x, (unsigned)y, (unsigned)z);
        out[l] = vol[g.at_xyz((unsigned)x, (unsigned)y, (unsigned)z)];
        if (!fr[l] || cur[l] == FILL_UNKNOWN) continue;
        st[1] += 1;
        bool kept = keep == HSK_FILL_ALL;
        for (int dz = -band; dz <= band && !kept; ++dz)
          for (int dy = -band; dy <= band && !kept; ++dy)
            for (int dx = -band; dx <= band && !kept; ++dx) {
              const int xx = x + dx, yy = y + dy, zz = z + dz;
              if (xx < 0 || yy < 0 || zz < 0 || xx >= X || yy >= Y || zz >= Z) continue;
              kept = cross[g.lin((unsigned)xx, (unsigned)yy, (unsigned)zz)] != 0;
            }
        if (!kept) continue;
        mask[l] = 1;
        out[l] = fill_word(fill_weight, cur[l]);
        st[2] += 1;
        st[3] += cur[l] < 0;
      }
  HarnessOut o(argv[2]);
  o.put(cur), o.put(mask), o.put(out), o.put(st, 5);
  return o.finish();
}
