// hsk_vol_sweep.h -- the walk over a WHOLE volume in the block layout that components.hip, fill.hip, diff.hip and volume_sweep.hip
// share: the grid with its 16-B vectors and its 16 x 16 x 8 tiles, and what turns a thread's number into voxels --
// a vector of the block layout, a quad of a row-major byte volume, a tile, a voxel of a box.  The geometry has two levels so that
// a kernel that works on vectors alone carries no tile counts in its arguments.
#pragma once
#include "hsk_dev.h"
#include "hsk_comp_point.h"

// the grid and its 16-B vectors (four x-adjacent voxels): X4 a row, Zg plane groups, n4 in all (padding planes included)
struct VolVectors {
  CompGrid g;
  unsigned X4, Zg, n4;
};
// ... and its tiles of 16 x 16 x 8 voxels: 4 lane-blocks wide, 16 rows, two plane groups
struct VolTiles : VolVectors {
  unsigned ntx, nty, ntz;
};
static inline VolVectors vol_vectors(const VolParams& vp) {
  VolVectors q;
  q.g.X = (unsigned)vp.X;
  q.g.Y = (unsigned)vp.Y;
  q.g.Z = (unsigned)vp.Z;
  q.X4 = (unsigned)vp.X >> 2;
  q.Zg = ((unsigned)vp.Z + 3u) >> 2;
  q.n4 = q.X4 * q.g.Y * q.Zg * 4u;
  return q;
}
static inline VolTiles vol_tiles(const VolParams& vp) {
  VolTiles q;
  (VolVectors&)q = vol_vectors(vp);
  q.ntx = ((unsigned)vp.X + 15u) >> 4;
  q.nty = ((unsigned)vp.Y + 15u) >> 4;
  q.ntz = (q.Zg + 1u) >> 1;
  return q;
}

static __device__ __forceinline__ void vol_words(const uint4& v, unsigned w[4]) {
  w[0] = v.x;
  w[1] = v.y;
  w[2] = v.z;
  w[3] = v.w;
}
// vector i of the block layout -> its first voxel; false: no voxel (beyond the end, or a padding plane)
static __device__ __forceinline__ bool vol_vector(const VolVectors& q, unsigned i, unsigned& x0, unsigned& y, unsigned& z) {
  const unsigned pl = i & 3u, t = i >> 2, xb = t % q.X4, t2 = t / q.X4;
  y = t2 % q.g.Y;
  z = 4u * (t2 / q.g.Y) + pl;
  x0 = 4u * xb;
  return i < q.n4 && z < q.g.Z;
}
// quad i of a row-major byte volume (four x-adjacent voxels, one aligned word: X is a multiple of 4) -> its first voxel; false:
// beyond the end
static __device__ __forceinline__ bool vol_quad(const VolVectors& q, unsigned i, unsigned& x0, unsigned& y, unsigned& z) {
  const unsigned xb = i % q.X4, r = i / q.X4;
  x0 = 4u * xb;
  y = r % q.g.Y;
  z = r / q.g.Y;
  return z < q.g.Z;
}
static inline unsigned vol_quads(const VolVectors& q) { return q.X4 * q.g.Y * q.g.Z; }
static __device__ __forceinline__ void vol_tile(const VolTiles& q, unsigned tile, unsigned& tx, unsigned& ty, unsigned& tz) {
  const unsigned tr = tile / q.ntx;
  tx = tile % q.ntx;
  ty = tr % q.nty;
  tz = tr / q.nty;
}
// element e of a box (not empty), row-major -> its voxel, counted from the box's lo
static __device__ __forceinline__ void vol_box_voxel(const VoxBox& b, unsigned e, unsigned& x, unsigned& y, unsigned& z) {
  const unsigned bx = (unsigned)(b.hi[0] - b.lo[0]), by = (unsigned)(b.hi[1] - b.lo[1]);
  const unsigned r = e / bx;
  x = e - r * bx;
  z = r / by;
  y = r - z * by;
}
