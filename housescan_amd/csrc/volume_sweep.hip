// volume_sweep.hip -- the kernels the passes over a whole volume share, for gfx950 (hsk_vol_sweep.h is their
// vocabulary): neither decodes what it moves.
// k_mask_dilate: a row-major byte volume of zeros and ones dilated along one axis, a word of four bytes a thread; three launches,
// one an axis, make a Chebyshev ball (a product of three intervals).  hsk_fill_holes' keep rule (`band`) and hsk_adopt_diff's halo.
// k_box_rows<T>: a box of a row-major field, row-major.  hsk_download_clearance and hsk_download_reach (uint32),
// hsk_download_fill_mask (bytes).  A thread an element; speed does not matter there.
// Every index below is formed from a quad inside the grid or a voxel inside the box, which lies inside the grid: no access leaves
// the buffers.  No kernel waits on another workgroup; no loop's trip count depends on data.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_vol_sweep.h"

// dst = src dilated by r along one axis (0 x, 1 y, 2 z); bytes are 0 or 1
__global__ __launch_bounds__(256) void k_mask_dilate(const unsigned char* __restrict__ src, VolVectors q, int axis, int r, unsigned* __restrict__ dst) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  if (!vol_quad(q, i, x0, y, z)) return;
  unsigned m = 0u;
  if (axis == 0) {
    const unsigned char* __restrict__ row = src + (size_t)q.g.lin(0u, y, z);
    for (int d = -r; d <= r + 3; ++d) {  // (at most 20 trips: r <= 8)
      const unsigned x = x0 + (unsigned)d;
      if (x >= q.g.X || !row[x]) continue;
      // voxel x reaches x0 + j for |x - (x0 + j)| <= r, that is j in d - r .. d + r
#pragma unroll
      for (int j = 0; j < 4; ++j) m |= (j >= d - r && j <= d + r) ? 1u << (8 * j) : 0u;
    }
  } else {
    for (int d = -r; d <= r; ++d) {  // (at most 17 trips)
      const unsigned yy = axis == 1 ? y + (unsigned)d : y, zz = axis == 2 ? z + (unsigned)d : z;
      if (yy >= q.g.Y || zz >= q.g.Z) continue;
      m |= ((const unsigned*)src)[(size_t)q.g.lin(x0, yy, zz) >> 2];
    }
  }
  dst[i] = m;
}

// the box lo <= (x, y, z) < hi of a row-major field, row-major.  32-bit indices: a volume has at most 2^31 voxels (the calls' state
// check), so n <= 2^31, the last block's thread numbers stay below 2^31 + 256 and every lin below 2^31.
template <class T>
__global__ __launch_bounds__(256) void k_box_rows(const T* __restrict__ field, CompGrid g, VoxBox box, unsigned n, T* __restrict__ out) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  unsigned x, y, z;
  vol_box_voxel(box, e, x, y, z);
  out[e] = field[g.lin(x + (unsigned)box.lo[0], y + (unsigned)box.lo[1], z + (unsigned)box.lo[2])];
}

void launch_mask_dilate3(hipStream_t s, const VolParams& vp, unsigned char* a, unsigned char* b, int r) {
  const VolVectors q = vol_vectors(vp);
  const dim3 grid((vol_quads(q) + 255u) / 256u);
  hipLaunchKernelGGL(k_mask_dilate, grid, dim3(256), 0, s, (const unsigned char*)a, q, 0, r, (unsigned*)b);
  hipLaunchKernelGGL(k_mask_dilate, grid, dim3(256), 0, s, (const unsigned char*)b, q, 1, r, (unsigned*)a);
  hipLaunchKernelGGL(k_mask_dilate, grid, dim3(256), 0, s, (const unsigned char*)a, q, 2, r, (unsigned*)b);
}

void launch_box_rows(hipStream_t s, const void* field, size_t elem_bytes, const VolParams& vp, const int lo[3], const int hi[3], size_t n, void* out) {
  const CompGrid g = vol_vectors(vp).g;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (elem_bytes == 1)
    hipLaunchKernelGGL((k_box_rows<unsigned char>), grid, dim3(256), 0, s, (const unsigned char*)field, g, vox_box(lo, hi), (unsigned)n, (unsigned char*)out);
  else
    hipLaunchKernelGGL((k_box_rows<unsigned>), grid, dim3(256), 0, s, (const unsigned*)field, g, vox_box(lo, hi), (unsigned)n, (unsigned*)out);
}

int sweep_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_mask_dilate);
}
