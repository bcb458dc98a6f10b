// color.hip -- the colour volume of an RGB-D scan (opt-in: hsk_enable_color) for gfx950.  One (r, g, b, w) byte quadruple
// per stored voxel, in a layout of its own: plain row-major, x fastest, word index (zz * Y + y) * X + x -- the host's layout
// too (hsk_download_color / hsk_upload_color copy it as it is), and independent of the TSDF's 64-B blocks.
//
// The rule (DESIGN.md "Colour"): voxel (x, y, z) is projected with the integrate's own arithmetic (tests/np_twin.py:
// _integrate -- the same expressions, association order, `front` test, rounding to a pixel (u, v) and scaled depth D_s); it
// takes the pixel's colour iff the pixel is in the image, D_s(u, v) != 0 and -band < sdf < band (sdf = D_s - dist, f32), as
//     c' = (c w + p + ((w + 1) >> 1)) / (w + 1)   (integers, truncating),   w' = min(w + 1, max_weight)
// The band is at most tau, so every voxel coloured is one the integrate has just updated.
//
// Cost: a wave takes a chunk of 16 x 16 voxels x 16 planes and first asks of the chunk's box, against the frame's 16-px tile
// table, whether any voxel in it can satisfy |sdf| < band (the box test of the integrate's coarse level, with the colour band
// for tau); almost every chunk of a scan cannot, and leaves after some 100 instructions.  Only chunks near the surface are
// swept voxel by voxel.  The test is conservative: the result is that of the full sweep (tests/test_gpu_color.py).
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_launch.h"

#define HSK_CCHUNK 16       // edge of a wave's chunk, in voxels (x, y and stored planes)
#define HSK_CSPARSE_LEVELS 4  // levels per axis of the 16-px sparse tile table (integrate.hip: HSK_SPARSE_LEVELS)

__global__ __launch_bounds__(256) void k_color_integrate(const TrackState* __restrict__ st, const int* __restrict__ has_color,
                                                         const float* __restrict__ scaled, const unsigned char* __restrict__ rgb,
                                                         const float2* __restrict__ sparse, unsigned* __restrict__ col, VolParams vp,
                                                         int W, int H, Intr in, float band, int max_w) {
  // a lost frame (or one dropped in flight behind it) integrates nothing and colours nothing; a depth-only frame colours nothing
  if (st->lost || *has_color == 0) return;
  const int cxn = (vp.X + HSK_CCHUNK - 1) / HSK_CCHUNK, cyn = (vp.Y + HSK_CCHUNK - 1) / HSK_CCHUNK;
  const int czn = (vp.nzs + HSK_CCHUNK - 1) / HSK_CCHUNK;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  if (wave >= cxn * cyn * czn) return;
  const int lane = threadIdx.x & 63;
  const int cxi = wave % cxn, cyi = (wave / cxn) % cyn, czi = wave / (cxn * cyn);
  const int xa = cxi * HSK_CCHUNK, ya = cyi * HSK_CCHUNK, za = czi * HSK_CCHUNK;  // (za: a stored plane)
  const int xb = min(xa + HSK_CCHUNK - 1, vp.X - 1), yb = min(ya + HSK_CCHUNK - 1, vp.Y - 1), zb = min(za + HSK_CCHUNK - 1, vp.nzs - 1);
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = st->R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = st->t[i];
  // ---- the chunk's box.  gx, gy, gz are monotone in x, y, z, so the voxel centres' offsets from the camera fill the box of
  // the two extreme centres; camera z is affine in them (its extremes sit at corners), and with every corner well in front the
  // pixels of all voxels lie in the box of the corners' pixels (+-1 px: the rounding to a pixel and float error).
  {
    const float g0[3] = {((float)xa + 0.5f) * vp.cell[0] - t[0], ((float)ya + 0.5f) * vp.cell[1] - t[1],
                         ((float)(vp.zs0 + za) + 0.5f) * vp.cell[2] - t[2]};
    const float g1[3] = {((float)xb + 0.5f) * vp.cell[0] - t[0], ((float)yb + 0.5f) * vp.cell[1] - t[1],
                         ((float)(vp.zs0 + zb) + 0.5f) * vp.cell[2] - t[2]};
    float umin = 1e30f, umax = -1e30f, vmin = 1e30f, vmax = -1e30f, zmn = 1e30f, zmx = -1e30f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float gx = (c & 1) ? g1[0] : g0[0], gy = (c & 2) ? g1[1] : g0[1], gz = (c & 4) ? g1[2] : g0[2];
      const float cxm = (R[0] * gx + R[3] * gy) + R[6] * gz, cym = (R[1] * gx + R[4] * gy) + R[7] * gz;
      const float czm = (R[2] * gx + R[5] * gy) + R[8] * gz;
      const float rq = 1.0f / czm;
      const float uq = (cxm * in.fx) * rq + in.cx, vq = (cym * in.fy) * rq + in.cy;
      zmn = fminf(zmn, czm);
      zmx = fmaxf(zmx, czm);
      umin = fminf(umin, uq);
      umax = fmaxf(umax, uq);
      vmin = fminf(vmin, vq);
      vmax = fmaxf(vmax, vq);
    }
    if (zmx < -1.0e-3f) return;  // wholly behind the camera: no voxel passes `front`
    if (zmn > 0.05f) {
      umin -= 1.0f;
      vmin -= 1.0f;
      umax += 1.0f;
      vmax += 1.0f;
      if ((umax < 0.0f) | (vmax < 0.0f) | (umin > (float)(W - 1)) | (vmin > (float)(H - 1))) return;  // no voxel has a pixel
      const int tw = (W + 15) / 16, th = (H + 15) / 16;
      const int tu0 = (int)fminf(fmaxf(umin, 0.0f), (float)(W - 1)) >> 4, tu1 = (int)fminf(fmaxf(umax, 0.0f), (float)(W - 1)) >> 4;
      const int tv0 = (int)fminf(fmaxf(vmin, 0.0f), (float)(H - 1)) >> 4, tv1 = (int)fminf(fmaxf(vmax, 0.0f), (float)(H - 1)) >> 4;
      const int nx = tu1 - tu0 + 1, ny = tv1 - tv0 + 1;
      if ((nx <= (2 << (HSK_CSPARSE_LEVELS - 1))) & (ny <= (2 << (HSK_CSPARSE_LEVELS - 1)))) {
        // (the four blocks of 2^kx x 2^ky tiles in the range's corners cover it: k_tile_tables)
        const int kx = min(31 - __clz(nx), HSK_CSPARSE_LEVELS - 1), ky = min(31 - __clz(ny), HSK_CSPARSE_LEVELS - 1);
        const float2* __restrict__ lv = sparse + (size_t)(ky * HSK_CSPARSE_LEVELS + kx) * tw * th;
        const int ub = tu1 - (1 << kx) + 1, vb = tv1 - (1 << ky) + 1;
        const float2 q00 = lv[tv0 * tw + tu0], q01 = lv[tv0 * tw + ub], q10 = lv[vb * tw + tu0], q11 = lv[vb * tw + ub];
        const float Dx = fmaxf(fmaxf(q00.x, q01.x), fmaxf(q10.x, q11.x));  // the largest depth under the box
        const float Dn = fminf(fminf(q00.y, q01.y), fminf(q10.y, q11.y));  // the smallest, 0 when a pixel has none
        float d_hi2 = 0.0f, d_lo2 = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float p0 = g0[a] * g0[a], p1 = g1[a] * g1[a];
          d_hi2 += fmaxf(p0, p1);
          d_lo2 += (g0[a] <= 0.0f && g1[a] >= 0.0f) ? 0.0f : fminf(p0, p1);
        }
        const float d_hi = sqrtf(d_hi2), d_lo = sqrtf(d_lo2);
        if (d_lo * 0.99999f - Dx > band) return;         // every voxel: sdf < -band
        if (d_hi * 1.00001f + band <= Dn) return;        // every voxel with a pixel: sdf >= band
      }
    }
  }
  // ---- the chunk voxel by voxel: a lane per x (16) and row of four (y), the planes in turn
  const int x = xa + (lane & 15);
  if (x > xb) return;
  const float gx = ((float)x + 0.5f) * vp.cell[0] - t[0];
  for (int y = ya + (lane >> 4); y <= yb; y += 4) {
    const float gy = ((float)y + 0.5f) * vp.cell[1] - t[1];
    const float ax = R[0] * gx + R[3] * gy, ay = R[1] * gx + R[4] * gy, az = R[2] * gx + R[5] * gy;
    const float pxy = gx * gx + gy * gy;
    for (int zz = za; zz <= zb; ++zz) {
      const float gz = ((float)(vp.zs0 + zz) + 0.5f) * vp.cell[2] - t[2];
      const float c0 = ax + R[6] * gz, c1 = ay + R[7] * gz, c2 = az + R[8] * gz;
      if (!(c2 >= 1.17549435e-38f)) continue;  // `front` (a denormal camera-space depth is not in front)
      const float inv_z = 1.0f / c2;
      const float fu = (c0 * in.fx) * inv_z + in.cx, fv = (c1 * in.fy) * inv_z + in.cy;
      int u, v;
      if (!hsk_rint_guard(fu, u) || !hsk_rint_guard(fv, v)) continue;
      if (u < 0 || v < 0 || u >= W || v >= H) continue;
      const float Ds = scaled[v * W + u];
      if (Ds == 0.0f) continue;
      const float dist = sqrtf(gz * gz + pxy);
      const float sdf = Ds - dist;
      if (!(sdf > -band && sdf < band)) continue;
      const size_t vi = ((size_t)zz * vp.Y + y) * vp.X + x;
      const size_t pi = ((size_t)v * W + u) * 3;
      const unsigned cw = col[vi];
      const int w = (int)(cw >> 24), w1 = w + 1, half = w1 >> 1;
      const int r = ((int)(cw & 255u) * w + (int)rgb[pi] + half) / w1;
      const int g = ((int)((cw >> 8) & 255u) * w + (int)rgb[pi + 1] + half) / w1;
      const int b = ((int)((cw >> 16) & 255u) * w + (int)rgb[pi + 2] + half) / w1;
      const int nw = w1 < max_w ? w1 : max_w;
      col[vi] = (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16) | ((unsigned)nw << 24);
    }
  }
}

// tiles: the frame's tile tables (hsk_dev.h: the sparse 16-px table sits behind the raw tables and the 8-px / 4-px forms)
void launch_color_integrate(hipStream_t s, unsigned* col, const TrackState* st, const int* has_color, const float* scaled,
                            const unsigned char* rgb, const float* tiles, const VolParams& vp, int W, int H, Intr in, float band,
                            int max_w) {
  const float2* sparse = (const float2*)(tiles + 4 * hsk_tiles_n16(W, H)) + (size_t)50 * hsk_tiles_n8(W, H);
  const long waves = (long)((vp.X + HSK_CCHUNK - 1) / HSK_CCHUNK) * ((vp.Y + HSK_CCHUNK - 1) / HSK_CCHUNK) *
                     ((vp.nzs + HSK_CCHUNK - 1) / HSK_CCHUNK);
  hipLaunchKernelGGL(k_color_integrate, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, st, has_color, scaled, rgb, sparse, col, vp,
                     W, H, in, band, max_w);
}
