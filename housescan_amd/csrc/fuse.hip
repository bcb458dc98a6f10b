// fuse.hip -- volume fusion for gfx950 (hsk_fuse_volume; DESIGN.md 3.10 the kernels, 8d the rule): one TSDF (+ colour) volume
// resampled through a rigid transform into another and merged by weight, on the device.
//
// The rule (tests/fuse_twin.py restates it in numpy): destination voxel (x, y, z) has the centre
// pd_i = ((float)i + 0.5f) * cell_d[i]; its source point is ps_i = ((A[i][0] pd_x + A[i][1] pd_y) + A[i][2] pd_z) + b[i], (A, b)
// the inverse of the rigid source -> destination matrix (hsk_invert_rigid).  Fs is the raycast's trilinear sample of the source
// at ps (the oracle's rc_trilinear: the same guards, cell choice, fractions and summation order), Ws the smallest weight of the
// same eight taps.  A NaN sample (the outer shell) or Ws == 0 (a tap never observed) leaves the voxel alone; otherwise
//     q = clamp((int)rintf(Fs * 32767), +-32767),  n = raw_d W_d + q Ws,  W = W_d + Ws,
//     raw' = sign(n) ((2 |n| + W) / (2 W))   (integers: rounded to nearest),   W' = min(W, HSK_MAX_WEIGHT)
// and, when both volumes carry colour, the colour of the source voxel that contains ps (weight w_s != 0) is merged per channel as
//     c' = (c_d w_d + c_s w_s + ((w_d + w_s) >> 1)) / (w_d + w_s),   w' = min(w_d + w_s, the destination's max_weight).
//
// Cost: a wave takes a chunk of 16 x 16 x 16 destination voxels of the footprint and first asks whether any voxel in it can
// take a sample: the chunk's eight corner centres are mapped into the source (the map is affine: the chunk's image lies in the
// hull of the corners' images), the box of the images is padded by the taps' reach and the float slack, and the chunk leaves
// when that box misses the source's interior or when no 8^3 brick of the source it touches holds an observed voxel -- a table
// of one bit per brick that a streaming pre-pass over the source builds (k_fuse_bricks) and the sweep stages in LDS.  Deep
// unobserved space is what most of a house volume sees of any one room.  The test is conservative: the result is that of the
// full sweep (tests/test_gpu_fuse.py compares against a twin that sweeps every voxel).
//
// A swept chunk: a lane takes a lane-block row -- 4 x-adjacent voxels of one plane, 16 B of the destination's 64-B block
// (hsk_dev.h: hsk_vox_index) -- reads it with one load, samples the source with eight 4-B gathers per voxel (both halves of the
// pair: the TSDF and the weight), and writes the 16 B back with one store if a voxel changed.  The colour volumes are row-major,
// so the same four voxels are 16 contiguous bytes there too.
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_launch.h"

#define HSK_FCHUNK 16  // edge of a wave's chunk, in destination voxels

// one bit per 8^3 brick of the source: "holds a voxel with a non-zero weight".  A thread takes one column of 16-B vectors (4
// x-adjacent voxels of one plane) through a brick layer: 8 rows (y) of the 2 plane groups a brick spans, 16 independent
// loads; a wave's load is 1 KiB contiguous.  Eight consecutive lanes hold the 8 x-voxels by 4 planes of a lane-block pair, so
// together they hold one whole brick and a byte of the wave's ballot is that brick: at most eight lanes of a wave touch the
// table, each once (a read, then an atomicOr if the bit is still clear: 32 bricks share a word) -- and none in unobserved space.
__global__ __launch_bounds__(256) void k_fuse_bricks(const uint4* __restrict__ vol, unsigned n_threads, int X, int Y, int n_groups,
                                                     int nbx, int nby, unsigned* __restrict__ tab) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  const unsigned c = t % (unsigned)X, r = t / (unsigned)X;  // column of vectors within a row; brick row (by, bz)
  const unsigned by = r % (unsigned)nby, bz = r / (unsigned)nby;
  unsigned acc = 0u;
  if (t < n_threads) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const unsigned zg = 2u * bz + (unsigned)g;
      if (zg < (unsigned)n_groups) {
        const uint4* __restrict__ p = vol + ((size_t)zg * (unsigned)Y + 8u * by) * (unsigned)X + c;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
          const uint4 v = p[(size_t)y * (unsigned)X];
          acc |= v.x | v.y | v.z | v.w;
        }
      }
    }
  }
  const bool any = (acc >> 16) != 0u;  // (the weight is the pair's upper half)
  const unsigned long long bal = __ballot(any);
  const int lane = threadIdx.x & 63;
  if ((lane & 7) != 0 || ((bal >> lane) & 0xffull) == 0ull) return;
  const unsigned bit = (bz * (unsigned)nby + by) * (unsigned)nbx + (c >> 3);
  const unsigned m = 1u << (bit & 31u);
  if ((tab[bit >> 5] & m) == 0u) atomicOr(&tab[bit >> 5], m);
}

// One destination voxel: `dw` its (tsdf, weight) pair, (px, py, pz) its source point.  Returns true when the voxel took a
// sample (dw rewritten); (cx, cy, cz) is then the source voxel that contains the point (the colour rule's voxel).  The sample
// is hsk_sample.h's: branch-free up to the taps, so the gathers of a lane's four voxels can be in flight together.
static __device__ __forceinline__ bool fuse_sample_merge(const unsigned* __restrict__ src, const SampleVol& sv, float px, float py,
                                                         float pz, unsigned& dw, int& cx, int& cy, int& cz) {
  const SampleCell sc = hsk_sample_cell(sv, px, py, pz);
  cx = sc.cx;
  cy = sc.cy;
  cz = sc.cz;
  unsigned w[8];
  float f[8];
  hsk_sample_words(src, sv, sc, w);
  const int Ws = hsk_sample_min_weight(w);
  const bool take = sc.in && Ws > 0;  // not the NaN of the sample, and no tap never observed
  hsk_sample_values(w, f);
  const float res = hsk_sample_blend(f, sc.a, sc.b, sc.c);
  // (the merge too is computed for every voxel and selected: a lane's four voxels then share one instruction stream, where a
  // branch per voxel cost the sweep its scalar registers)
  const int q = min(max(__float2int_rn(take ? res * 32767.0f : 0.0f), -32767), 32767);
  const int Wd = hsk_pair_wgt(dw);
  const int n = hsk_pair_raw(dw) * Wd + q * Ws, W = max(Wd + Ws, 1);
  const unsigned mag = (2u * (unsigned)abs(n) + (unsigned)W) / (2u * (unsigned)W);
  const int raw = n < 0 ? -(int)mag : (int)mag;
  dw = take ? (((unsigned)raw & 0xffffu) | ((unsigned)min(W, HSK_MAX_WEIGHT) << 16)) : dw;
  return take;
}

static __device__ __forceinline__ unsigned fuse_color_merge(unsigned cd, unsigned cs, int max_w) {
  const unsigned wd = cd >> 24, ws = cs >> 24, w = max(wd + ws, 1u), half = w >> 1;  // (callers select: ws != 0 where it counts)
  const unsigned r = ((cd & 255u) * wd + (cs & 255u) * ws + half) / w;
  const unsigned g = (((cd >> 8) & 255u) * wd + ((cs >> 8) & 255u) * ws + half) / w;
  const unsigned b = (((cd >> 16) & 255u) * wd + ((cs >> 16) & 255u) * ws + half) / w;
  return r | (g << 8) | (b << 16) | (min(w, (unsigned)max_w) << 24);
}

struct FuseArgs {
  float A[9], b[3];   // destination -> source
  float slack[3];     // per source axis: what the float evaluation of ps can be off by, generously
  int c0[3], cn[3];   // the footprint in chunks: first voxel (a multiple of HSK_FCHUNK) and count per axis
  int nbx, nby;       // bricks of the source per row and per plane of bricks
  int tab_words;      // words of the brick table (a multiple of 4)
  int max_w;          // the destination's colour max_weight
};

// counts: [0] voxels fused, [1] voxels coloured, [2] chunks swept.  Persistent waves: a workgroup stages the brick table once
// (LDS: it fits 64 KiB) and its waves stride over the footprint's chunks; a wave adds its counts once, at its end.
template <bool LDS, bool COLOR>
__global__ __launch_bounds__(256) void k_fuse_sweep(const unsigned* __restrict__ src, const unsigned* __restrict__ scol,
                                                    unsigned* __restrict__ dst, unsigned* __restrict__ dcol, SampleVol sv, SampleVol dv,
                                                    FuseArgs fa, const unsigned* __restrict__ tab, unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_tab[];  // (staged with 16-B stores)
  if (LDS) {
    for (int i = threadIdx.x; i < (fa.tab_words >> 2); i += 256) ((uint4*)s_tab)[i] = ((const uint4*)tab)[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int wave0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const int n_waves = (int)gridDim.x * 4, n_chunks = fa.cn[0] * fa.cn[1] * fa.cn[2];
  unsigned n_fused = 0, n_colored = 0, n_swept = 0;
  for (int chunk = wave0; chunk < n_chunks; chunk += n_waves) {
    const int cxi = chunk % fa.cn[0], cyi = (chunk / fa.cn[0]) % fa.cn[1], czi = chunk / (fa.cn[0] * fa.cn[1]);
    const int xa = fa.c0[0] + cxi * HSK_FCHUNK, ya = fa.c0[1] + cyi * HSK_FCHUNK, za = fa.c0[2] + czi * HSK_FCHUNK;
    const int xb = min(xa + HSK_FCHUNK - 1, dv.X - 1), yb = min(ya + HSK_FCHUNK - 1, dv.Y - 1), zb = min(za + HSK_FCHUNK - 1, dv.Z - 1);
    // ---- can a voxel of the chunk take a sample?
    {
      const float p0[3] = {((float)xa + 0.5f) * dv.cell[0], ((float)ya + 0.5f) * dv.cell[1], ((float)za + 0.5f) * dv.cell[2]};
      const float p1[3] = {((float)xb + 0.5f) * dv.cell[0], ((float)yb + 0.5f) * dv.cell[1], ((float)zb + 0.5f) * dv.cell[2]};
      float mn[3] = {1e30f, 1e30f, 1e30f}, mx[3] = {-1e30f, -1e30f, -1e30f};
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float qx = (c & 1) ? p1[0] : p0[0], qy = (c & 2) ? p1[1] : p0[1], qz = (c & 4) ? p1[2] : p0[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float s = ((fa.A[3 * i] * qx + fa.A[3 * i + 1] * qy) + fa.A[3 * i + 2] * qz) + fa.b[i];
          mn[i] = fminf(mn[i], s);
          mx[i] = fmaxf(mx[i], s);
        }
      }
      const int dims[3] = {sv.X, sv.Y, sv.Z};
      int ta[3], tb[3];  // the taps the chunk's voxels can reach
      bool miss = false;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        // the voxel of every source point lies in [ga, gb]: the quotient is monotone in the point
        // (a point that is not finite has no voxel; fminf / fmaxf pass it over, and a chunk of such points alone misses)
        const float qa = floorf(hsk_div_by_const(mn[i] - fa.slack[i], sv.icell[i])), qb = floorf(hsk_div_by_const(mx[i] + fa.slack[i], sv.icell[i]));
        const int ga = (int)fminf(fmaxf(qa, -2.0f), (float)(dims[i] + 1)), gb = (int)fminf(fmaxf(qb, -2.0f), (float)(dims[i] + 1));
        miss |= (gb < 1) | (ga > dims[i] - 2);
        ta[i] = max(ga, 1) - 1;
        tb[i] = min(gb, dims[i] - 2) + 1;
      }
      if (miss) continue;  // every sample is the NaN of the outer shell
      const int bax = ta[0] >> 3, bay = ta[1] >> 3, baz = ta[2] >> 3;
      const int nx = (tb[0] >> 3) - bax + 1, ny = (tb[1] >> 3) - bay + 1, nz = (tb[2] >> 3) - baz + 1;
      const int nb = nx * ny * nz;
      bool seen = false;
      for (int base = 0; base < nb && !seen; base += 64) {
        const int i = base + lane;
        bool mine = false;
        if (i < nb) {
          const int bx = bax + i % nx, by = bay + (i / nx) % ny, bz = baz + i / (nx * ny);
          const unsigned bit = ((unsigned)bz * (unsigned)fa.nby + (unsigned)by) * (unsigned)fa.nbx + (unsigned)bx;
          const unsigned word = LDS ? s_tab[bit >> 5] : tab[bit >> 5];
          mine = ((word >> (bit & 31u)) & 1u) != 0u;
        }
        seen = __any(mine);
      }
      if (!seen) continue;  // every tap the chunk can reach has weight 0
    }
    n_swept += 1;
    // ---- the chunk voxel by voxel: a lane per lane-block column (4 x) and row (y), the planes in turn
    const int x0 = xa + ((lane & 3) << 2), y = ya + (lane >> 2);
    if (x0 > xb || y > yb) continue;
    const float pdy = ((float)y + 0.5f) * dv.cell[1];
    float pdx[4], sxy[3][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pdx[j] = ((float)(x0 + j) + 0.5f) * dv.cell[0];
#pragma unroll
      for (int i = 0; i < 3; ++i) sxy[i][j] = fa.A[3 * i] * pdx[j] + fa.A[3 * i + 1] * pdy;
    }
    const unsigned dpitch = (unsigned)((dv.X >> 2) << 4);
    const unsigned drow = (unsigned)y * dpitch + (((unsigned)x0 >> 2) << 4);
    for (int zz = za; zz <= zb; ++zz) {
      const float pdz = ((float)zz + 0.5f) * dv.cell[2];
      const float sz0 = fa.A[2] * pdz, sz1 = fa.A[5] * pdz, sz2 = fa.A[8] * pdz;
      const unsigned wi = ((unsigned)zz >> 2) * (unsigned)dv.Y * dpitch + (((unsigned)zz & 3u) << 2) + drow;
      uint4 d4 = *(const uint4*)(dst + wi);
      unsigned dw[4] = {d4.x, d4.y, d4.z, d4.w};
      unsigned cs[4] = {0u, 0u, 0u, 0u};
      unsigned took = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float px = (sxy[0][j] + sz0) + fa.b[0], py = (sxy[1][j] + sz1) + fa.b[1], pz = (sxy[2][j] + sz2) + fa.b[2];
        int cx, cy, cz;
        if (fuse_sample_merge(src, sv, px, py, pz, dw[j], cx, cy, cz)) took |= 1u << j;
        if (COLOR) cs[j] = ((unsigned)cz * (unsigned)sv.Y + (unsigned)cy) * (unsigned)sv.X + (unsigned)cx;  // (a valid voxel, taken or not)
      }
      if (took == 0u) continue;
      n_fused += __popc(took);
      if (COLOR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[j] = scol[cs[j]];
      }
      d4.x = dw[0];
      d4.y = dw[1];
      d4.z = dw[2];
      d4.w = dw[3];
      *(uint4*)(dst + wi) = d4;
      if (COLOR) {
        const unsigned has = (((cs[0] >> 24) != 0u ? 1u : 0u) | ((cs[1] >> 24) != 0u ? 2u : 0u) | ((cs[2] >> 24) != 0u ? 4u : 0u) |
                              ((cs[3] >> 24) != 0u ? 8u : 0u)) & took;
        if (has != 0u) {
          uint4* cp = (uint4*)(dcol + (((unsigned)zz * (unsigned)dv.Y + (unsigned)y) * (unsigned)dv.X + (unsigned)x0));
          uint4 c4 = *cp;
          c4.x = (has & 1u) ? fuse_color_merge(c4.x, cs[0], fa.max_w) : c4.x;
          c4.y = (has & 2u) ? fuse_color_merge(c4.y, cs[1], fa.max_w) : c4.y;
          c4.z = (has & 4u) ? fuse_color_merge(c4.z, cs[2], fa.max_w) : c4.z;
          c4.w = (has & 8u) ? fuse_color_merge(c4.w, cs[3], fa.max_w) : c4.w;
          *cp = c4;
          n_colored += __popc(has);
        }
      }
    }
  }
  const unsigned long long f = hsk_wave_sum(n_fused), c = hsk_wave_sum(n_colored);
  if (lane == 0) {
    if (f) atomicAdd(&counts[0], f);
    if (c) atomicAdd(&counts[1], c);
    if (n_swept) atomicAdd(&counts[2], (unsigned long long)n_swept);
  }
}

size_t fuse_table_words(const VolParams& sv) {
  const size_t bits = (size_t)(sv.X >> 3) * (size_t)(sv.Y >> 3) * (size_t)((sv.nzs + 7) >> 3);
  return ((bits + 31) / 32 + 3) / 4 * 4;
}

void launch_fuse_bricks(hipStream_t s, const void* src_vol, const VolParams& sv, unsigned* tab) {
  // (a row of one plane group -- X / 4 lane-blocks of 4 vectors -- is X vectors; X and Y are multiples of 8)
  const int n_groups = (sv.nzs + 3) >> 2, nby = sv.Y >> 3, nbz = (sv.nzs + 7) >> 3;
  const unsigned n_threads = (unsigned)sv.X * (unsigned)nby * (unsigned)nbz;
  hipLaunchKernelGGL(k_fuse_bricks, dim3((n_threads + 255u) / 256u), dim3(256), 0, s, (const uint4*)src_vol, n_threads, sv.X, sv.Y, n_groups,
                     sv.X >> 3, nby, tab);
}

void launch_fuse_sweep(hipStream_t s, const void* src_vol, const unsigned* src_col, void* dst_vol, unsigned* dst_col, const VolParams& sv,
                       const VolParams& dv, const float A[9], const float b[3], const int box[6], const unsigned* tab, int max_w,
                       unsigned long long* counts, unsigned long long* chunks_total) {
  FuseArgs fa;
  for (int i = 0; i < 9; ++i) fa.A[i] = A[i];
  long total = 1;
  for (int i = 0; i < 3; ++i) {
    fa.b[i] = b[i];
    // |ps_i|'s terms are bounded by mag; four roundings of 2^-24 each stay below 2.4e-7 mag
    const float mag = ((fabsf(A[3 * i]) * dv.size[0] + fabsf(A[3 * i + 1]) * dv.size[1]) + fabsf(A[3 * i + 2]) * dv.size[2]) + fabsf(b[i]);
    fa.slack[i] = 1.0e-6f * mag + 1.0e-7f;
    fa.c0[i] = box[2 * i] / HSK_FCHUNK * HSK_FCHUNK;
    fa.cn[i] = (box[2 * i + 1] - fa.c0[i] + HSK_FCHUNK - 1) / HSK_FCHUNK;
    total *= fa.cn[i];
  }
  fa.nbx = sv.X >> 3;
  fa.nby = sv.Y >> 3;
  fa.tab_words = (int)fuse_table_words(sv);
  fa.max_w = max_w;
  *chunks_total = (unsigned long long)total;
  const size_t tab_bytes = (size_t)fa.tab_words * 4;
  const bool lds = tab_bytes <= 64u * 1024u;
  // persistent waves: enough workgroups to fill the device a few times over, no more than the chunks need
  const long want = (total + 3) / 4;
  const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
  const unsigned* s32 = (const unsigned*)src_vol;
  unsigned* d32 = (unsigned*)dst_vol;
  const bool color = src_col && dst_col;
  const SampleVol fsv = hsk_sample_vol(sv), fdv = hsk_sample_vol(dv);
#define HSK_FUSE_LAUNCH(L, C) \
  hipLaunchKernelGGL((k_fuse_sweep<L, C>), dim3(blocks), dim3(256), (L) ? tab_bytes : 0, s, s32, src_col, d32, dst_col, fsv, fdv, fa, tab, counts)
  if (lds && color)
    HSK_FUSE_LAUNCH(true, true);
  else if (lds)
    HSK_FUSE_LAUNCH(true, false);
  else if (color)
    HSK_FUSE_LAUNCH(false, true);
  else
    HSK_FUSE_LAUNCH(false, false);
#undef HSK_FUSE_LAUNCH
}
