// fill.hip -- hole filling by volumetric diffusion for gfx950 (hsk_fill_holes, hsk_download_fill_mask; DESIGN.md 3.22 the kernels,
// 8p the rule; tests/fill_twin.py restates the rule in numpy).  The rule's text is hsk_fill_point.h; what stands here is where
// its operands live and which work may be left out.
//
// THE STATE is one int16 per stored voxel at the voxel's own place in the block layout (hsk_vox_index), FILL_UNKNOWN in the
// padding planes, in two buffers: iteration i reads buffer (i - 1) & 1 and writes buffer i & 1, the final states are those of
// buffer iterations & 1.  A tile is hsk_vol_sweep.h's: 16 x 16 x 8 voxels, 4 lane-blocks wide, 16 rows, two plane groups; a thread
// owns planes 2 h, 2 h + 1 of one lane-block of one row of one plane group: two adjacent 16-B vectors of the volume and ONE 16-B
// vector of a state buffer.
// k_fill_init: a workgroup per tile writes both state buffers from the volume, a byte per thread with its eight voxels' FREE
// bits (a non-source voxel inside the box: the voxels the iteration may change), and per tile whether it holds a FREE voxel (a
// candidate), whether it holds a source (the "changed" byte iteration 1 reads) and a zero (the byte iteration 1 writes).
// k_fill_round: a workgroup per tile; see the argument at its test for which tiles work.  A working tile stages its states and a
// one-voxel halo in LDS (18 x 18 x 10 int16), applies fill_step to its FREE voxels and stores every vector of the tile.
// k_fill_cross: the keep rule of HSK_FILL_SURFACE in row-major bytes -- the crossing voxels (a workgroup per tile, staged as an
// iteration stages it); volume_sweep.hip's k_mask_dilate then dilates them by `band` along x, y and z in turn.  The bytes live in
// the state buffer that does not hold the final states: its first half and its second half in turn.
// k_fill_count: the mask (a row-major byte per voxel: this voxel is written) and the counts, a thread per lane-block;
// k_fill_commit: the words, through the mask -- a vector of the volume is stored only when one of its words changes.
// No kernel waits on another workgroup; no loop's trip count depends on data.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_vol_sweep.h"
#include "hsk_fill_point.h"

#define FT_X 18u  // a staged tile's extents: the tile and a one-voxel halo
#define FT_Y 18u
#define FT_Z 10u

// a thread's place in its tile: lane-block lb, row yl, plane group gg, plane pair h -- eight consecutive threads cover 128
// contiguous bytes of a state buffer and 256 of the volume
struct FillThread {
  unsigned lb, h, gg, yl;
  unsigned x0, y, zg;  // the first voxel's x, the row, the plane group, in the grid
  bool stored;         // the thread's vectors exist
  size_t v16;          // its vector of a state buffer, in 16-B units; its two of the volume are 2 v16, 2 v16 + 1
};
static __device__ __forceinline__ FillThread fill_thread(const VolTiles& q, unsigned tx, unsigned ty, unsigned tz, unsigned tid) {
  FillThread t;
  t.h = tid & 1u;
  t.lb = (tid >> 1) & 3u;
  t.gg = (tid >> 3) & 1u;
  t.yl = tid >> 4;
  t.x0 = 16u * tx + 4u * t.lb;
  t.y = 16u * ty + t.yl;
  t.zg = 2u * tz + t.gg;
  t.stored = t.x0 < q.g.X && t.y < q.g.Y && t.zg < q.Zg;  // (X is a multiple of 4: a vector lies inside the grid or outside it)
  t.v16 = (((size_t)t.zg * q.g.Y + t.y) * q.X4 + (t.x0 >> 2)) * 2u + t.h;
  return t;
}
// eight states <-> a 16-B vector (element e in the low or high half of word e / 2)
static __device__ __forceinline__ void fill_unpack(const uint4& v, int s[8]) {
  unsigned w[4];
  vol_words(v, w);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s[2 * i] = (int)(short)(w[i] & 0xffffu);
    s[2 * i + 1] = (int)(short)(w[i] >> 16);
  }
}
static __device__ __forceinline__ uint4 fill_pack(const int s[8]) {
  unsigned w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = ((unsigned)s[2 * i] & 0xffffu) | ((unsigned)s[2 * i + 1] << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}
#define FILL_UNKNOWN_VEC make_uint4(0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u)

__global__ __launch_bounds__(256) void k_fill_init(const uint4* __restrict__ vol, VolTiles q, VoxBox box, uint4* __restrict__ st0, uint4* __restrict__ st1,
                                                   unsigned char* __restrict__ tile_free, unsigned char* __restrict__ cand,
                                                   unsigned char* __restrict__ flag0, unsigned char* __restrict__ flag1, unsigned* __restrict__ counts) {
  __shared__ unsigned s_n[2];
  const unsigned tid = threadIdx.x, tile = blockIdx.x;
  unsigned tx, ty, tz;
  vol_tile(q, tile, tx, ty, tz);
  const FillThread t = fill_thread(q, tx, ty, tz, tid);
  if (tid < 2u) s_n[tid] = 0u;
  uint4 v[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {  // (a padding plane is no voxel: not read, no source, not FREE)
    v[p] = make_uint4(0u, 0u, 0u, 0u);
    if (t.stored && 4u * t.zg + 2u * t.h + (unsigned)p < q.g.Z) v[p] = vol[t.v16 * 2u + (unsigned)p];
  }
  int s[8];
  unsigned free_bits = 0u, n_src = 0u;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    unsigned w[4];
    vol_words(v[p], w);
    const unsigned z = 4u * t.zg + 2u * t.h + (unsigned)p;
    const bool voxel = t.stored && z < q.g.Z;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[4 * p + j] = fill_initial(w[j]);  // (no voxel: the word is 0, FILL_UNKNOWN)
      const bool src = fill_is_source(w[j]);
      n_src += src ? 1u : 0u;
      const bool fr = voxel && !src && vox_in_box(box, (int)(t.x0 + (unsigned)j), (int)t.y, (int)z);
      free_bits |= (fr ? 1u : 0u) << (4 * p + j);
    }
  }
  if (t.stored) {
    const uint4 o = fill_pack(s);
    st0[t.v16] = o;
    st1[t.v16] = o;
  }
  tile_free[(size_t)tile * 256u + tid] = (unsigned char)free_bits;
  __syncthreads();
  const unsigned nf = hsk_wave_sum((unsigned)__popc(free_bits)), ns = hsk_wave_sum(n_src);  // (every lane arrives: nothing above returns)
  if ((tid & 63u) == 0u) {
    if (nf) atomicAdd(&s_n[0], nf);
    if (ns) atomicAdd(&s_n[1], ns);
  }
  __syncthreads();
  if (tid == 0u) {
    cand[tile] = s_n[0] ? 1 : 0;
    flag0[tile] = s_n[1] ? 1 : 0;
    flag1[tile] = 0;
    if (s_n[0]) atomicAdd(&counts[0], s_n[0]);
  }
}

// a halo voxel's state: FILL_UNKNOWN outside the grid (x, y, z may be -1 as unsigned or one past the end).  The padding planes
// hold FILL_UNKNOWN, so z is tested against the stored planes only.
static __device__ __forceinline__ int fill_halo(const short* __restrict__ st, const VolTiles& q, unsigned x, unsigned y, unsigned z) {
  if (x >= q.g.X || y >= q.g.Y || z >= 4u * q.Zg) return FILL_UNKNOWN;
  return (int)st[q.g.at_xyz(x, y, z)];
}

// local voxel (xl, yl, zl) of a staged tile, -1 .. the extent
#define FT_AT(xl, yl, zl) ((((zl) + 1u) * FT_Y + ((yl) + 1u)) * FT_X + ((xl) + 1u))
// The tile's states and a one-voxel halo of them into s_st (FT_Z x FT_Y x FT_X; the halo's edges and corners are not staged: a
// voxel's six face neighbours never lie there), the thread's own eight into s.  Every load is issued before the first is used:
// the thread's vector and its four halo voxels.  Every thread of the workgroup arrives (it ends in a barrier).
static __device__ __forceinline__ void fill_stage(const short* __restrict__ rd, const VolTiles& q, const FillThread& t, unsigned tx, unsigned ty, unsigned tz,
                                                  unsigned tid, short* __restrict__ s_st, int s[8]) {
  const uint4 own = t.stored ? ((const uint4*)rd)[t.v16] : FILL_UNKNOWN_VEC;
  const unsigned a = tid & 15u, b = tid >> 4, f = tid >> 7, c = (tid >> 4) & 7u;
  const unsigned bx = 16u * tx, by = 16u * ty, bz = 8u * tz;
  const int h0 = fill_halo(rd, q, bx + a, by + b, bz - 1u);                      // the face below: (a, b) = (x, y)
  const int h1 = fill_halo(rd, q, bx + a, by + b, bz + 8u);                      // the face above
  const int h2 = fill_halo(rd, q, bx + a, f ? by + 16u : by - 1u, bz + c);       // the faces y - 1 and y + 16: (a, c) = (x, z)
  const int h3 = fill_halo(rd, q, f ? bx + 16u : bx - 1u, by + a, bz + c);       // the faces x - 1 and x + 16: (a, c) = (y, z)
  fill_unpack(own, s);
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) s_st[FT_AT(4u * t.lb + (unsigned)j, t.yl, 4u * t.gg + 2u * t.h + (unsigned)p)] = (short)s[4 * p + j];
  s_st[FT_AT(a, b, 0u) - FT_Y * FT_X] = (short)h0;
  s_st[FT_AT(a, b, 8u)] = (short)h1;
  s_st[f ? FT_AT(a, 16u, c) : FT_AT(a, 0u, c) - FT_X] = (short)h2;
  s_st[f ? FT_AT(16u, a, c) : FT_AT(0u, a, c) - 1u] = (short)h3;
  __syncthreads();
}

__global__ __launch_bounds__(256) void k_fill_round(const short* __restrict__ rd, uint4* __restrict__ wr, VolTiles q, const unsigned char* __restrict__ tile_free,
                                                    const unsigned char* __restrict__ cand, const unsigned char* __restrict__ flag_rd,
                                                    unsigned char* __restrict__ flag_wr, unsigned* __restrict__ changed, unsigned* __restrict__ visits) {
  __shared__ short s_st[FT_Z * FT_Y * FT_X];
  __shared__ unsigned s_changed;
  const unsigned tid = threadIdx.x, tile = blockIdx.x;
  unsigned tx, ty, tz;
  vol_tile(q, tile, tx, ty, tz);
  // WHICH TILES WORK.  Write S_i(T) for tile T's states after iteration i (S_0: k_fill_init's), and c_i(T) for "S_i(T) differs
  // from S_{i-1}(T)", with c_0(T) = "T holds a KNOWN voxel".  Iteration i reads buffer R = (i - 1) & 1 and writes W = i & 1.
  // Invariant before iteration i: R holds S_{i-1} everywhere, W holds S_{i-2}(T) (i = 1: S_0) in every tile, and flag_rd[T] =
  // c_{i-1}(T).  It holds for i = 1 by k_fill_init, which writes both buffers alike.
  // (a) A tile without a FREE voxel never changes: S_i(T) = S_0(T) for all i, both buffers hold it from k_fill_init on, and its
  //     byte is 0 from iteration 1 on (in iteration 1 its neighbours read c_0 of it, which k_fill_init wrote).
  // (b) fill_step of a voxel of T reads S_{i-1} of T and of T's six face-neighbour tiles only (a voxel and its six face
  //     neighbours).  If none of the seven changed in iteration i - 1, the operands equal those of iteration i - 1, so S_i(T) =
  //     S_{i-1}(T); and c_{i-1}(T) = 0 says S_{i-1}(T) = S_{i-2}(T), which is what W holds: leaving W alone leaves S_i(T) in it.
  //     For i = 1: none of the seven holds a KNOWN voxel, every count n is 0, every voxel stays FILL_UNKNOWN = S_0(T).
  // In both cases the tile writes c_i(T) = 0 into flag_wr and is done; otherwise it computes all of S_i(T) into W.  Either way the
  // invariant holds for i + 1.  The bytes are ping-ponged with the states: no workgroup reads a byte or a state that another
  // writes in the same launch.
  bool work = cand[tile] != 0;
  if (work) {
    work = flag_rd[tile] != 0 || (tx > 0u && flag_rd[tile - 1u]) || (tx + 1u < q.ntx && flag_rd[tile + 1u]) || (ty > 0u && flag_rd[tile - q.ntx]) ||
           (ty + 1u < q.nty && flag_rd[tile + q.ntx]) || (tz > 0u && flag_rd[tile - q.ntx * q.nty]) || (tz + 1u < q.ntz && flag_rd[tile + q.ntx * q.nty]);
  }
  if (!work) {  // (the whole workgroup: the bytes are the same for all its threads)
    if (tid == 0u) flag_wr[tile] = 0;
    return;
  }
  const FillThread t = fill_thread(q, tx, ty, tz, tid);
  if (tid == 0u) s_changed = 0u;
  const unsigned free_bits = tile_free[(size_t)tile * 256u + tid];  // (issued with the stage's loads, before the first of them is used)
  int s[8];
  fill_stage(rd, q, t, tx, ty, tz, tid, s_st, s);
  unsigned n_changed = 0u;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((free_bits >> (4 * p + j)) & 1u)) continue;
      const unsigned l = FT_AT(4u * t.lb + (unsigned)j, t.yl, 4u * t.gg + 2u * t.h + (unsigned)p);
      const int n7[7] = {s[4 * p + j],           (int)s_st[l - 1u],           (int)s_st[l + 1u],          (int)s_st[l - FT_X],
                         (int)s_st[l + FT_X],    (int)s_st[l - FT_Y * FT_X],  (int)s_st[l + FT_Y * FT_X]};
      const int nv = fill_step(n7);
      n_changed += nv != s[4 * p + j] ? 1u : 0u;
      s[4 * p + j] = nv;
    }
  if (t.stored) wr[t.v16] = fill_pack(s);
  const unsigned nw = hsk_wave_sum(n_changed);  // (every lane arrives: the return above takes the whole workgroup)
  if ((tid & 63u) == 0u && nw) atomicAdd(&s_changed, nw);
  __syncthreads();
  if (tid == 0u) {
    flag_wr[tile] = s_changed ? 1 : 0;
    if (s_changed) atomicAdd(changed, s_changed);
    atomicAdd(visits, 1u);
  }
}

// the crossing voxels of the final states, a row-major byte each: a workgroup per tile, staged as an iteration stages it
__global__ __launch_bounds__(256) void k_fill_cross(const short* __restrict__ st, VolTiles q, unsigned* __restrict__ out) {
  __shared__ short s_st[FT_Z * FT_Y * FT_X];
  const unsigned tid = threadIdx.x, tile = blockIdx.x;
  unsigned tx, ty, tz;
  vol_tile(q, tile, tx, ty, tz);
  const FillThread t = fill_thread(q, tx, ty, tz, tid);
  int s[8];
  fill_stage(st, q, t, tx, ty, tz, tid, s_st, s);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const unsigned z = 4u * t.zg + 2u * t.h + (unsigned)p;
    if (!t.stored || z >= q.g.Z) continue;  // (a padding plane is no voxel and has no byte)
    unsigned m = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned l = FT_AT(4u * t.lb + (unsigned)j, t.yl, 4u * t.gg + 2u * t.h + (unsigned)p);
      const int n7[7] = {s[4 * p + j],        (int)s_st[l - 1u],          (int)s_st[l + 1u],         (int)s_st[l - FT_X],
                         (int)s_st[l + FT_X], (int)s_st[l - FT_Y * FT_X], (int)s_st[l + FT_Y * FT_X]};
      m |= (fill_crossing_voxel(n7) ? 1u : 0u) << (8 * j);
    }
    out[(size_t)q.g.lin(t.x0, t.y, z) >> 2] = m;  // (X is a multiple of 4: the four bytes of voxels x0 .. x0 + 3 are one aligned word)
  }
}

// the mask and the counts: counts[1] the FILLED voxels, [2] those that are written, [3] those of them with a negative value.  A
// thread per lane-block (4 x-adjacent voxels by 4 planes): 64 contiguous bytes of the volume, 32 of the states, and one word of
// the keep bytes and of the mask in each of its planes -- consecutive threads, consecutive words in all four arrays.
__global__ __launch_bounds__(256) void k_fill_count(const uint4* __restrict__ vol, const uint4* __restrict__ st, const unsigned* __restrict__ keep, VolVectors q,
                                                    VoxBox box, unsigned* __restrict__ mask, unsigned* __restrict__ counts) {
  unsigned n_reached = 0u, n_written = 0u, n_neg = 0u;
  // (four lane-blocks a thread and one set of atomics a workgroup: at 512^3 the three counters take 8 192 additions each, not the
  // 131 072 a wave-wise sum would send to the same three words)
  for (unsigned c = 0u; c < 4u; ++c) {
    const unsigned i = (blockIdx.x * 4u + c) * 256u + threadIdx.x;
    if (i >= q.n4 >> 2) continue;
    const unsigned xb = i % q.X4, r = i / q.X4, y = r % q.g.Y, zg = r / q.g.Y, x0 = 4u * xb;
    uint4 v[4];
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) v[pl] = vol[(size_t)i * 4u + (unsigned)pl];  // (padding planes hold zeros: read, not used)
    int s[16];
    fill_unpack(st[(size_t)i * 2u], s);
    fill_unpack(st[(size_t)i * 2u + 1u], s + 8);
    unsigned kp[4];
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) {
      const unsigned z = 4u * zg + (unsigned)pl;
      kp[pl] = (keep && z < q.g.Z) ? keep[(size_t)q.g.lin(x0, y, z) >> 2] : 0x01010101u;
    }
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) {
      const unsigned z = 4u * zg + (unsigned)pl;
      if (z >= q.g.Z) continue;
      unsigned w[4];
      vol_words(v[pl], w);
      unsigned m = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sj = s[4 * pl + j];
        const bool filled = !fill_is_source(w[j]) && sj != FILL_UNKNOWN && vox_in_box(box, (int)(x0 + (unsigned)j), (int)y, (int)z);
        const bool written = filled && ((kp[pl] >> (8 * j)) & 0xffu) != 0u;
        n_reached += filled ? 1u : 0u;
        n_written += written ? 1u : 0u;
        n_neg += (written && sj < 0) ? 1u : 0u;
        m |= (written ? 1u : 0u) << (8 * j);
      }
      mask[(size_t)q.g.lin(x0, y, z) >> 2] = m;
    }
  }
  const unsigned sums[3] = {hsk_wave_sum(n_reached), hsk_wave_sum(n_written), hsk_wave_sum(n_neg)};  // (every lane arrives)
  const unsigned total = hsk_block_meet<HskSum>(sums);  // (thread v < 3: the workgroup's word v)
  if (threadIdx.x < 3u && total) atomicAdd(&counts[1u + threadIdx.x], total);
}

__global__ __launch_bounds__(256) void k_fill_commit(uint4* __restrict__ vol, const uint2* __restrict__ st, const unsigned* __restrict__ mask, VolVectors q,
                                                     int fill_weight) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  if (!vol_vector(q, i, x0, y, z)) return;
  const unsigned m = mask[(size_t)q.g.lin(x0, y, z) >> 2];
  if (m == 0u) return;
  unsigned w[4];
  vol_words(vol[i], w);
  const uint2 sv = st[i];
  const int s[4] = {(int)(short)(sv.x & 0xffffu), (int)(short)(sv.x >> 16), (int)(short)(sv.y & 0xffffu), (int)(short)(sv.y >> 16)};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if ((m >> (8 * j)) & 0xffu) w[j] = fill_word(fill_weight, s[j]);
  vol[i] = make_uint4(w[0], w[1], w[2], w[3]);
}

size_t fill_layout(const VolParams& vp, void* base, FillBufs* b) {
  const VolTiles q = vol_tiles(vp);
  const size_t n_tiles = (size_t)q.ntx * q.nty * q.ntz;
  ScratchCarve c{base};
  FillBufs out;
  out.counts = (unsigned*)c.take((FILL_COUNTS + 256) * 4);
  out.tile_free = (unsigned char*)c.take(n_tiles * 256);
  out.cand = (unsigned char*)c.take(n_tiles);
  out.flag[0] = (unsigned char*)c.take(n_tiles);
  out.flag[1] = (unsigned char*)c.take(n_tiles);
  out.state[0] = (short*)c.take(hsk_vol_words(vp) * 2);
  out.state[1] = (short*)c.take(hsk_vol_words(vp) * 2);
  out.n_tiles = (unsigned)n_tiles;
  if (b) *b = out;
  return c.bytes;
}

void launch_fill_init(hipStream_t s, const void* vol, const VolParams& vp, const int lo[3], const int hi[3], const FillBufs& b) {
  const VolTiles q = vol_tiles(vp);
  (void)hipMemsetAsync(b.counts, 0, (FILL_COUNTS + 256) * 4, s);
  hipLaunchKernelGGL(k_fill_init, dim3(b.n_tiles), dim3(256), 0, s, (const uint4*)vol, q, vox_box(lo, hi), (uint4*)b.state[0], (uint4*)b.state[1], b.tile_free,
                     b.cand, b.flag[0], b.flag[1], b.counts);
}

void launch_fill_round(hipStream_t s, const VolParams& vp, const FillBufs& b, int it) {
  const VolTiles q = vol_tiles(vp);
  const int rd = (it - 1) & 1, wr = it & 1;
  hipLaunchKernelGGL(k_fill_round, dim3(b.n_tiles), dim3(256), 0, s, (const short*)b.state[rd], (uint4*)b.state[wr], q, (const unsigned char*)b.tile_free,
                     (const unsigned char*)b.cand, (const unsigned char*)b.flag[rd], b.flag[wr], b.counts + FILL_COUNTS + it, b.counts + 4);
}

void launch_fill_keep(hipStream_t s, const VolParams& vp, const FillBufs& b, int fin, int band) {
  const VolTiles q = vol_tiles(vp);
  unsigned char* m0 = fill_mask_bytes(vp, b, fin);
  hipLaunchKernelGGL(k_fill_cross, dim3(b.n_tiles), dim3(256), 0, s, (const short*)b.state[fin], q, (unsigned*)m0);
  launch_mask_dilate3(s, vp, m0, fill_keep_bytes(vp, b, fin), band);  // (the result: the keep bytes)
}

void launch_fill_count(hipStream_t s, const void* vol, const VolParams& vp, const int lo[3], const int hi[3], const FillBufs& b, int fin, bool keep_all) {
  const VolVectors q = vol_vectors(vp);
  hipLaunchKernelGGL(k_fill_count, dim3(((q.n4 >> 2) + 1023u) / 1024u), dim3(256), 0, s, (const uint4*)vol, (const uint4*)b.state[fin],
                     keep_all ? (const unsigned*)nullptr : (const unsigned*)fill_keep_bytes(vp, b, fin), q, vox_box(lo, hi), (unsigned*)fill_mask_bytes(vp, b, fin),
                     b.counts);
}

void launch_fill_commit(hipStream_t s, void* vol, const VolParams& vp, const FillBufs& b, int fin, int fill_weight) {
  const VolVectors q = vol_vectors(vp);
  hipLaunchKernelGGL(k_fill_commit, dim3((q.n4 + 255u) / 256u), dim3(256), 0, s, (uint4*)vol, (const uint2*)b.state[fin],
                     (const unsigned*)fill_mask_bytes(vp, b, fin), q, fill_weight);
}

int fill_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_fill_round);
}
