// simplify.hip -- the simplified mesh read-out for gfx950 (hsk_extract_mesh_simplified; DESIGN.md 3.17 the kernels, 8k the rule):
// quadric vertex clustering (Lindstrom 2000) of the indexed marching-cubes mesh on a grid of cells of c voxels.  The rule's
// arithmetic is hsk_simplify_point.h, shared with the host; here is who gathers what.  NO kernel adds into a shared address
// per triangle or per vertex: the sums of a cluster are GATHERED by the wave that owns it, from the c^3 voxels of its cell (its
// vertices) and the (c + 1)^3 cubes from one below the cell on every axis (the triangles that touch it), reduced over the
// wave's lanes in registers -- integer sums, so the order is free -- and stored once.
//   faces    (a wave per cube row, counting): every triangle's three clusters; a face survives when they differ; the row's
//            surviving faces are counted and their clusters marked "referenced", one byte per cluster of the grid, by plain
//            stores of the same value (idempotent)
//   rows     (a wave per cluster row): the referenced bytes become 0x80 | rank within their 64-cluster segment, the
//            segments' bases and the row's count are kept (the output order: plane, row, x -- launch_scan_rows orders the
//            rows); and the clusters that hold a vertex at all are counted from the indexed mesh's edge bits (a statistic)
//   list     (a wave per cluster row): the referenced clusters' numbers, in output order
//   gather   (a wave per OUTPUT vertex; four waves at c = 8, sixteen at c = 16): the cluster's 20 sums
//   solve    (a lane per output vertex): hsk_simplify_point.h's simp_vertex, the normal, the colour; the statistics
//   faces    (the cube rows again, writing): each surviving face's corners are its clusters' output numbers
// What is read of the indexed mesh's count pass (extract.hip): the cube rows' triangle counts (an empty row is skipped
// without touching the volume) and the edge bits (which edges carry a vertex; a 64-cube segment without one is skipped).
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_simplify_point.h"

static __device__ __forceinline__ unsigned simp_word(const unsigned* __restrict__ vol, const VolParams& vp, int x, int y, int z) {
  return vol[hsk_vox_index(vp, x, y, z)];
}
static __device__ __forceinline__ void simp_load_cube(const unsigned* __restrict__ vol, const VolParams& vp, int x, int y, int z, unsigned* w) {
#pragma unroll
  for (int c = 0; c < 8; ++c) w[c] = simp_word(vol, vp, x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2));
}
// inclusive scan of v over the wave's 64 lanes
static __device__ __forceinline__ int simp_wave_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
// `width` (<= 48) bits from bit b0 of a grid row's edge bits
static __device__ __forceinline__ unsigned long long simp_bit_field(const unsigned long long* __restrict__ w, int b0, int width) {
  const int j = b0 >> 6, sh = b0 & 63;
  unsigned long long f = w[j] >> sh;
  if (sh + width > 64) f |= w[j + 1] << (64 - sh);
  return f & ((1ull << width) - 1ull);
}

size_t simp_layout(const VolParams& vp, int s, void* base, SimpBufs* b) {
  const int c = 1 << s;
  SimpBufs m;
  m.s = s;
  m.CX = (vp.X + c - 1) >> s;
  m.CY = (vp.Y + c - 1) >> s;
  m.CZ = (vp.Z + c - 1) >> s;
  m.crows = m.CY * m.CZ;
  m.cseg = (m.CX + 63) / 64;
  m.frows = (vp.Y - 1) * (vp.Z - 1);
  ScratchCarve carve{base};
  m.totals = (unsigned long long*)carve.take(128);
  m.ref = (unsigned char*)carve.take((size_t)m.CX * m.crows);
  m.cl_cnt = (unsigned*)carve.take((size_t)m.crows * 4);
  m.cl_off = (unsigned long long*)carve.take(hsk_scan_scratch_entries(m.crows) * 8);
  m.tc_cnt = (unsigned*)carve.take((size_t)m.crows * 4);
  m.tc_off = (unsigned long long*)carve.take(hsk_scan_scratch_entries(m.crows) * 8);
  m.segbase = (unsigned short*)carve.take((size_t)m.crows * m.cseg * 2);
  m.sf_cnt = (unsigned*)carve.take((size_t)m.frows * 4);
  m.sf_off = (unsigned long long*)carve.take(hsk_scan_scratch_entries(m.frows) * 8);
  if (b) *b = m;
  return carve.bytes;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_simp_faces(const unsigned* __restrict__ vol, VolParams vp, const CubeTable* __restrict__ ct,
                                                    const unsigned* __restrict__ tri_count, MeshIndexBufs mb, SimpBufs sb,
                                                    int* __restrict__ faces) {
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (row >= sb.frows) return;
  const int y = row % (vp.Y - 1), z = row / (vp.Y - 1);
  if (tri_count[row] == 0u) {  // (the indexed mesh's count pass found no triangle here)
    if (!WRITE && lane == 0) sb.sf_cnt[row] = 0u;
    return;
  }
  if (WRITE && sb.sf_cnt[row] == 0u) return;
  unsigned long long base = WRITE ? sb.sf_off[row] : 0ull;
  unsigned total = 0u;
  for (int xb = 0; xb < vp.X - 1; xb += 64) {
    // a cut cube has a cut edge whose lower corner has the cube's own x (its x face's corners agree, or an x edge is cut), on
    // one of its four grid rows: a segment whose edge bits are all clear there holds no triangle
    unsigned long long any = 0ull;
    for (int r = 0; r < 4; ++r) {
      const unsigned long long* w = mb.bits + ((size_t)((z + (r >> 1)) * vp.Y + y + (r & 1)) * mb.nseg + (xb >> 6)) * 3;
      any |= w[0] | w[1] | w[2];
    }
    if (any == 0ull) continue;
    const int x = xb + lane;
    unsigned m8 = 0u;
    int n = 0;
    if (x < vp.X - 1) {
      unsigned w[8];
      simp_load_cube(vol, vp, x, y, z, w);
      m8 = simp_m8(w);
      const int nt = m8 ? (int)ct->ntri[m8] : 0;
      for (int t = 0; t < nt; ++t) {
        unsigned ids[3];
        if (!simp_face_clusters(ct->edge[m8][t], x, y, z, sb.s, sb.CX, sb.CY, ids)) continue;
        ++n;
        if (!WRITE) sb.ref[ids[0]] = 1, sb.ref[ids[1]] = 1, sb.ref[ids[2]] = 1;
      }
    }
    if constexpr (WRITE) {
      const int scan = simp_wave_scan(n);
      unsigned long long at = base + (unsigned long long)(scan - n);
      const int nt = n ? (int)ct->ntri[m8] : 0;
      for (int t = 0; t < nt; ++t) {
        unsigned ids[3];
        if (!simp_face_clusters(ct->edge[m8][t], x, y, z, sb.s, sb.CX, sb.CY, ids)) continue;
        for (int q = 0; q < 3; ++q) {
          const unsigned crow = ids[q] / (unsigned)sb.CX, cx = ids[q] - crow * (unsigned)sb.CX;
          faces[3 * at + q] = (int)(sb.cl_off[crow] + sb.segbase[(size_t)crow * sb.cseg + (cx >> 6)] + (sb.ref[ids[q]] & 63u));
        }
        ++at;
      }
      base += (unsigned long long)__shfl(scan, 63, 64);
    } else {
      total += hsk_wave_sum((unsigned)n);
    }
  }
  if (!WRITE && lane == 0) sb.sf_cnt[row] = total;
}

__global__ __launch_bounds__(256) void k_simp_rows(MeshIndexBufs mb, SimpBufs sb, int Y, int Z) {
  const int lane = threadIdx.x & 63;
  const int crow = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (crow >= sb.crows) return;
  const int c = 1 << sb.s, cy = crow % sb.CY, cz = crow / sb.CY;
  unsigned carry = 0u, touched = 0u;
  for (int seg = 0; seg < sb.cseg; ++seg) {
    const int cx = seg * 64 + lane;
    unsigned char* rp = sb.ref + (size_t)crow * sb.CX + cx;
    const bool flag = cx < sb.CX && *rp != 0;
    const unsigned long long mask = __ballot(flag);
    if (flag) *rp = (unsigned char)(0x80u | (unsigned)__popcll(mask & ((1ull << lane) - 1ull)));
    if (lane == 0) sb.segbase[(size_t)crow * sb.cseg + seg] = (unsigned short)carry;
    carry += (unsigned)__popcll(mask);
    // the clusters of this row that hold a vertex: an edge bit among the c x c grid rows, 3 c bits each
    // (every row's bits are read, the empty rows' zeros too: the loads of different rows do not depend on one another and go
    // out together -- a test of the row's vertex count in front of each made 256 dependent round trips of a row at c = 16)
    unsigned long long any = 0ull;
    if (cx < sb.CX) {
#pragma unroll 4
      for (int d = 0; d < c * c; ++d) {
        const int gy = min(cy * c + (d & (c - 1)), Y - 1), gz = min(cz * c + (d >> sb.s), Z - 1);  // (clamped: a row again, not past the grid)
        any |= simp_bit_field(mb.bits + (size_t)(gz * Y + gy) * 3 * mb.nseg, 3 * c * cx, 3 * c);
      }
    }
    touched += (unsigned)__popcll(__ballot(any != 0ull));
  }
  if (lane == 0) sb.cl_cnt[crow] = carry, sb.tc_cnt[crow] = touched;
}

__global__ __launch_bounds__(256) void k_simp_list(SimpBufs sb, unsigned* __restrict__ list) {
  const int lane = threadIdx.x & 63;
  const int crow = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (crow >= sb.crows) return;
  if (sb.cl_cnt[crow] == 0u) return;
  const unsigned long long row_base = sb.cl_off[crow];
  for (int seg = 0; seg < sb.cseg; ++seg) {
    const int cx = seg * 64 + lane;
    if (cx >= sb.CX) continue;
    const unsigned b = sb.ref[(size_t)crow * sb.CX + cx];
    if (b & 0x80u) list[row_base + sb.segbase[(size_t)crow * sb.cseg + seg] + (b & 63u)] = (unsigned)(crow * sb.CX + cx);
  }
}

// WAVES waves share a cluster: 1 (four clusters to a block of 256), or 4 or 16 (a block of 64 WAVES threads to a cluster, their
// partial sums added through LDS) -- a cell of 16 voxels has 4913 cubes to look at, 77 trips of one wave
template <int WAVES>
__global__ __launch_bounds__(WAVES == 16 ? 1024 : 256) void k_simp_gather(const unsigned* __restrict__ vol, const unsigned* __restrict__ colv, VolParams vp,
                                                                        const CubeTable* __restrict__ ct, MeshIndexBufs mb, SimpBufs sb,
                                                                        const unsigned* __restrict__ list, unsigned n_out, simp_i64* __restrict__ sums) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned j = (unsigned)__builtin_amdgcn_readfirstlane(WAVES == 1 ? blockIdx.x * 4 + wave : blockIdx.x);
  if (j >= n_out) return;  // (WAVES == 1: a whole wave leaves, and no barrier follows; otherwise the grid is n_out blocks)
  const int first = WAVES == 1 ? lane : wave * 64 + lane, stride = 64 * WAVES;
  const unsigned id = list[j];
  const int s = sb.s, c = 1 << s;
  const int cl[3] = {(int)(id % (unsigned)sb.CX), (int)((id / (unsigned)sb.CX) % (unsigned)sb.CY), (int)(id / (unsigned)(sb.CX * sb.CY))};
  const int base[3] = {cl[0] << s, cl[1] << s, cl[2] << s};
  simp_i64 rec[SIMP_REC];
#pragma unroll
  for (int t = 0; t < SIMP_REC; ++t) rec[t] = 0;
  // the cluster's vertices: the edges that start on its c^3 voxels and carry a vertex of the indexed mesh
  for (int i = first; i < c * c * c; i += stride) {
    const int g[3] = {base[0] + (i & (c - 1)), base[1] + ((i >> s) & (c - 1)), base[2] + (i >> (2 * s))};
    if (g[0] >= vp.X || g[1] >= vp.Y || g[2] >= vp.Z) continue;
    const int grow = g[2] * vp.Y + g[1];
    if (grow >= mb.rows) continue;
    const unsigned b3 = (unsigned)simp_bit_field(mb.bits + (size_t)grow * 3 * mb.nseg, 3 * g[0], 3);
    if (b3 == 0u) continue;
    const int fa = hsk_pair_raw(simp_word(vol, vp, g[0], g[1], g[2]));
    const unsigned ca = colv ? colv[((size_t)g[2] * vp.Y + g[1]) * vp.X + g[0]] : 0u;
    for (int k = 0; k < 3; ++k) {
      if (!((b3 >> k) & 1u)) continue;
      const int h[3] = {g[0] + (k == 0 ? 1 : 0), g[1] + (k == 1 ? 1 : 0), g[2] + (k == 2 ? 1 : 0)};
      const int fb = hsk_pair_raw(simp_word(vol, vp, h[0], h[1], h[2]));
      simp_i64 p[3];
      simp_position(g, k, fa, fb, base, c, p);
      const unsigned cw = colv ? simp_color_pick(fa, fb, ca, colv[((size_t)h[2] * vp.Y + h[1]) * vp.X + h[0]]) : 0u;
      simp_add_vertex(rec, p, cw);
    }
  }
  // the triangles that touch it: the cubes from one below the cell on every axis
  const int n1 = c + 1;
  for (int i = first; i < n1 * n1 * n1; i += stride) {
    const int dz = i / (n1 * n1), r = i - dz * n1 * n1, dy = r / n1, dx = r - dy * n1;
    const int x = base[0] - 1 + dx, y = base[1] - 1 + dy, z = base[2] - 1 + dz;
    if (x < 0 || y < 0 || z < 0 || x >= vp.X - 1 || y >= vp.Y - 1 || z >= vp.Z - 1) continue;
    unsigned w[8];
    simp_load_cube(vol, vp, x, y, z, w);
    const unsigned m8 = simp_m8(w);
    if (m8) simp_cube_triangles(*ct, w, m8, x, y, z, s, cl, rec);
  }
#pragma unroll
  for (int t = 0; t < SIMP_REC; ++t) rec[t] = hsk_wave_sum(rec[t]);
  if constexpr (WAVES == 1) {
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < SIMP_REC; ++t) sums[(size_t)j * SIMP_REC + t] = rec[t];
    }
  } else {
    __shared__ simp_i64 part[WAVES][SIMP_REC];  // (every thread of the block arrives: nothing above leaves a block of this form)
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < SIMP_REC; ++t) part[wave][t] = rec[t];
    }
    __syncthreads();
    if (threadIdx.x < SIMP_REC) {
      simp_i64 total = 0;
      for (int w = 0; w < WAVES; ++w) total += part[w][threadIdx.x];
      sums[(size_t)j * SIMP_REC + threadIdx.x] = total;
    }
  }
}

__global__ __launch_bounds__(256) void k_simp_solve(VolParams vp, SimpBufs sb, const unsigned* __restrict__ list, unsigned n_out,
                                                    const simp_i64* __restrict__ sums, int mode, double floor_rel, float* __restrict__ xyz,
                                                    float* __restrict__ normals, unsigned char* __restrict__ rgb) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned counts[6] = {0u, 0u, 0u, 0u, 0u, 0u};  // rank 0 .. 3, clamped, uncoloured
  if (j < n_out) {
    simp_i64 rec[SIMP_REC];
#pragma unroll
    for (int t = 0; t < SIMP_REC; ++t) rec[t] = sums[(size_t)j * SIMP_REC + t];
    const unsigned id = list[j];
    const int c = 1 << sb.s;
    const int cl[3] = {(int)(id % (unsigned)sb.CX), (int)((id / (unsigned)sb.CX) % (unsigned)sb.CY), (int)(id / (unsigned)(sb.CX * sb.CY))};
    double x[3];
    int rank, clamped;
    simp_vertex(rec, c, mode, floor_rel, x, &rank, &clamped);
#pragma unroll
    for (int r = 0; r < 4; ++r) counts[r] = rank == r ? 1u : 0u;
    counts[4] = (unsigned)clamped;
    if (xyz) {
      float m[3];
      simp_metres(x, c, cl, vp.cell, m);
      xyz[3 * (size_t)j] = m[0], xyz[3 * (size_t)j + 1] = m[1], xyz[3 * (size_t)j + 2] = m[2];
    }
    if (normals) {
      float nr[3] = {HSK_NANF, HSK_NANF, HSK_NANF};
      (void)simp_normal(rec, vp.cell, nr);
      normals[3 * (size_t)j] = nr[0], normals[3 * (size_t)j + 1] = nr[1], normals[3 * (size_t)j + 2] = nr[2];
    }
    if (rgb) {
      unsigned char col[3];
      counts[5] = simp_rgb(rec, col) ? 0u : 1u;
      rgb[3 * (size_t)j] = col[0], rgb[3 * (size_t)j + 1] = col[1], rgb[3 * (size_t)j + 2] = col[2];
    }
  }
  // (one addition per wave and counter that has something to add: at most six per 64 output vertices)
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const unsigned sum = hsk_wave_sum(counts[r]);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(sb.totals + 4 + r, (unsigned long long)sum);
  }
}

// the count pass behind the indexed mesh's (tri_count: its cube rows' triangle counts): the surviving faces per cube row, the
// referenced clusters per cluster row, the clusters that hold a vertex; totals[0] faces, [1] vertices, [2] clusters touched
void launch_simp_count(hipStream_t s, const void* vol, const VolParams& vp, const CubeTable* ct_dev, const unsigned* tri_count,
                       const MeshIndexBufs& mb, const SimpBufs& sb) {
  (void)hipMemsetAsync(sb.totals, 0, 128, s);
  if (sb.frows <= 0 || mb.rows <= 0) return;
  (void)hipMemsetAsync(sb.ref, 0, (size_t)sb.CX * sb.crows, s);
  hipLaunchKernelGGL(k_simp_faces<false>, dim3((unsigned)((sb.frows + 3) / 4)), dim3(256), 0, s, (const unsigned*)vol, vp, ct_dev, tri_count, mb, sb,
                     (int*)nullptr);
  hipLaunchKernelGGL(k_simp_rows, dim3((unsigned)((sb.crows + 3) / 4)), dim3(256), 0, s, mb, sb, vp.Y, vp.Z);
  launch_scan_rows(s, sb.sf_cnt, sb.sf_off, sb.frows, sb.totals);
  launch_scan_rows(s, sb.cl_cnt, sb.cl_off, sb.crows, sb.totals + 1);
  launch_scan_rows(s, sb.tc_cnt, sb.tc_off, sb.crows, sb.totals + 2);
}
// ... and behind it, for n_out > 0 output vertices: their list and sums (list: n_out words, sums: 20 n_out), the solve (any of
// xyz / normals / rgb may be null; the statistics at totals[4 .. 9] always), the faces when asked for
void launch_simp_write(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const CubeTable* ct_dev,
                       const unsigned* tri_count, const MeshIndexBufs& mb, const SimpBufs& sb, unsigned n_out, unsigned* list, long long* sums,
                       int mode, double floor_rel, float* xyz, float* normals, unsigned char* rgb, int* faces) {
  (void)hipMemsetAsync(sb.totals + 4, 0, 6 * 8, s);
  hipLaunchKernelGGL(k_simp_list, dim3((unsigned)((sb.crows + 3) / 4)), dim3(256), 0, s, sb, list);
  // (a wave looks at 64 of the (c + 1)^3 cubes a trip: 27 and 125 are a wave's, 729 four waves', 4913 sixteen's)
  if (sb.s <= 2)
    hipLaunchKernelGGL(k_simp_gather<1>, dim3((n_out + 3) / 4), dim3(256), 0, s, (const unsigned*)vol, colv, vp, ct_dev, mb, sb, (const unsigned*)list,
                       n_out, (simp_i64*)sums);
  else if (sb.s == 3)
    hipLaunchKernelGGL(k_simp_gather<4>, dim3(n_out), dim3(256), 0, s, (const unsigned*)vol, colv, vp, ct_dev, mb, sb, (const unsigned*)list, n_out,
                       (simp_i64*)sums);
  else
    hipLaunchKernelGGL(k_simp_gather<16>, dim3(n_out), dim3(1024), 0, s, (const unsigned*)vol, colv, vp, ct_dev, mb, sb, (const unsigned*)list, n_out,
                       (simp_i64*)sums);
  hipLaunchKernelGGL(k_simp_solve, dim3((n_out + 255) / 256), dim3(256), 0, s, vp, sb, (const unsigned*)list, n_out, (const simp_i64*)sums, mode,
                     floor_rel, xyz, normals, rgb);
  if (faces)
    hipLaunchKernelGGL(k_simp_faces<true>, dim3((unsigned)((sb.frows + 3) / 4)), dim3(256), 0, s, (const unsigned*)vol, vp, ct_dev, tri_count, mb, sb,
                       faces);
}

int simplify_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_simp_gather<1>);
}
