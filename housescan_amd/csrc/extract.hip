// extract.hip -- read-out kernels for gfx950: zero-crossing cloud extraction, marching tetrahedra and
// marching cubes meshes with their host-built tables.
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_march.h"  // (trilinear: the normals are the raycast's)
#include <type_traits>

// inclusive scan of v over the wave's 64 lanes
static __device__ __forceinline__ int wave_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}
static __device__ __forceinline__ void store3(float* __restrict__ dst, float a, float b, float c) {
  dst[0] = a;
  dst[1] = b;
  dst[2] = c;
}

// ------------------------------------------------------------------------------------------------------
// extractCloud (A.7): a wave per (y,z) row; pass 1 counts, an exclusive scan orders the rows, pass 2 writes
// the points in voxel order (deterministic, identical to the sequential restatement).
// ------------------------------------------------------------------------------------------------------
// the zero crossings from voxel (x, y, z) to its +x, +y, +z neighbours: their count, their points when pts is given, and
// their axes when axes is (two bits each, the first crossing lowest)
static __device__ __forceinline__ int crossing_count(const short2* __restrict__ vol, const VolParams& vp, int x, int y,
                                                     int z, float* pts /* up to 9 floats or null */, unsigned* axes = nullptr) {
  if (axes) *axes = 0u;
  const short2 c = vol[hsk_vox_index(vp, x, y, z - vp.zs0)];
  if (c.y == 0 || c.x == HSK_DIVISOR) return 0;
  const float F = (float)c.x / 32767.0f;
  const float V0 = ((float)x + 0.5f) * vp.cell[0], V1 = ((float)y + 0.5f) * vp.cell[1], V2 = ((float)z + 0.5f) * vp.cell[2];
  int n = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int g = k == 0 ? x : (k == 1 ? y : z);
    const int dim = k == 0 ? vp.X : (k == 1 ? vp.Y : vp.Z);
    if (g + 1 >= dim) continue;
    if (k == 2 && (z + 1 - vp.zs0) >= vp.nzs) continue;  // neighbour plane not stored (cannot happen with halo >= 1)
    const short2 nb = vol[hsk_vox_index(vp, x + (k == 0 ? 1 : 0), y + (k == 1 ? 1 : 0), z - vp.zs0 + (k == 2 ? 1 : 0))];
    if (nb.y == 0 || nb.x == HSK_DIVISOR) continue;
    if (!((c.x > 0 && nb.x < 0) || (c.x < 0 && nb.x > 0))) continue;
    if (pts) {
      const float Fn = (float)nb.x / 32767.0f;
      const float cellk = vp.cell[k];
      const float Vk = k == 0 ? V0 : (k == 1 ? V1 : V2);
      const float Vn = Vk + cellk;
      const float d_inv = 1.0f / (fabsf(F) + fabsf(Fn));
      const float pk = (Vk * fabsf(Fn) + Vn * fabsf(F)) * d_inv;
      pts[3 * n + 0] = k == 0 ? pk : V0;
      pts[3 * n + 1] = k == 1 ? pk : V1;
      pts[3 * n + 2] = k == 2 ? pk : V2;
    }
    if (axes) *axes |= (unsigned)k << (2 * n);
    ++n;
  }
  return n;
}

// A zero crossing, or a cube the level set cuts, needs a NEGATIVE TSDF among the voxels x .. x+1, y .. y+1, z .. z+1.  The
// brick bitfield (integrate: mark_brick_negative; rebuilt on upload) says which bricks have ever held one: a segment of a
// row whose bricks are all clear holds no product -- decided on a few scalar words (the whole field is 4 KiB), without
// touching the volume.  Most of a scanned room is such space: the read-out sweeps follow the surfaces, not the volume
// (round 5; every voxel of the volume was visited three times per cloud before).  Wave-uniform arguments.
// (the row's part of it, once per row: the OR of the brick rows y .. y+1, z .. z+1 as a mask over the x bricks -- up to 64 of
// them; a volume with more bricks along x reports every brick set, i.e. skips nothing)
static __device__ __forceinline__ unsigned long long row_brick_mask(const unsigned* __restrict__ flags, const VolParams& vp, int y, int z) {
  const int bs = vp.bshift, bxn = vp.X >> bs, byn = vp.Y >> bs;
  if (bxn > 64) return ~0ull;
  const int zz0 = z - vp.zs0, zz1 = min(zz0 + 1, vp.nzs - 1);
  const int by0 = y >> bs, by1 = min(y + 1, vp.Y - 1) >> bs;
  const int bz0 = zz0 >> bs, bz1 = zz1 >> bs;
  unsigned long long m = 0ull;
  for (int bz = bz0; bz <= bz1; ++bz)
    for (int by = by0; by <= by1; ++by) {
      const int bit0 = (bz * byn + by) * bxn;  // the brick row's first bit; its bxn bits span at most three words
      // (the words behind the last brick row's own are clamped into the field -- they are super-brick words today, but
      // nothing here depends on what follows the brick bits: whatever is read beyond the row's bxn bits is masked off below)
      const int w0 = bit0 >> 5, sh = bit0 & 31, wlast = hsk_flag_words_total(vp) - 1;
      const unsigned long long lo = (unsigned long long)flags[w0] | ((unsigned long long)flags[min(w0 + 1, wlast)] << 32);
      unsigned long long bits = lo >> sh;
      if (sh != 0 && sh + bxn > 64) bits |= (unsigned long long)flags[min(w0 + 2, wlast)] << (64 - sh);
      m |= bits;
    }
  return bxn == 64 ? m : m & ((1ull << bxn) - 1ull);
}
static __device__ __forceinline__ bool segment_may_hold_negative(unsigned long long row_mask, const VolParams& vp, int xa, int xb) {
  const int bx0 = xa >> vp.bshift, bx1 = min(xb + 1, vp.X - 1) >> vp.bshift;
  if (bx1 >= 64) return true;
  const unsigned long long seg = ((bx1 == 63 ? ~0ull : ((1ull << (bx1 + 1)) - 1ull))) & ~((1ull << bx0) - 1ull);
  return (row_mask & seg) != 0ull;
}

// The sweep every product shares: a wave per row (y, z) -- ny rows per plane, nplanes planes from zo0 -- and a lane per cell
// x < nx, 64 cells at a time.  count(x, y, z, zr) -> the items of the cell (zr = z - zo0).  The count pass (!WRITE) leaves
// the rows' totals in row_count; the write pass takes a row's first slot from row_offset (launch_scan_rows) and calls
// write(x, y, z, zr, n, at) for a cell with n > 0 items: they go to slots at .. at + n - 1, in voxel order.  What a cell
// computes in count and needs again in write, the callers' lambdas keep in a captured local.
template <bool WRITE, class RowCount, class Count, class Write>
static __device__ __forceinline__ void sweep_row(const VolParams& vp, const unsigned* __restrict__ flags, int ny, int nplanes, int nx,
                                                 RowCount* __restrict__ row_count, const unsigned long long* __restrict__ row_offset,
                                                 Count count, Write write) {
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (row >= ny * nplanes) return;
  const int y = row % ny, zr = row / ny, z = vp.zo0 + zr;
  if (WRITE && row_count[row] == 0u) return;  // (the count pass found the row empty)
  unsigned long long base = WRITE ? row_offset[row] : 0;  // (asked for before the mask's loads, used after them)
  const unsigned long long row_mask = row_brick_mask(flags, vp, y, z);
  if (row_mask == 0ull) {
    if constexpr (!WRITE)
      if (lane == 0) row_count[row] = 0u;
    return;
  }
  unsigned total = 0;
  for (int xb = 0; xb < nx; xb += 64) {
    if (!segment_may_hold_negative(row_mask, vp, xb, min(xb + 63, nx - 1))) continue;
    const int x = xb + lane;
    const int n = x < nx ? count(x, y, z, zr) : 0;
    if constexpr (WRITE) {
      const int scan = wave_scan(n);
      if (n) write(x, y, z, zr, n, base + (unsigned long long)(scan - n));
      base += __shfl(scan, 63, 64);
    } else {
      total += hsk_wave_sum((unsigned)n);
    }
  }
  if constexpr (!WRITE)
    if (lane == 0) row_count[row] = total;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_extract(const short2* __restrict__ vol, VolParams vp,
                                                 unsigned* __restrict__ row_count,
                                                 const unsigned long long* __restrict__ row_offset,
                                                 float* __restrict__ xyz, unsigned long long cap, const unsigned* __restrict__ flags) {
  float pts[9];
  sweep_row<WRITE>(
      vp, flags, vp.Y, vp.zo1 - vp.zo0, vp.X, row_count, row_offset,
      [&](int x, int y, int z, int) { return crossing_count(vol, vp, x, y, z, WRITE ? pts : nullptr); },
      [&](int, int, int, int, int n, unsigned long long at) {
        for (int q = 0; q < n; ++q, ++at)
          if (at < cap) store3(xyz + 3 * at, pts[3 * q], pts[3 * q + 1], pts[3 * q + 2]);
      });
}

// exclusive scan of the row counts (up to a few million rows), three small launches: per block of 1024 rows its sum; the
// scan of those sums and the total (one block); the rows' offsets.  (One block walking all the rows, 1024 at a time with a
// Hillis-Steele scan each, took 0.3 ms of a cloud's 3 ms at 512^3.)
static __device__ __forceinline__ unsigned long long block_scan_1024(unsigned long long v, unsigned long long* sh, unsigned long long* total) {
  // inclusive scan over the block's 1024 threads: inside each wave by shuffles, then across the 16 waves
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) sh[wv] = incl;
  __syncthreads();
  unsigned long long base = 0, all = 0;
  for (int w = 0; w < 16; ++w) {
    const unsigned long long t = sh[w];
    if (w < wv) base += t;
    all += t;
  }
  __syncthreads();
  *total = all;
  return base + incl;
}
__global__ __launch_bounds__(1024) void k_scan_rows_sum(const unsigned* __restrict__ cnt, int n, unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long sh[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  unsigned long long all;
  (void)block_scan_1024(i < n ? cnt[i] : 0u, sh, &all);
  if (threadIdx.x == 0) bsum[blockIdx.x] = all;
}
__global__ __launch_bounds__(1024) void k_scan_rows_top(unsigned long long* __restrict__ bsum, int nb, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long sh[16];
  unsigned long long carry = 0;
  for (int b = 0; b < nb; b += 1024) {  // (block-uniform trip count)
    const int i = b + threadIdx.x;
    const unsigned long long v = i < nb ? bsum[i] : 0;
    unsigned long long all;
    const unsigned long long incl = block_scan_1024(v, sh, &all);
    if (i < nb) bsum[i] = carry + incl - v;
    carry += all;
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ __launch_bounds__(1024) void k_scan_rows_fill(const unsigned* __restrict__ cnt, int n, const unsigned long long* __restrict__ bsum,
                                                         unsigned long long* __restrict__ off) {
  __shared__ unsigned long long sh[16];
  const int i = blockIdx.x * 1024 + threadIdx.x;
  const unsigned long long v = i < n ? cnt[i] : 0u;
  unsigned long long all;
  const unsigned long long incl = block_scan_1024(v, sh, &all);
  if (i < n) off[i] = bsum[blockIdx.x] + incl - v;
}
// (row_offset has room for its n entries and, behind them, the per-block sums: hsk_scan_scratch_entries)
size_t hsk_scan_scratch_entries(int nrows) { return (size_t)nrows + (size_t)(nrows + 1023) / 1024; }
void launch_scan_rows(hipStream_t s, const unsigned* cnt, unsigned long long* off, int n, unsigned long long* total) {
  const int nb = (n + 1023) / 1024;
  unsigned long long* bsum = off + n;
  hipLaunchKernelGGL(k_scan_rows_sum, dim3(nb), dim3(1024), 0, s, cnt, n, bsum);
  hipLaunchKernelGGL(k_scan_rows_top, dim3(1), dim3(1024), 0, s, bsum, nb, total);
  hipLaunchKernelGGL(k_scan_rows_fill, dim3(nb), dim3(1024), 0, s, cnt, n, (const unsigned long long*)bsum, off);
}

// ------------------------------------------------------------------------------------------------------
// Mesh extraction ("next" row 3): marching tetrahedra over the TSDF, triangle soup in voxel order.
// A cube (x..x+1, y..y+1, z..z+1) is cut into the six Kuhn tetrahedra round its main diagonal (the same cut in
// every cube, so faces of neighbouring cubes agree); corner i sits at offset (i&1, i>>1&1, i>>2&1).  A cube counts
// only when all eight weights are non-zero; a corner is inside when its TSDF is negative.  An edge vertex is
// P = Pa + (Fa / (Fa - Fb)) (Pb - Pa) with a the LOWER corner index, so both cubes that share an edge produce the
// same bits (the mesh can be welded by exact comparison).  Triangles wind so that the normal points to free space.
// ------------------------------------------------------------------------------------------------------
void hsk_build_tet_table(TetTable* tt) {
  static const int tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
  for (int t = 0; t < 6; ++t)
    for (int m = 0; m < 16; ++m) {
      int in[4], out[4], ni = 0, no = 0;
      for (int v = 0; v < 4; ++v) {
        if ((m >> v) & 1)
          in[ni++] = tet[t][v];
        else
          out[no++] = tet[t][v];
      }
      int e[2][3][2];
      int nt = 0;
      if (ni == 1 || ni == 3) {
        const int apex = ni == 1 ? in[0] : out[0];
        const int* base = ni == 1 ? out : in;
        for (int q = 0; q < 3; ++q) e[0][q][0] = apex, e[0][q][1] = base[q];
        nt = 1;
      } else if (ni == 2) {
        const int quad[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
        const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
        for (int k = 0; k < 2; ++k)
          for (int q = 0; q < 3; ++q) e[k][q][0] = quad[pick[k][q]][0], e[k][q][1] = quad[pick[k][q]][1];
        nt = 2;
      }
      // orientation: the normal of (p0, p1, p2) (edge midpoints) must point from the inside corners to the outside ones
      double ci[3] = {0, 0, 0}, co[3] = {0, 0, 0};
      for (int v = 0; v < ni; ++v)
        for (int a = 0; a < 3; ++a) ci[a] += ((in[v] >> a) & 1) / (double)(ni ? ni : 1);
      for (int v = 0; v < no; ++v)
        for (int a = 0; a < 3; ++a) co[a] += ((out[v] >> a) & 1) / (double)(no ? no : 1);
      for (int k = 0; k < nt; ++k) {
        double pnt[3][3];
        for (int q = 0; q < 3; ++q)
          for (int a = 0; a < 3; ++a) pnt[q][a] = 0.5 * (((e[k][q][0] >> a) & 1) + ((e[k][q][1] >> a) & 1));
        const double u[3] = {pnt[1][0] - pnt[0][0], pnt[1][1] - pnt[0][1], pnt[1][2] - pnt[0][2]};
        const double w[3] = {pnt[2][0] - pnt[0][0], pnt[2][1] - pnt[0][1], pnt[2][2] - pnt[0][2]};
        const double nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double dir = nrm[0] * (co[0] - ci[0]) + nrm[1] * (co[1] - ci[1]) + nrm[2] * (co[2] - ci[2]);
        if (dir < 0)
          for (int a = 0; a < 2; ++a) {
            const int tmp = e[k][1][a];
            e[k][1][a] = e[k][2][a];
            e[k][2][a] = tmp;
          }
      }
      tt->ntri[t][m] = (unsigned char)nt;
      for (int k = 0; k < 2; ++k)
        for (int q = 0; q < 3; ++q) {
          const int a = k < nt ? e[k][q][0] : 0, b = k < nt ? e[k][q][1] : 0;
          tt->edge[t][m][k][q] = (unsigned char)((a < b ? a : b) | ((a < b ? b : a) << 4));  // low corner first
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// Marching cubes (the form PCL's KinFu exports its .ply from, README.md:16-17): one table entry per 8-bit inside mask.
// PCL's 256-case table is not in the reference and cannot be fetched, so the table is GENERATED: on every face of the
// cube the cut edges are joined by segments -- two cut edges: one segment; four (the two diagonal corners inside): two
// segments, each cutting ONE INSIDE corner off, a rule that depends on the face's four signs only, so the two cubes that
// share the face draw the same segments and the surface is closed wherever the cubes are valid.  Every cut edge then has
// exactly two segments: they chain into closed loops, each loop is wound so that its normal points from the inside
// corners to the outside ones and is cut into a fan of triangles from its lowest edge (or the next whose fan keeps out of
// the cube's faces).  820 triangles over the 256
// cases, at most 5 per cube (the classic table's counts).  Vertices as in the tetrahedra form: from the LOWER corner.
// ------------------------------------------------------------------------------------------------------
int hsk_build_cube_table(CubeTable* ct) {
  struct Edge {
    int a, b;  // corners, a < b
  };
  auto code = [](int a, int b) { return a < b ? (a | (b << 4)) : (b | (a << 4)); };
  int worst = 0;
  for (int m = 0; m < 256; ++m) {
    // segments between cut edges, found face by face; link[e][0..1]: the two edges an edge is joined to
    int link[256][2], nlink[256];
    bool cut_edge[256];
    for (int i = 0; i < 256; ++i) nlink[i] = 0, cut_edge[i] = false;
    auto join = [&](int e0, int e1) {
      link[e0][nlink[e0]++] = e1;
      link[e1][nlink[e1]++] = e0;
      cut_edge[e0] = cut_edge[e1] = true;
    };
    for (int ax = 0; ax < 3; ++ax) {
      const int u = ax == 0 ? 1 : 0, v = ax == 2 ? 1 : 2;
      for (int side = 0; side < 2; ++side) {
        int cyc[4];
        const int uv[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
        for (int i = 0; i < 4; ++i) cyc[i] = (side << ax) | (uv[i][0] << u) | (uv[i][1] << v);
        int fe[4], ncut = 0;
        bool cut[4], in[4];
        for (int i = 0; i < 4; ++i) in[i] = ((m >> cyc[i]) & 1) != 0;
        for (int i = 0; i < 4; ++i) {
          fe[i] = code(cyc[i], cyc[(i + 1) & 3]);
          cut[i] = in[i] != in[(i + 1) & 3];
          ncut += cut[i] ? 1 : 0;
        }
        if (ncut == 2) {
          int e0 = -1, e1 = -1;
          for (int i = 0; i < 4; ++i)
            if (cut[i]) (e0 < 0 ? e0 : e1) = fe[i];
          join(e0, e1);
        } else if (ncut == 4) {
          for (int i = 0; i < 4; ++i)
            if (in[i]) join(fe[(i + 3) & 3], fe[i]);  // the two edges that meet in inside corner i
        }
      }
    }
    int nt = 0;
    bool used[256];
    for (int i = 0; i < 256; ++i) used[i] = false;
    for (int start = 0; start < 256; ++start) {  // (edge codes in ascending order: the loops' order, and each loop's first edge)
      if (!cut_edge[start] || used[start]) continue;
      int loop[12], len = 0, prev = -1, cur = start;
      for (;;) {
        loop[len++] = cur;
        used[cur] = true;
        int next = -1;
        for (int q = 0; q < 2; ++q)
          if (link[cur][q] != prev && !used[link[cur][q]]) {
            next = link[cur][q];
            break;
          }
        if (next < 0) break;
        prev = cur;
        cur = next;
      }
      // winding: Newell normal of the loop of edge midpoints against the summed inside -> outside edge directions
      double mid[12][3], nrm[3] = {0, 0, 0}, dir[3] = {0, 0, 0};
      for (int i = 0; i < len; ++i) {
        const int a = loop[i] & 15, b = loop[i] >> 4;
        const bool a_in = ((m >> a) & 1) != 0;
        for (int k = 0; k < 3; ++k) {
          const double pa = (a >> k) & 1, pb = (b >> k) & 1;
          mid[i][k] = 0.5 * (pa + pb);
          dir[k] += a_in ? pb - pa : pa - pb;
        }
      }
      for (int i = 0; i < len; ++i) {
        const double* p = mid[i];
        const double* q = mid[(i + 1) % len];
        nrm[0] += p[1] * q[2] - p[2] * q[1];
        nrm[1] += p[2] * q[0] - p[0] * q[2];
        nrm[2] += p[0] * q[1] - p[1] * q[0];
      }
      if (nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2] < 0)
        for (int i = 1, j = len - 1; i < j; ++i, --j) {
          const int t = loop[i];
          loop[i] = loop[j];
          loop[j] = t;
        }
      // the fan's origin: the first edge of the wound loop none of whose diagonals lies IN a face of the cube (both edges on
      // one face: the neighbour across that face could draw the same line, and the welded mesh would use it four times);
      // one of the first three always qualifies
      auto in_one_face = [](int e, int f) {
        for (int k = 0; k < 3; ++k) {
          const int b = ((e & 15) >> k) & 1;
          if ((((e >> 4) >> k) & 1) == b && (((f & 15) >> k) & 1) == b && (((f >> 4) >> k) & 1) == b) return true;
        }
        return false;
      };
      int origin = 0;
      for (int o = 0; o < len; ++o) {
        bool clean = true;
        for (int k = 2; k + 1 < len; ++k) clean = clean && !in_one_face(loop[o], loop[(o + k) % len]);
        if (clean) {
          origin = o;
          break;
        }
      }
      for (int i = 1; i + 1 < len; ++i) {
        if (nt < HSK_MC_MAXT) {
          ct->edge[m][nt][0] = (unsigned char)loop[origin];
          ct->edge[m][nt][1] = (unsigned char)loop[(origin + i) % len];
          ct->edge[m][nt][2] = (unsigned char)loop[(origin + i + 1) % len];
        }
        ++nt;
      }
    }
    worst = nt > worst ? nt : worst;
    ct->ntri[m] = (unsigned char)(nt < HSK_MC_MAXT ? nt : HSK_MC_MAXT);
    for (int t = nt; t < HSK_MC_MAXT; ++t) ct->edge[m][t][0] = ct->edge[m][t][1] = ct->edge[m][t][2] = 0;
  }
  return worst;  // 5: the table's row length (checked by the caller)
}

// the cube at (x, y, z): its 8 voxels and the inside mask (a corner is inside when its TSDF is negative) -- 0 when a corner
// has never been observed or the level set does not cut the cube
struct Cube {
  short2 v[8];
  unsigned m8;
};
static __device__ __forceinline__ Cube load_cube(const short2* __restrict__ vol, const VolParams& vp, int x, int y, int z) {
  Cube cb;
  bool ok = true;
  cb.m8 = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    cb.v[c] = vol[hsk_vox_index(vp, x + (c & 1), y + ((c >> 1) & 1), z + (c >> 2) - vp.zs0)];
    ok = ok && cb.v[c].y != 0;
    cb.m8 |= (cb.v[c].x < 0 ? 1u : 0u) << c;
  }
  if (!ok || cb.m8 == 255u) cb.m8 = 0u;
  return cb;
}
// the vertex of the edge from voxel ga (TSDF fa; the LOWER corner) to voxel gb (TSDF fb)
static __device__ __forceinline__ void edge_vertex(const VolParams& vp, short fa, short fb, const int* ga, const int* gb, float* p) {
  const float Fa = (float)fa / 32767.0f, Fb = (float)fb / 32767.0f;
  const float w = Fa / (Fa - Fb);
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const float pa = ((float)ga[ax] + 0.5f) * vp.cell[ax];
    const float pb = ((float)gb[ax] + 0.5f) * vp.cell[ax];
    p[ax] = pa + w * (pb - pa);
  }
}
// a triangle of the cube at (x, y, z) from its three edge codes (lower corner | upper corner << 4): 9 floats
static __device__ __forceinline__ void write_triangle(const VolParams& vp, const Cube& cb, int x, int y, int z, const unsigned char* codes,
                                                      float* __restrict__ out) {
  for (int q = 0; q < 3; ++q) {
    const unsigned code = codes[q];
    const int a = (int)(code & 15u), b = (int)(code >> 4);
    // dynamic corner selection without a scratch array
    short fa = 0, fb = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      fa = c == a ? cb.v[c].x : fa;
      fb = c == b ? cb.v[c].x : fb;
    }
    const int ga[3] = {x + (a & 1), y + ((a >> 1) & 1), z + (a >> 2)};
    const int gb[3] = {x + (b & 1), y + ((b >> 1) & 1), z + (b >> 2)};
    float p[3];
    edge_vertex(vp, fa, fb, ga, gb, p);
    store3(out + 3 * q, p[0], p[1], p[2]);
  }
}

// triangles of the cube cb at (x, y, z); when WRITE, stores 9 floats per triangle at tri + 9 * (at + i) while at + i < cap
// ... by marching tetrahedra
template <bool WRITE>
static __device__ int cube_triangles(const VolParams& vp, const TetTable& tt, const Cube& cb, int x, int y, int z, float* __restrict__ tri,
                                     unsigned long long at, unsigned long long cap) {
  if (cb.m8 == 0u) return 0;
  const int tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
  int n = 0;
  for (int t = 0; t < 6; ++t) {
    const unsigned m = ((cb.m8 >> tet[t][0]) & 1u) | (((cb.m8 >> tet[t][1]) & 1u) << 1) | (((cb.m8 >> tet[t][2]) & 1u) << 2) |
                       (((cb.m8 >> tet[t][3]) & 1u) << 3);
    const int nt = tt.ntri[t][m];
    if (WRITE) {
      for (int k = 0; k < nt; ++k) {
        const unsigned long long slot = at + (unsigned long long)(n + k);
        if (slot < cap) write_triangle(vp, cb, x, y, z, tt.edge[t][m][k], tri + 9 * slot);
      }
    }
    n += nt;
  }
  return n;
}
// ... and by marching cubes: straight from the table (in device memory: 4 KiB)
template <bool WRITE>
static __device__ int cube_triangles(const VolParams& vp, const CubeTable* __restrict__ ct, const Cube& cb, int x, int y, int z,
                                     float* __restrict__ tri, unsigned long long at, unsigned long long cap) {
  if (cb.m8 == 0u) return 0;
  const int nt = ct->ntri[cb.m8];
  if (WRITE) {
    for (int k = 0; k < nt; ++k) {
      const unsigned long long slot = at + (unsigned long long)k;
      if (slot < cap) write_triangle(vp, cb, x, y, z, ct->edge[cb.m8][k], tri + 9 * slot);
    }
  }
  return nt;
}

// a row of cubes of either soup: Table is TetTable or const CubeTable*
template <bool WRITE, class Table>
static __device__ __forceinline__ void soup_row(const short2* __restrict__ vol, const VolParams& vp, const Table& table,
                                                unsigned* __restrict__ row_count, const unsigned long long* __restrict__ row_offset,
                                                float* __restrict__ tri, unsigned long long cap, int z_end, const unsigned* __restrict__ flags) {
  Cube cb;
  sweep_row<WRITE>(
      vp, flags, vp.Y - 1, z_end - vp.zo0, vp.X - 1, row_count, row_offset,
      [&](int x, int y, int z, int) {
        cb = load_cube(vol, vp, x, y, z);
        return cube_triangles<false>(vp, table, cb, x, y, z, nullptr, 0, 0);
      },
      [&](int x, int y, int z, int, int, unsigned long long at) { cube_triangles<true>(vp, table, cb, x, y, z, tri, at, cap); });
}
template <bool WRITE>
__global__ __launch_bounds__(256) void k_extract_mesh(const short2* __restrict__ vol, VolParams vp, TetTable tt,
                                                      unsigned* __restrict__ row_count,
                                                      const unsigned long long* __restrict__ row_offset,
                                                      float* __restrict__ tri, unsigned long long cap, int z_end, const unsigned* __restrict__ flags) {
  soup_row<WRITE>(vol, vp, tt, row_count, row_offset, tri, cap, z_end, flags);
}
template <bool WRITE>
__global__ __launch_bounds__(256) void k_extract_mesh_mc(const short2* __restrict__ vol, VolParams vp, const CubeTable* __restrict__ ct,
                                                         unsigned* __restrict__ row_count,
                                                         const unsigned long long* __restrict__ row_offset,
                                                         float* __restrict__ tri, unsigned long long cap, int z_end, const unsigned* __restrict__ flags) {
  soup_row<WRITE>(vol, vp, ct, row_count, row_offset, tri, cap, z_end, flags);
}

// cubes whose base plane this context owns and whose upper plane is stored
int hsk_mesh_z_end(const VolParams& vp) {
  int z_end = vp.zo1;
  if (z_end > vp.zs0 + vp.nzs - 1) z_end = vp.zs0 + vp.nzs - 1;
  if (z_end > vp.Z - 1) z_end = vp.Z - 1;
  return z_end > vp.zo0 ? z_end : vp.zo0;
}

// Both passes of a product over nrows rows, a block per four: without an output buffer the count pass -- launch(false_type,
// grid) and the rows' scan, whose total is zeroed when there are no rows -- and with one the write pass, launch(true_type, grid).
template <class Launch>
static void launch_two_pass(hipStream_t s, int nrows, unsigned* row_count, unsigned long long* row_offset, unsigned long long* total,
                            bool write, Launch launch) {
  if (nrows <= 0) {
    if (!write) (void)hipMemsetAsync(total, 0, 8, s);
    return;
  }
  const dim3 grid((unsigned)((nrows + 3) / 4));
  if (write) {
    launch(std::true_type{}, grid);
  } else {
    launch(std::false_type{}, grid);
    launch_scan_rows(s, row_count, row_offset, nrows, total);
  }
}
void launch_extract(hipStream_t s, const void* vol, const VolParams& vp, unsigned* row_count, unsigned long long* row_offset,
                    unsigned long long* total, float* xyz, unsigned long long cap, const unsigned* flags) {
  launch_two_pass(s, vp.Y * (vp.zo1 - vp.zo0), row_count, row_offset, total, xyz != nullptr, [&](auto write, dim3 grid) {
    hipLaunchKernelGGL(k_extract<decltype(write)::value>, grid, dim3(256), 0, s, (const short2*)vol, vp, row_count,
                       (const unsigned long long*)row_offset, xyz, cap, flags);
  });
}
void launch_extract_mesh(hipStream_t s, const void* vol, const VolParams& vp, const TetTable& tt, unsigned* row_count,
                         unsigned long long* row_offset, unsigned long long* total, float* tri, unsigned long long cap, const unsigned* flags) {
  const int z_end = hsk_mesh_z_end(vp);
  launch_two_pass(s, (vp.Y - 1) * (z_end - vp.zo0), row_count, row_offset, total, tri != nullptr, [&](auto write, dim3 grid) {
    hipLaunchKernelGGL(k_extract_mesh<decltype(write)::value>, grid, dim3(256), 0, s, (const short2*)vol, vp, tt, row_count,
                       (const unsigned long long*)row_offset, tri, cap, z_end, flags);
  });
}
void launch_extract_mesh_mc(hipStream_t s, const void* vol, const VolParams& vp, const CubeTable* ct_dev, unsigned* row_count,
                            unsigned long long* row_offset, unsigned long long* total, float* tri, unsigned long long cap, const unsigned* flags) {
  const int z_end = hsk_mesh_z_end(vp);
  launch_two_pass(s, (vp.Y - 1) * (z_end - vp.zo0), row_count, row_offset, total, tri != nullptr, [&](auto write, dim3 grid) {
    hipLaunchKernelGGL(k_extract_mesh_mc<decltype(write)::value>, grid, dim3(256), 0, s, (const short2*)vol, vp, ct_dev, row_count,
                       (const unsigned long long*)row_offset, tri, cap, z_end, flags);
  });
}

// ------------------------------------------------------------------------------------------------------
// The cloud with normals and colour (hsk_extract_cloud_attrs): the write pass of the cloud again, in a kernel of its own;
// the points, their count and order come from k_extract's sweep and crossing_count, so xyz is bit-identical.
//   normal: the raycast's -- central differences of the trilinear TSDF one cell either side, scaled by 1 / |n| -- where
//           floor(p / cell) lies in (1, dims - 2) on every axis (tests/np_twin.py: the raycast's `deep`), NaN elsewhere
//   colour: of the crossing's voxel with the smaller |tsdf| (the first on a tie), of the other when that one has colour
//           weight 0, (0, 0, 0) and one count in n_uncolored when both have
// ------------------------------------------------------------------------------------------------------
// the normal rule at p: NaN x 3 outside the (1, dims - 2) interior (shared by the cloud's and the indexed mesh's attributes)
static __device__ __forceinline__ void attr_normal(const short2* __restrict__ vol, const VolParams& vp, float px, float py, float pz,
                                                   float* nx, float* ny, float* nz) {
  *nx = HSK_NANF, *ny = HSK_NANF, *nz = HSK_NANF;
  const float qx = floorf(px / vp.cell[0]), qy = floorf(py / vp.cell[1]), qz = floorf(pz / vp.cell[2]);
  if (qx > 1.0f && qx < (float)(vp.X - 2) && qy > 1.0f && qy < (float)(vp.Y - 2) && qz > 1.0f && qz < (float)(vp.Z - 2)) {
    // (one axis at a time, in a loop that stays a loop: written out, the six branch-free samples keep all 48 taps in flight and
    // cost both kernels waves -- profiles/r16/refactor_notes.md; p +- 0.0f is p)
    float gxn = 0.0f, gyn = 0.0f, gzn = 0.0f;
#pragma nounroll
    for (int ax = 0; ax < 3; ++ax) {
      const float ex = ax == 0 ? vp.cell[0] : 0.0f, ey = ax == 1 ? vp.cell[1] : 0.0f, ez = ax == 2 ? vp.cell[2] : 0.0f;
      const float d = trilinear(vol, vp, px + ex, py + ey, pz + ez) - trilinear(vol, vp, px - ex, py - ey, pz - ez);
      gxn = ax == 0 ? d : gxn;
      gyn = ax == 1 ? d : gyn;
      gzn = ax == 2 ? d : gzn;
    }
    const float ninv = 1.0f / sqrtf(hsk_dot3(gxn, gyn, gzn, gxn, gyn, gzn));
    *nx = gxn * ninv;
    *ny = gyn * ninv;
    *nz = gzn * ninv;
  }
}
// the colour rule of the edge between voxel a = (x, y, zz) and its neighbour b (stored planes): the (r, g, b, w) word chosen,
// 0 with one count in *uncol when neither voxel has colour weight
static __device__ __forceinline__ unsigned attr_color(const short2* __restrict__ vol, const unsigned* __restrict__ colv, const VolParams& vp,
                                                      int x, int y, int zz, int bx, int by, int bzz, unsigned* uncol) {
  const int ta = vol[hsk_vox_index(vp, x, y, zz)].x, tb = vol[hsk_vox_index(vp, bx, by, bzz)].x;
  const unsigned ca = colv[((size_t)zz * vp.Y + y) * vp.X + x], cb = colv[((size_t)bzz * vp.Y + by) * vp.X + bx];
  const bool take_a = (ta < 0 ? -ta : ta) <= (tb < 0 ? -tb : tb);
  unsigned cw = take_a ? ca : cb;
  if ((cw >> 24) == 0u) cw = take_a ? cb : ca;
  if ((cw >> 24) == 0u) {
    cw = 0u;
    *uncol += 1u;
  }
  return cw;
}
// the attributes of item `at`, a point p on the edge between voxel (x, y, zz) and its neighbour (bx, by, bzz) (stored planes):
// the normal rule at p, the colour rule on the edge (either array may be null)
static __device__ __forceinline__ void write_attrs(const short2* __restrict__ vol, const unsigned* __restrict__ colv, const VolParams& vp,
                                                   unsigned long long at, const float* p, int x, int y, int zz, int bx, int by, int bzz,
                                                   float* __restrict__ normals, unsigned char* __restrict__ rgb, unsigned* uncol) {
  if (normals) {
    float nx, ny, nz;
    attr_normal(vol, vp, p[0], p[1], p[2], &nx, &ny, &nz);
    store3(normals + 3 * at, nx, ny, nz);
  }
  if (rgb) {
    const unsigned cw = attr_color(vol, colv, vp, x, y, zz, bx, by, bzz, uncol);
    rgb[3 * at] = (unsigned char)(cw & 255u);
    rgb[3 * at + 1] = (unsigned char)((cw >> 8) & 255u);
    rgb[3 * at + 2] = (unsigned char)((cw >> 16) & 255u);
  }
}
// ... and, once per wave, the lanes' uncoloured items into the product's counter
static __device__ __forceinline__ void add_uncolored(unsigned uncol, const unsigned char* rgb, unsigned long long* __restrict__ n_uncolored) {
  if (rgb && n_uncolored) {
    const unsigned sum = hsk_wave_sum(uncol);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(n_uncolored, (unsigned long long)sum);
  }
}

__global__ __launch_bounds__(256) void k_extract_attrs(const short2* __restrict__ vol, const unsigned* __restrict__ colv, VolParams vp,
                                                       const unsigned* __restrict__ row_count,
                                                       const unsigned long long* __restrict__ row_offset, float* __restrict__ xyz,
                                                       float* __restrict__ normals, unsigned char* __restrict__ rgb,
                                                       unsigned long long cap, unsigned long long* __restrict__ n_uncolored,
                                                       const unsigned* __restrict__ flags) {
  float pts[9];
  unsigned axes = 0, uncol = 0;
  sweep_row<true>(
      vp, flags, vp.Y, vp.zo1 - vp.zo0, vp.X, row_count, row_offset,
      [&](int x, int y, int z, int) { return crossing_count(vol, vp, x, y, z, pts, &axes); },
      [&](int x, int y, int z, int, int n, unsigned long long at) {
        for (int q = 0; q < n; ++q, ++at) {
          if (at >= cap) continue;
          store3(xyz + 3 * at, pts[3 * q], pts[3 * q + 1], pts[3 * q + 2]);
          const int k = (int)((axes >> (2 * q)) & 3u), zz = z - vp.zs0;
          write_attrs(vol, colv, vp, at, pts + 3 * q, x, y, zz, x + (k == 0 ? 1 : 0), y + (k == 1 ? 1 : 0), zz + (k == 2 ? 1 : 0), normals, rgb,
                      &uncol);
        }
      });
  add_uncolored(uncol, rgb, n_uncolored);
}

// the write pass of the cloud with its attributes, behind launch_extract's count pass on the same volume
void launch_extract_attrs(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const unsigned* row_count,
                          const unsigned long long* row_offset, float* xyz, float* normals, unsigned char* rgb,
                          unsigned long long cap, unsigned long long* n_uncolored, const unsigned* flags) {
  const int nrows = vp.Y * (vp.zo1 - vp.zo0);
  hipLaunchKernelGGL(k_extract_attrs, dim3((nrows + 3) / 4), dim3(256), 0, s, (const short2*)vol, colv, vp, row_count, row_offset, xyz,
                     normals, rgb, cap, n_uncolored, flags);
}

// ------------------------------------------------------------------------------------------------------
// The marching-cubes surface as an INDEXED mesh (hsk_extract_mesh_indexed), welded by edge identity: a vertex is computed
// from its edge's lower corner, so every cube that shares an edge produces the same bits, and the edge names the vertex.
// A GRID ROW (y, z) holds the edges whose lower corner lies on it, bit 3 x + axis, in segments of 64 voxels (3 words):
//   mark     (the cubes' sweep, counting): each valid, cut cube ORs the bits of its cut edges into the
//            four grid rows its edges start on, and the row's triangles are counted (the faces' row offsets)
//   rows     (a wave per grid row): its vertex count, and per segment the count of the segments before it
//   (both row counts scanned by launch_scan_rows: the vertex order is the bits' order -- plane, row, x, axis)
//   vertices (a wave per grid row, a lane per voxel): the soup's edge_vertex, the cloud's write_attrs
//   faces    (the cubes' sweep, writing): each corner's index is its edge's rank, at most three popcounts
// ------------------------------------------------------------------------------------------------------
// set bits below bit o (0 .. 191) of a segment's three words
static __device__ __forceinline__ unsigned mi_rank(unsigned long long w0, unsigned long long w1, unsigned long long w2, int o) {
  const unsigned long long m0 = o >= 64 ? ~0ull : ((1ull << o) - 1ull);
  const unsigned long long m1 = o >= 128 ? ~0ull : (o <= 64 ? 0ull : ((1ull << (o - 64)) - 1ull));
  const unsigned long long m2 = o <= 128 ? 0ull : ((1ull << (o - 128)) - 1ull);
  return (unsigned)(__popcll(w0 & m0) + __popcll(w1 & m1) + __popcll(w2 & m2));
}

size_t mesh_index_layout(const VolParams& vp, void* base, MeshIndexBufs* b) {
  const int z_end = hsk_mesh_z_end(vp);
  const int rows = z_end > vp.zo0 ? vp.Y * (z_end - vp.zo0 + 1) : 0;
  const int nseg = (vp.X + 63) / 64;
  ScratchCarve c{base};
  MeshIndexBufs m;
  m.rows = rows;
  m.nseg = nseg;
  m.totals = (unsigned long long*)c.take(32);
  m.bits = (unsigned long long*)c.take((size_t)rows * 3 * nseg * 8);
  m.voff = (unsigned long long*)c.take(hsk_scan_scratch_entries(rows) * 8);
  m.vcount = (unsigned*)c.take((size_t)rows * 4);
  m.segbase = (unsigned short*)c.take((size_t)rows * nseg * 2);
  if (b) *b = m;
  return c.bytes;
}

__global__ __launch_bounds__(256) void k_mesh_index_mark(const short2* __restrict__ vol, VolParams vp, const CubeTable* __restrict__ ct,
                                                         unsigned* __restrict__ row_count, unsigned* __restrict__ bits, int nseg, int z_end,
                                                         const unsigned* __restrict__ flags) {
  const size_t row_words = (size_t)nseg * 6;  // (32-bit words of a grid row)
  sweep_row<false>(
      vp, flags, vp.Y - 1, z_end - vp.zo0, vp.X - 1, row_count, (const unsigned long long*)nullptr,
      [&](int x, int y, int z, int zr) {
        const unsigned m8 = load_cube(vol, vp, x, y, z).m8;
        if (m8 == 0u) return 0;
        // the cut edges by the grid row they start on (dy, dz), as bits 0 .. 5 above bit 3 x: the x edge of the row's corner
        // (bit 0), and on the lower rows the y edges (bits 1, 4) or z edges (bits 2, 5) of the corners x and x + 1
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int dy = r & 1, dz = r >> 1;
          const int c0 = dy * 2 + dz * 4;
          unsigned m = ((m8 >> c0) ^ (m8 >> (c0 + 1))) & 1u;
          if (dy == 0)
            m |= ((((m8 >> c0) ^ (m8 >> (c0 + 2))) & 1u) << 1) | ((((m8 >> (c0 + 1)) ^ (m8 >> (c0 + 3))) & 1u) << 4);
          if (dz == 0)
            m |= ((((m8 >> c0) ^ (m8 >> (c0 + 4))) & 1u) << 2) | ((((m8 >> (c0 + 1)) ^ (m8 >> (c0 + 5))) & 1u) << 5);
          if (m == 0u) continue;
          const int bit = 3 * x;
          unsigned* w = bits + (size_t)((zr + dz) * vp.Y + y + dy) * row_words + (bit >> 5);
          const int sh = bit & 31;
          atomicOr(w, m << sh);
          if (sh > 26 && (m >> (32 - sh)) != 0u) atomicOr(w + 1, m >> (32 - sh));
        }
        return (int)ct->ntri[m8];
      },
      [](int, int, int, int, int, unsigned long long) {});
}

__global__ __launch_bounds__(256) void k_mesh_index_rows(const unsigned long long* __restrict__ bits, int rows, int nseg,
                                                         unsigned* __restrict__ vcount, unsigned short* __restrict__ segbase) {
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (row >= rows) return;
  const unsigned long long* w = bits + (size_t)row * 3 * nseg;
  unsigned carry = 0;
  for (int j0 = 0; j0 < 3 * nseg; j0 += 64) {  // a lane per word
    const int j = j0 + lane;
    const unsigned c = j < 3 * nseg ? (unsigned)__popcll(w[j]) : 0u;
    unsigned incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (j < 3 * nseg && j % 3 == 0) segbase[(size_t)row * nseg + j / 3] = (unsigned short)(carry + incl - c);
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) vcount[row] = carry;
}

__global__ __launch_bounds__(256) void k_mesh_index_verts(const short2* __restrict__ vol, const unsigned* __restrict__ colv, VolParams vp,
                                                          MeshIndexBufs mb, float* __restrict__ xyz, float* __restrict__ normals,
                                                          unsigned char* __restrict__ rgb, unsigned long long* __restrict__ n_uncolored) {
  const int lane = threadIdx.x & 63;
  const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (row >= mb.rows) return;
  if (mb.vcount[row] == 0u) return;
  const int y = row % vp.Y, z = vp.zo0 + row / vp.Y, zz = z - vp.zs0;
  const unsigned long long* w = mb.bits + (size_t)row * 3 * mb.nseg;
  const unsigned long long row_base = mb.voff[row];
  unsigned uncol = 0;
  for (int s = 0; s < mb.nseg; ++s) {
    const unsigned long long w0 = w[3 * s], w1 = w[3 * s + 1], w2 = w[3 * s + 2];
    if ((w0 | w1 | w2) == 0ull) continue;
    const int o = 3 * lane, j = o >> 6, sh = o & 63;
    const unsigned long long lo = j == 0 ? w0 : (j == 1 ? w1 : w2), hi = j == 0 ? w1 : w2;
    const unsigned b3 = ((unsigned)(lo >> sh) | (sh > 61 ? (unsigned)(hi << (64 - sh)) : 0u)) & 7u;
    if (b3 == 0u) continue;
    const int x = 64 * s + lane;
    unsigned long long at = row_base + mb.segbase[(size_t)row * mb.nseg + s] + mi_rank(w0, w1, w2, o);
    const short fa = vol[hsk_vox_index(vp, x, y, zz)].x;
    for (int k = 0; k < 3; ++k) {
      if (!((b3 >> k) & 1u)) continue;
      const int bx = x + (k == 0 ? 1 : 0), by = y + (k == 1 ? 1 : 0), bzz = zz + (k == 2 ? 1 : 0);
      const short fb = vol[hsk_vox_index(vp, bx, by, bzz)].x;
      const int ga[3] = {x, y, z};
      const int gb[3] = {bx, by, z + (k == 2 ? 1 : 0)};
      float p[3];
      edge_vertex(vp, fa, fb, ga, gb, p);
      if (xyz) store3(xyz + 3 * at, p[0], p[1], p[2]);
      write_attrs(vol, colv, vp, at, p, x, y, zz, bx, by, bzz, normals, rgb, &uncol);
      ++at;
    }
  }
  add_uncolored(uncol, rgb, n_uncolored);
}

__global__ __launch_bounds__(256) void k_mesh_index_faces(const short2* __restrict__ vol, VolParams vp, const CubeTable* __restrict__ ct,
                                                          const unsigned* __restrict__ row_count, const unsigned long long* __restrict__ row_offset,
                                                          MeshIndexBufs mb, int* __restrict__ faces, int z_end, const unsigned* __restrict__ flags) {
  unsigned m8 = 0;
  sweep_row<true>(
      vp, flags, vp.Y - 1, z_end - vp.zo0, vp.X - 1, row_count, row_offset,
      [&](int x, int y, int z, int) {
        m8 = load_cube(vol, vp, x, y, z).m8;
        return m8 ? (int)ct->ntri[m8] : 0;
      },
      [&](int x, int y, int, int zr, int n, unsigned long long at) {
        for (int t = 0; t < n; ++t)
          for (int q = 0; q < 3; ++q) {
            const unsigned code = ct->edge[m8][t][q];
            const int a = (int)(code & 15u), ab = (int)((code >> 4) ^ code) & 7;  // (b ^ a: the edge's axis as 1, 2 or 4)
            const int axis = ab == 1 ? 0 : (ab == 2 ? 1 : 2);
            const int gx = x + (a & 1), g = (zr + (a >> 2)) * vp.Y + y + ((a >> 1) & 1);
            const int s = gx >> 6;
            const unsigned long long* w = mb.bits + ((size_t)g * mb.nseg + s) * 3;
            const unsigned long long idx = mb.voff[g] + mb.segbase[(size_t)g * mb.nseg + s] + mi_rank(w[0], w[1], w[2], 3 * (gx & 63) + axis);
            faces[3 * (at + t) + q] = (int)idx;
          }
      });
}

// the count pass: zeroed edge bits, marked, the grid rows' counts; both row scans (totals[0] vertices, totals[1] faces)
void launch_mesh_index_count(hipStream_t s, const void* vol, const VolParams& vp, const CubeTable* ct_dev, unsigned* row_count,
                             unsigned long long* row_offset, const MeshIndexBufs& mb, const unsigned* flags) {
  const int z_end = hsk_mesh_z_end(vp);
  const int nrows = (vp.Y - 1) * (z_end - vp.zo0);
  if (nrows <= 0 || mb.rows <= 0) {
    (void)hipMemsetAsync(mb.totals, 0, 16, s);
    return;
  }
  (void)hipMemsetAsync(mb.bits, 0, (size_t)mb.rows * 3 * mb.nseg * 8, s);
  hipLaunchKernelGGL(k_mesh_index_mark, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, (const short2*)vol, vp, ct_dev, row_count,
                     (unsigned*)mb.bits, mb.nseg, z_end, flags);
  hipLaunchKernelGGL(k_mesh_index_rows, dim3((unsigned)((mb.rows + 3) / 4)), dim3(256), 0, s, (const unsigned long long*)mb.bits, mb.rows,
                     mb.nseg, mb.vcount, mb.segbase);
  launch_scan_rows(s, mb.vcount, mb.voff, mb.rows, mb.totals);
  launch_scan_rows(s, row_count, row_offset, nrows, mb.totals + 1);
}
// the write passes behind it: the vertices (any of xyz / normals / rgb; rgb needs colv), the faces (when non-null)
void launch_mesh_index_write(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const CubeTable* ct_dev,
                             const unsigned* row_count, const unsigned long long* row_offset, const MeshIndexBufs& mb, float* xyz,
                             float* normals, unsigned char* rgb, unsigned long long* n_uncolored, int* faces, const unsigned* flags) {
  const int z_end = hsk_mesh_z_end(vp);
  const int nrows = (vp.Y - 1) * (z_end - vp.zo0);
  if (nrows <= 0 || mb.rows <= 0) return;
  if (xyz || normals || rgb)
    hipLaunchKernelGGL(k_mesh_index_verts, dim3((unsigned)((mb.rows + 3) / 4)), dim3(256), 0, s, (const short2*)vol, colv, vp, mb, xyz,
                       normals, rgb, n_uncolored);
  if (faces)
    hipLaunchKernelGGL(k_mesh_index_faces, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s, (const short2*)vol, vp, ct_dev, row_count,
                       row_offset, mb, faces, z_end, flags);
}

// The code object of this file is loaded when one of its kernels is first used (deferred loading): 0.7 ms that the first
// product of a process would otherwise pay on whatever thread asks for it.  hsk_prepare_readout asks here instead.
int extract_warm() {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, (const void*)k_extract<false>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_extract<true>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_extract_mesh_mc<false>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_extract_mesh_mc<true>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_extract_mesh<false>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_extract_mesh<true>);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_scan_rows_sum);
  return (int)e;
}

