// components.hip -- surface components for gfx950 (hsk_label_components, hsk_download_components, hsk_prune_components; DESIGN.md
// 3.16 the kernels, 8j the rule; tests/components_twin.py restates the rule in numpy): a connected-component labelling of the
// volume's INSIDE voxels (observed, TSDF < 0) under the 6-neighbourhood, as a lock-free union-find over one parent per voxel.
// A voxel's number is lin = (z Y + y) X + x; its parent lives at the voxel's own place in the block layout and holds a lin value.
// The label of a component is its smallest lin, so the result is a set of integers no schedule can change.
//
// TERMINATION.  parent[v] <= v always (hsk_comp_point.h): every walk is strictly decreasing and ends.  No kernel here waits on
// another workgroup, wave or lane: no spin, no flag, no ticket.  Every loop below states why it ends.
//
// k_comp_local: a workgroup owns a tile of 16 x 16 x 8 voxels -- 4 lane-blocks wide, 16 rows, two plane groups: per plane group
// and row 256 contiguous bytes.  A thread loads its two 16-B vectors (both issued before the first is used), the tile's INSIDE
// voxels are united in LDS (8 KiB of labels, local number = (z 16 + y) 16 + x: the same order as lin, so the local root is the
// tile's smallest lin of the component) and each voxel's parent is stored as the lin of its local root -- 16-B stores over the
// whole tile, 0xFFFFFFFF where there is no member, the padding planes included.
// k_comp_merge: the same grid; a workgroup takes its tile's three low faces (256 + 128 + 128 voxel pairs) and unites across them
// in global memory: find on both sides, an atomic minimum on the larger root's entry, again with what the minimum returned.
// k_comp_flatten: a thread per 16-B vector of parents; every member's entry becomes its root, and the roots are counted per grid
// row (y, z).  launch_pack_scan turns the counts into offsets: the roots in ascending lin.
// k_comp_roots: a wave per row that has a root writes the row's roots to their places and resets their records.
// k_comp_records: a thread per vector again; the members' count and box go to their root's record (found by bisection in the
// ascending roots) with integer atomics -- any order gives the same bits.  A wave whose members all share one root (nearly all
// of a wall's) adds once for the wave, behind seven butterflies.
// k_comp_prune: one sweep that rewrites only the words of pruned components.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_vol_sweep.h"

#define CT_VOX 2048u  // voxels of a tile (hsk_vol_sweep.h): 16 x 16 x 8

__global__ __launch_bounds__(256) void k_comp_local(const uint4* __restrict__ vol, uint4* __restrict__ parent, VolTiles q) {
  __shared__ unsigned s_lab[CT_VOX];
  const unsigned tid = threadIdx.x;
  unsigned tx, ty, tz;
  vol_tile(q, blockIdx.x, tx, ty, tz);
  const unsigned c = tid & 15u, yl = tid >> 4, lb = c >> 2, pl = c & 3u;
  const unsigned x0 = 16u * tx + 4u * lb, y = 16u * ty + yl;
  const bool column = x0 < q.g.X && y < q.g.Y;  // (X is a multiple of 4: a vector lies inside the grid or outside it)
  uint4 v[2];
  size_t at[2];
  bool stored[2];
#pragma unroll
  for (int gg = 0; gg < 2; ++gg) {
    const unsigned zg = 2u * tz + (unsigned)gg;
    stored[gg] = column && zg < q.Zg;
    at[gg] = (((size_t)zg * q.g.Y + y) * q.X4 + (x0 >> 2)) * 4u + pl;
    v[gg] = make_uint4(0u, 0u, 0u, 0u);
    if (stored[gg] && 4u * zg + pl < q.g.Z) v[gg] = vol[at[gg]];  // (a padding plane is no voxel: not read, not INSIDE)
  }
  unsigned in = 0u;  // bit 4 gg + j: voxel j of vector gg is INSIDE
#pragma unroll
  for (int gg = 0; gg < 2; ++gg) {
    unsigned w[4];
    vol_words(v[gg], w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned l = (((4u * (unsigned)gg + pl) * 16u + yl) * 16u) + 4u * lb + (unsigned)j;
      const bool inside = comp_inside(w[j]);
      in |= (inside ? 1u : 0u) << (4 * gg + j);
      s_lab[l] = inside ? l : COMP_NONE;
    }
  }
  __syncthreads();
  const CompDirect direct{};
#pragma unroll
  for (int gg = 0; gg < 2; ++gg) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((in >> (4 * gg + j)) & 1u)) continue;
      const unsigned zl = 4u * (unsigned)gg + pl, xl = 4u * lb + (unsigned)j;
      const unsigned l = ((zl * 16u + yl) * 16u) + xl;
      // (an entry that is not COMP_NONE never becomes it: the test for membership can be made at any time.  comp_unite ends
      // by the decreasing invariant, hsk_comp_point.h)
      if (xl > 0u && CompLdsOps::load(&s_lab[l - 1u]) != COMP_NONE) comp_unite<CompLdsOps>(s_lab, direct, l, l - 1u);
      if (yl > 0u && CompLdsOps::load(&s_lab[l - 16u]) != COMP_NONE) comp_unite<CompLdsOps>(s_lab, direct, l, l - 16u);
      if (zl > 0u && CompLdsOps::load(&s_lab[l - 256u]) != COMP_NONE) comp_unite<CompLdsOps>(s_lab, direct, l, l - 256u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int gg = 0; gg < 2; ++gg) {
    if (!stored[gg]) continue;
    unsigned o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = COMP_NONE;
      if ((in >> (4 * gg + j)) & 1u) {
        const unsigned l = (((4u * (unsigned)gg + pl) * 16u + yl) * 16u) + 4u * lb + (unsigned)j;
        const unsigned r = comp_find<CompLdsOps>(s_lab, direct, l);  // (ends: decreasing)
        o[j] = q.g.lin(16u * tx + (r & 15u), 16u * ty + ((r >> 4) & 15u), 8u * tz + (r >> 8));
      }
    }
    parent[at[gg]] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// the members on either side of a tile face become one component
static __device__ __forceinline__ void comp_pair(unsigned* __restrict__ parent, const CompGrid& g, unsigned x, unsigned y, unsigned z, unsigned nx,
                                                 unsigned ny, unsigned nz) {
  const unsigned a = CompGlobalOps::load(parent + g.at_xyz(x, y, z)), b = CompGlobalOps::load(parent + g.at_xyz(nx, ny, nz));
  // (what the entries hold are members of the two voxels' components: as good a start for find as the voxels themselves.
  // comp_unite ends by the decreasing invariant and waits for nobody)
  if (a != COMP_NONE && b != COMP_NONE) comp_unite<CompGlobalOps>(parent, g, a, b);
}
__global__ __launch_bounds__(256) void k_comp_merge(unsigned* __restrict__ parent, VolTiles q) {
  const unsigned tid = threadIdx.x;
  unsigned tx, ty, tz;
  vol_tile(q, blockIdx.x, tx, ty, tz);
  {  // the face z = 8 tz against the plane before it
    const unsigned x = 16u * tx + (tid & 15u), y = 16u * ty + (tid >> 4), z = 8u * tz;
    if (tz > 0u && x < q.g.X && y < q.g.Y && z < q.g.Z) comp_pair(parent, q.g, x, y, z, x, y, z - 1u);
  }
  if (tid < 128u) {  // the face y = 16 ty
    const unsigned x = 16u * tx + (tid & 15u), y = 16u * ty, z = 8u * tz + (tid >> 4);
    if (ty > 0u && x < q.g.X && y < q.g.Y && z < q.g.Z) comp_pair(parent, q.g, x, y, z, x, y - 1u, z);
  } else {  // the face x = 16 tx
    const unsigned t = tid - 128u;
    const unsigned x = 16u * tx, y = 16u * ty + (t & 15u), z = 8u * tz + (t >> 4);
    if (tx > 0u && x < q.g.X && y < q.g.Y && z < q.g.Z) comp_pair(parent, q.g, x, y, z, x - 1u, y, z);
  }
}

__global__ __launch_bounds__(256) void k_comp_flatten(uint4* __restrict__ parent, VolVectors q, unsigned* __restrict__ rows) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  if (!vol_vector(q, i, x0, y, z)) return;
  unsigned p[4];
  vol_words(parent[i], p);
  if ((p[0] & p[1] & p[2] & p[3]) == COMP_NONE) return;
  const unsigned own = q.g.lin(x0, y, z);
  unsigned n_roots = 0u;
  bool changed = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] == COMP_NONE) continue;
    // (no entry is a root's unless it is final: nothing unites any more, so the walk -- which ends, decreasing -- ends at the
    // component's root, whichever of the old or new entries of other voxels it passes)
    const unsigned r = comp_find<CompGlobalOps>((const unsigned*)parent, q.g, p[j]);
    n_roots += r == own + (unsigned)j ? 1u : 0u;
    changed |= r != p[j];
    p[j] = r;
  }
  if (changed) parent[i] = make_uint4(p[0], p[1], p[2], p[3]);
  if (n_roots) atomicAdd(&rows[z * q.g.Y + y], n_roots);
}

// a wave per grid row: the row's roots to their places in the ascending list, their records reset
__global__ __launch_bounds__(256) void k_comp_roots(const unsigned* __restrict__ parent, VolVectors q, const unsigned* __restrict__ rows,
                                                    unsigned* __restrict__ roots, unsigned* __restrict__ table) {
  const unsigned row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= q.g.Y * q.g.Z) return;  // (the whole wave)
  const unsigned off = rows[row], cnt = rows[row + 1u] - off;
  if (cnt == 0u) return;  // (the whole wave)
  const unsigned y = row % q.g.Y, z = row / q.g.Y;
  unsigned run = 0u;
  for (unsigned xb = 0u; xb < q.g.X; xb += 64u) {  // (a wave-uniform trip count)
    const unsigned x = xb + lane, l = q.g.lin(x, y, z);
    const bool is = x < q.g.X && parent[q.g.at_xyz(x, y, z)] == l;
    const unsigned long long b = __ballot(is);
    if (is) {
      const unsigned pos = off + run + (unsigned)__popcll(b & ((1ull << lane) - 1ull));
      roots[pos] = l;
      unsigned* __restrict__ t = table + (size_t)pos * 8u;
      t[0] = 0u;
      t[1] = q.g.X;
      t[2] = q.g.Y;
      t[3] = q.g.Z;
      t[4] = 0u;
      t[5] = 0u;
      t[6] = 0u;
      t[7] = 0u;
    }
    run += (unsigned)__popcll(b);
  }
}

static __device__ __forceinline__ void comp_record_add(unsigned* __restrict__ t, unsigned n, unsigned x_lo, unsigned x_hi, unsigned y_lo, unsigned y_hi,
                                                       unsigned z_lo, unsigned z_hi) {
  atomicAdd(&t[0], n);
  // a bound is only ever lowered (lo) or raised (hi): whatever a load sees, even an old value, is no better than what the entry
  // holds now, so an atomic that would not improve on it is left out -- all but the first few of a large component's.  (The
  // count's add stays, one a wave: what this kernel's time is made of)
  if (x_lo < CompGlobalOps::load(&t[1])) atomicMin(&t[1], x_lo);
  if (y_lo < CompGlobalOps::load(&t[2])) atomicMin(&t[2], y_lo);
  if (z_lo < CompGlobalOps::load(&t[3])) atomicMin(&t[3], z_lo);
  if (x_hi > CompGlobalOps::load(&t[4])) atomicMax(&t[4], x_hi);
  if (y_hi > CompGlobalOps::load(&t[5])) atomicMax(&t[5], y_hi);
  if (z_hi > CompGlobalOps::load(&t[6])) atomicMax(&t[6], z_hi);
}
__global__ __launch_bounds__(256) void k_comp_records(const uint4* __restrict__ parent, VolVectors q, unsigned n, const unsigned* __restrict__ roots,
                                                      unsigned* __restrict__ table) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  unsigned x0, y, z;
  const bool live = vol_vector(q, i, x0, y, z);
  unsigned p[4] = {COMP_NONE, COMP_NONE, COMP_NONE, COMP_NONE};
  if (live) vol_words(parent[i], p);
  // this thread's members: their root when they share one, how many, their span in x
  unsigned key = COMP_NONE, cnt = 0u, j_lo = 4u, j_hi = 0u;
  bool one = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] == COMP_NONE) continue;
    one = one && (key == COMP_NONE || key == p[j]);
    key = key == COMP_NONE ? p[j] : key;
    cnt += 1u;
    j_lo = j_lo < (unsigned)j ? j_lo : (unsigned)j;
    j_hi = (unsigned)j + 1u;
  }
  const bool has = key != COMP_NONE;
  const unsigned k_min = hsk_wave_fold<HskMin>(key);  // (every lane of the wave arrives here: nothing above returns)
  if (__all(one && (!has || key == k_min))) {
    if (k_min == COMP_NONE) return;  // (the whole wave)
    const unsigned c = hsk_wave_sum(cnt);
    const unsigned x_lo = hsk_wave_fold<HskMin>(has ? x0 + j_lo : COMP_NONE), x_hi = hsk_wave_max(has ? x0 + j_hi : 0u);
    const unsigned y_lo = hsk_wave_fold<HskMin>(has ? y : COMP_NONE), y_hi = hsk_wave_max(has ? y + 1u : 0u);
    const unsigned z_lo = hsk_wave_fold<HskMin>(has ? z : COMP_NONE), z_hi = hsk_wave_max(has ? z + 1u : 0u);
    if (lane == 0u) {
      const unsigned at = comp_search(roots, n, k_min);  // (ends: the interval halves)
      if (at < n) comp_record_add(table + (size_t)at * 8u, c, x_lo, x_hi, y_lo, y_hi, z_lo, z_hi);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] == COMP_NONE) continue;
    const unsigned at = comp_search(roots, n, p[j]);
    if (at < n) comp_record_add(table + (size_t)at * 8u, 1u, x0 + (unsigned)j, x0 + (unsigned)j + 1u, y, y + 1u, z, z + 1u);
  }
}

template <bool COLOR>
__global__ __launch_bounds__(256) void k_comp_prune(uint4* __restrict__ vol, unsigned* __restrict__ col, const uint4* __restrict__ parent, VolVectors q,
                                                    const unsigned* __restrict__ roots, const unsigned* __restrict__ table, unsigned n,
                                                    unsigned min_voxels, const unsigned* __restrict__ keep, unsigned n_keep, int fill_free) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  if (!vol_vector(q, i, x0, y, z)) return;
  unsigned p[4];
  vol_words(parent[i], p);
  if ((p[0] & p[1] & p[2] & p[3]) == COMP_NONE) return;
  unsigned w[4];
  vol_words(vol[i], w);
  unsigned last = COMP_NONE;
  bool last_pruned = false, changed = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] == COMP_NONE) continue;
    if (p[j] != last) {  // (x-adjacent members share their root: one look-up a run)
      last = p[j];
      const unsigned at = comp_search(roots, n, last);  // (ends: the interval halves)
      last_pruned = at < n && (table[(size_t)at * 8u] < min_voxels || (n_keep > 0u && comp_search(keep, n_keep, last) == n_keep));
    }
    if (!last_pruned) continue;
    w[j] = fill_free ? ((w[j] & 0xffff0000u) | 0x7fffu) : 0u;
    if (COLOR) col[(size_t)q.g.lin(x0 + (unsigned)j, y, z)] = 0u;
    changed = true;
  }
  if (changed) vol[i] = make_uint4(w[0], w[1], w[2], w[3]);
}

size_t comp_layout(const VolParams& vp, void* base, CompBufs* b) {
  const size_t n_rows = (size_t)vp.Y * (size_t)vp.Z + 1;
  ScratchCarve c{base};
  CompBufs out;
  out.counts = (unsigned*)c.take(64);
  out.rows = (unsigned*)c.take(n_rows * 4);
  out.bsum = (unsigned*)c.take((pack_scan_blocks(n_rows) + 1) * 4);
  out.parent = (unsigned*)c.take(hsk_vol_words(vp) * 4);
  if (b) *b = out;
  return c.bytes;
}

void launch_comp_label(hipStream_t s, const void* vol, const VolParams& vp, const CompBufs& b) {
  const VolTiles q = vol_tiles(vp);
  const size_t n_rows = (size_t)vp.Y * (size_t)vp.Z + 1;
  const unsigned n_tiles = q.ntx * q.nty * q.ntz;
  (void)hipMemsetAsync(b.rows, 0, n_rows * 4, s);
  hipLaunchKernelGGL(k_comp_local, dim3(n_tiles), dim3(256), 0, s, (const uint4*)vol, (uint4*)b.parent, q);
  hipLaunchKernelGGL(k_comp_merge, dim3(n_tiles), dim3(256), 0, s, b.parent, q);
  hipLaunchKernelGGL(k_comp_flatten, dim3((q.n4 + 255u) / 256u), dim3(256), 0, s, (uint4*)b.parent, q, b.rows);
  launch_pack_scan(s, b.rows, n_rows, b.bsum, b.counts);  // (counts -> offsets in place; the last entry and counts[4]: the roots)
}

void launch_comp_records(hipStream_t s, const VolParams& vp, const CompBufs& b, unsigned n, unsigned* roots, unsigned* table) {
  const VolVectors q = vol_vectors(vp);
  const unsigned n_rows = q.g.Y * q.g.Z;
  hipLaunchKernelGGL(k_comp_roots, dim3((n_rows + 3u) / 4u), dim3(256), 0, s, (const unsigned*)b.parent, q, (const unsigned*)b.rows, roots, table);
  hipLaunchKernelGGL(k_comp_records, dim3((q.n4 + 255u) / 256u), dim3(256), 0, s, (const uint4*)b.parent, q, n, (const unsigned*)roots, table);
}

void launch_comp_prune(hipStream_t s, void* vol, unsigned* col, const VolParams& vp, const unsigned* parent, const unsigned* roots,
                       const unsigned* table, unsigned n, unsigned min_voxels, const unsigned* keep, unsigned n_keep, bool fill_free) {
  const VolVectors q = vol_vectors(vp);
  const dim3 grid((q.n4 + 255u) / 256u);
  if (col)
    hipLaunchKernelGGL((k_comp_prune<true>), grid, dim3(256), 0, s, (uint4*)vol, col, (const uint4*)parent, q, roots, table, n, min_voxels, keep, n_keep,
                       fill_free ? 1 : 0);
  else
    hipLaunchKernelGGL((k_comp_prune<false>), grid, dim3(256), 0, s, (uint4*)vol, col, (const uint4*)parent, q, roots, table, n, min_voxels, keep, n_keep,
                       fill_free ? 1 : 0);
}

int comp_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_comp_local);
}
