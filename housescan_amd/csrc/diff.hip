// diff.hip -- volume differencing for gfx950 (hsk_diff_volume, hsk_download_diff, hsk_diff_at, hsk_adopt_diff; DESIGN.md 3.23 the
// kernels, 8q the rule; tests/diff_twin.py restates the rule in numpy): what changed between two volumes on the same grid.  All
// integers: counts are sums of ones, labels are smallest lin values -- no schedule can change a bit of the result.
//
// k_diff_classify: one streaming sweep over both volumes in the block layout.  A thread takes four 16-B vectors of each (four
// x-adjacent voxels a vector), all eight loads issued before the first is used, and stores four vectors of CLASS WORDS
// (hsk_diff_point.h): pair words in the volume's own layout that components.hip labels as it labels a volume.  A voxel's class is
// made of selects, no branch.  The seven counts ride in one 64-bit register, a byte a class (at most 16 voxels a thread); a wave
// folds them, the block's four waves meet, seven atomics a workgroup of 4096 voxels.
// The regions are components.hip's work, unchanged: launch_comp_label on the class words, launch_comp_records for count and
// box, launch_comp_prune with the FREE fill for the MINOR step (api_diff.hip).
// k_diff_records: per kept region its APPEARED and VANISHED voxels; a wave whose members share one root adds once.
// k_diff_box, k_diff_gather: a box of class bytes and labels, row-major; the point query.  A thread an item.
// k_diff_mark, k_diff_adopt: the adopt set.  Targets as bytes, row-major, a word of four bytes a thread; volume_sweep.hip's three
// passes of Chebyshev reach, one an axis; then the masked copy of cur's words (and colour) into ref, counted first without a
// write (the host writes nothing, and flushes nothing, when the set is empty).
// Every index below is formed from a vector number below n4 or a voxel inside the grid: no access leaves the buffers.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_vol_sweep.h"
#include "hsk_clear_point.h"
#include "hsk_diff_point.h"

__global__ __launch_bounds__(256) void k_diff_classify(const uint4* __restrict__ ref, const uint4* __restrict__ cur, uint4* __restrict__ cls, VolVectors q,
                                                       int thresh, int min_weight, unsigned* __restrict__ counts) {
  uint4 a[4], b[4];
  unsigned at[4];
  bool stored[4], voxels[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    at[c] = (blockIdx.x * 4u + (unsigned)c) * 256u + threadIdx.x;
    unsigned x0, y, z;
    voxels[c] = vol_vector(q, at[c], x0, y, z);
    stored[c] = at[c] < q.n4;
    a[c] = b[c] = make_uint4(0u, 0u, 0u, 0u);
    if (voxels[c]) {  // (a padding plane is no voxel: not read, its class words 0)
      a[c] = ref[at[c]];
      b[c] = cur[at[c]];
    }
  }
  unsigned long long n = 0ull;  // byte k: this thread's voxels of class k
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    unsigned wa[4], wb[4], o[4];
    vol_words(a[c], wa);
    vol_words(b[c], wb);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = diff_class(wa[j], wb[j], thresh, min_weight);
      o[j] = diff_class_word(k);
      n += (voxels[c] ? 1ull : 0ull) << (8 * k);
    }
    if (stored[c]) cls[at[c]] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  unsigned sums[DIFF_CLASSES];
#pragma unroll
  for (int k = 0; k < DIFF_CLASSES; ++k) sums[k] = hsk_wave_sum((unsigned)((n >> (8 * k)) & 0xffull));  // (every lane arrives: nothing above returns)
  const unsigned total = hsk_block_meet<HskSum>(sums);  // (thread v < 7: the workgroup's word v)
  if (threadIdx.x < (unsigned)DIFF_CLASSES && total) atomicAdd(&counts[threadIdx.x], total);
}

// av[2 at] the APPEARED, av[2 at + 1] the VANISHED voxels of region roots[at]; only kept regions have members left
__global__ __launch_bounds__(256) void k_diff_records(const uint4* __restrict__ cls, const uint4* __restrict__ parent, VolVectors q, unsigned n,
                                                      const unsigned* __restrict__ roots, unsigned* __restrict__ av) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
  unsigned x0, y, z;
  const bool live = vol_vector(q, i, x0, y, z);
  unsigned w[4] = {0u, 0u, 0u, 0u}, p[4] = {COMP_NONE, COMP_NONE, COMP_NONE, COMP_NONE};
  if (live) {
    vol_words(cls[i], w);
    vol_words(parent[i], p);
  }
  unsigned key = COMP_NONE, n_a = 0u, n_v = 0u;
  bool one = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = diff_word_class(w[j]);
    if (!diff_changed(c)) p[j] = COMP_NONE;  // (a MINOR voxel keeps its parent entry and is no member)
    if (p[j] == COMP_NONE) continue;
    one = one && (key == COMP_NONE || key == p[j]);
    key = key == COMP_NONE ? p[j] : key;
    n_a += c == DIFF_APPEARED ? 1u : 0u;
    n_v += c == DIFF_VANISHED ? 1u : 0u;
  }
  const bool has = key != COMP_NONE;
  const unsigned k_min = hsk_wave_fold<HskMin>(key);  // (every lane of the wave arrives here: nothing above returns)
  if (__all(one && (!has || key == k_min))) {
    if (k_min == COMP_NONE) return;  // (the whole wave)
    const unsigned s_a = hsk_wave_sum(n_a), s_v = hsk_wave_sum(n_v);
    if (lane == 0u) {
      const unsigned at = comp_search(roots, n, k_min);  // (ends: the interval halves)
      if (at < n && s_a) atomicAdd(&av[2u * at], s_a);
      if (at < n && s_v) atomicAdd(&av[2u * at + 1u], s_v);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] == COMP_NONE) continue;
    const unsigned at = comp_search(roots, n, p[j]);
    if (at < n) atomicAdd(&av[2u * at + (diff_word_class(w[j]) == DIFF_VANISHED ? 1u : 0u)], 1u);
  }
}

// the box lo <= (x, y, z) < hi, row-major: class bytes and (region not null) labels
__global__ __launch_bounds__(256) void k_diff_box(const unsigned* __restrict__ cls, const unsigned* __restrict__ parent, VolVectors q, VoxBox box, unsigned n,
                                                  unsigned char* __restrict__ out, unsigned* __restrict__ region) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  unsigned x, y, z;
  vol_box_voxel(box, i, x, y, z);
  const size_t at = q.g.at_xyz(x + (unsigned)box.lo[0], y + (unsigned)box.lo[1], z + (unsigned)box.lo[2]);
  const int c = diff_word_class(cls[at]);
  out[i] = (unsigned char)c;
  if (region) region[i] = diff_changed(c) ? parent[at] : COMP_NONE;
}

struct DiffClassAt {
  const unsigned* cls;
  CompGrid g;
  HSK_HD_MEMBER int operator()(unsigned x, unsigned y, unsigned z) const { return diff_word_class(cls[g.at_xyz(x, y, z)]); }
};
__global__ __launch_bounds__(256) void k_diff_gather(const unsigned* __restrict__ cls, const unsigned* __restrict__ parent, VolVectors q, SampleVol sv,
                                                     const float* __restrict__ xyz, unsigned n, int radius, unsigned* __restrict__ region,
                                                     unsigned char* __restrict__ out) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  unsigned x, y, z;
  bool inside;
  clear_point_voxel(sv, xyz[3u * e], xyz[3u * e + 1u], xyz[3u * e + 2u], x, y, z, inside);
  int c = DIFF_UNSEEN;
  unsigned l = COMP_NONE;
  if (inside) l = diff_at_pick(q.g, x, y, z, radius, DiffClassAt{cls, q.g}, &c);  // (ends: at most 9^3 trips)
  out[e] = (unsigned char)c;
  region[e] = l == COMP_NONE ? COMP_NONE : parent[q.g.at(l)];
}

// the targets as bytes (0 or 1), row-major; counts[8]: how many
__global__ __launch_bounds__(256) void k_diff_mark(const uint4* __restrict__ cls, VolVectors q, int which, unsigned* __restrict__ mask,
                                                   unsigned* __restrict__ counts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  const bool live = vol_vector(q, i, x0, y, z);
  unsigned m = 0u, n_t = 0u;
  if (live) {
    unsigned w[4];
    vol_words(cls[i], w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool t = diff_adopt_target(diff_word_class(w[j]), which);
      m |= (t ? 1u : 0u) << (8 * j);
      n_t += t ? 1u : 0u;
    }
    mask[(size_t)q.g.lin(x0, y, z) >> 2] = m;
  }
  const unsigned s = hsk_wave_sum(n_t);  // (every lane arrives)
  if ((threadIdx.x & 63u) == 0u && s) atomicAdd(&counts[8], s);
}

// MODE 0: count the adopt set (counts[9]); 1: write cur's words; 2: and cur's colour words; 3: and the colour word 0
template <int MODE>
__global__ __launch_bounds__(256) void k_diff_adopt(uint4* __restrict__ ref, const uint4* __restrict__ cur, unsigned* __restrict__ ref_col,
                                                    const unsigned* __restrict__ cur_col, const unsigned* __restrict__ mask, VolVectors q,
                                                    unsigned* __restrict__ counts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  const bool live = vol_vector(q, i, x0, y, z);
  unsigned n_s = 0u;
  const unsigned m = live ? mask[(size_t)q.g.lin(x0, y, z) >> 2] : 0u;
  if (m != 0u) {
    unsigned wb[4];
    vol_words(cur[i], wb);
    unsigned take = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool s = diff_adopts(((m >> (8 * j)) & 0xffu) != 0u, wb[j]);
      take |= (s ? 1u : 0u) << j;
      n_s += s ? 1u : 0u;
    }
    if (MODE != 0 && take != 0u) {
      unsigned wa[4];
      vol_words(ref[i], wa);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!((take >> j) & 1u)) continue;
        wa[j] = wb[j];
        const size_t l = (size_t)q.g.lin(x0 + (unsigned)j, y, z);
        if (MODE == 2) ref_col[l] = cur_col[l];
        if (MODE == 3) ref_col[l] = 0u;
      }
      ref[i] = make_uint4(wa[0], wa[1], wa[2], wa[3]);
    }
  }
  if (MODE == 0) {
    const unsigned s = hsk_wave_sum(n_s);  // (every lane arrives: nothing above returns)
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(&counts[9], s);
  }
}

size_t diff_layout(const VolParams& vp, void* base, DiffBufs* b) {
  ScratchCarve c{base};
  DiffBufs out;
  out.counts = (unsigned*)c.take(DIFF_COUNTS * 4);
  out.cls = (unsigned*)c.take(hsk_vol_words(vp) * 4);
  out.mask[0] = (unsigned char*)c.take((size_t)vp.X * vp.Y * vp.Z);
  out.mask[1] = (unsigned char*)c.take((size_t)vp.X * vp.Y * vp.Z);
  char* comp = c.take(comp_layout(vp, nullptr, nullptr));
  comp_layout(vp, comp, &out.comp);
  if (b) *b = out;
  return c.bytes;
}

void launch_diff_classify(hipStream_t s, const void* ref, const void* cur, const VolParams& vp, const DiffBufs& b, int thresh, int min_weight) {
  const VolVectors q = vol_vectors(vp);
  (void)hipMemsetAsync(b.counts, 0, DIFF_COUNTS * 4, s);
  hipLaunchKernelGGL(k_diff_classify, dim3((q.n4 + 1023u) / 1024u), dim3(256), 0, s, (const uint4*)ref, (const uint4*)cur, (uint4*)b.cls, q, thresh,
                     min_weight, b.counts);
}

void launch_diff_records(hipStream_t s, const VolParams& vp, const DiffBufs& b, unsigned n, const unsigned* roots, unsigned* av) {
  const VolVectors q = vol_vectors(vp);
  (void)hipMemsetAsync(av, 0, (size_t)n * 8, s);
  hipLaunchKernelGGL(k_diff_records, dim3((q.n4 + 255u) / 256u), dim3(256), 0, s, (const uint4*)b.cls, (const uint4*)b.comp.parent, q, n, roots, av);
}

void launch_diff_box(hipStream_t s, const VolParams& vp, const DiffBufs& b, const int lo[3], const int hi[3], size_t n, unsigned char* cls,
                     unsigned* region) {
  const VolVectors q = vol_vectors(vp);
  hipLaunchKernelGGL(k_diff_box, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const unsigned*)b.cls, (const unsigned*)b.comp.parent, q,
                     vox_box(lo, hi), (unsigned)n, cls, region);
}

void launch_diff_gather(hipStream_t s, const VolParams& vp, const DiffBufs& b, const float* xyz, unsigned n, int radius, unsigned* region,
                        unsigned char* cls) {
  const VolVectors q = vol_vectors(vp);
  hipLaunchKernelGGL(k_diff_gather, dim3((n + 255u) / 256u), dim3(256), 0, s, (const unsigned*)b.cls, (const unsigned*)b.comp.parent, q,
                     hsk_sample_vol(vp), xyz, n, radius, region, cls);
}

void launch_diff_halo(hipStream_t s, const void* cur, const VolParams& vp, const DiffBufs& b, int which, int halo) {
  const VolVectors q = vol_vectors(vp);
  const dim3 vectors((q.n4 + 255u) / 256u);
  (void)hipMemsetAsync(b.counts + 8, 0, 8, s);
  hipLaunchKernelGGL(k_diff_mark, vectors, dim3(256), 0, s, (const uint4*)b.cls, q, which, (unsigned*)b.mask[0], b.counts);
  launch_mask_dilate3(s, vp, b.mask[0], b.mask[1], halo);  // (the result: mask[1])
  hipLaunchKernelGGL((k_diff_adopt<0>), vectors, dim3(256), 0, s, (uint4*)nullptr, (const uint4*)cur, (unsigned*)nullptr, (const unsigned*)nullptr,
                     (const unsigned*)b.mask[1], q, b.counts);
}

void launch_diff_adopt(hipStream_t s, void* ref, const void* cur, unsigned* ref_col, const unsigned* cur_col, const VolParams& vp, const DiffBufs& b) {
  const VolVectors q = vol_vectors(vp);
  const dim3 vectors((q.n4 + 255u) / 256u);
  const unsigned* m = (const unsigned*)b.mask[1];
  if (!ref_col)
    hipLaunchKernelGGL((k_diff_adopt<1>), vectors, dim3(256), 0, s, (uint4*)ref, (const uint4*)cur, ref_col, cur_col, m, q, b.counts);
  else if (cur_col)
    hipLaunchKernelGGL((k_diff_adopt<2>), vectors, dim3(256), 0, s, (uint4*)ref, (const uint4*)cur, ref_col, cur_col, m, q, b.counts);
  else
    hipLaunchKernelGGL((k_diff_adopt<3>), vectors, dim3(256), 0, s, (uint4*)ref, (const uint4*)cur, ref_col, cur_col, m, q, b.counts);
}

int diff_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_diff_classify);
}
