// split.hip -- the scene split for gfx950 (hsk_split_scene, hsk_download_split, hsk_split_at, hsk_remove_objects; DESIGN.md 3.24 the
// kernels, 8r the rule; tests/split_twin.py restates the rule in numpy): which INSIDE voxels belong to the building's planes and
// which to the things standing in it.  Integers, and the ALIGNED test's three binary64 products, formed the same way by every
// thread: counts are sums of ones, labels are smallest lin values, masks are ORs, heights are minima and maxima -- no schedule can
// change a bit of the result.
//
// k_split_classify: one streaming sweep over the volume in the block layout, a thread a 16-B vector (four x-adjacent voxels), one
// vector load.  A wave none of whose voxels is INSIDE -- over 90 % of a room -- stores its zeros and leaves.  A thread with an
// INSIDE voxel loads the four neighbour vectors in y and z and the two neighbour words in x, forms the gradients, and walks the
// planes (at most 64, from a device table, the index wave-uniform): a plane's distance is formed once for the vector's first voxel
// and advances along x by 2 Q_x.  It stores four CLASS WORDS (hsk_split_point.h): pair words in the volume's own layout that
// components.hip labels as it labels a volume.
// The objects are components.hip's work, unchanged: launch_comp_label on the class words, launch_comp_records for count and box,
// launch_comp_prune with the FREE fill for the MINOR step (api_split.hip).
// k_split_records: per kept object the sums of its voxels' coordinates, its contacts by kind, its plane mask and its heights over
// the floor: integer atomics only.
// k_split_box, k_split_gather: a box of class bytes, plane bytes and labels, row-major; the point query.  A thread an item.
// k_split_mark, k_split_restore: the removal.  The selected objects' voxels as bytes, row-major, a word of four bytes a thread;
// volume_sweep.hip's three passes of Chebyshev reach; then the masked write of rules 1 and 2, counted first without a write (the
// host writes nothing, and flushes nothing, when nothing would be written).
// No loop's trip count depends on data beyond the bisection of comp_search (the interval halves); no kernel waits on another
// workgroup.  Every index below is formed from a vector number below n4 or a voxel inside the grid: no access leaves the buffers.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_vol_sweep.h"
#include "hsk_clear_point.h"
#include "hsk_split_point.h"

__global__ __launch_bounds__(256) void k_split_classify(const uint4* __restrict__ vol, uint4* __restrict__ cls, VolVectors q,
                                                        const SplitPlaneQ* __restrict__ planes, SplitRule r, unsigned* __restrict__ counts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  const bool live = vol_vector(q, i, x0, y, z);
  unsigned w[4] = {0u, 0u, 0u, 0u};
  if (live) vol_words(vol[i], w);  // (a padding plane is no voxel: not read, its class words 0)
  unsigned in = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) in |= (comp_inside(w[j]) ? 1u : 0u) << j;
  if (!__any(in != 0u)) {  // (the whole wave)
    if (i < q.n4) cls[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  unsigned o[4] = {0u, 0u, 0u, 0u};
  unsigned n_cls[SPLIT_CLASSES] = {0u, 0u, 0u, 0u, 0u, 0u, 0u}, n_edge = 0u, n_flat = 0u;
  if (in != 0u) {
    const unsigned* __restrict__ words = (const unsigned*)vol;
    unsigned row[6] = {0u, w[0], w[1], w[2], w[3], 0u};
    unsigned ym[4] = {0u, 0u, 0u, 0u}, yp[4] = {0u, 0u, 0u, 0u}, zm[4] = {0u, 0u, 0u, 0u}, zp[4] = {0u, 0u, 0u, 0u};
    if (x0 > 0u) row[0] = words[q.g.at_xyz(x0 - 1u, y, z)];
    if (x0 + 4u < q.g.X) row[5] = words[q.g.at_xyz(x0 + 4u, y, z)];
    if (y > 0u) vol_words(vol[q.g.at_xyz(x0, y - 1u, z) >> 2], ym);
    if (y + 1u < q.g.Y) vol_words(vol[q.g.at_xyz(x0, y + 1u, z) >> 2], yp);
    if (z > 0u) vol_words(vol[q.g.at_xyz(x0, y, z - 1u) >> 2], zm);
    if (z + 1u < q.g.Z) vol_words(vol[q.g.at_xyz(x0, y, z + 1u) >> 2], zp);
    long long G[4][3], G2[4];
    SplitPick c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      G[j][0] = (long long)split_grad(row[j], row[j + 1], row[j + 2]) * r.w[0];
      G[j][1] = (long long)split_grad(ym[j], w[j], yp[j]) * r.w[1];
      G[j][2] = (long long)split_grad(zm[j], w[j], zp[j]) * r.w[2];
      G2[j] = G[j][0] * G[j][0] + G[j][1] * G[j][1] + G[j][2] * G[j][2];
      c[j] = split_pick_none();
    }
    for (int k = 0; k < r.n_planes; ++k) {  // (a wave-uniform trip count)
      const SplitPlaneQ p = planes[k];
      long long s = split_s(p, x0, y, z);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool near = ((in >> j) & 1u) != 0u && split_near(s, r);
        split_pick_feed(c[j], k, s, near, near && split_aligned(G[j], G2[j], p, r.cos2));
        s += 2 * p.Q[0];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!((in >> j) & 1u)) continue;
      bool edge;
      const unsigned plane = split_pick_plane(c[j], &edge);
      const int kc = plane == SPLIT_NO_PLANE ? SPLIT_OBJECT : planes[plane].kind;
      o[j] = split_class_word(kc, plane);
#pragma unroll
      for (int t = 1; t <= SPLIT_OBJECT; ++t) n_cls[t] += kc == t ? 1u : 0u;
      n_edge += edge ? 1u : 0u;
      n_flat += G2[j] == 0 ? 1u : 0u;
    }
  }
  if (i < q.n4) cls[i] = make_uint4(o[0], o[1], o[2], o[3]);
  // (every lane of the wave arrives here: only whole waves returned above)
#pragma unroll
  for (int t = 1; t <= SPLIT_OBJECT; ++t) {
    const unsigned s = hsk_wave_sum(n_cls[t]);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(&counts[t], s);
  }
  const unsigned s_e = hsk_wave_sum(n_edge), s_f = hsk_wave_sum(n_flat);
  if ((threadIdx.x & 63u) == 0u && s_e) atomicAdd(&counts[6], s_e);
  if ((threadIdx.x & 63u) == 0u && s_f) atomicAdd(&counts[7], s_f);
}

struct SplitWordAt {
  const unsigned* cls;
  CompGrid g;
  HSK_HD_MEMBER unsigned operator()(unsigned x, unsigned y, unsigned z) const { return cls[g.at_xyz(x, y, z)]; }
};

// rec[16 at ..]: the record of object roots[at] (SPLIT_REC_*, hsk_launch.h); only kept objects have members left
__global__ __launch_bounds__(256) void k_split_records(const uint4* __restrict__ cls, const uint4* __restrict__ parent, VolVectors q, unsigned n,
                                                       const unsigned* __restrict__ roots, unsigned* __restrict__ rec,
                                                       const SplitPlaneQ* __restrict__ planes, int floor_plane) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  if (!vol_vector(q, i, x0, y, z)) return;
  unsigned w[4], p[4];
  vol_words(cls[i], w);
  if (!(comp_inside(w[0]) || comp_inside(w[1]) || comp_inside(w[2]) || comp_inside(w[3]))) return;
  vol_words(parent[i], p);
  const SplitWordAt word_at{(const unsigned*)cls, q.g};
  unsigned last = COMP_NONE, at = n;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!comp_inside(w[j]) || p[j] == COMP_NONE) continue;
    if (p[j] != last) {  // (x-adjacent members share their root: one look-up a run)
      last = p[j];
      at = comp_search(roots, n, last);  // (ends: the interval halves)
    }
    if (at >= n) continue;
    const unsigned x = x0 + (unsigned)j;
    unsigned* __restrict__ t = rec + (size_t)at * SPLIT_REC_WORDS;
    unsigned long long* __restrict__ t64 = (unsigned long long*)t;
    atomicAdd(&t64[0], (unsigned long long)x);
    atomicAdd(&t64[1], (unsigned long long)y);
    atomicAdd(&t64[2], (unsigned long long)z);
    unsigned kinds;
    unsigned long long mask;
    split_contacts(q.g, x, y, z, word_at, &kinds, &mask);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if ((kinds >> c) & 1u) atomicAdd(&t[SPLIT_REC_CONTACT + c], 1u);
    if (mask) atomicOr(&t64[SPLIT_REC_MASK / 2], mask);
    if (floor_plane >= 0) {
      const unsigned key = (unsigned)split_height(planes[floor_plane], x, y, z) ^ 0x80000000u;  // (the order of int in unsigned)
      atomicMax(&t[SPLIT_REC_HLO], ~key);
      atomicMax(&t[SPLIT_REC_HHI], key);
    }
  }
}

// the box lo <= (x, y, z) < hi, row-major: class bytes and (not null) plane bytes and labels
__global__ __launch_bounds__(256) void k_split_box(const unsigned* __restrict__ cls, const unsigned* __restrict__ parent, VolVectors q, VoxBox box, unsigned n,
                                                   unsigned char* __restrict__ out, unsigned char* __restrict__ plane, unsigned* __restrict__ object) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  unsigned x, y, z;
  vol_box_voxel(box, i, x, y, z);
  const size_t at = q.g.at_xyz(x + (unsigned)box.lo[0], y + (unsigned)box.lo[1], z + (unsigned)box.lo[2]);
  const unsigned w = cls[at];
  out[i] = (unsigned char)split_word_class(w);
  if (plane) plane[i] = (unsigned char)split_word_plane(w);
  if (object) object[i] = comp_inside(w) ? parent[at] : COMP_NONE;
}

__global__ __launch_bounds__(256) void k_split_gather(const unsigned* __restrict__ cls, const unsigned* __restrict__ parent, VolVectors q, SampleVol sv,
                                                      const float* __restrict__ xyz, unsigned n, int radius, unsigned char* __restrict__ out,
                                                      unsigned char* __restrict__ plane, unsigned* __restrict__ object) {
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= n) return;
  unsigned x, y, z;
  bool inside;
  clear_point_voxel(sv, xyz[3u * e], xyz[3u * e + 1u], xyz[3u * e + 2u], x, y, z, inside);
  unsigned l = COMP_NONE;
  if (inside) l = split_at_pick(q.g, x, y, z, radius, SplitWordAt{cls, q.g});  // (ends: at most 9^3 trips)
  unsigned w = 0u, lab = COMP_NONE;
  if (l != COMP_NONE) {
    const size_t at = q.g.at(l);
    w = cls[at];
    lab = comp_inside(w) ? parent[at] : COMP_NONE;
  }
  out[e] = (unsigned char)split_word_class(w);
  if (plane) plane[e] = (unsigned char)split_word_plane(w);
  if (object) object[e] = lab;
}

// a member of a selected object.  n_sel trips.
static __device__ __forceinline__ bool split_target(unsigned word, unsigned root, const SplitSelected* __restrict__ sel, unsigned n_sel) {
  if (!comp_inside(word)) return false;
  bool t = false;
  for (unsigned o = 0u; o < n_sel; ++o) t = t || sel[o].root == root;
  return t;
}

// T as bytes (0 or 1), row-major; counts[8]: how many
__global__ __launch_bounds__(256) void k_split_mark(const uint4* __restrict__ cls, const uint4* __restrict__ parent, VolVectors q,
                                                    const SplitSelected* __restrict__ sel, unsigned n_sel, unsigned* __restrict__ mask,
                                                    unsigned* __restrict__ counts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  const bool live = vol_vector(q, i, x0, y, z);
  unsigned m = 0u, n_t = 0u;
  if (live) {
    unsigned w[4], p[4];
    vol_words(cls[i], w);
    vol_words(parent[i], p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool t = split_target(w[j], p[j], sel, n_sel);
      m |= (t ? 1u : 0u) << (8 * j);
      n_t += t ? 1u : 0u;
    }
    mask[(size_t)q.g.lin(x0, y, z) >> 2] = m;
  }
  const unsigned s = hsk_wave_sum(n_t);  // (every lane arrives)
  if ((threadIdx.x & 63u) == 0u && s) atomicAdd(&counts[8], s);
}

// MODE 0: count the written (counts[9]) and the restored voxels (counts[10]); 1: write the words; 2: and the colour word 0
template <int MODE>
__global__ __launch_bounds__(256) void k_split_restore(uint4* __restrict__ vol, unsigned* __restrict__ col, const uint4* __restrict__ cls,
                                                       const uint4* __restrict__ parent, const unsigned* __restrict__ halo, VolVectors q,
                                                       const SplitSelected* __restrict__ sel, unsigned n_sel, VoxBox uni,
                                                       const SplitPlaneQ* __restrict__ planes, SplitRule r, int mode, int fill_weight,
                                                       unsigned* __restrict__ counts) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  unsigned x0, y, z;
  const bool live = vol_vector(q, i, x0, y, z);
  unsigned n_w = 0u, n_r = 0u;
  // (H and T lie inside the union of the grown boxes: a vector outside it stays)
  if (live && (int)y >= uni.lo[1] && (int)y < uni.hi[1] && (int)z >= uni.lo[2] && (int)z < uni.hi[2] && (int)x0 + 4 > uni.lo[0] && (int)x0 < uni.hi[0]) {
    unsigned w[4], cw[4], p[4];
    vol_words(vol[i], w);
    vol_words(cls[i], cw);
    vol_words(parent[i], p);
    const unsigned h = halo[(size_t)q.g.lin(x0, y, z) >> 2];
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned x = x0 + (unsigned)j;
      unsigned long long A;
      const bool in_box = split_boxes_at(sel, n_sel, (int)x, (int)y, (int)z, &A);  // (n_sel trips)
      const int act = split_remove_rule(mode, in_box, A, ((h >> (8 * j)) & 0xffu) != 0u, split_target(cw[j], p[j], sel, n_sel), w[j]);
      if (act == 0) continue;
      const unsigned nw = act == 1 ? split_plane_word(planes, r, A, x, y, z, fill_weight) : 0u;
      n_w += 1u;
      n_r += nw != 0u ? 1u : 0u;
      if (MODE != 0) {
        w[j] = nw;
        changed = true;
        if (MODE == 2) col[(size_t)q.g.lin(x, y, z)] = 0u;
      }
    }
    if (MODE != 0 && changed) vol[i] = make_uint4(w[0], w[1], w[2], w[3]);
  }
  if (MODE == 0) {
    const unsigned s_w = hsk_wave_sum(n_w), s_r = hsk_wave_sum(n_r);  // (every lane arrives: nothing above returns)
    if ((threadIdx.x & 63u) == 0u && s_w) atomicAdd(&counts[9], s_w);
    if ((threadIdx.x & 63u) == 0u && s_r) atomicAdd(&counts[10], s_r);
  }
}

size_t split_layout(const VolParams& vp, void* base, SplitBufs* b) {
  ScratchCarve c{base};
  SplitBufs out;
  out.counts = (unsigned*)c.take(SPLIT_COUNTS * 4);
  out.planes = (SplitPlaneQ*)c.take(SPLIT_MAX_PLANES * sizeof(SplitPlaneQ));
  out.sel = (SplitSelected*)c.take(SPLIT_MAX_SELECTED * sizeof(SplitSelected));
  out.cls = (unsigned*)c.take(hsk_vol_words(vp) * 4);
  out.mask[0] = (unsigned char*)c.take((size_t)vp.X * vp.Y * vp.Z);
  out.mask[1] = (unsigned char*)c.take((size_t)vp.X * vp.Y * vp.Z);
  char* comp = c.take(comp_layout(vp, nullptr, nullptr));
  comp_layout(vp, comp, &out.comp);
  if (b) *b = out;
  return c.bytes;
}

void launch_split_classify(hipStream_t s, const void* vol, const VolParams& vp, const SplitBufs& b, const SplitRule& r) {
  const VolVectors q = vol_vectors(vp);
  (void)hipMemsetAsync(b.counts, 0, SPLIT_COUNTS * 4, s);
  hipLaunchKernelGGL(k_split_classify, dim3((q.n4 + 255u) / 256u), dim3(256), 0, s, (const uint4*)vol, (uint4*)b.cls, q, (const SplitPlaneQ*)b.planes, r,
                     b.counts);
}

void launch_split_records(hipStream_t s, const VolParams& vp, const SplitBufs& b, unsigned n, const unsigned* roots, unsigned* rec, int floor_plane) {
  const VolVectors q = vol_vectors(vp);
  (void)hipMemsetAsync(rec, 0, (size_t)n * SPLIT_REC_WORDS * 4, s);
  hipLaunchKernelGGL(k_split_records, dim3((q.n4 + 255u) / 256u), dim3(256), 0, s, (const uint4*)b.cls, (const uint4*)b.comp.parent, q, n, roots, rec,
                     (const SplitPlaneQ*)b.planes, floor_plane);
}

void launch_split_box(hipStream_t s, const VolParams& vp, const SplitBufs& b, const int lo[3], const int hi[3], size_t n, unsigned char* cls,
                      unsigned char* plane, unsigned* object) {
  const VolVectors q = vol_vectors(vp);
  hipLaunchKernelGGL(k_split_box, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const unsigned*)b.cls, (const unsigned*)b.comp.parent, q,
                     vox_box(lo, hi), (unsigned)n, cls, plane, object);
}

void launch_split_gather(hipStream_t s, const VolParams& vp, const SplitBufs& b, const float* xyz, unsigned n, int radius, unsigned char* cls,
                         unsigned char* plane, unsigned* object) {
  const VolVectors q = vol_vectors(vp);
  hipLaunchKernelGGL(k_split_gather, dim3((n + 255u) / 256u), dim3(256), 0, s, (const unsigned*)b.cls, (const unsigned*)b.comp.parent, q,
                     hsk_sample_vol(vp), xyz, n, radius, cls, plane, object);
}

void launch_split_halo(hipStream_t s, const void* vol, const VolParams& vp, const SplitBufs& b, unsigned n_sel, const int uni_lo[3], const int uni_hi[3],
                       const SplitRule& r, int mode, int halo, int fill_weight) {
  const VolVectors q = vol_vectors(vp);
  const dim3 vectors((q.n4 + 255u) / 256u);
  (void)hipMemsetAsync(b.counts + 8, 0, 12, s);
  hipLaunchKernelGGL(k_split_mark, vectors, dim3(256), 0, s, (const uint4*)b.cls, (const uint4*)b.comp.parent, q, (const SplitSelected*)b.sel, n_sel,
                     (unsigned*)b.mask[0], b.counts);
  launch_mask_dilate3(s, vp, b.mask[0], b.mask[1], halo);  // (the result: mask[1])
  hipLaunchKernelGGL((k_split_restore<0>), vectors, dim3(256), 0, s, (uint4*)const_cast<void*>(vol), (unsigned*)nullptr, (const uint4*)b.cls,
                     (const uint4*)b.comp.parent, (const unsigned*)b.mask[1], q, (const SplitSelected*)b.sel, n_sel, vox_box(uni_lo, uni_hi),
                     (const SplitPlaneQ*)b.planes, r, mode, fill_weight, b.counts);
}

void launch_split_restore(hipStream_t s, void* vol, unsigned* col, const VolParams& vp, const SplitBufs& b, unsigned n_sel, const int uni_lo[3],
                          const int uni_hi[3], const SplitRule& r, int mode, int fill_weight) {
  const VolVectors q = vol_vectors(vp);
  const dim3 vectors((q.n4 + 255u) / 256u);
  if (col)
    hipLaunchKernelGGL((k_split_restore<2>), vectors, dim3(256), 0, s, (uint4*)vol, col, (const uint4*)b.cls, (const uint4*)b.comp.parent,
                       (const unsigned*)b.mask[1], q, (const SplitSelected*)b.sel, n_sel, vox_box(uni_lo, uni_hi), (const SplitPlaneQ*)b.planes, r, mode,
                       fill_weight, b.counts);
  else
    hipLaunchKernelGGL((k_split_restore<1>), vectors, dim3(256), 0, s, (uint4*)vol, col, (const uint4*)b.cls, (const uint4*)b.comp.parent,
                       (const unsigned*)b.mask[1], q, (const SplitSelected*)b.sel, n_sel, vox_box(uni_lo, uni_hi), (const SplitPlaneQ*)b.planes, r, mode,
                       fill_weight, b.counts);
}

int split_warm() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, (const void*)k_split_classify);
}
