// api_components.hip -- the C ABI's surface components (include/hskinfu.h "Surface components"; DESIGN.md 3.16 the kernels, 8j the
// rule): hsk_default_prune_params, hsk_label_components, hsk_download_components, hsk_prune_components.  Labelling reads the
// volume as it stands, with NO flush of the deferred weights (as the coverage calls, api_cover.hip): the rule asks of a weight
// only whether it is zero and of the TSDF its sign -- no deferred weight is zero in the volume's own copy, and the TSDF values
// are current.  The labelling stays on the device (comp, a HeldPass) with its records on the host (comp_recs) while vol_epoch stands.
// Pruning writes the volume in api_volume.hip's pattern: flush the deferred weights, write, volume_replaced.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <new>

#include "hsk_ctx.h"
#include "hsk_comp_point.h"

extern "C" void hsk_default_prune_params(const hsk_ctx* k, hsk_prune_params* p) {
  if (!p) return;
  float tau, cell[3];
  context_cells(k, cell, &tau);
  memset(p, 0, sizeof(*p));
  // the voxels of a cube of edge 4 tau, in binary64 from the binary32 fields
  const double e = 4.0 * (double)tau;
  p->min_voxels = (uint64_t)std::ceil(((e * e) * e) / (((double)cell[0] * (double)cell[1]) * (double)cell[2]));
  p->keep_largest = 0;
  p->fill = HSK_PRUNE_UNSEEN;
}

int ensure_grown(hsk_ctx* k, void** buf, size_t* have, size_t want) {
  if (*have >= want) return HSK_OK;
  if (*buf) HIPCHK(k, hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  HIPCHK(k, hipMalloc(buf, want));
  *have = want;
  return HSK_OK;
}

RegionTab region_tab(const HeldPass& pass, size_t n, size_t extra_bytes) {
  ProductLayout l;
  char* base = (char*)pass.tab;
  RegionTab t;
  const size_t roots_at = l.take(n * 4), table_at = l.take(n * 32), extra_at = l.take(extra_bytes);
  t.roots = (unsigned*)(base + roots_at);
  t.table = (unsigned*)(base + table_at);
  t.extra = (unsigned*)(base + extra_at);
  t.bytes = l.bytes;
  return t;
}

int region_read(hsk_ctx* k, const CompBufs& b, HeldPass* pass, size_t extra_words, size_t tail_bytes, const char* too_many, const char* no_memory,
                void* minor_cls, uint64_t min_voxels, const std::function<void(const RegionTab&, unsigned)>& extra, RegionRead* r) {
  int rc = copy_out(k, &r->n, b.counts + 4, sizeof(r->n));
  if (rc != HSK_OK) return rc;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  const size_t n = r->n;
  if (n > HSK_COMPONENT_MAX) return too_many ? fail(k, HSK_ERR_ARG, too_many) : HSK_OK;
  try {
    r->roots.resize(n);
    r->table.resize(n * 8);
    r->extra.resize(n * extra_words);
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, no_memory);
  }
  if (n == 0) return HSK_OK;
  const size_t extra_bytes = n * extra_words * 4 + tail_bytes;
  rc = pass->grow_tab(k, region_tab(*pass, n, extra_bytes).bytes);
  if (rc != HSK_OK) return rc;
  const RegionTab t = region_tab(*pass, n, extra_bytes);
  launch_comp_records(k->stream, k->vp, b, r->n, t.roots, t.table);
  if (minor_cls) {  // the words of a region below min_voxels keep their class in the weight half and stop being members
    const unsigned below = min_voxels > 0xffffffffull ? 0xffffffffu : (unsigned)min_voxels;  // (no region has 2^32 voxels)
    launch_comp_prune(k->stream, minor_cls, nullptr, k->vp, b.parent, t.roots, t.table, r->n, below, t.roots, 0u, true);
  }
  if (extra) extra(t, r->n);
  HIPCHK(k, hipGetLastError());
  rc = copy_out(k, r->roots.data(), t.roots, n * 4);
  if (rc == HSK_OK) rc = copy_out(k, r->table.data(), t.table, n * 32);
  if (rc == HSK_OK && extra_words) rc = copy_out(k, r->extra.data(), t.extra, n * extra_words * 4);
  if (rc != HSK_OK) return rc;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

// The labelling of the volume as it stands: the parents in comp's scratch; with at most 2^24 components their records in
// comp_recs, in their order, and the labelling kept for later calls.  *n: the components; *reused: nothing had to be launched.
static int comp_label(hsk_ctx* k, size_t* n, bool* reused) {
  *reused = k->comp.stands(k);
  if (*reused) {
    *n = k->comp_recs.size();
    return HSK_OK;
  }
  k->comp.drop();
  int r = k->comp.grow(k, comp_layout(k->vp, nullptr, nullptr));
  if (r != HSK_OK) return r;
  CompBufs b;
  comp_layout(k->vp, k->comp.buf, &b);
  launch_comp_label(k->stream, k->d_vol, k->vp, b);
  HIPCHK(k, hipGetLastError());
  RegionRead rr;
  k->comp_recs.clear();
  k->comp_inside = 0;
  r = region_read(k, b, &k->comp, 0, 4096 * 4, nullptr, "surface components: out of host memory for the records", nullptr, 0, nullptr, &rr);
  *n = rr.n;
  if (r != HSK_OK || rr.n > HSK_COMPONENT_MAX) return r;  // (labelled, but no records: the callers refuse; nothing is kept for a later call)
  const CompGrid g{(unsigned)k->vp.X, (unsigned)k->vp.Y, (unsigned)k->vp.Z};
  try {
    comp_region_records(g, rr.roots.data(), rr.table.data(), rr.n, 0, &k->comp_recs, [&](const hsk_component& c, size_t) { k->comp_inside += c.n_voxels; });
  } catch (const std::bad_alloc&) {
    k->comp_recs.clear();
    return fail(k, HSK_ERR_STATE, "surface components: out of host memory for the records");
  }
  k->comp.stamp(k);
  return HSK_OK;
}

extern "C" int hsk_label_components(hsk_ctx* k, hsk_component* recs, size_t cap, size_t* n_components, hsk_component_stats* stats) {
  static_assert(sizeof(hsk_component) == 48, "hsk_component is 48 bytes");
  static_assert(sizeof(hsk_component_stats) == 32 && sizeof(hsk_prune_params) == 16 && sizeof(hsk_prune_stats) == 32, "the components' structs");
  if (!k) return HSK_ERR_ARG;
  if (!n_components) return fail(k, HSK_ERR_ARG, "hsk_label_components: n_components is null");
  if (int rc = volume_state_check(k, k, "hsk_label_components")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  size_t n = 0;
  bool reused = false;
  int r = comp_label(k, &n, &reused);
  if (r != HSK_OK) return r;
  hsk_component_stats st;
  memset(&st, 0, sizeof(st));
  st.n_components = n;
  *n_components = n;
  if (n > HSK_COMPONENT_MAX) {
    if (stats) *stats = st;
    return fail(k, HSK_ERR_ARG, "hsk_label_components: more than 2^24 components: no records are made");
  }
  st.n_inside = k->comp_inside;
  st.largest = n > 0 ? k->comp_recs[0].n_voxels : 0;
  st.labels_reused = reused ? 1 : 0;
  if (stats) *stats = st;
  return reply_records(k, k->comp_recs, recs, cap, n_components, "hsk_label_components: cap is below the number of components");
}

extern "C" int hsk_download_components(hsk_ctx* k, uint32_t* labels) {
  if (!k) return HSK_ERR_ARG;
  if (!labels) return fail(k, HSK_ERR_ARG, "hsk_download_components: labels is null");
  if (int rc = volume_state_check(k, k, "hsk_download_components")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  size_t n = 0;
  bool reused = false;
  int r = comp_label(k, &n, &reused);
  if (r != HSK_OK) return r;
  // the parents live in the volume's block layout: the volume's own conversion makes them row-major, in the product buffer
  const size_t bytes = (size_t)k->vp.X * k->vp.Y * k->vp.Z * 4;
  r = ensure_product_bytes(k, bytes);
  if (r != HSK_OK) return r;
  CompBufs b;
  comp_layout(k->vp, k->comp.buf, &b);
  launch_vol_to_linear(k->stream, b.parent, k->vp, 0, k->vp.Z, k->d_out);
  HIPCHK(k, hipGetLastError());
  return copy_out(k, labels, k->d_out, bytes);
}

extern "C" int hsk_prune_components(hsk_ctx* k, const hsk_prune_params* params, hsk_prune_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  hsk_prune_params p;
  if (params)
    p = *params;
  else
    hsk_default_prune_params(k, &p);
  if (p.keep_largest < 0 || p.keep_largest > 4096) return fail(k, HSK_ERR_ARG, "hsk_prune_components: keep_largest must lie in 0..4096");
  if (p.fill != HSK_PRUNE_UNSEEN && p.fill != HSK_PRUNE_FREE) return fail(k, HSK_ERR_ARG, "hsk_prune_components: fill is neither HSK_PRUNE_UNSEEN nor HSK_PRUNE_FREE");
  if (int rc = volume_state_check(k, k, "hsk_prune_components")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  size_t n = 0;
  bool reused = false;
  int r = comp_label(k, &n, &reused);
  if (r != HSK_OK) return r;
  if (n > HSK_COMPONENT_MAX) return fail(k, HSK_ERR_ARG, "hsk_prune_components: more than 2^24 components (hsk_label_components' limit)");
  // what the device will decide, counted on the host from the same records
  hsk_prune_stats st;
  memset(&st, 0, sizeof(st));
  st.n_components = n;
  const size_t n_keep = p.keep_largest > 0 ? std::min((size_t)p.keep_largest, n) : 0;
  for (size_t i = 0; i < n; ++i) {
    const bool pruned = k->comp_recs[i].n_voxels < p.min_voxels || (p.keep_largest > 0 && i >= (size_t)p.keep_largest);
    st.n_pruned += pruned ? 1 : 0;
    (pruned ? st.n_pruned_voxels : st.n_kept_voxels) += k->comp_recs[i].n_voxels;
  }
  if (st.n_pruned == 0) {  // nothing is written, vol_epoch does not move: cached passes stay valid
    if (stats) *stats = st;
    return HSK_OK;
  }
  const RegionTab t = region_tab(k->comp, n, 4096 * 4);  // (extra: the keep slots)
  CompBufs b;
  comp_layout(k->vp, k->comp.buf, &b);
  unsigned keep[4096];
  if (n_keep > 0) {  // the surviving roots, ascending, handed up
    const CompGrid g{(unsigned)k->vp.X, (unsigned)k->vp.Y, (unsigned)k->vp.Z};
    for (size_t i = 0; i < n_keep; ++i) {
      const hsk_component& c = k->comp_recs[i];
      keep[i] = g.lin((unsigned)c.root[0], (unsigned)c.root[1], (unsigned)c.root[2]);
    }
    std::sort(keep, keep + n_keep);
    HIPCHK(k, hipMemcpyAsync(t.extra, keep, n_keep * 4, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));  // (`keep` is this frame's)
  }
  const unsigned min_voxels = p.min_voxels > 0xffffffffull ? 0xffffffffu : (unsigned)p.min_voxels;  // (no component has 2^32 voxels)
  r = commit_volume_write(k, [&] {
    launch_comp_prune(k->stream, k->d_vol, k->d_color, k->vp, b.parent, t.roots, t.table, (unsigned)n, min_voxels, t.extra, (unsigned)n_keep,
                      p.fill == HSK_PRUNE_FREE);
  });
  if (r != HSK_OK) return r;
  if (stats) *stats = st;
  return HSK_OK;
}
