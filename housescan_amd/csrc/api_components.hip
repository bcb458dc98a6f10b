// api_components.hip -- the C ABI's surface components (include/hskinfu.h "Surface components"; DESIGN.md 3.16 the kernels, 8j the
// rule): hsk_default_prune_params, hsk_label_components, hsk_download_components, hsk_prune_components.  Labelling reads the
// volume as it stands, with NO flush of the deferred weights (as the coverage calls, api_cover.hip): the rule asks of a weight
// only whether it is zero and of the TSDF its sign -- no deferred weight is zero in the volume's own copy, and the TSDF values
// are current.  The labelling stays on the device (d_comp) with its records on the host (comp_recs) while vol_epoch stands.
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
  if (k) {
    tau = k->vp.tau;
    for (int i = 0; i < 3; ++i) cell[i] = k->vp.cell[i];
  } else {
    hsk_config c;
    hsk_default_config(&c, 256);
    tau = config_tau(&c);
    cell[0] = c.vol_size_m[0] / (float)c.vol_x;
    cell[1] = c.vol_size_m[1] / (float)c.vol_y;
    cell[2] = c.vol_size_m[2] / (float)c.vol_z;
  }
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

// d_comp_tab for n components: the roots, the records' eight words each, the survivors of a keep_largest prune
struct CompTab {
  size_t bytes;
  unsigned *roots, *table, *keep;
};
static CompTab comp_tab(const hsk_ctx* k, size_t n) {
  ProductLayout l;
  char* base = (char*)k->d_comp_tab;
  CompTab t;
  const size_t roots_at = l.take(n * 4), table_at = l.take(n * 32), keep_at = l.take(4096 * 4);
  t.roots = (unsigned*)(base + roots_at);
  t.table = (unsigned*)(base + table_at);
  t.keep = (unsigned*)(base + keep_at);
  t.bytes = l.bytes;
  return t;
}

// The labelling of the volume as it stands: the parents in d_comp; with at most 2^24 components their records in comp_recs, in
// their order, and the labelling kept for later calls.  *n: the components; *reused: nothing had to be launched.
static int comp_label(hsk_ctx* k, size_t* n, bool* reused) {
  if (k->comp_epoch != 0 && k->comp_epoch == k->vol_epoch) {
    *n = k->comp_recs.size();
    *reused = true;
    return HSK_OK;
  }
  *reused = false;
  k->comp_epoch = 0;
  int r = ensure_grown(k, &k->d_comp, &k->comp_bytes, comp_layout(k->vp, nullptr, nullptr));
  if (r != HSK_OK) return r;
  CompBufs b;
  comp_layout(k->vp, k->d_comp, &b);
  launch_comp_label(k->stream, k->d_vol, k->vp, b);
  HIPCHK(k, hipGetLastError());
  unsigned n_roots = 0;
  HIPCHK(k, hipMemcpyAsync(&n_roots, b.counts + 4, sizeof(n_roots), hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  *n = n_roots;
  if ((size_t)n_roots > HSK_COMPONENT_MAX) {  // labelled, but no records: the callers refuse; nothing is kept for a later call
    k->comp_recs.clear();
    k->comp_inside = 0;
    return HSK_OK;
  }
  std::vector<unsigned> roots, table;
  try {
    k->comp_recs.assign(n_roots, hsk_component{});
    roots.resize(n_roots);
    table.resize((size_t)n_roots * 8);
  } catch (const std::bad_alloc&) {
    k->comp_recs.clear();
    return fail(k, HSK_ERR_STATE, "surface components: out of host memory for the records");
  }
  k->comp_inside = 0;
  if (n_roots > 0) {
    r = ensure_grown(k, &k->d_comp_tab, &k->comp_tab_bytes, comp_tab(k, n_roots).bytes);
    if (r != HSK_OK) return r;
    const CompTab t = comp_tab(k, n_roots);
    launch_comp_records(k->stream, k->vp, b, n_roots, t.roots, t.table);
    HIPCHK(k, hipGetLastError());
    r = copy_out(k, roots.data(), t.roots, (size_t)n_roots * 4);
    if (r == HSK_OK) r = copy_out(k, table.data(), t.table, (size_t)n_roots * 32);
    if (r != HSK_OK) return r;
    const CompGrid g{(unsigned)k->vp.X, (unsigned)k->vp.Y, (unsigned)k->vp.Z};
    for (size_t i = 0; i < n_roots; ++i) {
      hsk_component& c = k->comp_recs[i];
      unsigned x, y, z;
      g.xyz(roots[i], x, y, z);
      c.root[0] = (int32_t)x;
      c.root[1] = (int32_t)y;
      c.root[2] = (int32_t)z;
      const unsigned* t8 = &table[i * 8];
      c.n_voxels = t8[0];
      for (int a = 0; a < 3; ++a) {
        c.lo[a] = (int32_t)t8[1 + a];
        c.hi[a] = (int32_t)t8[4 + a];
      }
      k->comp_inside += t8[0];
    }
    std::sort(k->comp_recs.begin(), k->comp_recs.end(), [&](const hsk_component& a, const hsk_component& c) {
      return comp_record_before(a.n_voxels, g.lin((unsigned)a.root[0], (unsigned)a.root[1], (unsigned)a.root[2]), c.n_voxels,
                                g.lin((unsigned)c.root[0], (unsigned)c.root[1], (unsigned)c.root[2]));
    });
  }
  k->comp_epoch = k->vol_epoch;
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
  if (!recs) return HSK_OK;
  if (cap < n) return fail(k, HSK_ERR_ARG, "hsk_label_components: cap is below the number of components");
  if (n > 0) memcpy(recs, k->comp_recs.data(), n * sizeof(hsk_component));
  return HSK_OK;
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
  comp_layout(k->vp, k->d_comp, &b);
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
  const CompTab t = comp_tab(k, n);
  CompBufs b;
  comp_layout(k->vp, k->d_comp, &b);
  unsigned keep[4096];
  if (n_keep > 0) {  // the surviving roots, ascending, handed up
    const CompGrid g{(unsigned)k->vp.X, (unsigned)k->vp.Y, (unsigned)k->vp.Z};
    for (size_t i = 0; i < n_keep; ++i) {
      const hsk_component& c = k->comp_recs[i];
      keep[i] = g.lin((unsigned)c.root[0], (unsigned)c.root[1], (unsigned)c.root[2]);
    }
    std::sort(keep, keep + n_keep);
    HIPCHK(k, hipMemcpyAsync(t.keep, keep, n_keep * 4, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));  // (`keep` is this frame's)
  }
  flush_weights(k);  // the words that stay are to hold their weights
  const unsigned min_voxels = p.min_voxels > 0xffffffffull ? 0xffffffffu : (unsigned)p.min_voxels;  // (no component has 2^32 voxels)
  launch_comp_prune(k->stream, k->d_vol, k->d_color, k->vp, b.parent, t.roots, t.table, (unsigned)n, min_voxels, t.keep, (unsigned)n_keep,
                    p.fill == HSK_PRUNE_FREE);
  HIPCHK(k, hipGetLastError());
  r = volume_replaced(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  if (stats) *stats = st;
  return HSK_OK;
}
