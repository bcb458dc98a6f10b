// api_split.hip -- the C ABI's scene split (include/hskinfu.h "Scene split"; DESIGN.md 3.24 the kernels, 8r the rule):
// hsk_default_split_params, hsk_default_remove_params, hsk_split_plane_kinds, hsk_split_scene, hsk_download_split, hsk_split_at,
// hsk_remove_objects, hsk_release_split.  The rule asks of a weight only whether it is zero, so the split reads the volume as it
// stands, with NO flush of the deferred weights (as the labelling, api_components.hip).  The objects are components.hip's labelling
// run on the class words, in a scratch of the split's own (split, a HeldPass): hsk_label_components' cached labelling (comp) is
// neither read nor written.  The split stays on the device with its records and stats on the host while the volume, the planes and
// the parameters stand; a call with the same planes and parameters meanwhile is answered from them.  Removing writes the volume in
// hsk_prune_components' order: flush the deferred weights, write, volume_replaced.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <new>

#include "hsk_ctx.h"
#include "hsk_split_point.h"

static_assert(HSK_SPLIT_NONE == SPLIT_NONE && HSK_SPLIT_FLOOR == SPLIT_FLOOR && HSK_SPLIT_CEILING == SPLIT_CEILING && HSK_SPLIT_WALL == SPLIT_WALL &&
                  HSK_SPLIT_OTHER == SPLIT_OTHER && HSK_SPLIT_OBJECT == SPLIT_OBJECT && HSK_SPLIT_MINOR == SPLIT_MINOR && HSK_KIND_FLOOR == SPLIT_FLOOR &&
                  HSK_KIND_CEILING == SPLIT_CEILING && HSK_KIND_WALL == SPLIT_WALL && HSK_KIND_OTHER == SPLIT_OTHER && HSK_REMOVE_ERASE == SPLIT_REMOVE_ERASE &&
                  HSK_REMOVE_RESTORE == SPLIT_REMOVE_RESTORE && HSK_SPLIT_MAX_PLANES == SPLIT_MAX_PLANES && HSK_REMOVE_MAX_OBJECTS == SPLIT_MAX_SELECTED &&
                  HSK_COMPONENT_NONE == COMP_NONE,
              "hsk_split_point.h restates the header's numbers");
static_assert(sizeof(hsk_split_plane) == 24 && sizeof(hsk_split_params) == 24 && sizeof(hsk_object) == 104 && sizeof(hsk_split_stats) == 104 &&
                  sizeof(hsk_remove_params) == 12 && sizeof(hsk_remove_stats) == 40,
              "the split structs");
static_assert(sizeof(SplitPlaneQ) == 48 && sizeof(SplitSelected) == 40, "the split's device tables");

extern "C" void hsk_default_split_params(const hsk_ctx* k, hsk_split_params* p) {
  if (!p) return;
  hsk_prune_params pp;
  hsk_default_prune_params(k, &pp);
  float tau, cell[3];
  context_cells(k, cell, &tau);
  memset(p, 0, sizeof(*p));
  p->dist_m = 0.04f;
  p->back_m = tau + 0.04f;
  p->cos_min = 0.8660254f;  // cos 30 deg
  p->min_voxels = pp.min_voxels;
}

extern "C" void hsk_default_remove_params(const hsk_ctx* k, hsk_remove_params* p) {
  if (!p) return;
  float tau, cell[3];
  context_cells(k, cell, &tau);
  const float c_min = std::min(cell[0], std::min(cell[1], cell[2]));
  const double h = std::ceil((double)tau / (double)c_min) + 1.0;
  p->mode = HSK_REMOVE_RESTORE;
  p->halo = (int)std::min(8.0, std::max(1.0, h));
  p->fill_weight = 1;
}

extern "C" int hsk_split_plane_kinds(hsk_split_plane* planes, size_t n, const float up[3], float level_cos, float wall_sin) {
  auto bad = [](const char* msg) {
    create_error() = msg;
    return HSK_ERR_ARG;
  };
  if (!up || (n > 0 && !planes)) return bad("hsk_split_plane_kinds: null argument");
  if (!(level_cos >= 0.0f && level_cos <= 1.0f) || !(wall_sin >= 0.0f && wall_sin <= 1.0f))
    return bad("hsk_split_plane_kinds: level_cos and wall_sin must lie in [0, 1]");
  const double u[3] = {(double)up[0], (double)up[1], (double)up[2]};
  const double lu = std::sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  if (!std::isfinite(lu) || lu == 0.0) return bad("hsk_split_plane_kinds: up must be finite and not zero");
  for (size_t i = 0; i < n; ++i) {
    const double a[3] = {(double)planes[i].abcd[0], (double)planes[i].abcd[1], (double)planes[i].abcd[2]};
    const double la = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    if (!std::isfinite(la) || la == 0.0) return bad("hsk_split_plane_kinds: a normal is not finite or zero (no kind was set from it on)");
    const double t = ((a[0] * u[0] + a[1] * u[1]) + a[2] * u[2]) / (la * lu);
    planes[i].kind = t >= (double)level_cos ? HSK_KIND_FLOOR : (t <= -(double)level_cos ? HSK_KIND_CEILING : (std::fabs(t) <= (double)wall_sin ? HSK_KIND_WALL : HSK_KIND_OTHER));
    planes[i].pad = 0;
  }
  return HSK_OK;
}

// the rule's numbers for checked parameters and planes (include/hskinfu.h: the host converts once, in binary64, with rint)
static void split_rule_of(const hsk_ctx* k, const hsk_split_params& p, const hsk_split_plane* planes, size_t n, SplitRule* r, SplitPlaneQ* q) {
  const double two30 = 1073741824.0, two29 = 536870912.0;
  const float* c = k->vp.cell;
  const float c_min = std::min(c[0], std::min(c[1], c[2]));
  memset(r, 0, sizeof(*r));
  r->front = (long long)std::rint((double)p.dist_m * two30);
  r->back = (long long)std::rint((double)p.back_m * two30);
  r->tauq = (long long)std::rint((double)k->vp.tau * two30);
  r->cos2 = (double)p.cos_min * (double)p.cos_min;
  for (int j = 0; j < 3; ++j) r->w[j] = (int)std::rint((4096.0 * (double)c_min) / (double)c[j]);
  r->n_planes = (int)n;
  r->floor_plane = -1;
  for (size_t i = 0; i < n; ++i) {
    memset(&q[i], 0, sizeof(q[i]));
    for (int j = 0; j < 3; ++j) {
      q[i].Q[j] = (long long)std::rint(((double)planes[i].abcd[j] * (double)c[j]) * two29);
      q[i].N[j] = (int)std::rint((double)planes[i].abcd[j] * 4096.0);
    }
    q[i].Qd = (long long)std::rint((double)planes[i].abcd[3] * two30);
    q[i].kind = planes[i].kind;
    if (r->floor_plane < 0 && planes[i].kind == HSK_KIND_FLOOR) r->floor_plane = (int)i;
  }
}

#define SPLIT_NOT_HELD ": no split is held for the volume as it stands"

// the split's key: the zero-padded parameters, then the planes asked for, zero-padded too (compared as bytes)
struct SplitKey {
  hsk_split_params p;
  hsk_split_plane planes[HSK_SPLIT_MAX_PLANES];
};
static_assert(offsetof(SplitKey, planes) == sizeof(hsk_split_params), "the planes follow the parameters");
static size_t split_key_bytes(size_t n_planes) { return sizeof(hsk_split_params) + n_planes * sizeof(hsk_split_plane); }
// ... and the planes a held key was made for
static size_t split_key_planes(const HeldPass& pass) { return (pass.key.size() - sizeof(hsk_split_params)) / sizeof(hsk_split_plane); }

// hsk_split_scene's answer from the held records and stats
static int split_reply(hsk_ctx* k, hsk_object* recs, size_t cap, size_t* n_objects, hsk_split_stats* stats, bool reused) {
  if (stats) {
    *stats = k->split_stats;
    stats->reused = reused ? 1u : 0u;
  }
  return reply_records(k, k->split_recs, recs, cap, n_objects, "hsk_split_scene: cap is below the number of kept objects");
}

extern "C" int hsk_split_scene(hsk_ctx* k, const hsk_split_plane* planes, size_t n_planes, const hsk_split_params* params, hsk_object* recs, size_t cap,
                               size_t* n_objects, hsk_split_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  if (!n_objects || (n_planes > 0 && !planes)) return fail(k, HSK_ERR_ARG, "hsk_split_scene: null argument");
  if (n_planes > HSK_SPLIT_MAX_PLANES) return fail(k, HSK_ERR_ARG, "hsk_split_scene: more than 64 planes");
  SplitKey key;
  memset(&key, 0, sizeof(key));  // (compared as bytes: the padding is zero on both sides)
  hsk_split_params& p = key.p;
  hsk_default_split_params(k, &p);  // (zeroes the whole struct first)
  if (params) {
    p.dist_m = params->dist_m;
    p.back_m = params->back_m;
    p.cos_min = params->cos_min;
    p.min_voxels = params->min_voxels;
  }
  if (!(p.dist_m > 0.0f && p.dist_m <= 1.0f)) return fail(k, HSK_ERR_ARG, "hsk_split_scene: dist_m must lie in (0, 1]");
  if (!(p.back_m > 0.0f && p.back_m <= 2.0f)) return fail(k, HSK_ERR_ARG, "hsk_split_scene: back_m must lie in (0, 2]");
  if (!(p.cos_min >= 0.0f && p.cos_min <= 1.0f)) return fail(k, HSK_ERR_ARG, "hsk_split_scene: cos_min must lie in [0, 1]");
  if (p.min_voxels < 1) return fail(k, HSK_ERR_ARG, "hsk_split_scene: min_voxels must be at least 1");
  hsk_split_plane* pl = key.planes;
  for (size_t i = 0; i < n_planes; ++i) {
    const float* a = planes[i].abcd;
    const double len = std::sqrt(((double)a[0] * (double)a[0] + (double)a[1] * (double)a[1]) + (double)a[2] * (double)a[2]);
    if (!(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && std::isfinite(a[3])))
      return fail(k, HSK_ERR_ARG, "hsk_split_scene: a plane holds a number that is not finite");
    if (!(len >= 0.5 && len <= 2.0)) return fail(k, HSK_ERR_ARG, "hsk_split_scene: a plane's normal must have a length in [0.5, 2]");
    if (!(std::fabs((double)a[3]) <= 64.0)) return fail(k, HSK_ERR_ARG, "hsk_split_scene: a plane's |d| must not exceed 64");
    if (planes[i].kind < HSK_KIND_FLOOR || planes[i].kind > HSK_KIND_OTHER) return fail(k, HSK_ERR_ARG, "hsk_split_scene: a plane's kind is not one of HSK_KIND_*");
    memcpy(pl[i].abcd, a, sizeof(pl[i].abcd));
    pl[i].kind = planes[i].kind;
  }
  if (int rc = volume_state_check(k, k, "hsk_split_scene")) return rc;
  // the split of an earlier call still fits: the volume stands, the planes and the parameters are the same.  Nothing is launched
  const bool held = k->split.stands_for(k, &key, split_key_bytes(n_planes));
  if (held) return split_reply(k, recs, cap, n_objects, stats, true);
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  k->split.drop();  // (the scratch is about to be written: an earlier split goes)
  k->split_recs.clear();
  int r = k->split.grow(k, split_layout(k->vp, nullptr, nullptr));
  if (r != HSK_OK) return r;
  SplitBufs b;
  split_layout(k->vp, k->split.buf, &b);
  SplitRule rule;
  SplitPlaneQ q[HSK_SPLIT_MAX_PLANES];
  split_rule_of(k, p, pl, n_planes, &rule, q);
  if (n_planes > 0) {
    HIPCHK(k, hipMemcpyAsync(b.planes, q, n_planes * sizeof(SplitPlaneQ), hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));  // (`q` is this frame's)
  }
  launch_split_classify(k->stream, k->d_vol, k->vp, b, rule);
  launch_comp_label(k->stream, b.cls, k->vp, b.comp);
  HIPCHK(k, hipGetLastError());
  unsigned counts[SPLIT_COUNTS];
  r = copy_out(k, counts, b.counts, sizeof(counts));
  if (r != HSK_OK) return r;
  hsk_split_stats st;
  memset(&st, 0, sizeof(st));
  uint64_t classed = 0;
  for (int c = SPLIT_FLOOR; c <= SPLIT_OBJECT; ++c) {
    st.n_class[c] = counts[c];
    classed += counts[c];
  }
  st.n_class[SPLIT_NONE] = (uint64_t)k->vp.X * (uint64_t)k->vp.Y * (uint64_t)k->vp.Z - classed;
  st.n_edge = counts[6];
  st.n_no_normal = counts[7];
  *n_objects = 0;
  RegionRead rr;
  r = region_read(k, b.comp, &k->split, SPLIT_REC_WORDS, 0, "hsk_split_scene: more than 2^24 objects: nothing is held",
                  "hsk_split_scene: out of host memory for the records", b.cls, p.min_voxels,
                  [&](const RegionTab& t, unsigned n) { launch_split_records(k->stream, k->vp, b, n, t.roots, t.extra, rule.floor_plane); }, &rr);
  if (r != HSK_OK) return r;
  const CompGrid g{(unsigned)k->vp.X, (unsigned)k->vp.Y, (unsigned)k->vp.Z};
  uint64_t kept = 0;
  try {
    st.n_minor_objects = comp_region_records(g, rr.roots.data(), rr.table.data(), rr.n, p.min_voxels, &k->split_recs, [&](hsk_object& c, size_t i) {
      const unsigned* t16 = &rr.extra[i * SPLIT_REC_WORDS];
      for (int a = 0; a < 3; ++a) c.sum[a] = (uint64_t)t16[2 * a] | ((uint64_t)t16[2 * a + 1] << 32);
      for (int a = 0; a < 4; ++a) c.contact[a] = t16[SPLIT_REC_CONTACT + a];
      c.plane_mask = (uint64_t)t16[SPLIT_REC_MASK] | ((uint64_t)t16[SPLIT_REC_MASK + 1] << 32);
      if (rule.floor_plane >= 0) {
        c.height_lo = (int32_t)((~t16[SPLIT_REC_HLO]) ^ 0x80000000u);
        c.height_hi = (int32_t)(t16[SPLIT_REC_HHI] ^ 0x80000000u);
      }
      kept += c.n_voxels;
    });
  } catch (const std::bad_alloc&) {
    k->split_recs.clear();
    return fail(k, HSK_ERR_STATE, "hsk_split_scene: out of host memory for the records");
  }
  // the final classes: what the kept objects hold stays OBJECT, the rest is MINOR
  st.n_class[SPLIT_MINOR] = st.n_class[SPLIT_OBJECT] - kept;
  st.n_class[SPLIT_OBJECT] = kept;
  st.n_objects = k->split_recs.size();
  st.largest = k->split_recs.empty() ? 0 : k->split_recs[0].n_voxels;
  k->split_stats = st;
  k->split.stamp(k, &key, split_key_bytes(n_planes));
  return split_reply(k, recs, cap, n_objects, stats, false);
}

extern "C" int hsk_download_split(hsk_ctx* k, const hsk_voxel_box* box, uint8_t* cls, uint8_t* plane, uint32_t* object) {
  if (!k) return HSK_ERR_ARG;
  hsk_voxel_box bx;
  size_t n;
  if (int rc = clear_box_check(k, box, "hsk_download_split", &bx, &n)) return rc;
  if (n > 0 && !cls) return fail(k, HSK_ERR_ARG, "hsk_download_split: cls is null");
  if (int rc = volume_state_check(k, k, "hsk_download_split")) return rc;
  if (int rc = k->split.require(k, "hsk_download_split", SPLIT_NOT_HELD)) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  ProductArrays pa;
  const int a_cls = pa.add(cls, n), a_plane = pa.add(plane, n), a_object = pa.add(object, n * 4);
  if (int r = pa.place(k)) return r;
  SplitBufs b;
  split_layout(k->vp, k->split.buf, &b);
  launch_split_box(k->stream, k->vp, b, bx.lo, bx.hi, n, pa.dev<unsigned char>(a_cls), pa.dev<unsigned char>(a_plane), pa.dev<unsigned>(a_object));
  HIPCHK(k, hipGetLastError());
  return pa.copy_out(k);
}

extern "C" int hsk_split_at(hsk_ctx* k, const float* xyz, size_t n, int radius, uint8_t* cls, uint8_t* plane, uint32_t* object) {
  if (!k) return HSK_ERR_ARG;
  if (int rc = points_check(k, "hsk_split_at", xyz, cls, n, radius, 4)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_split_at")) return rc;
  if (int rc = k->split.require(k, "hsk_split_at", SPLIT_NOT_HELD)) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  ProductArrays pa;  // (the points first: kept for the gather, not handed back)
  const int a_pts = pa.add(nullptr, n * 12, true), a_cls = pa.add(cls, n), a_plane = pa.add(plane, n), a_object = pa.add(object, n * 4);
  if (int r = pa.place(k)) return r;
  SplitBufs b;
  split_layout(k->vp, k->split.buf, &b);
  HIPCHK(k, hipMemcpyAsync(pa.dev<float>(a_pts), xyz, n * 12, hipMemcpyHostToDevice, k->stream));
  launch_split_gather(k->stream, k->vp, b, pa.dev<float>(a_pts), (unsigned)n, radius, pa.dev<unsigned char>(a_cls), pa.dev<unsigned char>(a_plane),
                      pa.dev<unsigned>(a_object));
  HIPCHK(k, hipGetLastError());
  return pa.copy_out(k);
}

extern "C" int hsk_remove_objects(hsk_ctx* k, const uint32_t* roots, size_t n, const hsk_remove_params* params, hsk_remove_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  hsk_remove_params p;
  hsk_default_remove_params(k, &p);
  if (params) p = *params;
  if (p.mode != HSK_REMOVE_ERASE && p.mode != HSK_REMOVE_RESTORE) return fail(k, HSK_ERR_ARG, "hsk_remove_objects: mode is neither HSK_REMOVE_ERASE nor HSK_REMOVE_RESTORE");
  if (p.halo < 0 || p.halo > 8) return fail(k, HSK_ERR_ARG, "hsk_remove_objects: halo must lie in 0..8");
  if (p.fill_weight < 1 || p.fill_weight > 128) return fail(k, HSK_ERR_ARG, "hsk_remove_objects: fill_weight must lie in 1..128");
  if (roots && n > HSK_REMOVE_MAX_OBJECTS) return fail(k, HSK_ERR_ARG, "hsk_remove_objects: more than 256 roots");
  if (int rc = volume_state_check(k, k, "hsk_remove_objects")) return rc;
  if (int rc = k->split.require(k, "hsk_remove_objects", SPLIT_NOT_HELD)) return rc;
  if (!roots && k->split_recs.size() > HSK_REMOVE_MAX_OBJECTS)
    return fail(k, HSK_ERR_ARG, "hsk_remove_objects: more than 256 kept objects: name the roots");
  // the selected records, each once
  const CompGrid g{(unsigned)k->vp.X, (unsigned)k->vp.Y, (unsigned)k->vp.Z};
  const int dims[3] = {k->vp.X, k->vp.Y, k->vp.Z};
  SplitSelected sel[HSK_REMOVE_MAX_OBJECTS];
  unsigned n_sel = 0;
  auto lin_of = [&](const hsk_object& c) { return g.lin((unsigned)c.root[0], (unsigned)c.root[1], (unsigned)c.root[2]); };
  auto take = [&](const hsk_object& c) {
    SplitSelected& e = sel[n_sel++];
    memset(&e, 0, sizeof(e));
    e.plane_mask = c.plane_mask;
    e.root = lin_of(c);
    for (int a = 0; a < 3; ++a) {
      e.lo[a] = std::max(c.lo[a] - p.halo, 0);
      e.hi[a] = std::min(c.hi[a] + p.halo, dims[a]);
    }
  };
  if (!roots) {
    for (const hsk_object& c : k->split_recs) take(c);
  } else {
    for (size_t i = 0; i < n; ++i) {
      bool seen = false;
      for (unsigned o = 0; o < n_sel; ++o) seen = seen || sel[o].root == roots[i];
      if (seen) continue;
      const hsk_object* found = nullptr;
      for (const hsk_object& c : k->split_recs)
        if (lin_of(c) == roots[i]) found = &c;
      if (!found) return fail(k, HSK_ERR_ARG, "hsk_remove_objects: a root is no kept object's label");
      take(*found);
    }
  }
  hsk_remove_stats st;
  memset(&st, 0, sizeof(st));
  st.n_objects = n_sel;
  if (n_sel == 0) {  // nothing is selected: nothing is launched
    if (stats) *stats = st;
    return HSK_OK;
  }
  int uni_lo[3], uni_hi[3];
  for (int a = 0; a < 3; ++a) {
    uni_lo[a] = sel[0].lo[a];
    uni_hi[a] = sel[0].hi[a];
    for (unsigned o = 1; o < n_sel; ++o) {
      uni_lo[a] = std::min(uni_lo[a], sel[o].lo[a]);
      uni_hi[a] = std::max(uni_hi[a], sel[o].hi[a]);
    }
  }
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  SplitBufs b;
  split_layout(k->vp, k->split.buf, &b);
  SplitRule rule;
  SplitPlaneQ q[HSK_SPLIT_MAX_PLANES];
  SplitKey held;  // (the table on the device is the held split's)
  memcpy(&held, k->split.key.data(), k->split.key.size());
  split_rule_of(k, held.p, held.planes, split_key_planes(k->split), &rule, q);
  HIPCHK(k, hipMemcpyAsync(b.sel, sel, n_sel * sizeof(SplitSelected), hipMemcpyHostToDevice, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));  // (`sel` is this frame's)
  launch_split_halo(k->stream, k->d_vol, k->vp, b, n_sel, uni_lo, uni_hi, rule, p.mode, p.halo, p.fill_weight);
  HIPCHK(k, hipGetLastError());
  unsigned counts[3] = {0, 0, 0};
  int r = copy_out(k, counts, b.counts + 8, sizeof(counts));
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  st.n_targets = counts[0];
  st.n_written = counts[1];
  st.n_restored = counts[2];
  if (st.n_written > 0) {
    st.n_colored = k->d_color ? st.n_written : 0;
    r = commit_volume_write(k, [&] { launch_split_restore(k->stream, k->d_vol, k->d_color, k->vp, b, n_sel, uni_lo, uni_hi, rule, p.mode, p.fill_weight); });
    k->split.drop();  // (the held split described the volume as it was)
    if (r != HSK_OK) return r;
  }  // (else nothing is written, vol_epoch does not move: cached passes and the split stay valid)
  if (stats) *stats = st;
  return HSK_OK;
}

extern "C" int hsk_release_split(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const int r = k->split.release(k);
  k->split_recs.clear();
  return r;
}
