// api_diff.hip -- the C ABI's volume differencing (include/hskinfu.h "Volume differencing"; DESIGN.md 3.23 the kernels, 8q the
// rule): hsk_default_diff_params, hsk_diff_volume, hsk_download_diff, hsk_diff_at, hsk_adopt_diff, hsk_release_diff.  The rule
// compares weights with min_weight, so both contexts' deferred weights are written back first (as hsk_fuse_volume does; that
// changes nothing either context returns).  The regions are components.hip's labelling run on the class words, in a scratch of
// the diff's own (diff, a HeldPass): hsk_label_components' cached labelling (comp) is neither read nor written.  The diff
// stays on the device with its records and stats on the host while ref's volume and its key stand; a call with the same cur
// and parameters meanwhile is answered from them.  Adopting writes the volume in
// hsk_prune_components' order: flush the deferred weights, write, volume_replaced.
#pragma clang fp contract(off)
#include <algorithm>
#include <new>

#include "hsk_ctx.h"
#include "hsk_diff_point.h"

static_assert(HSK_DIFF_UNSEEN == DIFF_UNSEEN && HSK_DIFF_ONLY_REF == DIFF_ONLY_REF && HSK_DIFF_ONLY_CUR == DIFF_ONLY_CUR && HSK_DIFF_SAME == DIFF_SAME &&
                  HSK_DIFF_APPEARED == DIFF_APPEARED && HSK_DIFF_VANISHED == DIFF_VANISHED && HSK_DIFF_MINOR == DIFF_MINOR &&
                  HSK_ADOPT_APPEARED == DIFF_ADOPT_APPEARED && HSK_ADOPT_VANISHED == DIFF_ADOPT_VANISHED && HSK_COMPONENT_NONE == COMP_NONE,
              "hsk_diff_point.h restates the header's numbers");
static_assert(sizeof(hsk_diff_params) == 16 && sizeof(hsk_diff_region) == 64 && sizeof(hsk_diff_stats) == 80 && sizeof(hsk_adopt_params) == 8 &&
                  sizeof(hsk_adopt_stats) == 24,
              "the diff structs");

extern "C" void hsk_default_diff_params(const hsk_ctx* k, hsk_diff_params* p) {
  if (!p) return;
  hsk_prune_params pp;
  hsk_default_prune_params(k, &pp);
  memset(p, 0, sizeof(*p));
  p->thresh = 16384;
  p->min_weight = 1;
  p->min_voxels = pp.min_voxels;
}

#define DIFF_NOT_HELD ": no diff is held for the volume as it stands"

// the diff's key: cur's serial and cur's epoch (hsk_adopt_diff compares these two alone), then the zero-padded parameters
struct DiffKey {
  uint64_t cur[2];
  hsk_diff_params p;
};
static DiffKey diff_key_of(const hsk_ctx* cur, const hsk_diff_params& p) {
  DiffKey key;
  memset(&key, 0, sizeof(key));  // (compared as bytes: the padding, if any, is zero on both sides)
  key.cur[0] = cur->serial;
  key.cur[1] = cur->vol_epoch;
  key.p.thresh = p.thresh;
  key.p.min_weight = p.min_weight;
  key.p.min_voxels = p.min_voxels;
  return key;
}

// hsk_diff_volume's answer from the held records and stats
static int diff_reply(hsk_ctx* k, hsk_diff_region* recs, size_t cap, size_t* n_regions, hsk_diff_stats* stats) {
  if (stats) *stats = k->diff_stats;
  return reply_records(k, k->diff_recs, recs, cap, n_regions, "hsk_diff_volume: cap is below the number of kept regions");
}

extern "C" int hsk_diff_volume(hsk_ctx* ref, hsk_ctx* cur, const hsk_diff_params* params, hsk_diff_region* recs, size_t cap, size_t* n_regions,
                               hsk_diff_stats* stats) {
  if (!ref) return HSK_ERR_ARG;
  if (!cur || !n_regions) return fail(ref, HSK_ERR_ARG, "hsk_diff_volume: null argument");
  if (ref == cur) return fail(ref, HSK_ERR_ARG, "hsk_diff_volume: ref and cur are the same context");
  hsk_diff_params p;
  hsk_default_diff_params(ref, &p);  // (zeroes the whole struct first)
  if (params) {
    p.thresh = params->thresh;
    p.min_weight = params->min_weight;
    p.min_voxels = params->min_voxels;
  }
  if (p.thresh < 1 || p.thresh > 65534) return fail(ref, HSK_ERR_ARG, "hsk_diff_volume: thresh must lie in 1..65534");
  if (p.min_weight < 1 || p.min_weight > 128) return fail(ref, HSK_ERR_ARG, "hsk_diff_volume: min_weight must lie in 1..128");
  if (p.min_voxels < 1) return fail(ref, HSK_ERR_ARG, "hsk_diff_volume: min_voxels must be at least 1");
  for (hsk_ctx* c : {ref, cur})
    if (int rc = volume_state_check(c, ref, "hsk_diff_volume")) return rc;
  if (ref->vp.X != cur->vp.X || ref->vp.Y != cur->vp.Y || ref->vp.Z != cur->vp.Z || memcmp(ref->cfg.vol_size_m, cur->cfg.vol_size_m, 3 * sizeof(float)) != 0 ||
      memcmp(&ref->vp.tau, &cur->vp.tau, sizeof(float)) != 0)
    return fail(ref, HSK_ERR_ARG,
                "hsk_diff_volume: the volumes do not lie on the same grid (dims, size_m and effective truncation distance must be equal); resample cur first: "
                "hsk_fuse_volume into an empty context of ref's configuration");
  if (ref->cfg.device_id != cur->cfg.device_id) return fail(ref, HSK_ERR_ARG, "hsk_diff_volume: the contexts are on different devices");
  hsk_ctx* k = ref;
  // the diff of an earlier call still fits: both volumes stand, cur is the same context, the parameters are the same.  Nothing is
  // launched; the records and stats are the held ones (what a size query followed by the fill costs once, as the labelling's)
  const DiffKey key = diff_key_of(cur, p);
  if (k->diff.stands_for(k, &key, sizeof(key))) return diff_reply(k, recs, cap, n_regions, stats);
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  // cur: read only.  Its deferred weights are written back; everything its stream holds must have ended before ref's stream reads it
  flush_weights(cur);
  HIPCHK(k, hipStreamSynchronize(cur->stream));
  flush_weights(k);
  k->diff.drop();  // (the scratch is about to be written: an earlier diff goes)
  k->diff_recs.clear();
  int r = k->diff.grow(k, diff_layout(k->vp, nullptr, nullptr));
  if (r != HSK_OK) return r;
  DiffBufs b;
  diff_layout(k->vp, k->diff.buf, &b);
  launch_diff_classify(k->stream, k->d_vol, cur->d_vol, k->vp, b, p.thresh, p.min_weight);
  launch_comp_label(k->stream, b.cls, k->vp, b.comp);
  HIPCHK(k, hipGetLastError());
  unsigned counts[DIFF_COUNTS];
  r = copy_out(k, counts, b.counts, sizeof(counts));
  if (r != HSK_OK) return r;
  hsk_diff_stats st;
  memset(&st, 0, sizeof(st));
  for (int c = 0; c < DIFF_CLASSES; ++c) st.n_class[c] = counts[c];
  *n_regions = 0;
  RegionRead rr;
  r = region_read(k, b.comp, &k->diff, 2, 0, "hsk_diff_volume: more than 2^24 regions: nothing is held", "hsk_diff_volume: out of host memory for the records", b.cls,
                  p.min_voxels, [&](const RegionTab& t, unsigned n) { launch_diff_records(k->stream, k->vp, b, n, t.roots, t.extra); }, &rr);
  if (r != HSK_OK) return r;
  const CompGrid g{(unsigned)k->vp.X, (unsigned)k->vp.Y, (unsigned)k->vp.Z};
  uint64_t kept_a = 0, kept_v = 0;
  try {
    st.n_minor_regions = comp_region_records(g, rr.roots.data(), rr.table.data(), rr.n, p.min_voxels, &k->diff_recs, [&](hsk_diff_region& c, size_t i) {
      kept_a += c.n_appeared = rr.extra[2 * i];
      kept_v += c.n_vanished = rr.extra[2 * i + 1];
    });
  } catch (const std::bad_alloc&) {
    k->diff_recs.clear();
    return fail(k, HSK_ERR_STATE, "hsk_diff_volume: out of host memory for the records");
  }
  // the final classes: what the kept regions hold stays APPEARED or VANISHED, the rest of CHANGED is MINOR
  st.n_class[DIFF_MINOR] = (st.n_class[DIFF_APPEARED] - kept_a) + (st.n_class[DIFF_VANISHED] - kept_v);
  st.n_class[DIFF_APPEARED] = kept_a;
  st.n_class[DIFF_VANISHED] = kept_v;
  st.n_regions = k->diff_recs.size();
  st.largest = k->diff_recs.empty() ? 0 : k->diff_recs[0].n_voxels;
  k->diff_stats = st;
  k->diff.stamp(k, &key, sizeof(key));
  return diff_reply(k, recs, cap, n_regions, stats);
}

extern "C" int hsk_download_diff(hsk_ctx* k, const hsk_voxel_box* box, uint8_t* cls, uint32_t* region) {
  if (!k) return HSK_ERR_ARG;
  hsk_voxel_box bx;
  size_t n;
  if (int rc = clear_box_check(k, box, "hsk_download_diff", &bx, &n)) return rc;
  if (n > 0 && !cls) return fail(k, HSK_ERR_ARG, "hsk_download_diff: cls is null");
  if (int rc = volume_state_check(k, k, "hsk_download_diff")) return rc;
  if (int rc = k->diff.require(k, "hsk_download_diff", DIFF_NOT_HELD)) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  ProductArrays pa;
  const int a_cls = pa.add(cls, n), a_region = pa.add(region, n * 4);
  if (int r = pa.place(k)) return r;
  DiffBufs b;
  diff_layout(k->vp, k->diff.buf, &b);
  launch_diff_box(k->stream, k->vp, b, bx.lo, bx.hi, n, pa.dev<unsigned char>(a_cls), pa.dev<unsigned>(a_region));
  HIPCHK(k, hipGetLastError());
  return pa.copy_out(k);
}

extern "C" int hsk_diff_at(hsk_ctx* k, const float* xyz, size_t n, int radius, uint8_t* cls, uint32_t* region) {
  if (!k) return HSK_ERR_ARG;
  if (int rc = points_check(k, "hsk_diff_at", xyz, cls, n, radius, 4)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_diff_at")) return rc;
  if (int rc = k->diff.require(k, "hsk_diff_at", DIFF_NOT_HELD)) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  DiffBufs b;
  diff_layout(k->vp, k->diff.buf, &b);
  return gather_points(
      k, xyz, n, region, [&](const float* pts, unsigned* reg, unsigned char* c) { launch_diff_gather(k->stream, k->vp, b, pts, (unsigned)n, radius, reg, c); }, cls);
}

extern "C" int hsk_adopt_diff(hsk_ctx* ref, hsk_ctx* cur, const hsk_adopt_params* params, hsk_adopt_stats* stats) {
  if (!ref) return HSK_ERR_ARG;
  if (!cur) return fail(ref, HSK_ERR_ARG, "hsk_adopt_diff: null argument");
  if (ref == cur) return fail(ref, HSK_ERR_ARG, "hsk_adopt_diff: ref and cur are the same context");
  hsk_adopt_params p;
  p.which = HSK_ADOPT_APPEARED | HSK_ADOPT_VANISHED;
  p.halo = 2;
  if (params) p = *params;
  if (p.which < 1 || p.which > 3) return fail(ref, HSK_ERR_ARG, "hsk_adopt_diff: which must be HSK_ADOPT_APPEARED, HSK_ADOPT_VANISHED or both");
  if (p.halo < 0 || p.halo > 8) return fail(ref, HSK_ERR_ARG, "hsk_adopt_diff: halo must lie in 0..8");
  for (hsk_ctx* c : {ref, cur})
    if (int rc = volume_state_check(c, ref, "hsk_adopt_diff")) return rc;
  if (int rc = ref->diff.require(ref, "hsk_adopt_diff", DIFF_NOT_HELD)) return rc;
  const uint64_t cur_now[2] = {cur->serial, cur->vol_epoch};
  if (memcmp(ref->diff.key.data(), cur_now, sizeof(cur_now)) != 0)
    return fail(ref, HSK_ERR_STATE, "hsk_adopt_diff: no diff is held for the volumes as they stand (cur is another context, or its volume has changed)");
  hsk_ctx* k = ref;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  HIPCHK(k, hipStreamSynchronize(cur->stream));
  DiffBufs b;
  diff_layout(k->vp, k->diff.buf, &b);
  launch_diff_halo(k->stream, cur->d_vol, k->vp, b, p.which, p.halo);
  HIPCHK(k, hipGetLastError());
  unsigned counts[2] = {0, 0};
  int r = copy_out(k, counts, b.counts + 8, sizeof(counts));
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  hsk_adopt_stats st;
  memset(&st, 0, sizeof(st));
  st.n_targets = counts[0];
  st.n_adopted = counts[1];
  if (st.n_adopted > 0) {
    st.n_colored = (k->d_color && cur->d_color) ? st.n_adopted : 0;
    r = commit_volume_write(k, [&] { launch_diff_adopt(k->stream, k->d_vol, cur->d_vol, k->d_color, cur->d_color, k->vp, b); });
    k->diff.drop();  // (the held diff described the volume as it was)
    if (r != HSK_OK) return r;
  }  // (else nothing is written, vol_epoch does not move: cached passes and the diff stay valid)
  if (stats) *stats = st;
  return HSK_OK;
}

extern "C" int hsk_release_diff(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const int r = k->diff.release(k);
  k->diff_recs.clear();
  return r;
}
