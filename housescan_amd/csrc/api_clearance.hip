// api_clearance.hip -- the C ABI's clearance field (include/hskinfu.h "Clearance field"; DESIGN.md 3.18 the kernels, 8l the rule):
// hsk_default_clearance_params, hsk_clearance_d2, hsk_build_clearance, hsk_download_clearance, hsk_clearance_at,
// hsk_clearance_floor, hsk_release_clearance and the host-only hsk_rank_views_clear.  The field reads the volume as it stands, with
// NO flush of the deferred weights (as the coverage calls and the components): the rule asks of a weight only whether it is zero
// and of the TSDF its sign.  It stays on the device (clear, a HeldPass) while vol_epoch and the 20 device-relevant parameter bytes stand.
// Nothing the tracker reads is written; vol_epoch does not move.  The reads of the fields over it (api_reach.hip, api_partition.hip)
// and the census (api_cover.hip) take from here the box check, the floor map's grid and the point gather (hsk_ctx.h).
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>

#include "hsk_ctx.h"
#include "hsk_clear_point.h"

extern "C" void hsk_default_clearance_params(const hsk_ctx* k, hsk_clearance_params* p) {
  if (!p) return;
  float cell[3];
  context_cells(k, cell, nullptr);
  memset(p, 0, sizeof(*p));
  p->flags = HSK_CLEAR_UNKNOWN;
  const float cmin = std::min(cell[0], std::min(cell[1], cell[2]));
  uint32_t wmin = 1;
  if (cell[0] == cell[1] && cell[1] == cell[2]) {
    p->weight[0] = p->weight[1] = p->weight[2] = 1;
    p->unit_m = cmin;
  } else {
    wmin = 1024;
    for (int i = 0; i < 3; ++i) {
      const double q = (double)cell[i] / (double)cmin;
      p->weight[i] = (uint32_t)std::min(1024.0, std::rint(16.0 * (q * q)));
      wmin = std::min(wmin, p->weight[i]);
    }
    p->unit_m = (float)((double)cmin / 4.0);
  }
  const double inv = 1.0 / (double)p->unit_m;
  p->max_d2 = (uint32_t)std::min(std::ceil(inv * inv), 255.0 * 255.0 * (double)wmin);
}

extern "C" uint32_t hsk_clearance_d2(const hsk_clearance_params* p, float metres) {
  if (!p || !(std::isfinite(p->unit_m) && p->unit_m > 0.0f) || metres != metres) return 0xffffffffu;
  if (metres <= 0.0f) return 0u;
  const double q = (double)metres / (double)p->unit_m;
  const double d = std::ceil(q * q);
  return d >= 4294967295.0 ? 0xffffffffu : (uint32_t)d;
}

void context_cells(const hsk_ctx* k, float cell[3], float* tau) {
  if (k) {
    for (int i = 0; i < 3; ++i) cell[i] = k->vp.cell[i];
    if (tau) *tau = k->vp.tau;
    return;
  }
  hsk_config c;
  hsk_default_config(&c, 256);
  cell[0] = c.vol_size_m[0] / (float)c.vol_x;
  cell[1] = c.vol_size_m[1] / (float)c.vol_y;
  cell[2] = c.vol_size_m[2] / (float)c.vol_z;
  if (tau) *tau = config_tau(&c);
}

int points_check(hsk_ctx* k, const char* who, const void* xyz, const void* out, size_t n, int radius, int max_radius) {
  auto bad = [&](const std::string& what) { return fail(k, HSK_ERR_ARG, (who + what).c_str()); };
  if (n > 0 && (!xyz || !out)) return bad(": null argument");
  if (n > HSK_CLEAR_MAX_POINTS) return bad(": more than 2^20 points");
  if (max_radius >= 0 && (radius < 0 || radius > max_radius)) return bad(": radius must lie in 0.." + std::to_string(max_radius));
  return HSK_OK;
}

// the parameters a call works with (NULL: the defaults), checked -> the kernels' block
int clear_check(hsk_ctx* k, const hsk_clearance_params* params, const char* who, hsk_clearance_params* p, ClearGeom* q) {
  if (params)
    *p = *params;
  else
    hsk_default_clearance_params(k, p);
  auto bad = [&](const char* what) { return fail(k, HSK_ERR_ARG, (std::string(who) + what).c_str()); };
  if (p->flags & ~HSK_CLEAR_UNKNOWN) return bad(": unknown flag bits");
  q->X = (unsigned)k->vp.X;
  q->Y = (unsigned)k->vp.Y;
  q->Z = (unsigned)k->vp.Z;
  q->Zg = ((unsigned)k->vp.Z + 3u) >> 2;
  q->nw = ((unsigned)k->vp.X + CLEAR_MASK_BITS - 1u) / CLEAR_MASK_BITS;
  q->max_d2 = p->max_d2;
  q->flags = p->flags;
  for (int i = 0; i < 3; ++i) {
    if (p->weight[i] < 1 || p->weight[i] > 1024) return bad(": a weight must lie in 1..1024");
    q->w[i] = p->weight[i];
    const double r = floor(sqrt((double)p->max_d2 / (double)p->weight[i]));
    if (r > (double)HSK_CLEAR_MAX_REACH) return bad(": the reach floor(sqrt(max_d2 / weight)) must not exceed 255 voxels on any axis");
    q->R[i] = (unsigned)r;
  }
  return HSK_OK;
}

int volume_state_check(hsk_ctx* k, hsk_ctx* errs, const char* who) {
  if (int rs = require_whole_volume(k, errs, who)) return rs;
  if (int ri = require_idle(k, errs)) return ri;
  if ((uint64_t)k->vp.X * (uint64_t)k->vp.Y * (uint64_t)k->vp.Z > ((uint64_t)1 << 31))
    return fail(errs, HSK_ERR_ARG, (std::string(who) + ": the volume has more than 2^31 voxels").c_str());
  return HSK_OK;
}

int clear_box_check(hsk_ctx* k, const hsk_voxel_box* box, const char* who, hsk_voxel_box* b, size_t* n) {
  const int dims[3] = {k->vp.X, k->vp.Y, k->vp.Z};
  *n = 1;
  for (int i = 0; i < 3; ++i) {
    b->lo[i] = box ? box->lo[i] : 0;
    b->hi[i] = box ? box->hi[i] : dims[i];
    if (b->lo[i] < 0 || b->hi[i] > dims[i] || b->hi[i] < b->lo[i])
      return fail(k, HSK_ERR_ARG, (std::string(who) + ": the box must satisfy 0 <= lo <= hi <= the volume's dims on every axis").c_str());
    *n *= (size_t)(b->hi[i] - b->lo[i]);
  }
  return HSK_OK;
}

int clear_floor_grid(hsk_ctx* k, const ClearGeom& q, int axis, int lo, int hi, const char* who, FloorGrid* f) {
  if (axis < 0 || axis > 2) return fail(k, HSK_ERR_ARG, (std::string(who) + ": axis must be 0, 1 or 2").c_str());
  const int dims[3] = {k->vp.X, k->vp.Y, k->vp.Z};
  if (lo < 0 || hi > dims[axis] || hi < lo) return fail(k, HSK_ERR_ARG, (std::string(who) + ": the band must satisfy 0 <= lo <= hi <= the axis").c_str());
  f->au = axis == 0 ? 1 : 0;
  f->av = axis == 2 ? 1 : 2;
  f->nu = (unsigned)dims[f->au];
  f->nv = (unsigned)dims[f->av];
  const unsigned w[3] = {q.w[f->au], q.w[f->av], q.w[axis]};
  memcpy(f->w, w, sizeof(w));
  return HSK_OK;
}

int download_rows(hsk_ctx* k, const void* field, size_t elem_bytes, const hsk_voxel_box& b, size_t n, void* out) {
  if (n == 0) return HSK_OK;
  if (n == (size_t)k->vp.X * k->vp.Y * k->vp.Z) return copy_out(k, out, field, n * elem_bytes);
  int r = ensure_product_bytes(k, n * elem_bytes);
  if (r != HSK_OK) return r;
  launch_box_rows(k->stream, field, elem_bytes, k->vp, b.lo, b.hi, n, k->d_out);
  HIPCHK(k, hipGetLastError());
  return copy_out(k, out, k->d_out, n * elem_bytes);
}

int gather_points(hsk_ctx* k, const float* xyz, size_t n, uint32_t* out, const std::function<void(const float*, unsigned*, unsigned char*)>& launch,
                  uint8_t* bytes) {
  ProductLayout lay;
  const size_t pts_at = lay.take(n * 12), out_at = lay.take(n * 4), bytes_at = lay.take(bytes ? n : 0);
  int r = ensure_product_bytes(k, lay.bytes);
  if (r != HSK_OK) return r;
  char* base = (char*)k->d_out;
  HIPCHK(k, hipMemcpyAsync(base + pts_at, xyz, n * 12, hipMemcpyHostToDevice, k->stream));
  launch((const float*)(base + pts_at), (unsigned*)(base + out_at), bytes ? (unsigned char*)(base + bytes_at) : nullptr);
  HIPCHK(k, hipGetLastError());
  if (bytes) r = copy_out(k, bytes, base + bytes_at, n);
  if (r == HSK_OK && out) r = copy_out(k, out, base + out_at, n * 4);
  return r;
}

void clear_key_of(const hsk_clearance_params& p, uint32_t key[5]) {
  key[0] = p.weight[0];
  key[1] = p.weight[1];
  key[2] = p.weight[2];
  key[3] = p.max_d2;
  key[4] = p.flags;
}

// the field of the volume as it stands for the checked parameters, in clear's scratch; *reused: nothing had to be launched
int clear_build(hsk_ctx* k, const hsk_clearance_params& p, const ClearGeom& q, bool* reused) {
  uint32_t key[5];
  clear_key_of(p, key);
  *reused = k->clear.stands_for(k, key, sizeof(key));
  if (*reused) return HSK_OK;
  k->clear.drop();
  int r = k->clear.grow(k, clear_layout(k->vp, nullptr, nullptr));
  if (r != HSK_OK) return r;
  ClearBufs b;
  clear_layout(k->vp, k->clear.buf, &b);
  launch_clear_build(k->stream, k->d_vol, q, b);
  HIPCHK(k, hipGetLastError());
  unsigned long long counts[3];
  r = copy_out(k, counts, b.stats, sizeof(counts));
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  memcpy(k->clear_counts, counts, sizeof(counts));
  k->clear.stamp(k, key, sizeof(key));
  return HSK_OK;
}

extern "C" int hsk_build_clearance(hsk_ctx* k, const hsk_clearance_params* params, hsk_clearance_stats* stats) {
  static_assert(sizeof(hsk_clearance_params) == 24 && sizeof(hsk_clearance_stats) == 32, "the clearance structs");
  if (!k) return HSK_ERR_ARG;
  hsk_clearance_params p;
  ClearGeom q;
  if (int rc = clear_check(k, params, "hsk_build_clearance", &p, &q)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_build_clearance")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  bool reused = false;
  int r = clear_build(k, p, q, &reused);
  if (r != HSK_OK) return r;
  if (stats) {
    hsk_clearance_stats st;
    memset(&st, 0, sizeof(st));
    st.n_obstacle = k->clear_counts[0];
    st.n_far = k->clear_counts[1];
    st.max_d2_seen = (uint32_t)k->clear_counts[2];
    st.scratch_bytes = k->clear.bytes;
    st.reused = reused ? 1 : 0;
    *stats = st;
  }
  return HSK_OK;
}

extern "C" int hsk_download_clearance(hsk_ctx* k, const hsk_clearance_params* params, const hsk_voxel_box* box, uint32_t* d2) {
  if (!k) return HSK_ERR_ARG;
  if (!d2) return fail(k, HSK_ERR_ARG, "hsk_download_clearance: d2 is null");
  hsk_clearance_params p;
  ClearGeom q;
  if (int rc = clear_check(k, params, "hsk_download_clearance", &p, &q)) return rc;
  hsk_voxel_box b;
  size_t n;
  if (int rc = clear_box_check(k, box, "hsk_download_clearance", &b, &n)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_download_clearance")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  bool reused = false;
  int r = clear_build(k, p, q, &reused);
  if (r != HSK_OK) return r;
  ClearBufs cb;
  clear_layout(k->vp, k->clear.buf, &cb);
  return download_rows(k, cb.field, 4, b, n, d2);
}

extern "C" int hsk_clearance_at(hsk_ctx* k, const hsk_clearance_params* params, const float* xyz, size_t n, uint32_t* d2) {
  if (!k) return HSK_ERR_ARG;
  if (int rc = points_check(k, "hsk_clearance_at", xyz, d2, n, 0, -1)) return rc;
  hsk_clearance_params p;
  ClearGeom q;
  if (int rc = clear_check(k, params, "hsk_clearance_at", &p, &q)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_clearance_at")) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  bool reused = false;
  int r = clear_build(k, p, q, &reused);
  if (r != HSK_OK) return r;
  ClearBufs cb;
  clear_layout(k->vp, k->clear.buf, &cb);
  return gather_points(k, xyz, n, d2, [&](const float* pts, unsigned* out, unsigned char*) { launch_clear_gather(k->stream, cb.field, k->vp, pts, (unsigned)n, out); });
}

extern "C" int hsk_clearance_floor(hsk_ctx* k, const hsk_clearance_params* params, int axis, int lo, int hi, uint32_t* map, hsk_clearance_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  if (!map) return fail(k, HSK_ERR_ARG, "hsk_clearance_floor: map is null");
  hsk_clearance_params p;
  ClearGeom q;
  if (int rc = clear_check(k, params, "hsk_clearance_floor", &p, &q)) return rc;
  FloorGrid f;
  if (int rc = clear_floor_grid(k, q, axis, lo, hi, "hsk_clearance_floor", &f)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_clearance_floor")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const size_t n = (size_t)f.nu * f.nv;
  ProductLayout lay;
  const size_t a_at = lay.take(n * 4), b_at = lay.take(n * 4);
  int r = ensure_product_bytes(k, lay.bytes);
  if (r != HSK_OK) return r;
  char* base = (char*)k->d_out;
  launch_clear_floor(k->stream, k->d_vol, k->vp, q, axis, lo, hi, (unsigned*)(base + a_at), (unsigned*)(base + b_at));
  HIPCHK(k, hipGetLastError());
  r = copy_out(k, map, base + a_at, n * 4);
  if (r != HSK_OK) return r;
  if (stats) {  // (a few hundred KiB, already here: counted on the host.  Only an obstacle column has the value 0: a border term is at least a weight)
    hsk_clearance_stats st;
    memset(&st, 0, sizeof(st));
    for (size_t i = 0; i < n; ++i) {
      st.n_obstacle += map[i] == 0u ? 1 : 0;
      st.n_far += map[i] == HSK_CLEARANCE_FAR ? 1 : 0;
      if (map[i] != HSK_CLEARANCE_FAR && map[i] > st.max_d2_seen) st.max_d2_seen = map[i];
    }
    st.scratch_bytes = lay.bytes;
    *stats = st;
  }
  return HSK_OK;
}

extern "C" int hsk_release_clearance(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  return k->clear.release(k);
}

extern "C" int hsk_rank_views_clear(const hsk_view_score* s, const uint32_t* eye_d2, uint32_t min_d2, size_t n, uint32_t* order) {
  if (n > 0 && (!s || !eye_d2 || !order)) return HSK_ERR_ARG;
  if (n > 0xffffffffull) return HSK_ERR_ARG;
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  auto behind = [&](uint32_t a) { return s[a].eye_state != HSK_EYE_FREE || eye_d2[a] < min_d2 || eye_d2[a] == HSK_CLEARANCE_OUTSIDE; };
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {  // (stable: equal scores stay in index order)
    const bool sa = behind(a), sb = behind(b);
    if (sa != sb) return sb;
    if (s[a].gain != s[b].gain) return s[a].gain > s[b].gain;
    return s[a].n_frontier > s[b].n_frontier;
  });
  return HSK_OK;
}
