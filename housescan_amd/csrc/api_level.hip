// api_level.hip -- the C ABI's upright-frame estimate (include/hskinfu.h "Upright frame"; DESIGN.md 3.21 the kernels, 8o the rule):
// hsk_estimate_upright, hsk_estimate_upright_oriented, hsk_upright_sums, hsk_default_upright_params, the host steps
// hsk_upright_solve_* and hsk_level_config.  The order of the questions and every step between them is hsk_level_solve.h's
// (level_estimate); this file answers the questions with level.hip's kernels, and the host waits for each answer.
#pragma clang fp contract(off)
#include <cmath>
#include <new>
#include <vector>

#include "hsk_ctx.h"
#include "hsk_level_solve.h"

static_assert(HSK_UPRIGHT_HIST_BINS == HSK_LEVEL_HIST_BINS && HSK_UPRIGHT_HEIGHT_BINS == HSK_LEVEL_H_BINS, "the public sizes are the kernels'");
static_assert(sizeof(hsk_upright_params) == 36 && sizeof(hsk_upright) == 128, "the upright structs are 36 and 128 bytes");

// what the estimate adds to the alignment's scratch behind the cloud's planes: the histogram (and the valid count), the blocks'
// partial values, the 16 words they fold to, the height histograms' counts and sums
struct LevelScratch {
  size_t hist_at, partial_at, sums_at, hcount_at, hsum_at, bytes;
  explicit LevelScratch(size_t n) {
    ProductLayout L;
    hist_at = L.take((HSK_LEVEL_HIST_BINS + 1) * 4);
    partial_at = L.take((size_t)cloud_sweep_blocks((unsigned)n) * 16 * 8);
    sums_at = L.take(16 * 8);
    hcount_at = L.take((size_t)2 * HSK_LEVEL_H_BINS * 4);
    hsum_at = L.take((size_t)2 * HSK_LEVEL_H_BINS * 8);
    bytes = L.bytes;
  }
};

extern "C" void hsk_default_upright_params(hsk_upright_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->up_hint[1] = -1.0f;
  p->max_tilt_cos = 0.7071067811865476f;  // cos 45 degrees
  p->cone_cos = 0.984807753012208f;       // cos 10 degrees
  p->wall_sin = 0.25881904510252074f;     // sin 15 degrees
  p->min_fraction = 0.02f;
  p->refits = 3;
}

static bool cone_wall_ok(float cone_cos, float wall_sin) { return cone_cos > 0.0f && cone_cos <= 1.0f && wall_sin >= 0.0f && wall_sin <= 1.0f; }

// params (NULL: the defaults) -> p, or the refusal
static int upright_resolve(hsk_ctx* k, const hsk_upright_params* params, hsk_upright_params* p, const char* who) {
  if (params) *p = *params;
  else hsk_default_upright_params(p);
  double h[3];
  const bool ok = level_hint(p->up_hint, h) && p->max_tilt_cos >= -1.0f && p->max_tilt_cos <= 1.0f && cone_wall_ok(p->cone_cos, p->wall_sin) &&
                  std::isfinite(p->min_fraction) && p->min_fraction >= 0.0f && p->refits >= 0 && p->refits <= HSK_UPRIGHT_MAX_REFITS &&
                  (p->flags & ~HSK_UPRIGHT_NO_YAW) == 0u;
  return ok ? HSK_OK : fail(k, HSK_ERR_ARG, (std::string(who) + ": a parameter is outside its range").c_str());
}

// cell_weights (NULL: 1, 1, 1) -> w, or the refusal
static int weights_resolve(hsk_ctx* k, const float* cell_weights, LevelWeights* w, const char* who) {
  for (int c = 0; c < 3; ++c) {
    w->w[c] = cell_weights ? cell_weights[c] : 1.0f;
    if (!(w->w[c] > 0.0f && w->w[c] <= 1.0f)) return fail(k, HSK_ERR_ARG, (std::string(who) + ": a cell weight must lie in (0, 1]").c_str());
  }
  return HSK_OK;
}

static long long axis_len2(const int32_t a[3]) { return level_dot(a, a); }
static bool axis_ok(const int32_t a[3]) { return axis_len2(a) > 0 && axis_len2(a) <= (long long)HSK_UPRIGHT_AXIS_MAX2; }

// level_estimate's three questions, answered by the kernels over the n > 0 points in the scratch's planes
struct DeviceStages {
  hsk_ctx* k;
  const float* d_soa;
  unsigned n, pitch;
  LevelWeights w;
  double cone2, wall2;
  unsigned* d_hist;
  unsigned long long *d_partial, *d_sums, *d_hsum;
  unsigned* d_hcount;

  DeviceStages(hsk_ctx* k_, const CloudScratch& cs, size_t n_, const LevelWeights& w_, float cone_cos, float wall_sin)
      : k(k_), d_soa(cs.soa), n((unsigned)n_), pitch(cs.pitch), w(w_) {
    const LevelScratch L(n_);
    char* base = (char*)cs.extra;
    d_hist = (unsigned*)(base + L.hist_at);
    d_partial = (unsigned long long*)(base + L.partial_at);
    d_sums = (unsigned long long*)(base + L.sums_at);
    d_hcount = (unsigned*)(base + L.hcount_at);
    d_hsum = (unsigned long long*)(base + L.hsum_at);
    cone2 = (double)cone_cos * (double)cone_cos;
    wall2 = (double)wall_sin * (double)wall_sin;
  }
  int hist(uint32_t* hist_out, uint64_t* n_valid) {
    uint32_t tail = 0;
    HIPCHK(k, hipMemsetAsync(d_hist, 0, (HSK_LEVEL_HIST_BINS + 1) * 4, k->stream));
    launch_level_hist(k->stream, d_soa, n, pitch, w, d_hist);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(hist_out, d_hist, HSK_LEVEL_HIST_BINS * 4, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipMemcpyAsync(&tail, d_hist + HSK_LEVEL_HIST_BINS, 4, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    *n_valid = tail;
    return HSK_OK;
  }
  int sums(const int32_t A[3][3], int n_axes, int64_t s12[12], const int32_t W[3][3], int64_t w3[3]) {
    LevelAxes ax = {};
    ax.n_axes = n_axes;
    ax.wall = W ? 1 : 0;
    ax.cone2 = cone2, ax.wall2 = wall2;
    for (int a = 0; a < n_axes; ++a) {
      memcpy(ax.A[a], A[a], sizeof(ax.A[a]));
      ax.aa[a] = axis_len2(ax.A[a]);
    }
    if (W) {
      memcpy(ax.W, W, sizeof(ax.W));
      ax.waa = axis_len2(ax.W[0]);
    }
    long long s[15];
    launch_level_sums(k->stream, d_soa, n, pitch, w, ax, d_partial, d_sums);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(s, d_sums, sizeof(s), hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    for (int v = 0; v < 12; ++v) s12[v] = v < 4 * n_axes ? (int64_t)s[v] : 0;
    for (int v = 0; v < 3; ++v) w3[v] = W ? (int64_t)s[12 + v] : 0;
    return HSK_OK;
  }
  int extents(const int32_t R[3][3], bool classes, int32_t box[6], uint32_t* cnt, int64_t* sum) {
    LevelFrame fr = {};
    memcpy(fr.R, R, sizeof(fr.R));
    fr.raa = axis_len2(fr.R[1]);
    fr.cone2 = cone2;
    fr.classes = classes ? 1 : 0;
    if (classes) {
      HIPCHK(k, hipMemsetAsync(d_hcount, 0, (size_t)2 * HSK_LEVEL_H_BINS * 4, k->stream));
      HIPCHK(k, hipMemsetAsync(d_hsum, 0, (size_t)2 * HSK_LEVEL_H_BINS * 8, k->stream));
    }
    long long b[6];
    launch_level_extents(k->stream, d_soa, n, pitch, w, fr, d_partial, d_sums, d_hcount, d_hsum);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(b, d_sums, sizeof(b), hipMemcpyDeviceToHost, k->stream));
    if (classes) {
      HIPCHK(k, hipMemcpyAsync(cnt, d_hcount, (size_t)2 * HSK_LEVEL_H_BINS * 4, hipMemcpyDeviceToHost, k->stream));
      HIPCHK(k, hipMemcpyAsync(sum, d_hsum, (size_t)2 * HSK_LEVEL_H_BINS * 8, hipMemcpyDeviceToHost, k->stream));
    }
    HIPCHK(k, hipStreamSynchronize(k->stream));
    const bool any = b[0] <= b[3];  // (no valid point: the minima are still above the maxima)
    for (int v = 0; v < 6; ++v) box[v] = any ? (int32_t)b[v] : 0;
    return HSK_OK;
  }
};

// the estimate over the n > 0 points in the scratch's planes
static int level_run(hsk_ctx* k, const CloudScratch& cs, size_t n, const LevelWeights& w, const hsk_upright_params& p, hsk_upright* out) {
  std::vector<uint32_t> hist, cnt;
  std::vector<int64_t> sum;
  try {
    hist.resize(HSK_LEVEL_HIST_BINS);
    cnt.resize((size_t)2 * HSK_LEVEL_H_BINS);
    sum.resize((size_t)2 * HSK_LEVEL_H_BINS);
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, "upright estimate: out of host memory for the histograms");
  }
  DeviceStages st(k, cs, n, w, p.cone_cos, p.wall_sin);
  return level_estimate(st, (uint64_t)n, p, out, hist.data(), cnt.data(), sum.data());
}

extern "C" int hsk_estimate_upright_oriented(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const float cell_weights[3],
                                             const hsk_upright_params* params, hsk_upright* out) {
  if (!k) return HSK_ERR_ARG;
  if (!out || (n > 0 && (!xyz || !normals))) return fail(k, HSK_ERR_ARG, "hsk_estimate_upright_oriented: null argument");
  if (n > HSK_UPRIGHT_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_estimate_upright_oriented: more than 2^24 points");
  hsk_upright_params p;
  LevelWeights w;
  if (int rc = upright_resolve(k, params, &p, "hsk_estimate_upright_oriented")) return rc;
  if (int rc = weights_resolve(k, cell_weights, &w, "hsk_estimate_upright_oriented")) return rc;
  if (int ri = require_idle(k)) return ri;
  level_clear(out, n);
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  CloudScratch cs;
  if (int rc = align_scratch(k, n, LevelScratch(n).bytes, &cs)) return rc;
  if (int rc = cloud_upload(k, xyz, normals, n, 1, cs, nullptr, "hsk_estimate_upright_oriented")) return rc;
  return level_run(k, cs, n, w, p, out);
}

extern "C" int hsk_estimate_upright(hsk_ctx* k, const hsk_upright_params* params, hsk_upright* out) {
  if (!k) return HSK_ERR_ARG;
  if (!out) return fail(k, HSK_ERR_ARG, "hsk_estimate_upright: null argument");
  hsk_upright_params p;
  if (int rc = upright_resolve(k, params, &p, "hsk_estimate_upright")) return rc;
  if (int rs = require_whole_volume(k, k, "hsk_estimate_upright")) return rs;
  if (int ri = require_idle(k)) return ri;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  size_t n = 0;
  // the count pass alone says how many points there are: every refusal comes before the cloud is written
  if (int rc = cloud_count(k, &n)) return rc;
  if (n > HSK_UPRIGHT_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_estimate_upright: the cloud has more than 2^24 points");
  level_clear(out, n);
  if (n == 0) return HSK_OK;
  CloudScratch cs;
  if (int rc = cloud_from_volume(k, n, LevelScratch(n).bytes, &cs)) return rc;
  // the raycast's normals are differences over one cell per axis: w_k = c_min / c_k takes the cells' skew out
  float cmin = k->vp.cell[0];
  for (int c = 1; c < 3; ++c) cmin = k->vp.cell[c] < cmin ? k->vp.cell[c] : cmin;
  LevelWeights w;
  for (int c = 0; c < 3; ++c) w.w[c] = cmin / k->vp.cell[c];
  return level_run(k, cs, n, w, p, out);
}

extern "C" int hsk_upright_sums(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const float cell_weights[3], float cone_cos,
                                float wall_sin, uint32_t* hist, uint32_t* n_valid, const int32_t* axes, int n_axes, int64_t* axis_sums,
                                const int32_t* wall_axes, int64_t* wall_sums, const int32_t* frame, int32_t* box, uint32_t* height_counts,
                                int64_t* height_sums) {
  if (!k) return HSK_ERR_ARG;
  const char* who = "hsk_upright_sums";
  if (n > 0 && (!xyz || !normals)) return fail(k, HSK_ERR_ARG, "hsk_upright_sums: null argument");
  if (n > HSK_UPRIGHT_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_upright_sums: more than 2^24 points");
  if (!cone_wall_ok(cone_cos, wall_sin)) return fail(k, HSK_ERR_ARG, "hsk_upright_sums: cone_cos must lie in (0, 1] and wall_sin in [0, 1]");
  if (n_axes < 0 || n_axes > 3 || (axis_sums && n_axes > 0 && !axes) || (wall_sums && !wall_axes) || ((box || height_counts) && !frame) ||
      (height_counts != nullptr) != (height_sums != nullptr))
    return fail(k, HSK_ERR_ARG, "hsk_upright_sums: an output without its axes, or n_axes outside 0..3");
  const bool do_axes = axis_sums && n_axes > 0, do_wall = wall_sums != nullptr, do_frame = box || height_counts;
  bool ok = true;
  for (int a = 0; do_axes && a < n_axes; ++a) ok &= axis_ok(axes + 3 * a);
  for (int a = 0; do_wall && a < 3; ++a) ok &= axis_ok(wall_axes + 3 * a);
  for (int a = 0; do_frame && a < 3; ++a) ok &= axis_ok(frame + 3 * a);
  if (!ok) return fail(k, HSK_ERR_ARG, "hsk_upright_sums: an axis is zero or longer than 4100");
  LevelWeights w;
  if (int rc = weights_resolve(k, cell_weights, &w, who)) return rc;
  if (int ri = require_idle(k)) return ri;
  if (hist) memset(hist, 0, HSK_LEVEL_HIST_BINS * 4);
  if (n_valid) *n_valid = 0;
  if (do_axes) memset(axis_sums, 0, (size_t)n_axes * 4 * 8);
  if (do_wall) memset(wall_sums, 0, 3 * 8);
  if (box) memset(box, 0, 6 * 4);
  if (height_counts) memset(height_counts, 0, (size_t)2 * HSK_LEVEL_H_BINS * 4), memset(height_sums, 0, (size_t)2 * HSK_LEVEL_H_BINS * 8);
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  CloudScratch cs;
  if (int rc = align_scratch(k, n, LevelScratch(n).bytes, &cs)) return rc;
  if (int rc = cloud_upload(k, xyz, normals, n, 1, cs, nullptr, who)) return rc;
  DeviceStages st(k, cs, n, w, cone_cos, wall_sin);
  if (hist || n_valid) {
    std::vector<uint32_t> h(HSK_LEVEL_HIST_BINS);
    uint64_t nv = 0;
    if (int rc = st.hist(h.data(), &nv)) return rc;
    if (hist) memcpy(hist, h.data(), HSK_LEVEL_HIST_BINS * 4);
    if (n_valid) *n_valid = (uint32_t)nv;
  }
  if (do_axes || do_wall) {
    int32_t A[3][3] = {}, W[3][3] = {};
    int64_t s12[12], w3[3];
    if (do_axes) memcpy(A, axes, (size_t)n_axes * 12);
    if (do_wall) memcpy(W, wall_axes, sizeof(W));
    if (int rc = st.sums(A, do_axes ? n_axes : 0, s12, do_wall ? W : nullptr, w3)) return rc;
    if (do_axes) memcpy(axis_sums, s12, (size_t)n_axes * 4 * 8);
    if (do_wall) memcpy(wall_sums, w3, sizeof(w3));
  }
  if (do_frame) {
    int32_t R[3][3], b6[6];
    memcpy(R, frame, sizeof(R));
    if (int rc = st.extents(R, height_counts != nullptr, b6, height_counts, height_sums)) return rc;
    if (box) memcpy(box, b6, sizeof(b6));
  }
  return HSK_OK;
}

// ---- the host steps ----------------------------------------------------------------------------------------------------------------
extern "C" int hsk_upright_solve_seed(const uint32_t* hist, const float up_hint[3], float max_tilt_cos, uint64_t least, double axis[3],
                                      uint64_t* support, int* found) {
  double h[3];
  if (!hist || !up_hint || !axis || !support || !found || !level_hint(up_hint, h)) return HSK_ERR_ARG;
  bool f = false;
  level_solve_seed(hist, h, (double)max_tilt_cos, least, axis, support, &f);
  *found = f ? 1 : 0;
  return HSK_OK;
}
extern "C" int hsk_upright_solve_axis(const int64_t sums4[4], const float up_hint[3], double axis[3], int* ok) {
  double h[3];
  if (!sums4 || !up_hint || !axis || !ok || !level_hint(up_hint, h)) return HSK_ERR_ARG;
  *ok = level_solve_axis(sums4, h, axis) ? 1 : 0;
  return HSK_OK;
}
extern "C" int hsk_upright_solve_basis(const double up[3], double e1[3], double e2[3]) {
  if (!up || !e1 || !e2) return HSK_ERR_ARG;
  level_basis(up, e1, e2);
  return HSK_OK;
}
extern "C" int hsk_upright_solve_yaw(const int64_t wall3[3], uint64_t least, const double up[3], double x[3], int* found) {
  if (!wall3 || !up || !x || !found) return HSK_ERR_ARG;
  *found = level_solve_yaw(wall3, least, up, x) ? 1 : 0;
  return HSK_OK;
}
extern "C" int hsk_upright_solve_frame(const int64_t sums12[12], uint64_t least, const float up_hint[3], int yaw, double up[3], double x[3]) {
  double h[3];
  if (!sums12 || !up_hint || !up || !x || !level_hint(up_hint, h)) return HSK_ERR_ARG;
  level_solve_frame(sums12, least, h, yaw != 0, up, x);
  return HSK_OK;
}
extern "C" int hsk_upright_solve_rows(const double up[3], const double x[3], double rows9[9], int32_t axes9[9]) {
  if (!up || !x || !rows9) return HSK_ERR_ARG;
  double rows[3][3];
  level_rows(up, x, rows);
  memcpy(rows9, rows, sizeof(rows));
  for (int r = 0; axes9 && r < 3; ++r) level_quantise_axis(rows[r], axes9 + 3 * r);
  return HSK_OK;
}
extern "C" int hsk_upright_solve_heights(const uint32_t* height_counts, const int64_t* height_sums, uint64_t least, double* floor_m,
                                         double* ceiling_m, uint32_t* found) {
  if (!height_counts || !height_sums || !floor_m || !ceiling_m || !found) return HSK_ERR_ARG;
  *found = level_solve_heights(height_counts, height_sums, least, floor_m, ceiling_m);
  return HSK_OK;
}

// ---- hsk_level_config ----------------------------------------------------------------------------------------------------------------
extern "C" int hsk_level_config(hsk_ctx* src, const hsk_upright* up, float margin_m, hsk_config* cfg, float src_to_dst[16]) {
  if (!src) return HSK_ERR_ARG;
  if (!up || !cfg || !src_to_dst) return fail(src, HSK_ERR_ARG, "hsk_level_config: null argument");
  if (!(up->found & HSK_UPRIGHT_UP)) return fail(src, HSK_ERR_ARG, "hsk_level_config: the up direction was not found");
  if (!std::isfinite(margin_m)) return fail(src, HSK_ERR_ARG, "hsk_level_config: margin_m is not finite");
  float c = src->vp.cell[0];
  for (int a = 1; a < 3; ++a) c = src->vp.cell[a] > c ? src->vp.cell[a] : c;
  const float tau = config_tau(&src->cfg);
  const float margin = margin_m < 0.0f ? tau + 2.0f * c : margin_m;
  hsk_config out = src->cfg;
  int dims[3];
  double lo[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = (double)up->box_lo[a] - (double)margin;
    const double ext = ((double)up->box_hi[a] + (double)margin) - lo[a];
    if (!(ext >= 0.0) || !(ext / (double)c <= 4096.0)) return fail(src, HSK_ERR_ARG, "hsk_level_config: the box is not finite or needs more than 4096 voxels");
    int d = 8 * (int)std::ceil(ext / (double)c / 8.0);
    d = d < 8 ? 8 : d;
    float s;
    for (;; d += 8) {
      // the largest binary32 not above d c whose quotient by d does not exceed c: the destination's 2.1-cell clamp then never exceeds
      // the source's effective truncation distance
      s = (float)d * c;
      while (s / (float)d > c) s = nextafterf(s, 0.0f);
      if ((double)s >= ext) break;
    }
    if (d > 4096) return fail(src, HSK_ERR_ARG, "hsk_level_config: the box needs more than 4096 voxels");
    dims[a] = d;
    out.vol_size_m[a] = s;
  }
  out.vol_x = dims[0], out.vol_y = dims[1], out.vol_z = dims[2];
  out.trunc_dist_m = tau;
  out.own_z0 = 0, out.own_z1 = dims[2], out.halo = 0;
  float M[16];
  memcpy(M, up->level, sizeof(M));
  for (int a = 0; a < 3; ++a) M[4 * a + 3] = (float)(-lo[a]);
  M[12] = M[13] = M[14] = 0.0f, M[15] = 1.0f;
  float inv[16];
  if (hsk_invert_rigid(M, inv) != HSK_OK) return fail(src, HSK_ERR_ARG, "hsk_level_config: level is not rigid");
  float pose[16];
  if (int rc = hsk_get_pose(src, pose)) return rc;
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      double acc = 0.0;
      for (int j = 0; j < 4; ++j) acc += (double)M[4 * r + j] * (double)pose[4 * j + q];
      out.init_pose[4 * r + q] = (float)acc;
    }
  *cfg = out;
  memcpy(src_to_dst, M, sizeof(M));
  return HSK_OK;
}
