// api_cover.hip -- the C ABI's scan coverage (include/hskinfu.h "Scan coverage"; DESIGN.md 3.15 the kernels, 8i the rule):
// hsk_default_probe, hsk_coverage_census, hsk_score_views, hsk_render_coverage and the host-only hsk_rank_views.  The device calls
// are scheduled like hsk_render_view (api_readout.hip): one chain on the context's stream behind whatever it holds, the inputs
// through the first pinned staging buffer, everything they write in the product buffer, the results out through the pinned pair.
// No flush of the deferred weights (as for the products, api_readout.hip product_counts): the rule asks of a weight only whether
// it is zero, and of the TSDF its sign -- no deferred weight is zero in the volume's own copy, and the TSDF values are current.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>

#include "hsk_ctx.h"
#include "hsk_cover_point.h"

extern "C" void hsk_default_probe(const hsk_ctx* k, hsk_probe* p) {
  if (!p) return;
  hsk_config c;
  if (k)
    c = k->cfg;
  else
    hsk_default_config(&c, 256);
  const float tau = k ? k->vp.tau : config_tau(&c);
  memset(p, 0, sizeof(*p));
  p->width = c.width >> 2;
  p->height = c.height >> 2;
  p->fx = c.fx / 4.0f;
  p->fy = c.fy / 4.0f;
  p->cx = c.cx / 4.0f;
  p->cy = c.cy / 4.0f;
  p->near_m = 0.4f;
  p->far_m = 3.5f;
  p->step_m = 0.5f * tau;
}

// the probe a call works with (NULL: the default), checked -> the kernel's block
static int check_probe(hsk_ctx* k, const hsk_probe* probe, const char* who, CoverProbe* cp) {
  hsk_probe p;
  if (probe)
    p = *probe;
  else
    hsk_default_probe(k, &p);
  auto bad = [&](const char* what) { return fail(k, HSK_ERR_ARG, (std::string(who) + what).c_str()); };
  if (p.width < 1 || p.width > 4096 || p.height < 1 || p.height > 4096) return bad(": width and height must lie in 1..4096");
  if (!(std::isfinite(p.fx) && std::isfinite(p.fy) && p.fx > 0.0f && p.fy > 0.0f)) return bad(": fx and fy must be finite and positive");
  if (!(std::isfinite(p.cx) && std::isfinite(p.cy))) return bad(": cx and cy must be finite");
  if (!(std::isfinite(p.step_m) && p.step_m > 0.0f)) return bad(": step_m must be finite and positive");
  if (!(std::isfinite(p.near_m) && p.near_m >= 0.0f)) return bad(": near_m must be finite and not negative");
  if (!(std::isfinite(p.far_m) && p.far_m >= p.near_m)) return bad(": far_m must be finite and not below near_m");
  cp->W = p.width;
  cp->H = p.height;
  cp->n = cover_sample_count(p.near_m, p.far_m, p.step_m);
  cp->fx = p.fx;
  cp->fy = p.fy;
  cp->cx = p.cx;
  cp->cy = p.cy;
  cp->near_m = p.near_m;
  cp->step_m = p.step_m;
  return HSK_OK;
}

// The rays of `cp` under n > 0 checked poses: the scores to `scores` (may be NULL), and for one pose the pixels' values to the
// arrays that are not NULL.  Product buffer: the poses (12 floats each), the scores, the three images.
static int cover_run(hsk_ctx* k, const CoverProbe& cp, const float* poses, size_t n, hsk_view_score* scores, uint8_t* cls, uint16_t* depth_mm,
                     uint16_t* gain) {
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  int r = ensure_pinned(k);
  if (r != HSK_OK) return r;
  const size_t P = (size_t)cp.W * cp.H;
  ProductArrays pa;  // (the poses and the scores are the kernel's own: they lie there whether or not the scores are handed out)
  const int a_poses = pa.add(nullptr, n * 48, true), a_scores = pa.add(scores, n * sizeof(hsk_view_score), true);
  const int a_cls = pa.add(cls, P), a_dep = pa.add(depth_mm, P * 2), a_gain = pa.add(gain, P * 2);
  r = pa.place(k);
  if (r != HSK_OK) return r;
  float* h12 = (float*)k->h_pin[0];  // (free: every call that uses the pair waits for its own result before it returns; 65536 poses are 3 MiB)
  for (size_t j = 0; j < n; ++j) pose16_to_rt(poses + 16 * j, h12 + 12 * j, h12 + 12 * j + 9);
  HIPCHK(k, hipMemcpyAsync(pa.dev<float>(a_poses), h12, n * 48, hipMemcpyHostToDevice, k->stream));
  HIPCHK(k, hipMemsetAsync(pa.dev<hsk_view_score>(a_scores), 0, n * sizeof(hsk_view_score), k->stream));
  launch_cover_rays(k->stream, k->d_vol, k->vp, cp, pa.dev<float>(a_poses), (unsigned)n, pa.dev<hsk_view_score>(a_scores), pa.dev<unsigned char>(a_cls),
                    pa.dev<unsigned short>(a_dep), pa.dev<unsigned short>(a_gain));
  HIPCHK(k, hipGetLastError());
  // (copy_out's first piece goes through the first pinned buffer: behind the poses' copy in the stream's order)
  r = pa.copy_out(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));  // (a call without an output still ends with its work done)
  return HSK_OK;
}

extern "C" int hsk_score_views(hsk_ctx* k, const hsk_probe* probe, const float* poses, size_t n_poses, hsk_view_score* out) {
  static_assert(sizeof(hsk_view_score) == 32, "hsk_view_score is 32 bytes");
  if (!k) return HSK_ERR_ARG;
  if (n_poses > 0 && (!poses || !out)) return fail(k, HSK_ERR_ARG, "hsk_score_views: null argument");
  if (n_poses > HSK_COVER_MAX_POSES) return fail(k, HSK_ERR_ARG, "hsk_score_views: more than 65536 poses");
  CoverProbe cp;
  if (int rc = check_probe(k, probe, "hsk_score_views", &cp)) return rc;
  if (int rc = check_poses(k, poses, n_poses, "hsk_score_views")) return rc;
  if (int rs = require_whole_volume(k, k, "hsk_score_views", "views of a group are not composited")) return rs;
  if (n_poses == 0) return HSK_OK;
  return cover_run(k, cp, poses, n_poses, out, nullptr, nullptr, nullptr);
}

extern "C" int hsk_render_coverage(hsk_ctx* k, const hsk_probe* probe, const float pose[16], uint8_t* cls, uint16_t* depth_mm, uint16_t* gain,
                                   hsk_view_score* score) {
  if (!k) return HSK_ERR_ARG;
  if (!pose) return fail(k, HSK_ERR_ARG, "hsk_render_coverage: pose is null");
  CoverProbe cp;
  if (int rc = check_probe(k, probe, "hsk_render_coverage", &cp)) return rc;
  if (int rc = check_poses(k, pose, 1, "hsk_render_coverage")) return rc;
  if (int rs = require_whole_volume(k, k, "hsk_render_coverage", "views of a group are not composited")) return rs;
  return cover_run(k, cp, pose, 1, score, cls, depth_mm, gain);
}

extern "C" int hsk_coverage_census(hsk_ctx* k, const hsk_voxel_box* box, hsk_coverage* out) {
  static_assert(sizeof(hsk_coverage) == 80, "hsk_coverage is ten 64-bit words");
  if (!k) return HSK_ERR_ARG;
  if (!out) return fail(k, HSK_ERR_ARG, "hsk_coverage_census: out is null");
  hsk_voxel_box b;
  size_t n;
  if (int rc = clear_box_check(k, box, "hsk_coverage_census", &b, &n)) return rc;
  if (int rs = require_whole_volume(k, k, "hsk_coverage_census", "the census of a group is not summed")) return rs;
  if (n == 0) {
    memset(out, 0, sizeof(*out));
    return HSK_OK;
  }
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const CoverSweep g = cover_sweep(k->vp, b.lo, b.hi);
  ProductLayout lay;
  const size_t out_at = lay.take(sizeof(hsk_coverage)), partial_at = lay.take((size_t)cover_census_blocks(g) * 10 * 8);
  int r = ensure_product_bytes(k, lay.bytes);
  if (r != HSK_OK) return r;
  char* base = (char*)k->d_out;
  launch_cover_census(k->stream, k->d_vol, g, (unsigned long long*)(base + partial_at), (unsigned long long*)(base + out_at));
  HIPCHK(k, hipGetLastError());
  hsk_coverage got;
  r = copy_out(k, &got, base + out_at, sizeof(got));
  if (r != HSK_OK) return r;
  *out = got;
  return HSK_OK;
}

extern "C" int hsk_rank_views(const hsk_view_score* s, size_t n, uint32_t* order) {
  if (n > 0 && (!s || !order)) return HSK_ERR_ARG;
  if (n > 0xffffffffull) return HSK_ERR_ARG;
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {  // (stable: equal scores stay in index order)
    const bool sa = s[a].eye_state != HSK_EYE_FREE, sb = s[b].eye_state != HSK_EYE_FREE;
    if (sa != sb) return sb;
    if (s[a].gain != s[b].gain) return s[a].gain > s[b].gain;
    return s[a].n_frontier > s[b].n_frontier;
  });
  return HSK_OK;
}
