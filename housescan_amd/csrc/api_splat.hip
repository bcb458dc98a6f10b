// api_splat.hip -- the C ABI's cloud import (include/hskinfu.h "Cloud import"; DESIGN.md 3.27 the kernels, 8u the rule):
// hsk_default_splat_params, hsk_splat_cloud (one view of a cloud as a depth image) and hsk_import_cloud (the views fused, frame
// by frame, without leaving the device).
#pragma clang fp contract(off)
#include <cmath>
#include <new>
#include <vector>

#include "hsk_ctx.h"
#include "hsk_splat_point.h"

static_assert(HSK_SPLAT_DISC == SPLAT_DISC && HSK_SPLAT_SURFEL == SPLAT_SURFEL, "the rule's modes are the ABI's");
static_assert(SPLAT_CLASSES + 1 <= SPLAT_COUNT_WORDS, "a view's counters: the classes, then the pixels");

extern "C" void hsk_default_splat_params(const hsk_ctx* k, hsk_splat_params* p) {
  if (!p) return;
  float cell = 3.0f / 512.0f;
  if (k) cell = std::fmax(std::fmax(k->vp.cell[0], k->vp.cell[1]), k->vp.cell[2]);
  p->mode = HSK_SPLAT_DISC;
  p->point_size_m = cell;
  p->cover = 1.5f;
  p->min_half_px = 0.5f;
  p->max_half_px = 8.0f;
  p->near_m = 0.1f;
  p->far_m = 8.0f;
}

// the parameters as they hold (every 0 replaced by its default), or false (a NaN fails its comparison)
static bool splat_resolve(const hsk_ctx* k, const hsk_splat_params* in, hsk_splat_params* p) {
  hsk_splat_params d;
  hsk_default_splat_params(k, &d);
  if (!in) {
    *p = d;
    return true;
  }
  *p = *in;
  if (p->point_size_m == 0.0f) p->point_size_m = d.point_size_m;
  if (p->cover == 0.0f) p->cover = d.cover;
  if (p->min_half_px == 0.0f) p->min_half_px = d.min_half_px;
  if (p->max_half_px == 0.0f) p->max_half_px = d.max_half_px;
  if (p->near_m == 0.0f) p->near_m = d.near_m;
  if (p->far_m == 0.0f) p->far_m = d.far_m;
  return (p->mode == HSK_SPLAT_DISC || p->mode == HSK_SPLAT_SURFEL) && p->point_size_m > 0.0f && std::isfinite(p->point_size_m) &&
         p->cover >= 1.0f && std::isfinite(p->cover) && p->min_half_px >= 0.5f && p->max_half_px >= p->min_half_px &&
         p->max_half_px <= SPLAT_MAX_HALF_PX && p->near_m > 0.0f && p->far_m >= p->near_m && p->far_m <= 65.535f;
}

// the arguments and the state both calls ask for; p: the resolved parameters
static int splat_check(hsk_ctx* k, const char* who, const float* xyz, const float* normals, size_t n, const hsk_splat_params* params,
                       hsk_splat_params* p) {
  const std::string w(who);
  if (n > 0 && !xyz) return fail(k, HSK_ERR_ARG, (w + ": null argument").c_str());
  if (n > HSK_SPLAT_MAX_POINTS) return fail(k, HSK_ERR_ARG, (w + ": more than 2^24 points").c_str());
  if (!splat_resolve(k, params, p)) return fail(k, HSK_ERR_ARG, (w + ": a parameter is outside its range").c_str());
  if (p->mode == HSK_SPLAT_SURFEL && n > 0 && !normals) return fail(k, HSK_ERR_ARG, (w + ": HSK_SPLAT_SURFEL needs normals").c_str());
  return require_whole_volume(k, k, who);
}

// what the calls carve behind the cloud's planes: the z-buffer, one frame (hsk_splat_cloud's; the import writes the image buffers'
// own), the views' counters
struct SplatScratch {
  size_t zbuf_at, frame_at, counts_at, bytes;
  SplatScratch(size_t pixels, size_t n_views) {
    ProductLayout lay;
    zbuf_at = lay.take(pixels * 4);
    frame_at = lay.take(pixels * 2);
    counts_at = lay.take(n_views * SPLAT_COUNT_WORDS * 4);
    bytes = lay.bytes;
  }
};

static SplatCam splat_cam(const hsk_ctx* k) {
  const ImgLevel& lv = k->lv[0];
  return SplatCam{lv.W, lv.H, lv.in.fx, lv.in.fy, lv.in.cx, lv.in.cy};
}
static SplatArgs splat_args(const hsk_splat_params& p) {
  return SplatArgs{p.mode, (0.5f * p.point_size_m) * p.cover, p.min_half_px, p.max_half_px, p.near_m, p.far_m};
}
static hsk_splat_stats splat_stats_of(const unsigned* c) {
  return hsk_splat_stats{c[SPLAT_INVALID], c[SPLAT_CLIPPED], c[SPLAT_BACKFACING], c[SPLAT_OUTSIDE], c[SPLAT_DONE], c[SPLAT_CLASSES]};
}

// the scratch of a cloud of n points seen from n_views views, the cloud in its planes, the z-buffer armed and the counters zeroed
static int splat_begin(hsk_ctx* k, const char* who, const float* xyz, const float* normals, size_t n, const hsk_splat_params& p, size_t n_views,
                       CloudScratch* cs, SplatScratch* L) {
  const size_t pixels = (size_t)k->lv[0].W * (size_t)k->lv[0].H;
  *L = SplatScratch(pixels, n_views);
  if (int rc = align_scratch(k, n, L->bytes, cs)) return rc;
  if (n > 0)
    if (int rc = cloud_upload(k, xyz, p.mode == HSK_SPLAT_SURFEL ? normals : nullptr, n, 1, *cs, nullptr, who)) return rc;
  HIPCHK(k, hipMemsetAsync((char*)cs->extra + L->zbuf_at, 0xff, pixels * 4, k->stream));
  HIPCHK(k, hipMemsetAsync((char*)cs->extra + L->counts_at, 0, n_views * SPLAT_COUNT_WORDS * 4, k->stream));
  return HSK_OK;
}

extern "C" int hsk_splat_cloud(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const float pose[16], const hsk_splat_params* params,
                               uint16_t* depth_out, hsk_splat_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  if (!pose || !depth_out) return fail(k, HSK_ERR_ARG, "hsk_splat_cloud: null argument");
  hsk_splat_params p;
  if (int rc = splat_check(k, "hsk_splat_cloud", xyz, normals, n, params, &p)) return rc;
  if (int rc = check_poses(k, pose, 1, "hsk_splat_cloud")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  CloudScratch cs;
  SplatScratch L(0, 0);
  if (int rc = splat_begin(k, "hsk_splat_cloud", xyz, normals, n, p, 1, &cs, &L)) return rc;
  const SplatCam cam = splat_cam(k);
  const unsigned pixels = (unsigned)cam.w * (unsigned)cam.h;
  unsigned* zbuf = (unsigned*)((char*)cs.extra + L.zbuf_at);
  unsigned short* frame = (unsigned short*)((char*)cs.extra + L.frame_at);
  unsigned* counts = (unsigned*)((char*)cs.extra + L.counts_at);
  SplatPose sp;
  pose16_to_rt(pose, sp.R, sp.t);
  launch_splat_points(k->stream, cs.soa, (unsigned)n, cs.pitch, p.mode == HSK_SPLAT_SURFEL, cam, sp, splat_args(p), zbuf, counts);
  launch_splat_resolve(k->stream, zbuf, pixels, frame, counts);
  HIPCHK(k, hipGetLastError());
  unsigned c[SPLAT_COUNT_WORDS];
  HIPCHK(k, hipMemcpyAsync(c, counts, sizeof(c), hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  if (int rc = copy_out(k, depth_out, frame, (size_t)pixels * 2)) return rc;
  if (stats) *stats = splat_stats_of(c);
  return HSK_OK;
}

extern "C" int hsk_import_cloud(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const float* poses, size_t n_poses,
                                const hsk_splat_params* params, hsk_splat_stats* per_view) {
  if (!k) return HSK_ERR_ARG;
  if (n_poses > 0 && !poses) return fail(k, HSK_ERR_ARG, "hsk_import_cloud: null argument");
  if (n_poses > HSK_SPLAT_MAX_POSES) return fail(k, HSK_ERR_ARG, "hsk_import_cloud: more than 65536 poses");
  hsk_splat_params p;
  if (int rc = splat_check(k, "hsk_import_cloud", xyz, normals, n, params, &p)) return rc;
  if (int rc = check_poses(k, poses, n_poses, "hsk_import_cloud")) return rc;
  if (int ri = require_idle(k)) return ri;
  if (n_poses == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  std::vector<unsigned> c;
  try {
    c.resize(n_poses * SPLAT_COUNT_WORDS);
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, "hsk_import_cloud: out of host memory for the views' counters");
  }
  CloudScratch cs;
  SplatScratch L(0, 0);
  if (int rc = splat_begin(k, "hsk_import_cloud", xyz, normals, n, p, n_poses, &cs, &L)) return rc;
  const SplatCam cam = splat_cam(k);
  const SplatArgs args = splat_args(p);
  const unsigned pixels = (unsigned)cam.w * (unsigned)cam.h;
  unsigned* zbuf = (unsigned*)((char*)cs.extra + L.zbuf_at);
  unsigned* counts = (unsigned*)((char*)cs.extra + L.counts_at);
  for (size_t j = 0; j < n_poses; ++j) {
    // hsk_integrate of view j's image, every step on the stream: the pose into the device state, the frame where the upload
    // would have put it, the scaled depth, the integrate
    SplatPose sp;
    pose16_to_rt(poses + 16 * j, sp.R, sp.t);
    launch_splat_pose(k->stream, k->d_st, sp);
    launch_splat_points(k->stream, cs.soa, (unsigned)n, cs.pitch, p.mode == HSK_SPLAT_SURFEL, cam, sp, args, zbuf, counts + j * SPLAT_COUNT_WORDS);
    launch_splat_resolve(k->stream, zbuf, pixels, k->B().d_raw, counts + j * SPLAT_COUNT_WORDS);
    enqueue_integrate_staged(k);
    HIPCHK(k, hipGetLastError());
  }
  HIPCHK(k, hipMemcpyAsync(c.data(), counts, c.size() * 4, hipMemcpyDeviceToHost, k->stream));
  if (int rc = download_state(k)) return rc;  // (the host's copy of the state follows the device's, as hsk_integrate leaves it; the one wait)
  HIPCHK(k, hipGetLastError());
  if (per_view)
    for (size_t j = 0; j < n_poses; ++j) per_view[j] = splat_stats_of(c.data() + j * SPLAT_COUNT_WORDS);
  return HSK_OK;
}
