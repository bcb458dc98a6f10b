// api_reloc.hip -- the C ABI's pose search (include/hskinfu.h "Loss hold and relocalisation"; DESIGN.md 3.13 the kernel, 8g the
// rule): hsk_score_cloud, hsk_relocalize, and the host-only hsk_rank_scores and hsk_pose_lattice.  The loss policy itself is
// hskinfu_api.hip's (after_loss): it belongs to the frame paths.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "hsk_ctx.h"

#define HSK_RELOC_MAX_POINTS ((size_t)1 << 20)
#define HSK_RELOC_MAX_POSES ((size_t)65536)

// what scoring adds to the alignment's scratch behind the cloud's planes: the poses (12 floats each), the slabs' partial
// values, the scores
struct RelocScratch {
  size_t poses_at, partial_at, scores_at, bytes;
  RelocScratch(size_t n, size_t n_poses) {
    ProductLayout L;
    poses_at = L.take(n_poses * 12 * 4);
    partial_at = L.take(n_poses * reloc_slabs((unsigned)n, (unsigned)n_poses) * 8 * 8);
    scores_at = L.take(n_poses * sizeof(hsk_pose_score));
    bytes = L.bytes;
  }
};

int check_poses(hsk_ctx* k, const float* poses, size_t n_poses, const char* who) {
  for (size_t j = 0; j < n_poses; ++j) {
    float inv[16];
    if (hsk_invert_rigid(poses + 16 * j, inv) != HSK_OK)
      return fail(k, HSK_ERR_ARG, (std::string(who) + ": pose " + std::to_string(j) + " is not rigid (last row 0 0 0 1, |R^T R - I| <= 1e-4)").c_str());
  }
  return HSK_OK;
}

// the n points in the scratch's planes under the poses -> out (host).  n > 0, n_poses > 0.
static int score_planes(hsk_ctx* k, const CloudScratch& cs, size_t n, const float* poses, size_t n_poses, hsk_pose_score* out) {
  const RelocScratch L(n, n_poses);
  float* d_poses = (float*)((char*)cs.extra + L.poses_at);
  unsigned long long* d_partial = (unsigned long long*)((char*)cs.extra + L.partial_at);
  hsk_pose_score* d_scores = (hsk_pose_score*)((char*)cs.extra + L.scores_at);
  std::vector<float> p12;
  try {
    p12.resize(n_poses * 12);
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, "pose scoring: out of host memory for the poses");
  }
  for (size_t j = 0; j < n_poses; ++j) pose16_to_rt(poses + 16 * j, &p12[12 * j], &p12[12 * j + 9]);
  HIPCHK(k, hipMemcpyAsync(d_poses, p12.data(), p12.size() * 4, hipMemcpyHostToDevice, k->stream));
  flush_weights(k);  // the rule reads weights
  launch_reloc_score(k->stream, k->d_vol, k->vp, cs.soa, (unsigned)n, cs.pitch, d_poses, (unsigned)n_poses, d_partial, d_scores);
  HIPCHK(k, hipGetLastError());
  HIPCHK(k, hipMemcpyAsync(out, d_scores, n_poses * sizeof(hsk_pose_score), hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));  // (the vector leaves with this scope)
  return HSK_OK;
}

extern "C" int hsk_score_cloud(hsk_ctx* dst, const float* xyz, size_t n, const float* poses, size_t n_poses, hsk_pose_score* out) {
  static_assert(sizeof(hsk_pose_score) == 32, "hsk_pose_score is 32 bytes");
  if (!dst) return HSK_ERR_ARG;
  if ((n > 0 && !xyz) || (n_poses > 0 && (!poses || !out))) return fail(dst, HSK_ERR_ARG, "hsk_score_cloud: null argument");
  if (n > HSK_RELOC_MAX_POINTS) return fail(dst, HSK_ERR_ARG, "hsk_score_cloud: more than 2^20 points");
  if (n_poses > HSK_RELOC_MAX_POSES) return fail(dst, HSK_ERR_ARG, "hsk_score_cloud: more than 65536 poses");
  if (int rc = check_poses(dst, poses, n_poses, "hsk_score_cloud")) return rc;
  if (int rs = require_whole_volume(dst, dst, "hsk_score_cloud")) return rs;
  if (int ri = require_idle(dst)) return ri;
  hsk_ctx* k = dst;
  if (n_poses == 0) return HSK_OK;
  if (n == 0) {
    memset(out, 0, n_poses * sizeof(hsk_pose_score));
    return HSK_OK;
  }
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  CloudScratch cs;
  if (int rc = align_scratch(k, n, RelocScratch(n, n_poses).bytes, &cs)) return rc;
  if (int rc = cloud_upload(k, xyz, nullptr, n, 1, cs, nullptr, "hsk_score_cloud")) return rc;
  return score_planes(k, cs, n, poses, n_poses, out);
}

extern "C" int hsk_rank_scores(const hsk_pose_score* s, size_t n, uint32_t* order) {
  if (n > 0 && (!s || !order)) return HSK_ERR_ARG;
  if (n > 0xffffffffull) return HSK_ERR_ARG;
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  auto key = [&](uint32_t i) { return ((long long)s[i].n_near - (long long)s[i].n_free) - (long long)s[i].n_behind; };
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {  // (stable: equal scores stay in index order)
    const long long ka = key(a), kb = key(b);
    return ka != kb ? ka > kb : s[a].sum_abs < s[b].sum_abs;
  });
  return HSK_OK;
}

extern "C" int hsk_pose_lattice(const float centre[16], float step_m, int n_trans, float step_rad, int n_rot, float* poses, size_t cap,
                                size_t* n) {
  if (!centre || !n || n_trans < 0 || n_rot < 0 || !std::isfinite(step_m) || !std::isfinite(step_rad)) return HSK_ERR_ARG;
  if (n_trans > 20 || n_rot > 128) return HSK_ERR_ARG;  // (more than 65536 poses either way, and the count below cannot overflow)
  const size_t nt = (size_t)(2 * n_trans + 1), nr = (size_t)(2 * n_rot + 1), total = nt * nt * nt * nr * nr;
  if (total > HSK_RELOC_MAX_POSES) return HSK_ERR_ARG;
  *n = total;
  if (!poses) return HSK_OK;
  if (cap < total) return HSK_ERR_ARG;
  double C[12];
  for (int i = 0; i < 12; ++i) C[i] = (double)centre[i];
  float* o = poses;
  for (int i = -n_trans; i <= n_trans; ++i)
    for (int j = -n_trans; j <= n_trans; ++j)
      for (int k = -n_trans; k <= n_trans; ++k)
        for (int a = -n_rot; a <= n_rot; ++a)
          for (int b = -n_rot; b <= n_rot; ++b, o += 16) {
            if (i == 0 && j == 0 && k == 0 && a == 0 && b == 0) {
              memcpy(o, centre, 16 * sizeof(float));
              continue;
            }
            const double tx = (double)i * (double)step_m, ty = (double)j * (double)step_m, tz = (double)k * (double)step_m;
            const double ya = (double)a * (double)step_rad, xb = (double)b * (double)step_rad;
            const double cy = std::cos(ya), sy = std::sin(ya), cx = std::cos(xb), sx = std::sin(xb);
            // Ry(ya) Rx(xb)
            const double Q[9] = {cy, sy * sx, sy * cx, 0.0, cx, -sx, -sy, cy * sx, cy * cx};
            for (int r = 0; r < 3; ++r) {
              const double* c = C + 4 * r;
              for (int q = 0; q < 3; ++q) o[4 * r + q] = (float)((c[0] * Q[q] + c[1] * Q[3 + q]) + c[2] * Q[6 + q]);
              o[4 * r + 3] = (float)(((c[0] * tx + c[1] * ty) + c[2] * tz) + c[3]);
            }
            o[12] = o[13] = o[14] = 0.0f;
            o[15] = 1.0f;
          }
  return HSK_OK;
}

extern "C" void hsk_default_reloc_params(const hsk_ctx* k, hsk_reloc_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->level = 2;
  p->n_refine = 4;
  p->accept_fraction = 0.5f;
  p->accept_rms_m = k ? k->vp.tau / 4.0f : 0.0f;
  hsk_default_align_params(k, &p->align);
}

extern "C" int hsk_relocalize(hsk_ctx* k, const uint16_t* depth, int w, int h, const float* poses, size_t n_poses,
                              const hsk_reloc_params* params, float pose_out[16], hsk_reloc_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  if (!depth || !pose_out || (n_poses > 0 && !poses)) return fail(k, HSK_ERR_ARG, "hsk_relocalize: null argument");
  if (w != k->cfg.width || h != k->cfg.height) return fail(k, HSK_ERR_ARG, "hsk_relocalize: depth frame size does not match the context");
  hsk_reloc_params rp;
  hsk_default_reloc_params(k, &rp);
  if (params) {
    if (params->level != 0) rp.level = params->level;
    if (params->n_refine != 0) rp.n_refine = params->n_refine;
    if (params->accept_fraction != 0.0f) rp.accept_fraction = params->accept_fraction;
    if (params->accept_rms_m != 0.0f) rp.accept_rms_m = params->accept_rms_m;
  }
  if (rp.level == HSK_RELOC_FINEST) rp.level = 0;
  else if (rp.level < 1 || rp.level >= HSK_NLEVELS) return fail(k, HSK_ERR_ARG, "hsk_relocalize: level must be 1, 2 or HSK_RELOC_FINEST");
  if (rp.n_refine < 1 || rp.n_refine > HSK_RELOC_MAX_REFINE) return fail(k, HSK_ERR_ARG, "hsk_relocalize: n_refine must lie in 1..16");
  if (!(rp.accept_fraction > 0.0f && rp.accept_fraction <= 1.0f)) return fail(k, HSK_ERR_ARG, "hsk_relocalize: accept_fraction must lie in (0, 1]");
  if (!(rp.accept_rms_m > 0.0f) || !std::isfinite(rp.accept_rms_m)) return fail(k, HSK_ERR_ARG, "hsk_relocalize: accept_rms_m must be positive and finite");
  if (n_poses > HSK_RELOC_MAX_POSES) return fail(k, HSK_ERR_ARG, "hsk_relocalize: more than 65536 poses");
  if (int rc = check_poses(k, poses, n_poses, "hsk_relocalize")) return rc;
  const int l = rp.level;
  const size_t n = (size_t)k->lv[l].W * k->lv[l].H;
  if (n > HSK_RELOC_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_relocalize: more than 2^20 pixels at this level");
  const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  hsk_align_params ap;
  if (int rc = align_check(k, eye, params ? &params->align : nullptr, &ap, "hsk_relocalize")) return rc;  // (and the state)
  if (int rc = preprocess_frame(k, depth, w, h)) return rc;
  hsk_reloc_stats st;
  memset(&st, 0, sizeof(st));
  st.status = HSK_RELOC_EMPTY;
  st.best = -1;
  st.n_candidates = (uint32_t)n_poses;
  for (int r = 0; r < HSK_RELOC_MAX_REFINE; ++r) st.candidate[r] = -1;
  memcpy(pose_out, eye, sizeof(eye));
  if (n_poses == 0 || n == 0) {
    if (stats) *stats = st;
    return HSK_OK;
  }
  CloudScratch cs;
  if (int rc = align_scratch(k, n, RelocScratch(n, n_poses).bytes, &cs)) return rc;
  // the cloud stays on the device: every pixel for the scores ...
  launch_reloc_gather(k->stream, k->B().d_vcur[l], k->B().d_ncur[l], (unsigned)n, 1u, (unsigned)n, cs.pitch, cs.soa);
  std::vector<hsk_pose_score> sc;
  std::vector<uint32_t> order;
  try {
    sc.resize(n_poses);
    order.resize(n_poses);
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, "hsk_relocalize: out of host memory for the scores");
  }
  if (int rc = score_planes(k, cs, n, poses, n_poses, sc.data())) return rc;
  st.n_valid = (uint32_t)n - sc[0].n_skipped;
  if (st.n_valid == 0) {
    if (stats) *stats = st;
    return HSK_OK;
  }
  (void)hsk_rank_scores(sc.data(), n_poses, order.data());
  // ... and, as hsk_align_cloud takes a cloud, every stride-th of them for the refinements
  const size_t stride = (n + ap.max_points - 1) / ap.max_points, np = (n + stride - 1) / stride;
  if (stride > 1) launch_reloc_gather(k->stream, k->B().d_vcur[l], k->B().d_ncur[l], (unsigned)n, (unsigned)stride, (unsigned)np, cs.pitch, cs.soa);
  st.n_refined = (int32_t)std::min<size_t>((size_t)rp.n_refine, n_poses);
  st.status = HSK_RELOC_NONE;
  st.best = (int32_t)order[0];
  memcpy(pose_out, poses + 16 * (size_t)order[0], sizeof(eye));
  int win = -1;
  const double need = (double)rp.accept_fraction * (double)st.n_valid;
  for (int r = 0; r < st.n_refined; ++r) {
    const float* cand = poses + 16 * (size_t)order[r];
    hsk_align_stats as;
    memset(&as, 0, sizeof(as));
    float m[16];
    if (int rc = align_run(k, ap, cs.soa, np, cs.pitch, cand, m, &as)) return rc;
    const int last = as.iterations - 1;
    st.candidate[r] = (int32_t)order[r];
    st.score[r] = sc[order[r]];
    st.align_status[r] = as.status;
    st.iterations[r] = as.iterations;
    st.n_used[r] = last >= 0 ? as.n_used[last] : 0u;
    st.rms_m[r] = last >= 0 ? as.rms_m[last] : 0.0f;
    const bool accepted = as.status == HSK_ALIGN_CONVERGED && (double)st.n_used[r] >= need && st.rms_m[r] <= rp.accept_rms_m;
    if (accepted && (win < 0 || st.n_used[r] > st.n_used[win] || (st.n_used[r] == st.n_used[win] && st.rms_m[r] < st.rms_m[win]))) {
      win = r;
      memcpy(pose_out, m, sizeof(m));
    }
  }
  if (win >= 0) {
    st.status = HSK_RELOC_FOUND;
    st.best = st.candidate[win];
  }
  if (stats) *stats = st;
  return HSK_OK;
}
