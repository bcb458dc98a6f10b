// api_align.hip -- the C ABI's registration calls (include/hskinfu.h "Volume alignment"; DESIGN.md 3.12 the kernel, 8f the
// rule): hsk_align_cloud, hsk_align_volume, and the host step they share with the numpy twin's comparison, hsk_align_step.
#pragma clang fp contract(off)
#include <cmath>
#include <new>
#include <vector>

#include "hsk_ctx.h"
#include "hsk_plane_point.h"

#define HSK_ALIGN_MAX_POINTS (1u << 20)
#define HSK_ALIGN_REACH_M 8.0  // half the box's diagonal, and (probes + 1) tau: what keeps the sums exact

static float align_default_shift(int probes, float tau) { return (2.0f * (float)(probes + 1)) * tau; }

extern "C" void hsk_default_align_params(const hsk_ctx* dst, hsk_align_params* p) {
  if (!p) return;
  p->max_iters = 30;
  p->probes = 3;
  p->cos_gate = 0.5f;
  p->max_points = 262144u;
  p->min_points = 256u;
  p->eps_rot = 1.0e-5f;
  p->eps_trans_m = 1.0e-5f;
  p->max_rot = 0.2f;
  p->max_shift_m = dst ? align_default_shift(p->probes, dst->vp.tau) : 0.0f;
}

// the parameters as they hold (every 0 replaced by its default, `probes` the count to either side), or false
static bool align_resolve(const hsk_ctx* dst, const hsk_align_params* in, hsk_align_params* p) {
  hsk_align_params d;
  hsk_default_align_params(dst, &d);
  if (!in) {
    *p = d;
    return true;
  }
  *p = *in;
  if (p->max_iters == 0) p->max_iters = d.max_iters;
  if (p->probes == 0)
    p->probes = d.probes;
  else if (p->probes == HSK_ALIGN_DIRECT)
    p->probes = 0;
  else if (p->probes < 0 || p->probes > 8)
    return false;
  if (p->cos_gate == 0.0f) p->cos_gate = d.cos_gate;
  if (p->max_points == 0u) p->max_points = d.max_points;
  if (p->min_points == 0u) p->min_points = d.min_points;
  if (p->eps_rot == 0.0f) p->eps_rot = d.eps_rot;
  if (p->eps_trans_m == 0.0f) p->eps_trans_m = d.eps_trans_m;
  if (p->max_rot == 0.0f) p->max_rot = d.max_rot;
  if (p->max_shift_m == 0.0f) p->max_shift_m = align_default_shift(p->probes, dst->vp.tau);
  return p->max_iters >= 1 && p->max_iters <= HSK_ALIGN_MAX_ITERS_CAP && p->cos_gate > 0.0f && p->cos_gate <= 1.0f &&
         p->max_points <= HSK_ALIGN_MAX_POINTS && p->eps_rot > 0.0f && p->eps_trans_m > 0.0f && p->max_rot > 0.0f &&
         p->max_shift_m > 0.0f && std::isfinite(p->eps_rot) && std::isfinite(p->eps_trans_m) && std::isfinite(p->max_rot) &&
         std::isfinite(p->max_shift_m);   // (a NaN fails its comparison)
}

extern "C" int hsk_align_step(const double sums27[27], const float m[16], const float centre[3], float m_next[16], float x6[6], int* ok) {
  if (!sums27 || !m || !centre || !m_next || !x6 || !ok) return HSK_ERR_ARG;
  float x[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  const bool good = host_solve6(sums27, x);
  float out[16];
  memcpy(out, m, sizeof(out));
  if (good) {
    float R[9], t[3];
    pose16_to_rt(m, R, t);
    for (int i = 0; i < 3; ++i) t[i] = t[i] - centre[i];
    host_pose_update(R, t, x);
    for (int i = 0; i < 3; ++i) t[i] = t[i] + centre[i];
    rt_to_pose16(R, t, out);
    for (int i = 12; i < 16; ++i) out[i] = m[i];
  }
  for (int i = 0; i < 6; ++i) x6[i] = good ? x[i] : 0.0f;
  memcpy(m_next, out, sizeof(out));  // (m_next may be m)
  *ok = good ? 1 : 0;
  return HSK_OK;
}

static double max_abs3(const float* v) { return std::fmax(std::fmax(std::fabs((double)v[0]), std::fabs((double)v[1])), std::fabs((double)v[2])); }

// the state and the arguments every call ask of its destination
int align_check(hsk_ctx* dst, const float src_to_dst[16], const hsk_align_params* params, hsk_align_params* p, const char* who) {
  const std::string w(who);
  float inv[16];
  if (hsk_invert_rigid(src_to_dst, inv) != HSK_OK)
    return fail(dst, HSK_ERR_ARG, (w + ": src_to_dst is not rigid (last row 0 0 0 1, |R^T R - I| <= 1e-4)").c_str());
  if (!align_resolve(dst, params, p)) return fail(dst, HSK_ERR_ARG, (w + ": a parameter is outside its range").c_str());
  const double sx = dst->vp.size[0], sy = dst->vp.size[1], sz = dst->vp.size[2];
  if (!(0.5 * std::sqrt((sx * sx + sy * sy) + sz * sz) <= HSK_ALIGN_REACH_M))
    return fail(dst, HSK_ERR_ARG, (w + ": half the diagonal of the destination's box exceeds 8 m (the sums' exactness)").c_str());
  if (!((double)(p->probes + 1) * (double)dst->vp.tau <= HSK_ALIGN_REACH_M))
    return fail(dst, HSK_ERR_ARG, (w + ": (probes + 1) truncation distances exceed 8 m (the sums' exactness)").c_str());
  if (int rs = require_whole_volume(dst, dst, who)) return rs;
  return require_idle(dst);
}

// hsk_ctx.h: CloudScratch
int align_scratch(hsk_ctx* k, size_t np, size_t extra, CloudScratch* s) {
  const size_t acc_bytes = (size_t)HSK_ALIGN_ACC_WORDS * 8;
  s->pitch = (unsigned)((np + 63) & ~(size_t)63);
  const size_t planes = (((size_t)s->pitch * 6 * 4) + 255) & ~(size_t)255;
  const size_t want = acc_bytes + planes + extra;
  if (!k->h_align) HIPCHK(k, hipHostMalloc((void**)&k->h_align, acc_bytes, hipHostMallocDefault));
  if (k->align_bytes < want) {
    if (k->d_align) HIPCHK(k, hipFree(k->d_align));
    k->d_align = nullptr;
    k->align_bytes = 0;
    HIPCHK(k, hipMalloc(&k->d_align, want));
    k->align_bytes = want;
  }
  s->soa = (float*)((char*)k->d_align + acc_bytes);
  s->extra = (char*)k->d_align + acc_bytes + planes;
  return HSK_OK;
}

int cloud_upload(hsk_ctx* k, const float* xyz, const float* normals, size_t n, size_t stride, const CloudScratch& s, size_t* n_invalid,
                 const char* who) {
  std::vector<float> soa;
  try {
    soa.resize((size_t)s.pitch * (normals ? 6 : 3));
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, (std::string(who) + ": out of host memory for the cloud").c_str());
  }
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* q = xyz + 3 * i * stride;
    for (int c = 0; c < 3; ++c) soa[(size_t)c * s.pitch + i] = q[c];
    if (!normals) continue;
    const float* m = normals + 3 * i * stride;
    for (int c = 0; c < 3; ++c) soa[(size_t)(3 + c) * s.pitch + i] = m[c];
    if (n_invalid) bad += plane_point_valid(q[0], q[1], q[2], m[0], m[1], m[2]) ? 0 : 1;
  }
  if (n_invalid) *n_invalid = bad;
  HIPCHK(k, hipMemcpyAsync(s.soa, soa.data(), soa.size() * 4, hipMemcpyHostToDevice, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));  // (the vector leaves with this scope)
  return HSK_OK;
}

int cloud_from_volume(hsk_ctx* k, size_t n, size_t extra, CloudScratch* s) {
  const float* d_xyz = nullptr;
  const float* d_nrm = nullptr;
  if (int rc = cloud_attrs_on_device(k, n, &d_xyz, &d_nrm)) return rc;
  if (int rc = align_scratch(k, n, extra, s)) return rc;
  // the cloud stays on the device: from the product buffer into the scratch's planes
  launch_plane_gather(k->stream, d_xyz, d_nrm, (unsigned)n, s->pitch, s->soa);
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

// The iterations over a cloud that lies in the scratch: from src_to_dst to m, st's iteration fields filled (n_points and stride
// are the caller's).  p: resolved parameters.
int align_run(hsk_ctx* k, const hsk_align_params& p, const float* d_soa, size_t np, unsigned pitch, const float src_to_dst[16], float m_out[16],
              hsk_align_stats* stp) {
  const size_t acc_bytes = (size_t)HSK_ALIGN_ACC_WORDS * 8;
  flush_weights(k);  // the rule reads weights
  HIPCHK(k, hipGetLastError());
  const float centre[3] = {k->vp.size[0] * 0.5f, k->vp.size[1] * 0.5f, k->vp.size[2] * 0.5f};
  float m[16];
  memcpy(m, src_to_dst, sizeof(m));
  hsk_align_stats& st = *stp;
  unsigned long long* d_acc = (unsigned long long*)k->d_align;
  double rot_sum = 0.0, shift_sum = 0.0;
  st.status = HSK_ALIGN_MAX_ITERS;
  for (int it = 0; it < p.max_iters; ++it) {
    AlignPose ap;
    pose16_to_rt(m, ap.R, ap.t);
    HIPCHK(k, hipMemsetAsync(d_acc, 0, acc_bytes, k->stream));
    launch_align_iter(k->stream, k->d_vol, k->vp, d_soa, (unsigned)np, pitch, ap, p.probes, p.cos_gate, d_acc);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(k->h_align, d_acc, acc_bytes, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    long long tot[29];
    for (int v = 0; v < 29; ++v) {
      tot[v] = 0;
      for (int s = 0; s < HSK_ALIGN_SHARDS; ++s) tot[v] += (long long)k->h_align[s * 32 + v];
    }
    for (int v = 0; v < 28; ++v) st.sums_last[v] = (double)tot[v] * (1.0 / 67108864.0);
    const uint32_t n_used = (uint32_t)tot[28];
    st.iterations = it + 1;
    st.n_used[it] = n_used;
    st.rms_m[it] = n_used ? (float)std::sqrt(st.sums_last[27] / (double)n_used) : 0.0f;
    if (n_used < p.min_points) {
      st.status = HSK_ALIGN_FEW;
      break;
    }
    float next[16], x6[6];
    int ok = 0;
    (void)hsk_align_step(st.sums_last, m, centre, next, x6, &ok);
    if (!ok) {
      st.status = HSK_ALIGN_DEGENERATE;
      break;
    }
    memcpy(m, next, sizeof(m));
    memcpy(st.x_last, x6, sizeof(x6));
    const double rot = max_abs3(x6), shift = max_abs3(x6 + 3);
    rot_sum += rot;
    shift_sum += shift;
    if (rot_sum > (double)p.max_rot || shift_sum > (double)p.max_shift_m) {
      st.status = HSK_ALIGN_DIVERGED;
      memcpy(m, src_to_dst, sizeof(m));
      break;
    }
    if (rot < (double)p.eps_rot && shift < (double)p.eps_trans_m) {
      st.status = HSK_ALIGN_CONVERGED;
      break;
    }
  }
  memcpy(m_out, m, sizeof(m));
  return HSK_OK;
}

extern "C" int hsk_align_cloud(hsk_ctx* dst, const float* xyz, const float* normals, size_t n, const float src_to_dst[16],
                               const hsk_align_params* params, float out[16], hsk_align_stats* stats) {
  if (!dst) return HSK_ERR_ARG;
  if (!src_to_dst || !out || (n > 0 && (!xyz || !normals))) return fail(dst, HSK_ERR_ARG, "hsk_align_cloud: null argument");
  hsk_align_params p;
  if (int rc = align_check(dst, src_to_dst, params, &p, "hsk_align_cloud")) return rc;
  hsk_ctx* k = dst;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  hsk_align_stats st;
  memset(&st, 0, sizeof(st));
  const size_t stride = n == 0 ? 1 : (n + p.max_points - 1) / p.max_points;
  const size_t np = n == 0 ? 0 : (n + stride - 1) / stride;  // the points 0, stride, 2 stride, ..
  if (stride > 0xffffffffull) return fail(k, HSK_ERR_ARG, "hsk_align_cloud: more points than a 32-bit stride over max_points covers");
  st.stride = (uint32_t)stride;
  st.n_points = (uint32_t)np;
  CloudScratch cs;
  if (int rc = align_scratch(k, np, 0, &cs)) return rc;
  if (np > 0)
    if (int rc = cloud_upload(k, xyz, normals, np, stride, cs, nullptr, "hsk_align_cloud")) return rc;
  float m[16];
  if (int rc = align_run(k, p, cs.soa, np, cs.pitch, src_to_dst, m, &st)) return rc;
  memcpy(out, m, sizeof(m));
  if (stats) *stats = st;
  return HSK_OK;
}

extern "C" int hsk_align_volume(hsk_ctx* dst, hsk_ctx* src, const float src_to_dst[16], const hsk_align_params* params, float out[16],
                                hsk_align_stats* stats) {
  if (!dst) return HSK_ERR_ARG;
  if (!src || !src_to_dst || !out) return fail(dst, HSK_ERR_ARG, "hsk_align_volume: null argument");
  if (src == dst) return fail(dst, HSK_ERR_ARG, "hsk_align_volume: source and destination are the same context");
  hsk_align_params p;
  if (int rc0 = align_check(dst, src_to_dst, params, &p, "hsk_align_volume")) return rc0;
  if (int rs = require_whole_volume(src, dst, "hsk_align_volume")) return rs;
  if (int ri = require_idle(src, dst)) return ri;
  // the source's cloud with normals, through host memory: the iterations are the hot path, not the hand-over
  size_t total = 0;
  int rc = hsk_extract_cloud_attrs(src, nullptr, nullptr, nullptr, 0, &total, nullptr);
  if (rc != HSK_OK) return fail(dst, rc, src->err.c_str());
  std::vector<float> xyz, nrm;
  try {
    xyz.resize(total * 3);
    nrm.resize(total * 3);
  } catch (const std::bad_alloc&) {
    return fail(dst, HSK_ERR_STATE, "hsk_align_volume: out of host memory for the cloud");
  }
  if (total > 0) {
    size_t again = 0;
    rc = hsk_extract_cloud_attrs(src, xyz.data(), nrm.data(), nullptr, total, &again, nullptr);
    if (rc != HSK_OK) return fail(dst, rc, src->err.c_str());
    if (again != total) return fail(dst, HSK_ERR_STATE, "hsk_align_volume: the source's cloud changed between the two calls");
  }
  return hsk_align_cloud(dst, xyz.data(), nrm.data(), total, src_to_dst, params, out, stats);
}
