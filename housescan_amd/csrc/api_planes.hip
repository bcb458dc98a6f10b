// api_planes.hip -- the C ABI's oriented plane detection (include/hskinfu.h "Oriented plane detection"; DESIGN.md 3.14 the
// kernels, 8h the rule): hsk_detect_planes_oriented, hsk_detect_planes_volume, hsk_score_planes and hsk_default_plane_params.
// The round loop, the argmax and the refit (products.cpp: hsk_plane_refit) are the host's; the device is asked three kinds of
// question per round and the host waits for each answer: the hypotheses' counts, each refit's ten sums, the labelled count.
#pragma clang fp contract(off)
#include <cmath>
#include <new>
#include <vector>

#include "hsk_ctx.h"
#include "hsk_plane_point.h"

static_assert(HSK_PLANE_MAX_HYPOTHESES == HSK_PLANE_MAX_HYP, "the public limit of hypotheses is the size of k_plane_score's table in LDS");

// what plane detection adds to the alignment's scratch behind the cloud's planes: the labels, the seed points, the hypotheses
// (4 floats each), their counts, the score blocks' tables, the sweep blocks' sums (16 words each) and the 16 words they add up to
struct PlaneScratch {
  size_t labels_at, seeds_at, hyp_at, counts_at, tables_at, partial_at, sums_at, bytes;
  PlaneScratch(size_t n, size_t n_hyp) {
    ProductLayout L;
    labels_at = L.take(n * 4);
    seeds_at = L.take(n_hyp * 4);
    hyp_at = L.take(n_hyp * 16);
    counts_at = L.take(n_hyp * 4);
    tables_at = L.take((size_t)plane_score_blocks((unsigned)n) * n_hyp * 4);
    partial_at = L.take((size_t)cloud_sweep_blocks((unsigned)n) * 16 * 8);
    sums_at = L.take(16 * 8);
    bytes = L.bytes;
  }
};

extern "C" void hsk_default_plane_params(hsk_plane_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->dist_m = 0.02f;
  p->cos_min = 0.8660254037844387f;  // cos 30 degrees
  p->min_fraction = 0.03f;
  p->max_planes = 12;
  p->n_hypotheses = 512;
  p->refits = 2;
  p->seed = 0x9E3779B97F4A7C15ull;
}

static bool dist_cos_ok(float dist_m, float cos_min) { return dist_m > 0.0f && dist_m <= 1.0f && cos_min >= -1.0f && cos_min <= 1.0f; }

// params (NULL: the defaults) -> p, or the refusal
static int plane_resolve(hsk_ctx* k, const hsk_plane_params* params, hsk_plane_params* p, const char* who) {
  static_assert(sizeof(hsk_plane_params) == 32 && sizeof(hsk_plane_record) == 32, "the plane structs are 32 bytes each");
  if (params) *p = *params;
  else hsk_default_plane_params(p);
  const bool ok = dist_cos_ok(p->dist_m, p->cos_min) && std::isfinite(p->min_fraction) && p->min_fraction >= 0.0f && p->max_planes >= 1 &&
                  p->max_planes <= HSK_PLANE_MAX_PLANES && p->n_hypotheses >= 1 && p->n_hypotheses <= HSK_PLANE_MAX_HYPOTHESES &&
                  p->refits >= 0 && p->refits <= HSK_PLANE_MAX_REFITS;
  return ok ? HSK_OK : fail(k, HSK_ERR_ARG, (std::string(who) + ": a parameter is outside its range").c_str());
}

// The rounds over the n > 0 points in the scratch's planes: planes[0 .. *n_planes), and the labels (host, may be null).
static int plane_rounds(hsk_ctx* k, const CloudScratch& cs, size_t n, const hsk_plane_params& p, hsk_plane_record* planes, size_t* n_planes,
                        int32_t* labels) {
  const size_t H = (size_t)p.n_hypotheses;
  const PlaneScratch L(n, H);
  const float* d_soa = cs.soa;
  const unsigned pitch = cs.pitch;
  char* base = (char*)cs.extra;
  int* d_labels = (int*)(base + L.labels_at);
  unsigned* d_seeds = (unsigned*)(base + L.seeds_at);
  float* d_hyp = (float*)(base + L.hyp_at);
  unsigned* d_counts = (unsigned*)(base + L.counts_at);
  unsigned* d_tables = (unsigned*)(base + L.tables_at);
  unsigned long long* d_partial = (unsigned long long*)(base + L.partial_at);
  unsigned long long* d_sums = (unsigned long long*)(base + L.sums_at);
  std::vector<unsigned> seeds, counts;
  std::vector<float> hyp;
  try {
    seeds.resize(H);
    counts.resize(H);
    hyp.resize(H * 4);
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, "plane detection: out of host memory for the hypotheses");
  }
  HIPCHK(k, hipMemsetAsync(d_labels, 0xff, n * 4, k->stream));  // every label -1
  uint64_t rng = p.seed;
  const double min_inl = std::fmax(3.0, std::floor((double)p.min_fraction * (double)n));
  const unsigned un = (unsigned)n;
  size_t found = 0;
  while (found < (size_t)p.max_planes) {
    // 1, 2: the hypotheses and their scores
    for (size_t j = 0; j < H; ++j) seeds[j] = (unsigned)(plane_lcg_next(&rng) % (uint32_t)n);
    HIPCHK(k, hipMemcpyAsync(d_seeds, seeds.data(), H * 4, hipMemcpyHostToDevice, k->stream));
    launch_plane_seed(k->stream, d_soa, d_labels, d_seeds, (unsigned)H, pitch, d_hyp);
    launch_plane_score(k->stream, d_soa, d_labels, d_hyp, un, pitch, (unsigned)H, p.dist_m, p.cos_min, d_tables, d_counts);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(counts.data(), d_counts, H * 4, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipMemcpyAsync(hyp.data(), d_hyp, H * 16, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    size_t best = 0;
    for (size_t j = 1; j < H; ++j)
      if (counts[j] > counts[best]) best = j;  // (a tie stays with the lowest j)
    if ((double)counts[best] < min_inl) break;
    float abcd[4];
    memcpy(abcd, &hyp[4 * best], sizeof(abcd));
    // 3: the refits
    for (int r = 0; r < p.refits; ++r) {
      long long sums[10];
      launch_plane_moments(k->stream, d_soa, d_labels, abcd, un, pitch, p.dist_m, p.cos_min, d_partial, d_sums);
      HIPCHK(k, hipGetLastError());
      HIPCHK(k, hipMemcpyAsync(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost, k->stream));
      HIPCHK(k, hipStreamSynchronize(k->stream));
      int64_t s10[10];
      for (int v = 0; v < 10; ++v) s10[v] = (int64_t)sums[v];
      float next[4];
      int ok = 0;
      if (hsk_plane_refit(s10, abcd, next, &ok) != HSK_OK) return fail(k, HSK_ERR_STATE, "plane detection: the moments left their range");
      if (!ok) break;
      memcpy(abcd, next, sizeof(abcd));
    }
    // 4: the labels
    unsigned long long out2[2];
    launch_plane_label(k->stream, d_soa, d_labels, abcd, (int)found, un, pitch, p.dist_m, p.cos_min, d_partial, d_sums);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(out2, d_sums, sizeof(out2), hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    if ((double)out2[0] < min_inl) {  // the refit lost the support: its labels are taken back
      launch_plane_unlabel(k->stream, d_labels, (int)found, un);
      HIPCHK(k, hipGetLastError());
      break;
    }
    hsk_plane_record& rec = planes[found];
    memcpy(rec.abcd, abcd, sizeof(abcd));
    rec.n_inliers = (uint32_t)out2[0];
    rec.pad = 0;
    rec.sum_abs = out2[1];
    ++found;
  }
  *n_planes = found;
  if (labels) return copy_out(k, labels, d_labels, n * 4);
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}

extern "C" int hsk_detect_planes_oriented(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const hsk_plane_params* params,
                                          hsk_plane_record* planes, size_t cap, size_t* n_planes, int32_t* labels, size_t* n_invalid) {
  if (!k) return HSK_ERR_ARG;
  if (!planes || !n_planes || (n > 0 && (!xyz || !normals))) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_oriented: null argument");
  if (n > HSK_PLANE_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_oriented: more than 2^24 points");
  hsk_plane_params p;
  if (int rc = plane_resolve(k, params, &p, "hsk_detect_planes_oriented")) return rc;
  if (cap < (size_t)p.max_planes) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_oriented: cap is below max_planes");
  if (int ri = require_idle(k)) return ri;
  *n_planes = 0;
  if (n_invalid) *n_invalid = 0;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  CloudScratch cs;
  if (int rc = align_scratch(k, n, PlaneScratch(n, (size_t)p.n_hypotheses).bytes, &cs)) return rc;
  if (int rc = cloud_upload(k, xyz, normals, n, 1, cs, n_invalid, "hsk_detect_planes_oriented")) return rc;
  return plane_rounds(k, cs, n, p, planes, n_planes, labels);
}

extern "C" int hsk_detect_planes_volume(hsk_ctx* k, const hsk_plane_params* params, hsk_plane_record* planes, size_t cap, size_t* n_planes,
                                        int32_t* labels, size_t cap_labels, size_t* n_points) {
  if (!k) return HSK_ERR_ARG;
  if (!n_points) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_volume: null argument");
  const bool query = !planes && !labels;
  if (!query && (!planes || !n_planes)) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_volume: null argument");
  hsk_plane_params p;
  if (int rc = plane_resolve(k, params, &p, "hsk_detect_planes_volume")) return rc;
  if (!query && cap < (size_t)p.max_planes) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_volume: cap is below max_planes");
  if (int rs = require_whole_volume(k, k, "hsk_detect_planes_volume")) return rs;
  if (int ri = require_idle(k)) return ri;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  size_t n = 0;
  // the count pass alone says how many points there are: every refusal comes before the cloud is written
  if (int rc = cloud_count(k, &n)) return rc;
  *n_points = n;
  if (query) return HSK_OK;
  *n_planes = 0;
  if (n > HSK_PLANE_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_volume: the cloud has more than 2^24 points");
  if (labels && cap_labels < n) return fail(k, HSK_ERR_ARG, "hsk_detect_planes_volume: cap_labels is below the cloud's points");
  if (n == 0) return HSK_OK;
  CloudScratch cs;
  if (int rc = cloud_from_volume(k, n, PlaneScratch(n, (size_t)p.n_hypotheses).bytes, &cs)) return rc;
  return plane_rounds(k, cs, n, p, planes, n_planes, labels);
}

extern "C" int hsk_score_planes(hsk_ctx* k, const float* xyz, const float* normals, const int32_t* labels, size_t n, const float* planes_abcd,
                                size_t n_planes, float dist_m, float cos_min, uint32_t* counts) {
  if (!k) return HSK_ERR_ARG;
  if ((n > 0 && (!xyz || !normals)) || (n_planes > 0 && (!planes_abcd || !counts))) return fail(k, HSK_ERR_ARG, "hsk_score_planes: null argument");
  if (n > HSK_PLANE_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_score_planes: more than 2^24 points");
  if (n_planes > HSK_PLANE_MAX_HYPOTHESES) return fail(k, HSK_ERR_ARG, "hsk_score_planes: more than 4096 planes");
  if (!dist_cos_ok(dist_m, cos_min)) return fail(k, HSK_ERR_ARG, "hsk_score_planes: dist_m must lie in (0, 1] and cos_min in [-1, 1]");
  if (int ri = require_idle(k)) return ri;
  if (n_planes == 0) return HSK_OK;
  if (n == 0) {
    memset(counts, 0, n_planes * sizeof(uint32_t));
    return HSK_OK;
  }
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const PlaneScratch L(n, n_planes);
  CloudScratch cs;
  if (int rc = align_scratch(k, n, L.bytes, &cs)) return rc;
  if (int rc = cloud_upload(k, xyz, normals, n, 1, cs, nullptr, "hsk_score_planes")) return rc;
  char* base = (char*)cs.extra;
  int* d_labels = (int*)(base + L.labels_at);
  float* d_hyp = (float*)(base + L.hyp_at);
  unsigned* d_counts = (unsigned*)(base + L.counts_at);
  if (labels) HIPCHK(k, hipMemcpyAsync(d_labels, labels, n * 4, hipMemcpyHostToDevice, k->stream));
  HIPCHK(k, hipMemcpyAsync(d_hyp, planes_abcd, n_planes * 16, hipMemcpyHostToDevice, k->stream));
  launch_plane_score(k->stream, cs.soa, labels ? d_labels : nullptr, d_hyp, (unsigned)n, cs.pitch, (unsigned)n_planes, dist_m, cos_min,
                     (unsigned*)(base + L.tables_at), d_counts);
  HIPCHK(k, hipGetLastError());
  HIPCHK(k, hipMemcpyAsync(counts, d_counts, n_planes * 4, hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}
