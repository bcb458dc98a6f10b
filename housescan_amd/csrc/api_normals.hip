// api_normals.hip -- the C ABI's cloud normals (include/hskinfu.h "Cloud normals"; DESIGN.md 3.28 the kernels, 8v the rule):
// hsk_default_normal_params, hsk_estimate_normals, and the host mirror of one point's solve, hsk_normal_solve.
#pragma clang fp contract(off)
#include <cmath>
#include <string>

#include "hsk_ctx.h"
#include "hsk_normal_point.h"

static_assert(HSK_NORMAL_OK == NORMAL_OK && HSK_NORMAL_INVALID == NORMAL_INVALID && HSK_NORMAL_SPARSE == NORMAL_SPARSE &&
                  HSK_NORMAL_CROWDED == NORMAL_CROWDED && HSK_NORMAL_DEGENERATE == NORMAL_DEGENERATE,
              "the rule's classes are the ABI's");
static_assert(sizeof(hsk_normal_params) == 24 && sizeof(hsk_normal_stats) == 32, "the normal structs' sizes");
static_assert(NORMAL_CLASSES + 1 <= NORMAL_W_CELLS && NORMAL_W_VALID < NORMAL_WORDS, "the words: the classes, the pairs, then the named ones");

#define HSK_NORMAL_MIN_RADIUS_M (1.0f / 1024.0f)
#define HSK_NORMAL_MAX_RADIUS_M 0.25f

extern "C" void hsk_default_normal_params(const hsk_ctx* k, hsk_normal_params* p) {
  if (!p) return;
  float cell = 3.0f / 512.0f;
  if (k) cell = std::fmax(std::fmax(k->vp.cell[0], k->vp.cell[1]), k->vp.cell[2]);
  const float r = 3.0f * cell;
  p->radius_m = r < HSK_NORMAL_MIN_RADIUS_M ? HSK_NORMAL_MIN_RADIUS_M : (r > HSK_NORMAL_MAX_RADIUS_M ? HSK_NORMAL_MAX_RADIUS_M : r);
  p->min_neighbours = 8u;
  p->max_neighbours = 4096u;
  p->line_rel = 1.0e-3f;
  p->flags = 0u;
  p->pad = 0u;
}

static bool line_rel_ok(float line_rel) { return line_rel > 0.0f && line_rel <= 1.0f; }  // (a NaN fails both)

// the parameters as they hold (every 0 replaced by its default), or false (a NaN fails its comparison)
static bool normal_resolve(const hsk_ctx* k, const hsk_normal_params* in, hsk_normal_params* p) {
  hsk_normal_params d;
  hsk_default_normal_params(k, &d);
  if (!in) {
    *p = d;
    return true;
  }
  *p = *in;
  if (p->radius_m == 0.0f) p->radius_m = d.radius_m;
  if (p->min_neighbours == 0u) p->min_neighbours = d.min_neighbours;
  if (p->max_neighbours == 0u) p->max_neighbours = d.max_neighbours;
  if (p->line_rel == 0.0f) p->line_rel = d.line_rel;
  return p->radius_m >= HSK_NORMAL_MIN_RADIUS_M && p->radius_m <= HSK_NORMAL_MAX_RADIUS_M && p->min_neighbours >= 3u &&
         p->max_neighbours >= p->min_neighbours && p->max_neighbours <= (uint32_t)NORMAL_MAX_NEIGHBOURS && line_rel_ok(p->line_rel) &&
         p->flags == 0u;
}

static bool viewpoints_finite(const float* viewpoints, size_t n_viewpoints) {
  for (size_t i = 0; i < 3 * n_viewpoints; ++i)
    if (!std::isfinite(viewpoints[i])) return false;
  return true;
}

// what the call carves behind the cloud's planes: the cell table (keys, counts, first places with the scan's block sums, cursors),
// each point's slot, the points in cell order (three planes of q, their indices), the viewpoints, the words, the outputs
struct NormalScratch {
  size_t keys_at, counts_at, off_at, cursor_at, slot_at, sq_at, sidx_at, view_at, words_at, normals_at, curv_at, neigh_at, cls_at, bytes;
  size_t slots;
  NormalScratch(size_t n, size_t pitch) {
    slots = 128;
    while (slots < 2 * n) slots *= 2;  // (n <= 2^24: at most 2^25 slots, and never more than half of them taken)
    ProductLayout L;
    keys_at = L.take(slots * 8);
    counts_at = L.take(slots * 4);
    off_at = L.take(hsk_scan_scratch_entries((int)slots) * 8);
    cursor_at = L.take(slots * 4);
    slot_at = L.take(n * 4);
    sq_at = L.take(pitch * 3 * 4);
    sidx_at = L.take(n * 4);
    view_at = L.take((size_t)HSK_NORMAL_MAX_VIEWPOINTS * 3 * 4);
    words_at = L.take(NORMAL_WORDS * 8);
    normals_at = L.take(n * 12);
    curv_at = L.take(n * 4);
    neigh_at = L.take(n * 4);
    cls_at = L.take(n);
    bytes = L.bytes;
  }
};

extern "C" int hsk_estimate_normals(hsk_ctx* k, const float* xyz, size_t n, const float* viewpoints, size_t n_viewpoints, const hsk_normal_params* params,
                                    float* normals_out, float* curvature_out, uint32_t* neighbours_out, uint8_t* class_out, hsk_normal_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  if (!normals_out || (n > 0 && !xyz) || (n_viewpoints > 0 && !viewpoints)) return fail(k, HSK_ERR_ARG, "hsk_estimate_normals: null argument");
  if (n > HSK_NORMAL_MAX_POINTS) return fail(k, HSK_ERR_ARG, "hsk_estimate_normals: more than 2^24 points");
  if (n_viewpoints > HSK_NORMAL_MAX_VIEWPOINTS) return fail(k, HSK_ERR_ARG, "hsk_estimate_normals: more than 256 viewpoints");
  if (!viewpoints_finite(viewpoints, n_viewpoints)) return fail(k, HSK_ERR_ARG, "hsk_estimate_normals: a viewpoint is not finite");
  hsk_normal_params p;
  if (!normal_resolve(k, params, &p)) return fail(k, HSK_ERR_ARG, "hsk_estimate_normals: a parameter is outside its range");
  if (int rs = require_whole_volume(k, k, "hsk_estimate_normals")) return rs;
  if (int ri = require_idle(k)) return ri;
  if (stats) *stats = hsk_normal_stats{0u, 0u, 0u, 0u, 0u, 0u, 0ull};
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  CloudScratch cs;
  if (int rc = align_scratch(k, n, NormalScratch(n, (n + 63) & ~(size_t)63).bytes, &cs)) return rc;
  const NormalScratch L(n, cs.pitch);
  if (int rc = cloud_upload(k, xyz, nullptr, n, 1, cs, nullptr, "hsk_estimate_normals")) return rc;
  char* base = (char*)cs.extra;
  NormalIndex ix;
  ix.keys = (unsigned long long*)(base + L.keys_at);
  ix.counts = (unsigned*)(base + L.counts_at);
  ix.off = (unsigned long long*)(base + L.off_at);
  ix.cursor = (unsigned*)(base + L.cursor_at);
  ix.slot = (unsigned*)(base + L.slot_at);
  ix.sq = (int*)(base + L.sq_at);
  ix.sidx = (unsigned*)(base + L.sidx_at);
  ix.words = (unsigned long long*)(base + L.words_at);
  ix.mask = (unsigned)(L.slots - 1);
  const NormalOut out = {(float*)(base + L.normals_at), (float*)(base + L.curv_at), (unsigned*)(base + L.neigh_at), (unsigned char*)(base + L.cls_at)};
  float* d_view = (float*)(base + L.view_at);
  // the table armed for this call: no key, no count, no cursor (counts and cursors lie apart: two sets)
  HIPCHK(k, hipMemsetAsync(ix.keys, 0xff, L.slots * 8, k->stream));
  HIPCHK(k, hipMemsetAsync(ix.counts, 0, L.slots * 4, k->stream));
  HIPCHK(k, hipMemsetAsync(ix.cursor, 0, L.slots * 4, k->stream));
  HIPCHK(k, hipMemsetAsync(ix.words, 0, NORMAL_WORDS * 8, k->stream));
  if (n_viewpoints > 0) HIPCHK(k, hipMemcpyAsync(d_view, viewpoints, n_viewpoints * 12, hipMemcpyHostToDevice, k->stream));
  const int r_q = normal_radius_q(p.radius_m);
  const NormalArgs args = {p.min_neighbours, p.max_neighbours, (unsigned)n_viewpoints, p.line_rel};
  launch_normal_index(k->stream, cs.soa, (unsigned)n, cs.pitch, r_q, ix, out);
  launch_normal_gather(k->stream, cs.soa, (unsigned)n, cs.pitch, r_q, args, d_view, ix, out);
  HIPCHK(k, hipGetLastError());
  unsigned long long w[NORMAL_WORDS];
  HIPCHK(k, hipMemcpyAsync(w, ix.words, sizeof(w), hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  unsigned long long classes = 0;
  for (int c = 0; c < NORMAL_CLASSES; ++c) classes += w[c];
  if (w[NORMAL_W_ERROR] != 0ull || classes != (unsigned long long)n)
    return fail(k, HSK_ERR_STATE, "hsk_estimate_normals: the cell table's probe ran out of its bound (nothing was written)");
  if (int rc = copy_out(k, normals_out, out.normals, n * 12)) return rc;
  if (curvature_out)
    if (int rc = copy_out(k, curvature_out, out.curvature, n * 4)) return rc;
  if (neighbours_out)
    if (int rc = copy_out(k, neighbours_out, out.neighbours, n * 4)) return rc;
  if (class_out)
    if (int rc = copy_out(k, class_out, out.cls, n)) return rc;
  if (stats)
    *stats = hsk_normal_stats{(uint32_t)w[NORMAL_OK],       (uint32_t)w[NORMAL_INVALID], (uint32_t)w[NORMAL_SPARSE], (uint32_t)w[NORMAL_CROWDED],
                              (uint32_t)w[NORMAL_DEGENERATE], (uint32_t)w[NORMAL_W_CELLS], (uint64_t)w[NORMAL_CLASSES]};
  if (w[NORMAL_CROWDED] != 0ull)
    k->err = "hsk_estimate_normals: " + std::to_string(w[NORMAL_CROWDED]) +
             " points have more than max_neighbours neighbours (HSK_NORMAL_CROWDED): downsample the cloud (hsk_voxel_downsample) or shrink radius_m";
  return HSK_OK;
}

extern "C" int hsk_normal_solve(const int64_t sums10[10], const float point[3], const float* viewpoints, size_t n_viewpoints, float line_rel,
                                float normal_out[3], float* curvature_out, int* class_out) {
  if (!sums10 || !point || !normal_out || !curvature_out || !class_out || (n_viewpoints > 0 && !viewpoints)) return HSK_ERR_ARG;
  if (n_viewpoints > HSK_NORMAL_MAX_VIEWPOINTS || !viewpoints_finite(viewpoints, n_viewpoints) || !viewpoints_finite(point, 1) || !line_rel_ok(line_rel))
    return HSK_ERR_ARG;
  const int64_t m = sums10[0];
  if (m < 1 || m > (int64_t)NORMAL_MAX_NEIGHBOURS) return HSK_ERR_ARG;
  // what m neighbours within 1024 grid steps can make: |S_a| <= 2^10 m, |S_ab| <= 2^20 m (the matrix then stays inside 64 bits)
  normal_i64 s[NORMAL_SUMS];
  for (int v = 0; v < NORMAL_SUMS; ++v) {
    const int64_t lim = v == 0 ? m : (v < 4 ? m * NORMAL_MAX_RQ : m * NORMAL_MAX_RQ * NORMAL_MAX_RQ);
    if (sums10[v] > lim || sums10[v] < -lim) return HSK_ERR_ARG;
    s[v] = (normal_i64)sums10[v];
  }
  *class_out = normal_solve(s, point[0], point[1], point[2], viewpoints, n_viewpoints, line_rel, normal_out, curvature_out);
  return HSK_OK;
}
