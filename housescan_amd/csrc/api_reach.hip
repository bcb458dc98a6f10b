// api_reach.hip -- the C ABI's reach field (include/hskinfu.h "Reach field"; DESIGN.md 3.19 the kernels, 8m the rule):
// hsk_default_reach_params, hsk_build_reach, hsk_download_reach, hsk_reach_at, hsk_reach_path, hsk_reach_floor, hsk_release_reach,
// hsk_reach_tiles_relaxed and the host-only hsk_rank_views_reach and hsk_reach_metres.  The field is built from the clearance field
// (api_clearance.hip builds or reuses it first) and stays on the device (reach, a HeldPass) while vol_epoch, the 20 device-relevant
// clearance bytes, min_d2, max_cost and the seeds' voxels stand.  The host drives the rounds: it reads the next worklist's length
// after every round and stops at zero, or at HSK_REACH_MAX_ROUNDS (relax_rounds, which api_partition.hip drives its rounds with
// too).  Nothing the tracker reads is written; vol_epoch does not move.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>

#include "hsk_ctx.h"
#include "hsk_clear_point.h"
#include "hsk_reach_point.h"

static_assert(HSK_REACH_UNREACHED == REACH_UNREACHED && HSK_REACH_OUTSIDE == REACH_OUTSIDE && HSK_REACH_BLOCKED == REACH_BLOCKED &&
                  HSK_REACH_MAX_COST == REACH_MAX_COST && HSK_REACH_MAX_SEEDS == REACH_MAX_SEEDS && HSK_REACH_MAX_ROUNDS == REACH_MAX_ROUNDS &&
                  HSK_REACH_OUTSIDE == HSK_CLEARANCE_OUTSIDE,
              "the reach constants");
static_assert(sizeof(hsk_reach_params) == 16 && sizeof(hsk_reach_stats) == 40, "the reach structs");

extern "C" void hsk_default_reach_params(const hsk_ctx* k, const hsk_clearance_params* cp, hsk_reach_params* p) {
  if (!p) return;
  hsk_clearance_params c;
  if (cp)
    c = *cp;
  else
    hsk_default_clearance_params(k, &c);
  memset(p, 0, sizeof(*p));
  p->min_d2 = std::max(1u, std::min(hsk_clearance_d2(&c, 0.3f), c.max_d2));  // (a person's half width; a max_d2 of 0 has no legal min_d2)
  p->max_cost = HSK_REACH_MAX_COST;
}

extern "C" float hsk_reach_metres(const hsk_clearance_params* p, uint32_t g) {
  if (!p || g > HSK_REACH_MAX_COST) return NAN;
  return (float)((double)g * (double)p->unit_m / 16.0);
}

extern "C" int hsk_rank_views_reach(const hsk_view_score* s, const uint32_t* eye_g, uint32_t max_g, size_t n, uint32_t* order) {
  if (n > 0 && (!s || !eye_g || !order)) return HSK_ERR_ARG;
  if (n > 0xffffffffull) return HSK_ERR_ARG;
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  auto behind = [&](uint32_t a) { return eye_g[a] > HSK_REACH_MAX_COST || eye_g[a] > max_g; };
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {  // (stable: equal scores stay in index order)
    const bool ra = behind(a), rb = behind(b);
    if (ra != rb) return rb;
    const bool sa = s[a].eye_state != HSK_EYE_FREE, sb = s[b].eye_state != HSK_EYE_FREE;
    if (sa != sb) return sb;
    if (s[a].gain != s[b].gain) return s[a].gain > s[b].gain;
    return s[a].n_frontier > s[b].n_frontier;
  });
  return HSK_OK;
}

// the reach parameters a call works with (NULL: the defaults for the checked clearance parameters), checked
static int reach_check(hsk_ctx* k, const hsk_clearance_params& cp, const hsk_reach_params* params, const float* seeds, size_t n_seeds, const char* who,
                       hsk_reach_params* p) {
  auto bad = [&](const char* what) { return fail(k, HSK_ERR_ARG, (std::string(who) + what).c_str()); };
  if (params)
    *p = *params;
  else
    hsk_default_reach_params(k, &cp, p);
  if (p->flags != 0u) return bad(": flags must be 0");
  if (p->min_d2 < 1u || p->min_d2 > cp.max_d2) return bad(": min_d2 must lie in 1..max_d2 of the clearance parameters");
  if (p->max_cost > HSK_REACH_MAX_COST) return bad(": max_cost above HSK_REACH_MAX_COST");
  if (n_seeds > HSK_REACH_MAX_SEEDS) return bad(": more than 4096 seeds");
  if (n_seeds > 0 && !seeds) return bad(": seeds_xyz is null");
  return HSK_OK;
}

int relax_rounds(hsk_ctx* k, const std::function<hipError_t(int, unsigned)>& launch_round, const unsigned long long* lengths, unsigned long long n_active,
                 const char* what, uint32_t* rounds, unsigned long long* tiles) {
  *rounds = 0;
  *tiles = 0;
  int cur = 0;
  while (n_active) {  // (ends: at HSK_REACH_MAX_ROUNDS at the latest)
    if (*rounds >= HSK_REACH_MAX_ROUNDS)
      return fail(k, HSK_ERR_STATE, (std::string(what) + " did not settle within HSK_REACH_MAX_ROUNDS rounds").c_str());
    HIPCHK(k, launch_round(cur, (unsigned)n_active));
    *tiles += n_active;
    *rounds += 1;
    cur ^= 1;
    if (int r = read_u64(k, &n_active, lengths + cur)) return r;
  }
  return HSK_OK;
}

// The relaxation of one grid: init from the clearance values d2, the seeds (n_seeds voxels at d_seeds), rounds until a round marks
// no tile.  counts: passable, reached, the largest value, the seeds used.
static int reach_run(hsk_ctx* k, const unsigned* d2, const ReachGeom& q, const ReachBufs& b, const unsigned* d_seeds, unsigned n_seeds,
                     unsigned long long counts[4], uint32_t* rounds, unsigned long long* tiles) {
  HIPCHK(k, launch_reach_init(k->stream, d2, q, b));
  unsigned long long n_active = 0;
  if (n_seeds) {
    launch_reach_seed(k->stream, q, b, d_seeds, n_seeds);
    HIPCHK(k, hipGetLastError());
    if (int r = read_u64(k, &n_active, b.counters + 4)) return r;
  }
  auto round = [&](int cur, unsigned n) { return launch_reach_round(k->stream, q, b, cur, n); };
  if (int r = relax_rounds(k, round, b.counters + 4, n_active, "the reach field", rounds, tiles)) return r;
  launch_reach_stats(k->stream, q, b);
  HIPCHK(k, hipGetLastError());
  if (int r = read_u64(k, counts, b.counters, 4)) return r;
  counts[2] = counts[1] ? (unsigned long long)(uint32_t)~(uint32_t)counts[2] : 0ull;  // (the device keeps the complement)
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

static void reach_fill_stats(hsk_reach_stats* st, const unsigned long long counts[4], size_t scratch, uint32_t rounds, bool reused) {
  memset(st, 0, sizeof(*st));
  st->n_passable = counts[0];
  st->n_reached = counts[1];
  st->max_cost_seen = (uint32_t)counts[2];
  st->n_seeds_used = (uint32_t)counts[3];
  st->scratch_bytes = scratch;
  st->n_rounds = rounds;
  st->reused = reused ? 1 : 0;
}

extern "C" int hsk_build_reach(hsk_ctx* k, const hsk_clearance_params* cparams, const hsk_reach_params* params, const float* seeds_xyz, size_t n_seeds,
                               hsk_reach_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  hsk_clearance_params cp;
  ClearGeom cq;
  hsk_reach_params p;
  if (int rc = clear_check(k, cparams, "hsk_build_reach", &cp, &cq)) return rc;
  if (int rc = reach_check(k, cp, params, seeds_xyz, n_seeds, "hsk_build_reach", &p)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_build_reach")) return rc;
  // the key: the clearance key, min_d2, max_cost, then the seeds' voxels -- a point outside the grid, or with a NaN, is dropped
  // here; one on a voxel that is not passable on the device
  const SampleVol sv = hsk_sample_vol(k->vp);
  std::vector<uint32_t> key(7);
  key.reserve(7 + n_seeds);
  clear_key_of(cp, key.data());
  key[5] = p.min_d2;
  key[6] = p.max_cost;
  for (size_t i = 0; i < n_seeds; ++i) {
    unsigned x, y, z;
    bool inside;
    clear_point_voxel(sv, seeds_xyz[3 * i], seeds_xyz[3 * i + 1], seeds_xyz[3 * i + 2], x, y, z, inside);
    if (inside) key.push_back((uint32_t)(((size_t)z * (unsigned)sv.Y + y) * (unsigned)sv.X + x));
  }
  const uint32_t* vox = key.data() + 7;
  const size_t n_vox = key.size() - 7;
  const bool held = k->reach.stands_for(k, key.data(), key.size() * 4);
  if (!held) {
    HIPCHK(k, hipSetDevice(k->cfg.device_id));
    k->reach.drop();
    bool clear_reused = false;
    int r = clear_build(k, cp, cq, &clear_reused);
    if (r != HSK_OK) return r;
    ReachGeom q;
    reach_geom(cq.X, cq.Y, cq.Z, cq.w, p.min_d2, p.max_cost, &q);
    r = k->reach.grow(k, reach_layout(q, nullptr, nullptr));
    if (r != HSK_OK) return r;
    ReachBufs b;
    reach_layout(q, k->reach.buf, &b);
    ClearBufs cb;
    clear_layout(k->vp, k->clear.buf, &cb);
    if (n_vox) {
      r = ensure_product_bytes(k, n_vox * 4);
      if (r != HSK_OK) return r;
      HIPCHK(k, hipMemcpyAsync(k->d_out, vox, n_vox * 4, hipMemcpyHostToDevice, k->stream));
    }
    unsigned long long counts[4];
    uint32_t rounds = 0;
    unsigned long long tiles = 0;
    r = reach_run(k, cb.field, q, b, (const unsigned*)k->d_out, (unsigned)n_vox, counts, &rounds, &tiles);
    if (r != HSK_OK) return r;
    memcpy(k->reach_counts, counts, sizeof(counts));
    k->reach_q = q;
    k->reach_rounds = rounds;
    k->reach_tiles = tiles;
    k->reach.stamp(k, key.data(), key.size() * 4);
  }
  if (stats) reach_fill_stats(stats, k->reach_counts, k->reach.bytes, held ? 0u : k->reach_rounds, held);
  return HSK_OK;
}

// the reads: a field must be held
static int reach_held(hsk_ctx* k, const char* who) {
  if (int rc = volume_state_check(k, k, who)) return rc;
  return k->reach.require(k, who, ": no reach field of the volume as it stands is held (hsk_build_reach makes one)");
}

extern "C" int hsk_download_reach(hsk_ctx* k, const hsk_voxel_box* box, uint32_t* g) {
  if (!k) return HSK_ERR_ARG;
  if (!g) return fail(k, HSK_ERR_ARG, "hsk_download_reach: g is null");
  hsk_voxel_box b;
  size_t n;
  if (int rc = clear_box_check(k, box, "hsk_download_reach", &b, &n)) return rc;
  if (int rc = reach_held(k, "hsk_download_reach")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  ReachBufs rb;
  reach_layout(k->reach_q, k->reach.buf, &rb);
  return download_rows(k, rb.field, 4, b, n, g);
}

extern "C" int hsk_reach_at(hsk_ctx* k, const float* xyz, size_t n, uint32_t* g) {
  if (!k) return HSK_ERR_ARG;
  if (int rc = points_check(k, "hsk_reach_at", xyz, g, n, 0, -1)) return rc;
  if (int rc = reach_held(k, "hsk_reach_at")) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  ReachBufs rb;
  reach_layout(k->reach_q, k->reach.buf, &rb);
  // (the clearance field's gather: OUTSIDE is the same word)
  return gather_points(k, xyz, n, g, [&](const float* pts, unsigned* out, unsigned char*) { launch_clear_gather(k->stream, rb.field, k->vp, pts, (unsigned)n, out); });
}

extern "C" int hsk_reach_path(hsk_ctx* k, const float goal_xyz[3], int32_t* voxels_xyz, size_t cap, size_t* n) {
  if (!k) return HSK_ERR_ARG;
  if (!goal_xyz || !n || (cap > 0 && !voxels_xyz)) return fail(k, HSK_ERR_ARG, "hsk_reach_path: null argument");
  if (int rc = reach_held(k, "hsk_reach_path")) return rc;
  unsigned x, y, z;
  bool inside;
  clear_point_voxel(hsk_sample_vol(k->vp), goal_xyz[0], goal_xyz[1], goal_xyz[2], x, y, z, inside);
  if (!inside) {  // (OUTSIDE: not reached)
    *n = 0;
    return HSK_OK;
  }
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const ReachGeom& q = k->reach_q;
  ReachBufs rb;
  reach_layout(q, k->reach.buf, &rb);
  const unsigned goal = (unsigned)(((size_t)z * q.Y + y) * q.X + x);
  // the walk writes at most `room` voxels and counts them all: a first pass with room for most paths, a second one for a longer path
  unsigned long long res[2] = {0, 0};
  size_t room = std::min(cap, (size_t)65536);
  std::vector<int32_t> back;
  for (int pass = 0; pass < 2; ++pass) {
    ProductLayout lay;
    const size_t res_at = lay.take(16), out_at = lay.take(std::max(room, (size_t)1) * 12);
    int r = ensure_product_bytes(k, lay.bytes);
    if (r != HSK_OK) return r;
    char* base = (char*)k->d_out;
    launch_reach_path(k->stream, rb.field, q, goal, room, (int*)(base + out_at), (unsigned long long*)(base + res_at));
    HIPCHK(k, hipGetLastError());
    r = read_u64(k, res, (const unsigned long long*)(base + res_at), 2);
    if (r != HSK_OK) return r;
    if (res[1]) return fail(k, HSK_ERR_STATE, "hsk_reach_path: the field held is no fixpoint");
    if (res[0] > cap) {
      *n = (size_t)res[0];
      return fail(k, HSK_ERR_ARG, "hsk_reach_path: cap is smaller than the path (*n: its length)");
    }
    if (res[0] <= room) {
      back.resize((size_t)res[0] * 3);
      if (res[0]) {
        r = copy_out(k, back.data(), base + out_at, (size_t)res[0] * 12);
        if (r != HSK_OK) return r;
      }
      break;
    }
    room = (size_t)res[0];
  }
  const size_t len = (size_t)res[0];
  for (size_t i = 0; i < len; ++i)  // (from the seed to the goal)
    for (int c = 0; c < 3; ++c) voxels_xyz[3 * i + c] = back[3 * (len - 1 - i) + c];
  *n = len;
  return HSK_OK;
}

extern "C" int hsk_reach_floor(hsk_ctx* k, const hsk_clearance_params* cparams, int axis, int lo, int hi, const hsk_reach_params* params,
                               const float* seeds_xyz, size_t n_seeds, uint32_t* map, hsk_reach_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  if (!map) return fail(k, HSK_ERR_ARG, "hsk_reach_floor: map is null");
  hsk_clearance_params cp;
  ClearGeom cq;
  hsk_reach_params p;
  if (int rc = clear_check(k, cparams, "hsk_reach_floor", &cp, &cq)) return rc;
  if (int rc = reach_check(k, cp, params, seeds_xyz, n_seeds, "hsk_reach_floor", &p)) return rc;
  FloorGrid f;
  if (int rc = clear_floor_grid(k, cq, axis, lo, hi, "hsk_reach_floor", &f)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_reach_floor")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  // the map's grid: (u, v, 1), u the lower-numbered remaining axis; the same kernels, on which no move along the third axis is
  // ever allowed (its neighbours lie outside the grid)
  ReachGeom q;
  reach_geom(f.nu, f.nv, 1u, f.w, p.min_d2, p.max_cost, &q);
  // the seeds, projected by dropping the up axis: that coordinate does not count, whatever it holds
  const SampleVol sv = hsk_sample_vol(k->vp);
  std::vector<uint32_t> vox;
  vox.reserve(n_seeds);
  for (size_t i = 0; i < n_seeds; ++i) {
    float c[3] = {seeds_xyz[3 * i], seeds_xyz[3 * i + 1], seeds_xyz[3 * i + 2]};
    c[axis] = 0.0f;
    unsigned g[3];
    bool inside;
    clear_point_voxel(sv, c[0], c[1], c[2], g[0], g[1], g[2], inside);
    if (inside) vox.push_back((uint32_t)((size_t)g[f.av] * f.nu + g[f.au]));
  }
  const size_t n = (size_t)f.nu * f.nv;
  ProductLayout lay;
  const size_t a_at = lay.take(n * 4), b_at = lay.take(n * 4), seeds_at = lay.take((size_t)HSK_REACH_MAX_SEEDS * 4);
  const size_t reach_at = lay.take(reach_layout(q, nullptr, nullptr));
  int r = ensure_product_bytes(k, lay.bytes);
  if (r != HSK_OK) return r;
  char* base = (char*)k->d_out;
  launch_clear_floor(k->stream, k->d_vol, k->vp, cq, axis, lo, hi, (unsigned*)(base + a_at), (unsigned*)(base + b_at));
  HIPCHK(k, hipGetLastError());
  if (!vox.empty()) HIPCHK(k, hipMemcpyAsync(base + seeds_at, vox.data(), vox.size() * 4, hipMemcpyHostToDevice, k->stream));
  ReachBufs rb;
  reach_layout(q, base + reach_at, &rb);
  unsigned long long counts[4];
  uint32_t rounds = 0;
  unsigned long long tiles = 0;
  r = reach_run(k, (const unsigned*)(base + a_at), q, rb, (const unsigned*)(base + seeds_at), (unsigned)vox.size(), counts, &rounds, &tiles);
  if (r != HSK_OK) return r;
  r = copy_out(k, map, rb.field, n * 4);
  if (r != HSK_OK) return r;
  if (stats) reach_fill_stats(stats, counts, lay.bytes, rounds, false);
  return HSK_OK;
}

extern "C" int hsk_release_reach(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  return k->reach.release(k);
}

extern "C" int hsk_reach_tiles_relaxed(const hsk_ctx* k, uint64_t* tiles_relaxed, uint64_t* tiles) {
  if (!k) return HSK_ERR_ARG;
  if (tiles_relaxed) *tiles_relaxed = k->reach_tiles;
  if (tiles) *tiles = (uint64_t)k->reach_q.ntx * k->reach_q.nty * k->reach_q.ntz;
  return HSK_OK;
}
