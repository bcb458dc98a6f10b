// api_partition.hip -- the C ABI's room partition (include/hskinfu.h "Room partition"; DESIGN.md 3.20 the kernels, 8n the rule):
// hsk_default_partition_params, hsk_build_partition, hsk_partition_doors, hsk_download_partition, hsk_download_partition_cost,
// hsk_partition_at, hsk_partition_floor, hsk_release_partition, hsk_partition_tiles_relaxed and the host-only hsk_merge_rooms.
// The partition is built from the clearance field (api_clearance.hip builds or reuses it first) and stays on the device (part, a HeldPass)
// while vol_epoch, the 20 device-relevant clearance bytes and the four partition parameters stand.  The host drives it: it reads
// the number of kept cores and sorts their roots between the labelling and the init, reads the next worklist's length after every
// round and stops at zero or at HSK_REACH_MAX_ROUNDS (api_reach.hip: relax_rounds), orders the room records and sends the id table back before the door sweep.
// Nothing the tracker reads is written; vol_epoch does not move.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <numeric>

#include "hsk_ctx.h"
#include "hsk_clear_point.h"
#include "hsk_part_point.h"

static_assert(HSK_ROOM_UNASSIGNED == PART_ROOM_UNASSIGNED && HSK_ROOM_OUTSIDE == PART_ROOM_OUTSIDE && HSK_ROOM_BLOCKED == PART_ROOM_BLOCKED &&
                  HSK_ROOM_NONE == PART_ROOM_NONE && HSK_PARTITION_MAX_ROOMS == PART_MAX_ROOMS && HSK_PARTITION_MAX_RADIUS == PART_MAX_RADIUS &&
                  HSK_ROOM_OUTSIDE == HSK_CLEARANCE_OUTSIDE && HSK_ROOM_BLOCKED == HSK_REACH_BLOCKED,
              "the partition constants");
static_assert(sizeof(hsk_partition_params) == 24 && sizeof(hsk_room) == 88 && sizeof(hsk_door) == 72 && sizeof(hsk_partition_stats) == 56,
              "the partition structs");

extern "C" void hsk_default_partition_params(const hsk_ctx* k, const hsk_clearance_params* cp, hsk_partition_params* p) {
  if (!p) return;
  hsk_clearance_params c;
  if (cp)
    c = *cp;
  else
    hsk_default_clearance_params(k, &c);
  float cell[3];
  context_cells(k, cell, nullptr);
  memset(p, 0, sizeof(*p));
  p->core_d2 = std::max(1u, std::min(hsk_clearance_d2(&c, 0.5f), c.max_d2));  // (half a metre: a stated choice, not a measurement)
  p->min_d2 = 1u;
  // the voxels of a cube of edge 0.25 m, in binary64 from the binary32 cells (as hsk_default_prune_params)
  const double e = 0.25;
  p->min_core_voxels = (uint32_t)std::min(4294967295.0, std::ceil(((e * e) * e) / (((double)cell[0] * (double)cell[1]) * (double)cell[2])));
  p->max_cost = HSK_REACH_MAX_COST;
}

extern "C" int hsk_merge_rooms(const hsk_door* doors, size_t n_doors, size_t n_rooms, uint32_t merge_d2, uint32_t* map) {
  if ((n_doors > 0 && !doors) || (n_rooms > 0 && !map) || n_rooms > 0xffffffffull) return HSK_ERR_ARG;
  for (size_t i = 0; i < n_doors; ++i)
    if (doors[i].a >= n_rooms || doors[i].b >= n_rooms) return HSK_ERR_ARG;
  std::vector<uint32_t> parent(n_rooms);
  std::iota(parent.begin(), parent.end(), 0u);
  auto find = [&](uint32_t v) {  // (ends: parent[v] <= v, and falls until it names itself)
    while (parent[v] != v) v = parent[v];
    return v;
  };
  for (size_t i = 0; i < n_doors; ++i) {
    if (doors[i].max_d2 < merge_d2) continue;
    const uint32_t a = find(doors[i].a), b = find(doors[i].b);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  for (size_t i = 0; i < n_rooms; ++i) map[i] = find((uint32_t)i);
  return HSK_OK;
}

// the partition parameters a call works with (NULL: the defaults for the checked clearance parameters), checked
static int part_check(hsk_ctx* k, const hsk_clearance_params& cp, const hsk_partition_params* params, const char* who, hsk_partition_params* p) {
  auto bad = [&](const char* what) { return fail(k, HSK_ERR_ARG, (std::string(who) + what).c_str()); };
  if (params)
    *p = *params;
  else
    hsk_default_partition_params(k, &cp, p);
  if (p->flags != 0u) return bad(": flags must be 0");
  if (!(1u <= p->min_d2 && p->min_d2 <= p->core_d2 && p->core_d2 <= cp.max_d2))
    return bad(": the thresholds must satisfy 1 <= min_d2 <= core_d2 <= max_d2 of the clearance parameters");
  if (p->max_cost > HSK_REACH_MAX_COST) return bad(": max_cost above HSK_REACH_MAX_COST");
  return HSK_OK;
}

// what one partition of a grid left on the host
struct PartResult {
  unsigned long long counts[4] = {0, 0, 0, 0};  // passable, cores, kept cores, assigned
  uint32_t rounds = 0;
  unsigned long long tiles = 0, first = 0;
  std::vector<hsk_room> recs;
  std::vector<hsk_door> doors;
  bool too_many = false;
};

// The partition of one grid of clearance values d2: labelling, init, rounds until a round marks no tile, records, doors.  With more
// than HSK_PARTITION_MAX_ROOMS kept cores only counts[1], counts[2] and too_many are set, HSK_OK returned, and the keys are not made.
static int part_run(hsk_ctx* k, const unsigned* d2, const PartGeom& q, const PartBufs& b, PartResult* out) {
  HIPCHK(k, launch_part_label(k->stream, d2, q, b));
  unsigned long long c[4];
  if (int r = read_u64(k, c, b.counters, 4)) return r;
  out->counts[1] = c[1];
  out->counts[2] = c[2];
  if (c[2] > (unsigned long long)HSK_PARTITION_MAX_ROOMS) {
    out->too_many = true;
    return HSK_OK;
  }
  const unsigned n_kept = (unsigned)c[2];
  std::vector<uint32_t> roots(n_kept);
  if (n_kept) {
    if (int r = copy_out(k, roots.data(), b.roots_found, (size_t)n_kept * 4)) return r;
    std::sort(roots.begin(), roots.end());
    HIPCHK(k, hipMemcpyAsync(b.roots, roots.data(), (size_t)n_kept * 4, hipMemcpyHostToDevice, k->stream));
  }
  HIPCHK(k, launch_part_init(k->stream, d2, q, b, n_kept));
  unsigned long long n_active = 0;
  if (int r = read_u64(k, &n_active, b.counters + 4)) return r;
  out->first = n_active;
  if (!n_kept) n_active = 0;  // (no core: nothing can fall)
  auto round = [&](int cur, unsigned n) { return launch_part_round(k->stream, q, b, cur, n); };
  if (int r = relax_rounds(k, round, b.counters + 4, n_active, "the partition", &out->rounds, &out->tiles)) return r;
  if (int r = read_u64(k, &out->counts[0], b.counters)) return r;
  if (!n_kept) return HSK_OK;
  // the records: the device's sums per ascending root -> the order n_voxels descending, ties to the smaller root -> the id table
  HIPCHK(k, launch_part_records(k->stream, d2, q, b, n_kept));
  std::vector<unsigned long long> sums((size_t)n_kept * PART_REC_WORDS);
  if (int r = copy_out(k, sums.data(), b.recs, sums.size() * 8)) return r;
  std::vector<uint32_t> order(n_kept), rank(n_kept);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t i, uint32_t j) {
    return comp_record_before(sums[(size_t)i * PART_REC_WORDS], roots[i], sums[(size_t)j * PART_REC_WORDS], roots[j]);
  });
  out->recs.resize(n_kept);
  for (unsigned id = 0; id < n_kept; ++id) {
    const unsigned i = order[id];
    const unsigned long long* s = &sums[(size_t)i * PART_REC_WORDS];
    rank[i] = id;
    hsk_room rec;
    memset(&rec, 0, sizeof(rec));
    rec.n_voxels = s[0];
    rec.n_core_voxels = s[1];
    rec.root[0] = roots[i] % q.X;
    rec.root[1] = (roots[i] / q.X) % q.Y;
    rec.root[2] = roots[i] / (q.X * q.Y);
    for (int a = 0; a < 3; ++a) {
      rec.sum[a] = s[2 + a];
      rec.lo[a] = ~(uint32_t)s[5 + a];  // (the device keeps the largest complement)
      rec.hi[a] = (uint32_t)s[8 + a] + 1u;
    }
    rec.max_d2 = (uint32_t)s[11];
    rec.max_g = (uint32_t)s[12];
    out->recs[id] = rec;
    out->counts[3] += s[0];
  }
  HIPCHK(k, hipMemcpyAsync(b.rank, rank.data(), (size_t)n_kept * 4, hipMemcpyHostToDevice, k->stream));
  if (n_kept < 2u) {
    HIPCHK(k, hipStreamSynchronize(k->stream));  // (rank leaves the host before it goes out of scope)
    return HSK_OK;
  }
  // the doors: a dense table over the pairs of rooms, 64 bytes each, scanned on the host in (a, b) order
  const size_t words = (size_t)n_kept * n_kept * PART_DOOR_WORDS;
  if (int r = k->part.grow_tab(k, words * 8)) return r;
  HIPCHK(k, launch_part_doors(k->stream, d2, q, b, n_kept, (unsigned long long*)k->part.tab));
  std::vector<unsigned long long> table(words);
  if (int r = copy_out(k, table.data(), k->part.tab, words * 8)) return r;
  for (unsigned a = 0; a < n_kept; ++a)
    for (unsigned bb = a + 1u; bb < n_kept; ++bb) {
      const unsigned long long* t = &table[((size_t)a * n_kept + bb) * PART_DOOR_WORDS];
      uint32_t t32[10];
      memcpy(t32, t + 3, sizeof(t32));
      if (!(t32[0] | t32[1] | t32[2])) continue;
      hsk_door d;
      memset(&d, 0, sizeof(d));
      d.a = a;
      d.b = bb;
      for (int i = 0; i < 3; ++i) {
        d.sum2[i] = t[i];
        d.n_faces[i] = t32[i];
        d.lo[i] = ~t32[3 + i];
        d.hi[i] = t32[6 + i] + 1u;
      }
      d.max_d2 = t32[9];
      out->doors.push_back(d);
    }
  return HSK_OK;
}

static void part_fill_stats(hsk_partition_stats* st, const PartResult& res, size_t scratch, bool reused) {
  memset(st, 0, sizeof(*st));
  st->n_cores = res.counts[1];
  st->n_passable = res.counts[0];
  st->n_assigned = res.counts[3];
  st->scratch_bytes = scratch;
  st->n_dropped = res.counts[1] - res.counts[2];
  st->n_rooms = (uint32_t)std::min<unsigned long long>(res.counts[2], 0xffffffffull);
  st->n_doors = (uint32_t)res.doors.size();
  st->n_rounds = reused ? 0u : res.rounds;
  st->reused = reused ? 1 : 0;
}

extern "C" int hsk_build_partition(hsk_ctx* k, const hsk_clearance_params* cparams, const hsk_partition_params* params, hsk_room* recs, size_t cap,
                                   size_t* n_rooms, hsk_partition_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  hsk_clearance_params cp;
  ClearGeom cq;
  hsk_partition_params p;
  if (recs && !n_rooms) return fail(k, HSK_ERR_ARG, "hsk_build_partition: n_rooms is null");
  if (int rc = clear_check(k, cparams, "hsk_build_partition", &cp, &cq)) return rc;
  if (int rc = part_check(k, cp, params, "hsk_build_partition", &p)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_build_partition")) return rc;
  uint32_t key[9];
  clear_key_of(cp, key);
  key[5] = p.core_d2;
  key[6] = p.min_d2;
  key[7] = p.min_core_voxels;
  key[8] = p.max_cost;
  const bool held = k->part.stands_for(k, key, sizeof(key));
  if (!held) {
    HIPCHK(k, hipSetDevice(k->cfg.device_id));
    k->part.drop();
    bool clear_reused = false;
    int r = clear_build(k, cp, cq, &clear_reused);
    if (r != HSK_OK) return r;
    PartGeom q;
    part_geom(cq.X, cq.Y, cq.Z, cq.w, p.core_d2, p.min_d2, p.min_core_voxels, p.max_cost, &q);
    r = k->part.grow(k, part_layout(q, nullptr, nullptr));
    if (r != HSK_OK) return r;
    PartBufs b;
    part_layout(q, k->part.buf, &b);
    ClearBufs cb;
    clear_layout(k->vp, k->clear.buf, &cb);
    PartResult res;
    r = part_run(k, cb.field, q, b, &res);
    if (r != HSK_OK) return r;
    if (res.too_many) {
      if (stats) part_fill_stats(stats, res, k->part.bytes + k->part.tab_bytes, false);
      return fail(k, HSK_ERR_ARG, "hsk_build_partition: more than HSK_PARTITION_MAX_ROOMS cores are kept (raise core_d2 or min_core_voxels)");
    }
    memcpy(k->part_counts, res.counts, sizeof(res.counts));
    k->part_recs.swap(res.recs);
    k->part_doors.swap(res.doors);
    k->part_q = q;
    k->part_rounds = res.rounds;
    k->part_tiles = res.tiles;
    k->part_first = res.first;
    k->part.stamp(k, key, sizeof(key));
  }
  size_t n_unasked;  // (recs null and n_rooms null: a call for the stats alone)
  if (int rc = reply_records(k, k->part_recs, recs, cap, n_rooms ? n_rooms : &n_unasked,
                             "hsk_build_partition: cap is smaller than the number of rooms (*n_rooms: the count)"))
    return rc;
  if (stats) {
    PartResult res;
    memcpy(res.counts, k->part_counts, sizeof(res.counts));
    res.rounds = k->part_rounds;
    res.doors.resize(k->part_doors.size());
    part_fill_stats(stats, res, k->part.bytes + k->part.tab_bytes, held);
  }
  return HSK_OK;
}

// the reads: a partition must be held
static int part_held(hsk_ctx* k, const char* who) {
  if (int rc = volume_state_check(k, k, who)) return rc;
  return k->part.require(k, who, ": no partition of the volume as it stands is held (hsk_build_partition makes one)");
}

extern "C" int hsk_partition_doors(hsk_ctx* k, hsk_door* doors, size_t cap, size_t* n_doors) {
  if (!k) return HSK_ERR_ARG;
  if (!n_doors) return fail(k, HSK_ERR_ARG, "hsk_partition_doors: n_doors is null");
  if (int rc = part_held(k, "hsk_partition_doors")) return rc;
  return reply_records(k, k->part_doors, doors, cap, n_doors, "hsk_partition_doors: cap is smaller than the number of doors (*n_doors: the count)");
}

static int part_download(hsk_ctx* k, const hsk_voxel_box* box, uint32_t* out, bool cost, const char* who) {
  if (!k) return HSK_ERR_ARG;
  if (!out) return fail(k, HSK_ERR_ARG, (std::string(who) + ": the output is null").c_str());
  hsk_voxel_box b;
  size_t n;
  if (int rc = clear_box_check(k, box, who, &b, &n)) return rc;
  if (int rc = part_held(k, who)) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  PartBufs pb;
  part_layout(k->part_q, k->part.buf, &pb);
  if (n == 0) return HSK_OK;
  int r = ensure_product_bytes(k, n * 4);
  if (r != HSK_OK) return r;
  launch_part_box(k->stream, k->part_q, pb, (unsigned)k->part_recs.size(), b.lo, b.hi, cost, (unsigned*)k->d_out);
  HIPCHK(k, hipGetLastError());
  return copy_out(k, out, k->d_out, n * 4);
}

extern "C" int hsk_download_partition(hsk_ctx* k, const hsk_voxel_box* box, uint32_t* ids) {
  return part_download(k, box, ids, false, "hsk_download_partition");
}

extern "C" int hsk_download_partition_cost(hsk_ctx* k, const hsk_voxel_box* box, uint32_t* g) {
  return part_download(k, box, g, true, "hsk_download_partition_cost");
}

extern "C" int hsk_partition_at(hsk_ctx* k, const float* xyz, size_t n, int radius, uint32_t* ids) {
  if (!k) return HSK_ERR_ARG;
  static_assert(HSK_PARTITION_MAX_RADIUS == 4, "the radius refusal names 4");
  if (int rc = points_check(k, "hsk_partition_at", xyz, ids, n, radius, HSK_PARTITION_MAX_RADIUS)) return rc;
  if (int rc = part_held(k, "hsk_partition_at")) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  PartBufs pb;
  part_layout(k->part_q, k->part.buf, &pb);
  return gather_points(k, xyz, n, ids, [&](const float* pts, unsigned* out, unsigned char*) {
    launch_part_gather(k->stream, k->part_q, pb, (unsigned)k->part_recs.size(), k->vp, pts, (unsigned)n, radius, out);
  });
}

extern "C" int hsk_partition_floor(hsk_ctx* k, const hsk_clearance_params* cparams, int axis, int lo, int hi, const hsk_partition_params* params,
                                   uint32_t* map, hsk_room* recs, size_t rec_cap, size_t* n_rooms, hsk_door* doors, size_t door_cap, size_t* n_doors,
                                   hsk_partition_stats* stats) {
  if (!k) return HSK_ERR_ARG;
  if (!map) return fail(k, HSK_ERR_ARG, "hsk_partition_floor: map is null");
  if ((recs && !n_rooms) || (doors && !n_doors)) return fail(k, HSK_ERR_ARG, "hsk_partition_floor: records without a place for their count");
  hsk_clearance_params cp;
  ClearGeom cq;
  hsk_partition_params p;
  if (int rc = clear_check(k, cparams, "hsk_partition_floor", &cp, &cq)) return rc;
  if (int rc = part_check(k, cp, params, "hsk_partition_floor", &p)) return rc;
  FloorGrid f;
  if (int rc = clear_floor_grid(k, cq, axis, lo, hi, "hsk_partition_floor", &f)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_partition_floor")) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  // the map's grid: (u, v, 1), u the lower-numbered remaining axis; the same kernels, on which nothing ever crosses the third axis
  // (its neighbours lie outside the grid): the cores are 4-connected, the moves the 8 in-plane ones
  PartGeom q;
  part_geom(f.nu, f.nv, 1u, f.w, p.core_d2, p.min_d2, p.min_core_voxels, p.max_cost, &q);
  const size_t n = (size_t)f.nu * f.nv;
  ProductLayout lay;
  const size_t a_at = lay.take(n * 4), b_at = lay.take(n * 4), ids_at = lay.take(n * 4);
  const size_t part_at = lay.take(part_layout(q, nullptr, nullptr));
  int r = ensure_product_bytes(k, lay.bytes);
  if (r != HSK_OK) return r;
  char* base = (char*)k->d_out;
  launch_clear_floor(k->stream, k->d_vol, k->vp, cq, axis, lo, hi, (unsigned*)(base + a_at), (unsigned*)(base + b_at));
  HIPCHK(k, hipGetLastError());
  PartBufs pb;
  part_layout(q, base + part_at, &pb);
  PartResult res;
  r = part_run(k, (const unsigned*)(base + a_at), q, pb, &res);
  if (r != HSK_OK) return r;
  if (res.too_many) {
    if (stats) part_fill_stats(stats, res, lay.bytes, false);
    return fail(k, HSK_ERR_ARG, "hsk_partition_floor: more than HSK_PARTITION_MAX_ROOMS cores are kept (raise core_d2 or min_core_voxels)");
  }
  if ((recs && rec_cap < res.recs.size()) || (doors && door_cap < res.doors.size())) {
    if (n_rooms) *n_rooms = res.recs.size();
    if (n_doors) *n_doors = res.doors.size();
    return fail(k, HSK_ERR_ARG, "hsk_partition_floor: a cap is smaller than the number of records (*n_rooms, *n_doors: the counts)");
  }
  const int blo[3] = {0, 0, 0}, bhi[3] = {(int)f.nu, (int)f.nv, 1};
  launch_part_box(k->stream, q, pb, (unsigned)res.recs.size(), blo, bhi, false, (unsigned*)(base + ids_at));
  HIPCHK(k, hipGetLastError());
  r = copy_out(k, map, base + ids_at, n * 4);
  if (r != HSK_OK) return r;
  if (recs && !res.recs.empty()) memcpy(recs, res.recs.data(), res.recs.size() * sizeof(hsk_room));
  if (doors && !res.doors.empty()) memcpy(doors, res.doors.data(), res.doors.size() * sizeof(hsk_door));
  if (n_rooms) *n_rooms = res.recs.size();
  if (n_doors) *n_doors = res.doors.size();
  if (stats) part_fill_stats(stats, res, lay.bytes + k->part.tab_bytes, false);
  return HSK_OK;
}

extern "C" int hsk_release_partition(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const int r = k->part.release(k);
  k->part_recs.clear();
  k->part_doors.clear();
  return r;
}

extern "C" int hsk_partition_tiles_relaxed(const hsk_ctx* k, uint64_t* tiles_relaxed, uint64_t* first_tiles, uint64_t* tiles) {
  if (!k) return HSK_ERR_ARG;
  if (tiles_relaxed) *tiles_relaxed = k->part_tiles;
  if (first_tiles) *first_tiles = k->part_first;
  if (tiles) *tiles = (uint64_t)k->part_q.ntx * k->part_q.nty * k->part_q.ntz;
  return HSK_OK;
}
