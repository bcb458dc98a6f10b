// api_simplify.hip -- the C ABI's simplified mesh (include/hskinfu.h "Simplified mesh"; DESIGN.md 3.17 the kernels, 8k the rule):
// hsk_default_simplify_params, hsk_extract_mesh_simplified and hsk_cluster_vertex, the host mirror of the device solve (the same
// text, hsk_simplify_point.h).  The read-out stands on the indexed mesh's count pass (api_readout.hip: kind 4 of the count
// cache, asked for through hsk_extract_mesh_indexed's own counts-only call, so whichever of the two products asks first pays for
// it and everything that voids it there voids it here).  Its own count pass is kept while vol_epoch and the cluster size stand (a
// size query followed by the fill counts once); the gather, the solve and the faces' write pass run on every call that has an
// output vertex -- the statistics come from the solve.  It reads the volume as it stands, with no flush of the deferred weights,
// and writes nothing but its own scratch and the product buffer.
#pragma clang fp contract(off)
#include <cmath>

#include "hsk_ctx.h"
#include "hsk_simplify_point.h"

extern "C" void hsk_default_simplify_params(const hsk_ctx* k, hsk_simplify_params* p) {
  (void)k;  // (the defaults do not depend on the volume; the argument is there for the day they do)
  if (!p) return;
  p->cluster_voxels = 4;
  p->mode = HSK_SIMPLIFY_QUADRIC;
  p->sv_floor = 1.0e-3f;
}

// params (null: the defaults) with its zeros replaced by the defaults, checked; the message, or null when it is fine
static const char* simplify_params(const hsk_simplify_params* params, hsk_simplify_params* p) {
  hsk_default_simplify_params(nullptr, p);
  if (params) {
    if (params->cluster_voxels != 0) p->cluster_voxels = params->cluster_voxels;
    p->mode = params->mode;
    if (params->sv_floor != 0.0f) p->sv_floor = params->sv_floor;
  }
  if (simp_shift(p->cluster_voxels) < 0) return "cluster_voxels is none of 2, 4, 8, 16 (0: the default, 4)";
  if (p->mode != HSK_SIMPLIFY_QUADRIC && p->mode != HSK_SIMPLIFY_MEAN) return "mode is neither HSK_SIMPLIFY_QUADRIC nor HSK_SIMPLIFY_MEAN";
  if (!(std::isfinite(p->sv_floor) && p->sv_floor > 0.0f && p->sv_floor < 1.0f)) return "sv_floor must be finite and lie in [0, 1) (0: the default, 1e-3)";
  return nullptr;
}

extern "C" int hsk_cluster_vertex(const int64_t sums[16], int cluster_voxels, int mode, float sv_floor, double xyz_voxels[3], int* rank,
                                  int* clamped) {
  static_assert(sizeof(int64_t) == sizeof(simp_i64), "the sums are 64-bit");
  if (!sums || !xyz_voxels || !rank || !clamped) return HSK_ERR_ARG;
  hsk_simplify_params in{cluster_voxels, mode, sv_floor}, p;
  if (simplify_params(&in, &p)) return HSK_ERR_ARG;
  if (sums[0] <= 0) return HSK_ERR_ARG;  // (a cluster without a vertex has no mean)
  simp_i64 s[SIMP_SUMS];
  for (int i = 0; i < SIMP_SUMS; ++i) s[i] = (simp_i64)sums[i];
  double x[3];
  simp_vertex(s, p.cluster_voxels, p.mode, (double)p.sv_floor, x, rank, clamped);
  for (int i = 0; i < 3; ++i) xyz_voxels[i] = x[i] / (double)SIMP_UNIT;
  return HSK_OK;
}

extern "C" int hsk_extract_mesh_simplified(hsk_ctx* k, const hsk_simplify_params* params, float* vertices, float* normals, uint8_t* rgb,
                                           size_t cap_vertices, size_t* n_vertices, int32_t* faces, size_t cap_faces, size_t* n_faces,
                                           hsk_simplify_stats* stats) {
  static_assert(sizeof(hsk_simplify_params) == 12 && sizeof(hsk_simplify_stats) == 96, "the simplified mesh's structs");
  if (!k || !n_vertices || !n_faces) return HSK_ERR_ARG;
  hsk_simplify_params p;
  if (const char* why = simplify_params(params, &p)) return fail(k, HSK_ERR_ARG, (std::string("hsk_extract_mesh_simplified: ") + why).c_str());
  if (int rs = require_whole_volume(k, k, "hsk_extract_mesh_simplified", "clusters would straddle the slabs")) return rs;
  if (rgb && require_color(k)) return HSK_ERR_STATE;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  hsk_simplify_stats st;
  memset(&st, 0, sizeof(st));
  // the indexed mesh's count pass: found in place when nothing has touched the volume since it was last made
  size_t nv_in = 0, nf_in = 0;
  int r = hsk_extract_mesh_indexed(k, nullptr, nullptr, nullptr, 0, &nv_in, nullptr, 0, &nf_in, nullptr);
  if (r != HSK_OK) return r;
  st.n_in_vertices = nv_in;
  st.n_in_faces = nf_in;
  MeshIndexBufs mb;
  (void)mesh_index_layout(k->vp, k->mi.buf, &mb);
  const int s = simp_shift(p.cluster_voxels);
  r = k->simp.grow(k, simp_layout(k->vp, s, nullptr, nullptr));
  if (r != HSK_OK) return r;
  SimpBufs sb;
  (void)simp_layout(k->vp, s, k->simp.buf, &sb);
  // the clustering's own count pass: found in place when the last call counted this volume at this cluster size (the indexed
  // mesh's pass it stands on is a function of the volume alone, so vol_epoch covers it whoever made it again meanwhile)
  if (!k->simp.stands_for(k, &s, sizeof(s))) {
    k->simp.drop();
    launch_simp_count(k->stream, k->d_vol, k->vp, k->d_cube_tab, k->d_rowcnt, mb, sb);
    HIPCHK(k, hipGetLastError());
    r = read_u64(k, k->simp_totals, sb.totals, 3);
    if (r != HSK_OK) return r;
    k->simp.stamp(k, &s, sizeof(s));
  }
  const unsigned long long* totals = k->simp_totals;
  const size_t nf = (size_t)totals[0], nv = (size_t)totals[1];
  st.n_out_faces = nf;
  st.n_out_vertices = nv;
  st.n_clusters = totals[2];
  st.n_faces_collapsed = nf_in - nf;
  *n_vertices = nv;
  *n_faces = nf;
  if (stats) *stats = st;
  const bool want_v = vertices || normals || rgb;
  if ((want_v && cap_vertices < nv) || (faces && cap_faces < nf))
    return fail(k, HSK_ERR_ARG, "hsk_extract_mesh_simplified: a capacity below the total (the arrays are written whole or not at all)");
  if (nv == 0) return HSK_OK;  // (no face survives: nothing to solve, nothing to write)
  // what is proportional to the output: the clusters' numbers, then their sums
  ProductLayout scratch;
  const size_t list_at = scratch.take(nv * 4), sums_at = scratch.take(nv * SIMP_REC * 8);
  r = k->simp.grow_tab(k, scratch.bytes + (scratch.bytes >> 2));
  if (r != HSK_OK) return r;
  ProductArrays out;  // (an array that is not asked for takes no space)
  const int a_xyz = out.add(vertices, nv * 12), a_nrm = out.add(normals, nv * 12), a_rgb = out.add(rgb, nv * 3), a_fc = out.add(faces, nf * 12);
  r = out.place(k);
  if (r != HSK_OK) return r;
  launch_simp_write(k->stream, k->d_vol, rgb ? k->d_color : nullptr, k->vp, k->d_cube_tab, k->d_rowcnt, mb, sb, (unsigned)nv,
                    (unsigned*)((char*)k->simp.tab + list_at), (long long*)((char*)k->simp.tab + sums_at), p.mode, (double)p.sv_floor,
                    out.dev<float>(a_xyz), out.dev<float>(a_nrm), out.dev<unsigned char>(a_rgb), out.dev<int>(a_fc));
  HIPCHK(k, hipGetLastError());
  r = out.copy_out(k);
  if (r != HSK_OK) return r;
  unsigned long long counts[6];
  r = read_u64(k, counts, sb.totals + 4, 6);
  if (r != HSK_OK) return r;
  for (int i = 0; i < 4; ++i) st.n_rank[i] = counts[i];
  st.n_clamped = counts[4];
  st.n_uncolored = counts[5];
  if (stats) *stats = st;
  return HSK_OK;
}
