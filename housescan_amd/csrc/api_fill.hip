// api_fill.hip -- the C ABI's hole filling (include/hskinfu.h "Hole filling"; DESIGN.md 3.22 the kernels, 8p the rule):
// hsk_default_fill_params, hsk_fill_holes, hsk_download_fill_mask.  The iterations read the volume as it stands, with NO flush of
// the deferred weights (as the labelling, api_components.hip): the rule asks of a weight only whether it is zero.  The write
// follows hsk_prune_components' order: the state check, the rounds, then -- only when something will be written -- flush the
// deferred weights, write, volume_replaced, synchronise.  The mask stays on the device (fill, a HeldPass) while vol_epoch stands.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>

#include "hsk_ctx.h"
#include "hsk_fill_point.h"

extern "C" void hsk_default_fill_params(const hsk_ctx* k, hsk_fill_params* p) {
  if (!p) return;
  float cell[3];
  context_cells(k, cell, nullptr);
  memset(p, 0, sizeof(*p));
  // the voxels of 15 cm along the finest axis, in binary64 from the binary32 cells: the fronts from a gap's two rims meet
  const double m = (double)std::min(cell[0], std::min(cell[1], cell[2]));
  const double it = std::ceil(0.15 / m);
  p->iterations = !(it >= 1.0) ? 1 : it > 255.0 ? 255 : (int32_t)it;
  p->keep = HSK_FILL_SURFACE;
  p->band = 2;
  p->fill_weight = 1;
}

extern "C" int hsk_fill_holes(hsk_ctx* k, const hsk_fill_params* params, const hsk_voxel_box* box, hsk_fill_stats* stats) {
  static_assert(sizeof(hsk_fill_params) == 16 && sizeof(hsk_fill_stats) == 48, "the fill structs");
  if (!k) return HSK_ERR_ARG;
  hsk_fill_params p;
  if (params)
    p = *params;
  else
    hsk_default_fill_params(k, &p);
  if (p.iterations < 1 || p.iterations > 255) return fail(k, HSK_ERR_ARG, "hsk_fill_holes: iterations must lie in 1..255");
  if (p.keep != HSK_FILL_SURFACE && p.keep != HSK_FILL_ALL) return fail(k, HSK_ERR_ARG, "hsk_fill_holes: keep is neither HSK_FILL_SURFACE nor HSK_FILL_ALL");
  if (p.band < 0 || p.band > 8) return fail(k, HSK_ERR_ARG, "hsk_fill_holes: band must lie in 0..8");
  if (p.fill_weight < 1 || p.fill_weight > 128) return fail(k, HSK_ERR_ARG, "hsk_fill_holes: fill_weight must lie in 1..128");
  hsk_voxel_box b;
  size_t n_box;
  if (int rc = clear_box_check(k, box, "hsk_fill_holes", &b, &n_box)) return rc;
  if (int rc = volume_state_check(k, k, "hsk_fill_holes")) return rc;  // (prune's refusals: in flight, a slab, more than 2^31 voxels)
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  k->fill.drop();  // (the scratch is about to be written: the mask of an earlier fill goes)
  int r = k->fill.grow(k, fill_layout(k->vp, nullptr, nullptr));
  if (r != HSK_OK) return r;
  FillBufs fb;
  fill_layout(k->vp, k->fill.buf, &fb);
  launch_fill_init(k->stream, k->d_vol, k->vp, b.lo, b.hi, fb);
  // every iteration is enqueued: one that has nothing to do costs a launch whose workgroups read a few bytes and leave (fill.hip),
  // and the host learns iterations_run from the iterations' counters without a synchronisation between them
  for (int it = 1; it <= p.iterations; ++it) launch_fill_round(k->stream, k->vp, fb, it);
  const int fin = p.iterations & 1;
  if (p.keep == HSK_FILL_SURFACE) launch_fill_keep(k->stream, k->vp, fb, fin, p.band);
  launch_fill_count(k->stream, k->d_vol, k->vp, b.lo, b.hi, fb, fin, p.keep == HSK_FILL_ALL);
  HIPCHK(k, hipGetLastError());
  unsigned counts[FILL_COUNTS + 256];
  r = copy_out(k, counts, fb.counts, sizeof(counts));
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  hsk_fill_stats st;
  memset(&st, 0, sizeof(st));
  st.n_unseen = counts[0];
  st.n_reached = counts[1];
  st.n_written = counts[2];
  st.n_written_negative = counts[3];
  st.tile_visits = counts[4];
  st.iterations_run = p.iterations;
  for (int it = 1; it <= p.iterations; ++it)
    if (counts[FILL_COUNTS + it] == 0u) {
      st.iterations_run = it;
      break;
    }
  if (st.n_written > 0) {
    r = commit_volume_write(k, [&] { launch_fill_commit(k->stream, k->d_vol, k->vp, fb, fin, p.fill_weight); });
    if (r != HSK_OK) return r;
  }  // (else nothing is written, vol_epoch does not move: cached passes stay valid)
  k->fill_mask = fill_mask_bytes(k->vp, fb, fin);
  k->fill.stamp(k);
  if (stats) *stats = st;
  return HSK_OK;
}

extern "C" int hsk_download_fill_mask(hsk_ctx* k, const hsk_voxel_box* box, uint8_t* mask) {
  if (!k) return HSK_ERR_ARG;
  hsk_voxel_box b;
  size_t n;
  if (int rc = clear_box_check(k, box, "hsk_download_fill_mask", &b, &n)) return rc;
  if (n > 0 && !mask) return fail(k, HSK_ERR_ARG, "hsk_download_fill_mask: mask is null");
  if (int rc = volume_state_check(k, k, "hsk_download_fill_mask")) return rc;
  if (int rc = k->fill.require(k, "hsk_download_fill_mask", ": no fill is held for the volume as it stands")) return rc;
  if (n == 0) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  return download_rows(k, k->fill_mask, 1, b, n, mask);
}
