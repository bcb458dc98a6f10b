// hskinfu_api.hip -- the core of the C ABI (include/hskinfu.h) over the gfx950 kernels: the context (create, destroy, reset) and
// its device memory layout, the tracker state machine of SURVEY.md A.2 with its hipGraph replay, the pipelined ring and the
// recorded-stream feed, the stage-level entry points, colour's switch and RGB-D submissions, profiling, the z-slab building
// blocks.  What reaches the caller is api_readout.hip's, what replaces or serialises the volume api_volume.hip's (hsk_ctx.h).
// Host-side restatement of the role the external PCL KinFu app plays for HouseScan
// (/root/reference/README.md:13-14); the depth-frame type is HoniHelper.hs:20's (Vector Word16,(w,h)).
#pragma clang fp contract(off)
#include <sched.h>

#include <chrono>
#include <cmath>
#include <cstdlib>

#include "hsk_ctx.h"

#include "build/build_id.h"
extern "C" const char* hsk_build_id(void) { return HSK_BUILD_ID; }

std::string& create_error() {
  static thread_local std::string err;
  return err;
}

int fail(hsk_ctx* k, int code, const char* msg) {
  if (k) k->err = msg;
  return code;
}
int require_idle(const hsk_ctx* k, hsk_ctx* errs) {
  return k->ring_count > 0 ? fail(errs, HSK_ERR_STATE, "frames are in flight: collect them with hsk_wait_frame first") : HSK_OK;
}
int require_color(hsk_ctx* k) { return k->d_color ? HSK_OK : fail(k, HSK_ERR_STATE, "colour is not enabled (hsk_enable_color)"); }
int require_whole_volume(const hsk_ctx* k, hsk_ctx* errs, const char* who, const char* sentence) {
  if (!k->group_slab && k->vp.zs0 == 0 && k->vp.nzs == k->vp.Z && k->vp.zo0 == 0 && k->vp.zo1 == k->vp.Z) return HSK_OK;
  return fail(errs, HSK_ERR_STATE, (std::string(who) + ": not for a slab (" + sentence + ")").c_str());
}

void pose16_to_rt(const float m[16], float R[9], float t[3]) {
  for (int i = 0; i < 3; ++i) {
    R[i * 3] = m[i * 4];
    R[i * 3 + 1] = m[i * 4 + 1];
    R[i * 3 + 2] = m[i * 4 + 2];
    t[i] = m[i * 4 + 3];
  }
}
void rt_to_pose16(const float R[9], const float t[3], float m[16]) {
  for (int i = 0; i < 3; ++i) {
    m[i * 4] = R[i * 3];
    m[i * 4 + 1] = R[i * 3 + 1];
    m[i * 4 + 2] = R[i * 3 + 2];
    m[i * 4 + 3] = t[i];
  }
  m[12] = m[13] = m[14] = 0.0f;
  m[15] = 1.0f;
}

extern "C" void hsk_default_config(hsk_config* c, int n) {
  memset(c, 0, sizeof(*c));
  c->vol_x = c->vol_y = c->vol_z = n;
  c->vol_size_m[0] = c->vol_size_m[1] = c->vol_size_m[2] = 3.0f;
  c->trunc_dist_m = 0.03f;
  c->width = 640;
  c->height = 480;
  c->fx = c->fy = 525.0f;
  c->cx = 319.5f;
  c->cy = 239.5f;
  c->icp_iters[0] = 10;
  c->icp_iters[1] = 5;
  c->icp_iters[2] = 4;
  c->icp_dist_thresh_m = 0.10f;
  c->icp_angle_thresh_sin = 0.3420201433256687f;
  c->integrate_move_thresh = 0.0f;
  float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  float t[3] = {c->vol_size_m[0] / 2.0f, c->vol_size_m[1] / 2.0f, c->vol_size_m[2] / 2.0f - 1.2f * c->vol_size_m[2] / 2.0f};
  rt_to_pose16(R, t, c->init_pose);
  c->device_id = 0;
  c->own_z0 = 0;
  c->own_z1 = n;
  c->halo = 0;
  c->use_graph = 0;
}

extern "C" int hsk_bilateral_tables(float ws[169], float wc[512]) {
  const float sig_s = 4.5f, sig_c = 30.0f;
  const float s2 = 0.5f / (sig_s * sig_s);
  const float c2 = 0.5f / (sig_c * sig_c);
  for (int dy = -6; dy <= 6; ++dy)
    for (int dx = -6; dx <= 6; ++dx) {
      const float arg = (float)(dx * dx + dy * dy) * s2;
      ws[(dy + 6) * 13 + (dx + 6)] = (float)std::exp(-(double)arg);
    }
  for (int k = 0; k < 512; ++k) {
    const float arg = (float)(k * k) * c2;
    wc[k] = (float)std::exp(-(double)arg);
  }
  return HSK_OK;
}

static void free_all(hsk_ctx* k) {
  if (!k) return;
  (void)hipSetDevice(k->cfg.device_id);
  if (k->gexec) (void)hipGraphExecDestroy(k->gexec);
  if (k->graph) (void)hipGraphDestroy(k->graph);
  for (auto& g : k->pgexec)
    if (g) (void)hipGraphExecDestroy(g);
  for (auto& g : k->pgraph)
    if (g) (void)hipGraphDestroy(g);
  for (auto& g : k->sgexec)
    if (g) (void)hipGraphExecDestroy(g);
  for (auto& g : k->sgraph)
    if (g) (void)hipGraphDestroy(g);
  for (auto& e : k->ev_pre)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : k->ev_free)
    if (e) (void)hipEventDestroy(e);
  if (k->ev_src) (void)hipEventDestroy(k->ev_src);
  if (k->pstream) (void)hipStreamDestroy(k->pstream);
  auto F = [](void* p) {
    if (p) (void)hipFree(p);
  };
  F(k->d_vol);
  for (auto& b : k->ib) {
    F(b.d_raw);
    F(b.d_scaled);
    F(b.d_tmax);
    for (int l = 0; l < HSK_NLEVELS; ++l) {
      F(b.d_dep[l]);
      F(b.d_vcur[l]);
      F(b.d_ncur[l]);
    }
  }
  for (int l = 0; l < HSK_NLEVELS; ++l) {
    F(k->d_vmod[l]);
    F(k->d_nmod[l]);
  }
  F(k->d_st);
  F(k->d_partials);
  F(k->d_icp_pose);
  F(k->d_sums);
  F(k->d_wc);
  F(k->d_keys);
  F(k->d_flags);
  F(k->d_uni);
  F(k->d_zint);
  F(k->d_queue);
  F(k->d_cube_tab);
  F(k->d_counter);
  F(k->d_rowcnt);
  F(k->d_rowoff);
  F(k->d_out);
  F(k->d_color);
  F(k->d_has_color);
  F(k->d_view);
  F(k->d_fuse);
  F(k->d_align);
  for (HeldPass* p : k->passes) {
    F(p->buf);
    F(p->tab);
  }
  F(k->d_key);
  if (k->h_align) (void)hipHostFree(k->h_align);
  if (k->h_view) (void)hipHostFree(k->h_view);
  for (auto& b : k->ib) F(b.d_rgb);
  if (k->h_rgb_stage) (void)hipHostFree(k->h_rgb_stage);
  for (auto& p : k->h_pin)
    if (p) (void)hipHostFree(p);
  for (auto& e : k->ev_pin)
    if (e) (void)hipEventDestroy(e);
  if (k->h_st) (void)hipHostFree(k->h_st);
  if (k->h_stage) (void)hipHostFree(k->h_stage);
  if (k->h_ring) (void)hipHostFree(k->h_ring);
  if (k->h_slot_fifo) (void)hipHostFree(k->h_slot_fifo);
  if (k->d_ring_seq) (void)hipFree(k->d_ring_seq);
  for (auto& e : k->ring_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : k->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : k->ev_icp)
    if (e) (void)hipEventDestroy(e);
  if (k->own_stream && k->stream) (void)hipStreamDestroy(k->stream);
}

// The weights of deep free space live in the lane-block summaries until somebody reads the volume: bring the volume's
// copies up to date (k_summaries<true>), once -- a second read-out with no integrate in between finds them current.
void flush_weights(hsk_ctx* k) {
  if (!k->weights_pending) return;
  launch_materialize(k->stream, k->d_vol, k->vp, k->d_uni);
  k->weights_pending = false;
}

int upload_state(hsk_ctx* k) {
  HIPCHK(k, hipMemcpyAsync(k->d_st, k->h_st, sizeof(TrackState), hipMemcpyHostToDevice, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}
int download_state(hsk_ctx* k) {
  HIPCHK(k, hipMemcpyAsync(k->h_st, k->d_st, sizeof(TrackState), hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}

static int do_reset(hsk_ctx* k) {
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  HIPCHK(k, hipMemsetAsync(k->d_vol, 0, k->vol_bytes, k->stream));
  HIPCHK(k, hipMemsetAsync(k->d_flags, 0, k->flags_bytes, k->stream));
  HIPCHK(k, hipMemsetAsync(k->d_uni, 1, uniform_lane_bytes(k->vp), k->stream));  // 1: "all 16 voxels never observed"
  // ... and the coarse level behind them: 0, "nothing pending, nothing known" (a never-observed block is not quiet)
  HIPCHK(k, hipMemsetAsync(k->d_uni + uniform_lane_bytes(k->vp), 0, k->uni_bytes - uniform_lane_bytes(k->vp), k->stream));
  if (k->d_color) HIPCHK(k, hipMemsetAsync(k->d_color, 0, k->color_bytes, k->stream));  // (the colour goes with the TSDF)
  memset(k->h_st, 0, sizeof(TrackState));
  memcpy(k->h_st->R, k->init_R, sizeof(k->init_R));
  memcpy(k->h_st->t, k->init_t, sizeof(k->init_t));
  memcpy(k->h_st->Rp, k->init_R, sizeof(k->init_R));
  memcpy(k->h_st->tp, k->init_t, sizeof(k->init_t));
  k->frame = 0;
  k->vol_epoch += 1;
  k->pending_reset = false;
  return upload_state(k);
}

// A frame lost tracking: the one place that says what becomes of the scan.  HSK_LOSS_RESET restarts it (do_reset).
// HSK_LOSS_HOLD keeps everything and puts the tracker back where the last tracked frame left it: every frame path starts a
// frame with previous pose <- pose (k_icp_iter's first iteration, k_begin_frame) and a dropped frame leaves the state alone, so
// (Rp, tp) is the last tracked pose whatever the path left in (R, t); the sticky flags are cleared as hsk_resume_scan clears
// them.  The volume, the colour, the summaries, the brick flags, the model maps and the frame count are not touched.
static int after_loss(hsk_ctx* k) {
  if (k->loss_policy != HSK_LOSS_HOLD) return do_reset(k);
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  int r = download_state(k);
  if (r != HSK_OK) return r;
  memcpy(k->h_st->R, k->h_st->Rp, sizeof(k->h_st->R));
  memcpy(k->h_st->t, k->h_st->tp, sizeof(k->h_st->t));
  k->h_st->lost = 0;
  k->h_st->need_reset = 0;
  k->pending_reset = false;
  return upload_state(k);
}

extern "C" int hsk_set_loss_policy(hsk_ctx* k, int policy) {
  if (!k) return HSK_ERR_ARG;
  if (policy != HSK_LOSS_RESET && policy != HSK_LOSS_HOLD) return fail(k, HSK_ERR_ARG, "hsk_set_loss_policy: unknown policy");
  if (k->group_slab) return fail(k, HSK_ERR_STATE, "hsk_set_loss_policy: not for a slab (a group handles a loss itself)");
  if (int ri = require_idle(k)) return ri;
  k->loss_policy = policy;
  return HSK_OK;
}
extern "C" int hsk_get_loss_policy(const hsk_ctx* k) { return k ? k->loss_policy : -1; }

extern "C" int hsk_create(const hsk_config* c, hsk_ctx** out) {
  if (!c || !out) {
    create_error() = "hsk_create: null argument";
    return HSK_ERR_ARG;
  }
  *out = nullptr;
  if (c->vol_x <= 0 || c->vol_y <= 0 || c->vol_z <= 0 || (c->vol_x % 8) != 0 || (c->vol_y % 8) != 0 || c->width <= 0 || c->height <= 0 ||
      (c->width % 4) != 0 || (c->height % 4) != 0 || c->own_z0 < 0 || c->own_z1 > c->vol_z || c->own_z0 >= c->own_z1 ||
      c->halo < 0) {
    create_error() = "hsk_create: invalid configuration (vol_x, vol_y must be multiples of 8, image dims of 4; 0 <= own_z0 < own_z1 <= vol_z)";
    return HSK_ERR_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    create_error() = "hsk_create: no HIP device available (this library has no CPU fallback)";
    return HSK_ERR_NOGPU;
  }
  if (c->device_id < 0 || c->device_id >= ndev) {
    create_error() = "hsk_create: device_id out of range";
    return HSK_ERR_ARG;
  }
  {
    // The march kernels (raycast, views, sections) stage the whole brick bitfield in dynamic LDS.  What a block of this device may
    // ask for is the runtime's figure, read here; none of the kernels is opted in to more than HSK_MARCH_LDS_MAX (hsk_dev.h), so
    // the smaller of the two is the limit.  A volume whose X or Y stops the brick edge from growing (hsk_choose_bshift: 648^3
    // stays at 8^3 bricks, 66560 B) would be created fine and its first raycast could not be relied on: refuse it here,
    // before anything is allocated, with the remedy.
    VolParams g{};
    g.X = c->vol_x;
    g.Y = c->vol_y;
    const int zs0 = c->own_z0 - c->halo < 0 ? 0 : c->own_z0 - c->halo;
    g.nzs = (c->own_z1 + c->halo > c->vol_z ? c->vol_z : c->own_z1 + c->halo) - zs0;
    g.bshift = hsk_choose_bshift(g);
    int lds_block = 0;
    if (hipDeviceGetAttribute(&lds_block, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device_id) != hipSuccess || lds_block <= 0) {
      (void)hipGetLastError();
      create_error() = "hsk_create: the device does not report the shared memory of a block";
      return HSK_ERR_HIP;
    }
    const size_t lds_max = (size_t)lds_block < (size_t)HSK_MARCH_LDS_MAX ? (size_t)lds_block : (size_t)HSK_MARCH_LDS_MAX;
    const size_t staged = (size_t)hsk_flag_words_total(g) * 4;
    if (staged > lds_max) {
      create_error() = "hsk_create: the brick bitfield of this volume (" + std::to_string(staged) + " B) does not fit the " + std::to_string(lds_max) +
                       " B of LDS the raycast may stage it in (the device gives a block " + std::to_string(lds_block) +
                       " B): make vol_x and vol_y multiples of 16, or the next power of two";
      return HSK_ERR_ARG;
    }
  }
  hsk_ctx* k = new hsk_ctx();
  k->cfg = *c;
  auto bail = [&](int code) {
    create_error() = k->err;
    free_all(k);
    delete k;
    return code;
  };
#define CK(call)                                   \
  do {                                             \
    int r_ = [&]() -> int {                        \
      HIPCHK(k, call);                             \
      return HSK_OK;                               \
    }();                                           \
    if (r_ != HSK_OK) return bail(r_);             \
  } while (0)
  CK(hipSetDevice(c->device_id));
  CK(hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking));
  k->own_stream = true;
  // geometry
  VolParams& vp = k->vp;
  vp.X = c->vol_x;
  vp.Y = c->vol_y;
  vp.Z = c->vol_z;
  vp.zo0 = c->own_z0;
  vp.zo1 = c->own_z1;
  vp.zs0 = c->own_z0 - c->halo < 0 ? 0 : c->own_z0 - c->halo;
  const int zs1 = c->own_z1 + c->halo > c->vol_z ? c->vol_z : c->own_z1 + c->halo;
  vp.nzs = zs1 - vp.zs0;
  for (int i = 0; i < 3; ++i) vp.size[i] = c->vol_size_m[i];
  vp.cell[0] = vp.size[0] / (float)vp.X;
  vp.cell[1] = vp.size[1] / (float)vp.Y;
  vp.cell[2] = vp.size[2] / (float)vp.Z;
  for (int a = 0; a < 3; ++a) vp.icell[a] = 1.0 / (double)vp.cell[a];
  vp.stream_nt = 0;  // decided below, once the stored plane count is known
  vp.zchunk = 8;  // (decided below as well)
  vp.tau = config_tau(c);
  vp.tau_inv = 1.0f / vp.tau;
  for (int l = 0; l < HSK_NLEVELS; ++l) {
    const float s = (float)(1 << l);
    k->lv[l].W = c->width >> l;
    k->lv[l].H = c->height >> l;
    k->lv[l].in = Intr{c->fx / s, c->fy / s, c->cx / s, c->cy / s};
  }
  pose16_to_rt(c->init_pose, k->init_R, k->init_t);
  // memory
  k->vol_bytes = hsk_vol_words(vp) * 4;  // (stored planes padded to whole 64-B blocks of 4 planes: hsk_dev.h, hsk_vox_index)
  vp.stream_nt = k->vol_bytes > ((size_t)1 << 30) ? 1 : 0;  // > 1 GiB: four times the Infinity Cache and more
  vp.zchunk = hsk_pass_a_zchunk(vp.X, vp.Y, vp.nzs);
  CK(hipMalloc(&k->d_vol, k->vol_bytes));
  const size_t P0 = (size_t)c->width * c->height;
  for (auto& b : k->ib) {
    CK(hipMalloc((void**)&b.d_raw, P0 * 2));
    CK(hipMalloc((void**)&b.d_scaled, P0 * 4));
    CK(hipMalloc((void**)&b.d_tmax, tile_table_bytes(c->width, c->height)));
    CK(hipMemset(b.d_tmax, 0, tile_table_bytes(c->width, c->height)));  // (the validity mask's pad words are read, never written: they are zero)
    for (int l = 0; l < HSK_NLEVELS; ++l) {
      const size_t P = (size_t)k->lv[l].W * k->lv[l].H;
      CK(hipMalloc((void**)&b.d_dep[l], P * 2));
      CK(hipMalloc((void**)&b.d_vcur[l], P * 12));
      CK(hipMalloc((void**)&b.d_ncur[l], P * 12));
    }
  }
  for (int l = 0; l < HSK_NLEVELS; ++l) {
    const size_t P = (size_t)k->lv[l].W * k->lv[l].H;
    CK(hipMalloc((void**)&k->d_vmod[l], P * 12));
    CK(hipMalloc((void**)&k->d_nmod[l], P * 12));
  }
  {
    // The second stream (upload + preprocessing of the NEXT frame) at the LOWEST priority (round 6).  Not for the priority: streams
    // of different priorities come from different pools of hardware queues, so this stream can never be mapped onto the
    // hardware queue of the context's main stream -- HIP spreads a process's streams over four queues in turn, and with one
    // more stream alive in the process (an idle second context, the host application's own) the two streams of a context met
    // on one queue: the preprocessing then waited behind the previous frame's whole chain, 4440 -> 3730 frames/s
    // (tools/host_frames_probe.py --idle-ctx).  The main stream at the HIGHEST priority as well was measured too: four rooms
    // on one GPU fall from 7200 to 4700-5100 frames/s in all (profiles/r06/rooms_notes.md: more overlap, longer chains).
    int lo = 0, hi = 0;
    bool made = false;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi)
      made = hipStreamCreateWithPriority(&k->pstream, hipStreamNonBlocking, lo) == hipSuccess;
    if (!made) {  // (no priorities here: a plain stream, as before)
      (void)hipGetLastError();
      CK(hipStreamCreateWithFlags(&k->pstream, hipStreamNonBlocking));
    }
  }
  for (auto& e : k->ev_pre) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  for (auto& e : k->ev_free) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  CK(hipEventCreateWithFlags(&k->ev_src, hipEventDisableTiming));

  CK(hipMalloc((void**)&k->d_st, sizeof(TrackState)));
  CK(hipHostMalloc((void**)&k->h_st, sizeof(TrackState), hipHostMallocDefault));
  CK(hipHostMalloc((void**)&k->h_stage, P0 * 2 * (HSK_MAX_IN_FLIGHT + 1), hipHostMallocDefault));
  CK(hipHostMalloc((void**)&k->h_ring, sizeof(TrackState) * (HSK_MAX_IN_FLIGHT + 1), hipHostMallocDefault));
  CK(hipHostMalloc((void**)&k->h_slot_fifo, sizeof(int) * HSK_RING_FIFO, hipHostMallocDefault));
  memset(k->h_slot_fifo, 0, sizeof(int) * HSK_RING_FIFO);
  CK(hipHostGetDevicePointer((void**)&k->d_ring_view, k->h_ring, 0));
  CK(hipHostGetDevicePointer((void**)&k->d_fifo_view, k->h_slot_fifo, 0));
  CK(hipMalloc((void**)&k->d_ring_seq, sizeof(unsigned)));
  CK(hipMemset(k->d_ring_seq, 0, sizeof(unsigned)));
  for (auto& e : k->ring_ev) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const int nb0 = icp_num_blocks(c->width, c->height);
  CK(hipMalloc((void**)&k->d_partials, (size_t)nb0 * 27 * sizeof(double)));
  CK(hipMalloc(&k->d_icp_pose, icp_pose_bytes()));
  CK(hipMemset(k->d_icp_pose, 0, icp_pose_bytes()));  // accumulator slot 0 must be empty before the first tracked frame
  CK(hipMalloc((void**)&k->d_sums, 27 * sizeof(double)));
  CK(hipMalloc((void**)&k->d_wc, 512 * 4));
  CK(hipMalloc((void**)&k->d_keys, P0 * 4));
  vp.bshift = hsk_choose_bshift(vp);
  // integrate's queue entries are 28-bit lane-block ids (4 x-voxels x 4 planes) with 4 plane bits on top
  if ((size_t)((vp.nzs + 3) / 4) * vp.Y * (vp.X / 4) >= ((size_t)1 << 28)) {
    k->err = "hsk_create: volume too large for the 28-bit lane-block ids of integrate (more than 2^32 stored voxels)";
    return bail(HSK_ERR_ARG);
  }
  k->flags_bytes = (size_t)hsk_flag_words_total(vp) * 4;  // brick bits + super-brick bits (it fits a block's LDS: checked above)
  CK(hipMalloc((void**)&k->d_flags, k->flags_bytes));
  k->uni_bytes = uniform_bytes(vp);
  CK(hipMalloc((void**)&k->d_uni, k->uni_bytes));
  // integrate queues: 256 counters on their own 256-B lines + 256 queues, each sized for its share of pass A's tiles
  CK(hipMalloc((void**)&k->d_queue, integrate_queue_words(vp) * sizeof(unsigned)));
  CK(hipMalloc((void**)&k->d_zint, integrate_zint_entries(vp) * sizeof(int2)));
  CK(hipMalloc((void**)&k->d_counter, 16));
  {
    float ws[169], wc[512];
    hsk_bilateral_tables(ws, wc);
    memcpy(k->h_ws, ws, sizeof(ws));
    CK(hipMemcpy(k->d_wc, wc, sizeof(wc), hipMemcpyHostToDevice));
  }
  for (auto& e : k->ev) CK(hipEventCreate(&e));
  for (auto& e : k->ev_icp) CK(hipEventCreate(&e));
#undef CK
  int r = do_reset(k);
  if (r != HSK_OK) return bail(r);
  *out = k;
  return HSK_OK;
}

static int wait_slot(hsk_ctx* k, int slot, bool pose_only = false);
static int reset_behind_lost_frame(hsk_ctx* k, bool lost = false);
extern "C" int hsk_wait_frame(hsk_ctx* k, float pose_out[16], int* tracked);

extern "C" void hsk_destroy(hsk_ctx* k) {
  if (!k) return;
  if (k->pstream) (void)hipStreamSynchronize(k->pstream);
  if (k->stream) (void)hipStreamSynchronize(k->stream);  // frames in flight write into the pinned ring until they end
  free_all(k);
  delete k;
}

extern "C" int hsk_reset(hsk_ctx* k) {
  return k ? reset_behind_lost_frame(k) : HSK_ERR_ARG;  // (frames still in flight are dropped)
}

extern "C" const char* hsk_last_error(const hsk_ctx* k) { return k ? k->err.c_str() : create_error().c_str(); }

extern "C" void* hsk_stream(hsk_ctx* k) { return k ? (void*)k->stream : nullptr; }
extern "C" int hsk_set_stream(hsk_ctx* k, void* stream) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  if (k->stream) HIPCHK(k, hipStreamSynchronize(k->stream));
  if (k->own_stream && k->stream) (void)hipStreamDestroy(k->stream);
  k->stream = (hipStream_t)stream;
  k->own_stream = false;
  return HSK_OK;
}
extern "C" int hsk_synchronize(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// frame building blocks (enqueue only; no host synchronisation)
// ------------------------------------------------------------------------------------------------------
// three launches (round 5; they were nine): the bilateral filter with scaleDepth and the raw tile tables of all three
// granularities; the derived tile tables; pyrDown x 2 with the vertex / normal maps of the three levels
static void enqueue_preprocess(hsk_ctx* k, hipStream_t s) {
  launch_bilateral_scale(s, k->B().d_raw, k->lv[0].W, k->lv[0].H, k->lv[0].in, k->h_ws, k->d_wc, k->B().d_dep[0], k->B().d_scaled,
                         k->B().d_tmax);
  launch_tile_tables(s, k->lv[0].W, k->lv[0].H, k->B().d_tmax);
  launch_pyramid_maps(s, k->B().d_dep, k->lv, k->B().d_vcur, k->B().d_ncur);
}

// fin: leave the frame's last solve to the integrate that the caller enqueues next with the same descriptor (its first
// kernel does it in its prologue: one launch less); only where that integrate always follows
static void enqueue_icp(hsk_ctx* k, IcpFinal* fin = nullptr) {
  if (fin) *fin = IcpFinal{nullptr, nullptr, 0};
  launch_icp_fused(k->stream, k->B().d_vcur, k->B().d_ncur, k->d_vmod, k->d_nmod, k->lv, k->cfg.icp_iters, k->d_st,
                   k->cfg.icp_dist_thresh_m, k->cfg.icp_angle_thresh_sin, k->d_icp_pose, fin,
                   (k->prof && k->prof_levels && !fin) ? k->ev_icp : nullptr);
}

// the stage-level entry points' part of the preprocess: the scaled depth of the staged frame with its raw tile tables
static void enqueue_scaled_depth(hsk_ctx* k) {
  const int w = k->lv[0].W, h = k->lv[0].H;
  launch_scale_depth(k->stream, k->B().d_raw, w, h, k->lv[0].in, k->B().d_scaled);
  launch_tile_max(k->stream, k->B().d_scaled, w, h, k->B().d_tmax);
  launch_tile_fine(k->stream, k->B().d_scaled, w, h, k->B().d_tmax);
}

// the ICP sums of rows [row0, row1) of a level, at the pose of the device state, into 27 doubles on the device
static void enqueue_icp_row_sums(hsk_ctx* k, int level, int row0, int row1, double* sums27_dev) {
  const ImgLevel& lv = k->lv[level];
  launch_icp_accumulate(k->stream, k->B().d_vcur[level], k->B().d_ncur[level], k->d_vmod[level], k->d_nmod[level], lv.W, lv.H,
                        lv.in, k->d_st, k->cfg.icp_dist_thresh_m, k->cfg.icp_angle_thresh_sin, row0, row1, k->d_partials);
  launch_icp_reduce(k->stream, k->d_partials, icp_num_blocks(lv.W, row1 - row0), sums27_dev);
}

// report_early: a pipelined frame -- the integrate's first kernel, which ends the frame's ICP, tells the host the pose at
// once (pose_mark of the frame's ring slot); the raycast's report, an integrate later, then says that the frame's inputs
// are consumed (ring_mark)
static void enqueue_integrate(hsk_ctx* k, const IcpFinal* fin = nullptr, bool report_early = false) {
  k->weights_pending = true;
  k->vol_epoch += 1;
  const RingOut ring = {k->d_ring_view, k->d_fifo_view, k->d_ring_seq};
  launch_integrate(k->stream, k->d_vol, k->B().d_scaled, k->d_st, k->vp, k->lv[0].W, k->lv[0].H, k->lv[0].in, false,
                   k->d_counter, k->d_flags, k->B().d_tmax, k->d_zint, k->d_queue, (fin && fin->slots) ? fin : nullptr,
                   k->d_uni, report_early ? &ring : nullptr);
}

// hsk_integrate behind its pose and its upload, for a frame that is already in the set's d_raw (api_splat.hip: hsk_import_cloud)
void enqueue_integrate_staged(hsk_ctx* k) {
  enqueue_scaled_depth(k);
  enqueue_integrate(k);
}

// colour (hsk_enable_color): right behind the frame's integrate -- its pose is final there (the integrate's first kernel does
// the last solve) -- and before its raycast, whose report into the ring says the buffer set's inputs (the colour image with
// them) are consumed.  Nothing is launched while colour is off.
static void enqueue_color(hsk_ctx* k) {
  if (!k->d_color) return;
  launch_color_integrate(k->stream, k->d_color, k->d_st, k->d_has_color + k->cur, k->B().d_scaled, k->B().d_rgb, k->B().d_tmax, k->vp,
                         k->lv[0].W, k->lv[0].H, k->lv[0].in, k->color_band, k->color_max_w);
}

void enqueue_raycast_and_resize(hsk_ctx* k, int* keys, bool report) {
  hipStream_t s = k->stream;
  // report: the raycast (the frame's last reader of the tracker state) writes it into the pinned ring slot the host
  // assigned to this frame -- a copy node behind the graph cost ~20 us of idle GPU per frame around it
  const RingOut ring = {k->d_ring_view, k->d_fifo_view, k->d_ring_seq};
  const RingOut* rp = report ? &ring : nullptr;
  if (raycast_can_fuse_pyramid(k->vp, k->lv[0].W, k->lv[0].H)) {
    // the raycast writes levels 1 and 2 of the model maps from its own tiles: no second launch, no re-read
    const MapPyramid pyr = {k->d_vmod[1], k->d_nmod[1], k->d_vmod[2], k->d_nmod[2]};
    launch_raycast(s, k->d_vol, k->d_st, k->vp, k->lv[0].W, k->lv[0].H, k->lv[0].in, k->d_vmod[0], k->d_nmod[0], keys, k->d_flags,
                   &pyr, rp);
    return;
  }
  launch_raycast(s, k->d_vol, k->d_st, k->vp, k->lv[0].W, k->lv[0].H, k->lv[0].in, k->d_vmod[0], k->d_nmod[0], keys, k->d_flags,
                 nullptr, rp);
  launch_resize_maps2(s, k->d_vmod[0], k->d_nmod[0], k->lv[0].W, k->lv[0].H, k->d_vmod[1], k->d_nmod[1], k->d_vmod[2],
                      k->d_nmod[2], k->d_st);
}

// Integration gate (this build's specification of it: DESIGN.md section 4): the frame integrates
// iff (angle(R^T Rp) + |t - tp|) / 2 >= thr.  Host side, only when the threshold is positive; the pose pair comes from
// the tracker state the frame has just downloaded.  trace(R^T Rp) is taken column by column: column i of R against
// column i of Rp, the three column products added left to right.
static bool gate_passes(const TrackState* st, float thr) {
  if (!(thr > 0.0f)) return true;
  const float* a = st->R;
  const float* b = st->Rp;
  const float c0 = (a[0] * b[0] + a[3] * b[3]) + a[6] * b[6];
  const float c1 = (a[1] * b[1] + a[4] * b[4]) + a[7] * b[7];
  const float c2 = (a[2] * b[2] + a[5] * b[5]) + a[8] * b[8];
  float cs = (((c0 + c1) + c2) - 1.0f) / 2.0f;
  if (cs > 1.0f) cs = 1.0f;
  if (cs < -1.0f) cs = -1.0f;
  const float turn = acosf(cs);
  const float ex = st->t[0] - st->tp[0], ey = st->t[1] - st->tp[1], ez = st->t[2] - st->tp[2];
  const float shift = sqrtf((ex * ex + ey * ey) + ez * ez);
  return (turn + shift) / 2.0f >= thr;
}

// the steady-state frame: everything between the depth copy and the pose read-back
static void enqueue_tracked_frame(hsk_ctx* k, bool with_events) {
  hipStream_t s = k->stream;
  if (with_events) (void)hipEventRecord(k->ev[0], s);
  enqueue_preprocess(k, k->stream);
  if (with_events) (void)hipEventRecord(k->ev[1], s);
  enqueue_icp(k);
  if (with_events) (void)hipEventRecord(k->ev[2], s);
  enqueue_integrate(k);
  enqueue_color(k);
  if (with_events) (void)hipEventRecord(k->ev[3], s);
  enqueue_raycast_and_resize(k, nullptr);
  if (with_events) (void)hipEventRecord(k->ev[4], s);
}

// everything after the preprocessing of a tracked frame, on the main stream, for the buffer set k->cur
static void enqueue_tracked_rest(hsk_ctx* k) {
  IcpFinal fin;
  enqueue_icp(k, &fin);  // its first iteration also starts the frame (previous pose <- pose, lost flag)
  enqueue_integrate(k, &fin, true);  // ... and its last solve happens in the first kernel of the integrate, which reports the pose
  enqueue_color(k);
  enqueue_raycast_and_resize(k, nullptr, true);  // pipelined frames report their state through the ring
}

// what a synchronous frame hands back: the pose in the tracker state it has just downloaded, and its verdict
static int hand_back(const hsk_ctx* k, float pose_out[16], int* tracked, int verdict) {
  if (pose_out) rt_to_pose16(k->h_st->R, k->h_st->t, pose_out);
  if (tracked) *tracked = verdict;
  return HSK_OK;
}
// ... at the end of a tracked one: lost, and the scan restarts (the reset's pose goes back) or is held (the last tracked pose
// goes back); else the frame counts
static int end_tracked_frame(hsk_ctx* k, float pose_out[16], int* tracked) {
  if (k->h_st->lost) {
    const int r = after_loss(k);
    return r != HSK_OK ? r : hand_back(k, pose_out, tracked, 0);
  }
  k->frame += 1;
  return hand_back(k, pose_out, tracked, 1);
}

static int frame_common(hsk_ctx* k, float pose_out[16], int* tracked) {
  // depth is already in d_raw (enqueued on the stream)
  hipStream_t s = k->stream;
  const bool gated = k->cfg.integrate_move_thresh > 0.0f;
  if (k->frame == 0) {
    enqueue_preprocess(k, k->stream);
    enqueue_integrate(k);
    enqueue_color(k);
    for (int l = 0; l < HSK_NLEVELS; ++l)
      launch_transform_maps(s, k->B().d_vcur[l], k->B().d_ncur[l], k->lv[l].W * k->lv[l].H, k->d_st, k->d_vmod[l], k->d_nmod[l]);
    int r = download_state(k);
    if (r != HSK_OK) return r;
    HIPCHK(k, hipGetLastError());
    k->frame = 1;
    return hand_back(k, pose_out, tracked, 0);
  }
  if (gated) {
    // host decides whether to integrate: one extra synchronisation, only in this non-default mode
    enqueue_preprocess(k, k->stream);
    enqueue_icp(k);
    int r = download_state(k);
    if (r != HSK_OK) return r;
    if (!k->h_st->lost) {
      if (gate_passes(k->h_st, k->cfg.integrate_move_thresh)) {
        enqueue_integrate(k);
        enqueue_color(k);
      }
      enqueue_raycast_and_resize(k, nullptr);
    }
  } else if (k->prof) {
    enqueue_tracked_frame(k, true);
  } else if (k->cfg.use_graph == 1) {
    if (!k->graph_ready) {
      HIPCHK(k, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      enqueue_tracked_frame(k, false);
      HIPCHK(k, hipStreamEndCapture(s, &k->graph));
      HIPCHK(k, hipGraphInstantiate(&k->gexec, k->graph, nullptr, nullptr, 0));
      k->graph_ready = true;
    }
    HIPCHK(k, hipGraphLaunch(k->gexec, s));
    k->weights_pending = true;  // (the replayed graph integrates without passing through enqueue_integrate)
    k->vol_epoch += 1;
  } else {
    enqueue_tracked_frame(k, false);
  }
  int r = download_state(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipGetLastError());
  if (k->prof && !gated) {
    for (int i = 0; i < HSK_NSTAGES; ++i) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, k->ev[i], k->ev[i + 1]) == hipSuccess) k->stage_ms[i] += ms;
    }
    for (int i = 0; i < HSK_NLEVELS && k->prof_levels; ++i) {  // event i starts level HSK_NLEVELS - 1 - i
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, k->ev_icp[i], k->ev_icp[i + 1]) == hipSuccess) k->icp_level_ms[HSK_NLEVELS - 1 - i] += ms;
    }
    k->prof_frames += 1;
  }
  return end_tracked_frame(k, pose_out, tracked);
}

// the whole-frame entry points always work on buffer set 0 (their hipGraphs are captured with it); the slab entry
// points may have left the context on the other set or with a prefetch pending
void leave_slab_bookkeeping(hsk_ctx* k) {
  k->cur = 0;
  k->mgpu_set = 0;
  k->pf_ptr = nullptr;
  k->pf_set = -1;
}

static int check_dims(hsk_ctx* k, const void* depth, int w, int h) {
  if (!k) return HSK_ERR_ARG;
  if (!depth) return fail(k, HSK_ERR_ARG, "depth pointer is null");
  if (w != k->cfg.width || h != k->cfg.height) return fail(k, HSK_ERR_ARG, "depth frame size does not match the context");
  return HSK_OK;
}

static int stage_depth_host(hsk_ctx* k, const uint16_t* depth) {
  const size_t bytes = (size_t)k->cfg.width * k->cfg.height * 2;
  memcpy(k->h_stage, depth, bytes);  // caller's buffer may be freed on return (HoniHelper's Vector is only pinned in unsafeWith)
  HIPCHK(k, hipMemcpyAsync(k->B().d_raw, k->h_stage, bytes, hipMemcpyHostToDevice, k->stream));
  return HSK_OK;
}

// with colour enabled, every frame submission says on `s` whether buffer set `set` holds a colour image for it (and uploads
// the image from the staging buffer): a depth-only frame leaves the colour volume as it is
static hipError_t stage_color(hsk_ctx* k, int set, hipStream_t s) {
  if (!k->d_color) return hipSuccess;
  hipError_t e = hipSuccess;
  if (k->rgb_src) e = hipMemcpyAsync(k->ib[set].d_rgb, k->rgb_src, (size_t)k->cfg.width * k->cfg.height * 3, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(k->d_has_color + set), k->rgb_src ? 1 : 0, 1, s);
  return e;
}

// The synchronous calls of a steady-state frame go through the pipelined machinery (submit + wait: eager launches, the
// preprocessing on the second stream, the pose reported through the pinned ring), which leaves less idle GPU around the
// frame than a hipGraph launch followed by a copy and a stream synchronisation (2206 -> 2450 frames/s).  use_graph = 1
// keeps that older form; the first frame of a scan, the gated and the profiled modes always take frame_common.
static bool sync_via_ring(const hsk_ctx* k) {
  return k->cfg.use_graph != 1 && k->frame > 0 && !k->pending_reset && !(k->cfg.integrate_move_thresh > 0.0f) && !k->prof;
}
static int submit_frame(hsk_ctx* k, const void* src, hipMemcpyKind kind, int w, int h);

extern "C" int hsk_process_frame(hsk_ctx* k, const uint16_t* depth, int w, int h, float pose_out[16], int* tracked) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  if (int ri = require_idle(k)) return ri;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  if (sync_via_ring(k)) {
    memcpy(k->h_stage, depth, (size_t)w * h * 2);  // the caller's buffer may be gone when this returns
    r = submit_frame(k, k->h_stage, hipMemcpyHostToDevice, w, h);
    if (r != HSK_OK) return r;
    return hsk_wait_frame(k, pose_out, tracked);
  }
  leave_slab_bookkeeping(k);
  r = stage_depth_host(k, depth);
  if (r != HSK_OK) return r;
  HIPCHK(k, stage_color(k, k->cur, k->stream));
  return frame_common(k, pose_out, tracked);
}

extern "C" int hsk_process_frame_dev(hsk_ctx* k, const void* depth_dev, int w, int h, float pose_out[16], int* tracked) {
  int r = check_dims(k, depth_dev, w, h);
  if (r != HSK_OK) return r;
  if (int ri = require_idle(k)) return ri;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  if (sync_via_ring(k)) {
    r = submit_frame(k, depth_dev, hipMemcpyDeviceToDevice, w, h);
    if (r != HSK_OK) return r;
    return hsk_wait_frame(k, pose_out, tracked);
  }
  leave_slab_bookkeeping(k);
  HIPCHK(k, hipMemcpyAsync(k->B().d_raw, depth_dev, (size_t)w * h * 2, hipMemcpyDeviceToDevice, k->stream));
  HIPCHK(k, stage_color(k, k->cur, k->stream));
  return frame_common(k, pose_out, tracked);
}


// ------------------------------------------------------------------------------------------------------
// asynchronous submission
// ------------------------------------------------------------------------------------------------------
// Completion of the frame parked in a ring slot.  Pipelined single-device frames (kind 0 with a mark) are announced by
// the device itself: the raycast stores the frame's sequence number into the pinned slot after the state words, and
// the host polls it -- event records on the main stream cost ~16 us of idle GPU per frame (2334 -> 2426 frames/s).
// how long a pipelined frame may take to report before the wait gives up (HSK_FRAME_TIMEOUT_S, seconds; default 20): a
// frame takes milliseconds, so this only ever ends a wait behind a peer rank of a group that has died or hung
static double frame_timeout_s() {
  static const double t = []() {
    const char* e = getenv("HSK_FRAME_TIMEOUT_S");
    const double v = e ? atof(e) : 0.0;
    return v > 0.0 ? v : 20.0;
  }();
  return t;
}
// pose_only: the caller wants the frame's pose and verdict (final once its ICP has ended: pose_mark); otherwise that the
// frame has consumed its inputs and the stream has passed its integrate (ring_mark: buffer-set reuse, resets)
static int wait_slot(hsk_ctx* k, int slot, bool pose_only) {
  if (k->ring_expect[slot] == 0u) {
    HIPCHK(k, hipEventSynchronize(k->ring_ev[slot]));
    return HSK_OK;
  }
  volatile TrackState* w = (volatile TrackState*)&k->h_ring[slot];
  const auto t0 = std::chrono::steady_clock::now();
  // a frame takes well under 2 ms: spin that long before giving the core away (a yield can cost a whole time slice when
  // other threads of the process are runnable -- measured: 2620 -> 1450 frames/s with host frames under torch's threads)
  volatile unsigned* mark = pose_only ? &w->pose_mark : &w->ring_mark;
  for (unsigned long spin = 0; *mark != k->ring_expect[slot]; ++spin) {
    __builtin_ia32_pause();
    if ((spin & 4095u) == 4095u) {
      const auto dt = std::chrono::steady_clock::now() - t0;
      if (std::chrono::duration<double>(dt).count() > frame_timeout_s())
        return fail(k, HSK_ERR_TIMEOUT, "a pipelined frame did not report within HSK_FRAME_TIMEOUT_S (default 20 s)");
      if (dt > std::chrono::milliseconds(2)) sched_yield();
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return HSK_OK;
}

// Tracking was lost with frames still in flight: their results stay in the ring (they report tracked = 0), the reset
// itself happens here, before new work is enqueued.  lost: because of a loss (the policy decides); else hsk_reset's.
static int reset_behind_lost_frame(hsk_ctx* k, bool lost) {
  for (int i = 0; i < k->ring_count; ++i) {
    const int sl = (k->ring_head + i) % (HSK_MAX_IN_FLIGHT + 1);
    const int r = wait_slot(k, sl);
    if (r != HSK_OK) return r;
    if (k->ring_kind[sl] == 0) k->ring_kind[sl] = 2;  // dropped on the device (need_reset was set)
  }
  return lost ? after_loss(k) : do_reset(k);
}

extern "C" int hsk_submit_frame_dev(hsk_ctx* k, const void* depth_dev, int w, int h) {
  return submit_frame(k, depth_dev, hipMemcpyDeviceToDevice, w, h);
}

// the same for a frame in HOST memory (what takeDepthSnapshot hands over): copied into one of HSK_MAX_IN_FLIGHT + 1
// pinned staging frames before this returns, so the caller's buffer is free again; the upload overlaps the frame in flight
extern "C" int hsk_submit_frame(hsk_ctx* k, const uint16_t* depth, int w, int h) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  if (k->ring_count >= HSK_MAX_IN_FLIGHT) return fail(k, HSK_ERR_STATE, "too many frames in flight: call hsk_wait_frame first");
  const size_t px = (size_t)w * h;
  uint16_t* stage = k->h_stage + (size_t)(k->stage_turn % (HSK_MAX_IN_FLIGHT + 1)) * px;
  k->stage_turn += 1;
  const auto t0 = std::chrono::steady_clock::now();
  memcpy(stage, depth, px * 2);
  k->submit_us[0] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  return submit_frame(k, stage, hipMemcpyHostToDevice, w, h);
}

// src: device memory (kind D2D) or the context's pinned staging buffer (kind H2D)
static int submit_frame(hsk_ctx* k, const void* depth_dev, hipMemcpyKind kind, int w, int h) {
  int r = check_dims(k, depth_dev, w, h);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  if (k->ring_count >= HSK_MAX_IN_FLIGHT) return fail(k, HSK_ERR_STATE, "too many frames in flight: call hsk_wait_frame first");
  if (k->ring_count == 0) leave_slab_bookkeeping(k);
  hipStream_t s = k->stream;
  if (k->pending_reset) {  // (a restarted scan then takes the synchronous path with its first frame; a held one goes on pipelined)
    r = reset_behind_lost_frame(k, true);
    if (r != HSK_OK) return r;
  }
  const bool sync_path = k->frame == 0 || k->cfg.integrate_move_thresh > 0.0f || k->prof;
  if (sync_path) {
    // first frame of a (re)started scan, gated or profiled mode: run it synchronously and park the result
    HIPCHK(k, hipMemcpyAsync(k->B().d_raw, depth_dev, (size_t)w * h * 2, kind, s));
    HIPCHK(k, stage_color(k, k->cur, s));
    float pose[16];
    int tracked = 0;
    r = frame_common(k, pose, &tracked);
    if (r != HSK_OK) return r;
    const int slot = (k->ring_head + k->ring_count) % (HSK_MAX_IN_FLIGHT + 1);
    k->h_ring[slot] = *k->h_st;
    k->h_ring[slot].lost = tracked ? 0 : 1;
    k->ring_kind[slot] = 1;
    k->ring_expect[slot] = 0u;
    HIPCHK(k, hipEventRecord(k->ring_ev[slot], s));
    k->ring_count += 1;
    return HSK_OK;
  }
  // Overlapped path: depth copy + preprocessing of THIS frame go to the second stream and the other buffer set, so
  // they run while the previous frame is still in its ICP / integrate / raycast on the main stream.
  const int set = k->async_set;
  k->async_set ^= 1;
  k->cur = set;
  // the slot this frame reports into: published to the device through the pinned fifo before anything is launched
  const int slot = (k->ring_head + k->ring_count) % (HSK_MAX_IN_FLIGHT + 1);
  k->h_slot_fifo[k->ring_seq % HSK_RING_FIFO] = slot;
  k->ring_seq += 1;
  k->ring_expect[slot] = k->ring_seq | 0x80000000u;  // never 0 (0 = "this slot completes through its event")
  ((volatile TrackState*)&k->h_ring[slot])->ring_mark = 0u;
  ((volatile TrackState*)&k->h_ring[slot])->pose_mark = 0u;
  hipError_t e = hipSuccess;
  // no events on the main stream: the host itself sees, in the pinned ring, that the previous user of this buffer set has
  // finished (it normally has: its pose was collected before this call)
  if (k->set_used[set] && k->set_slot[set] >= 0 && k->ring_expect[k->set_slot[set]] == k->set_expect[set]) {
    const int r2 = wait_slot(k, k->set_slot[set]);
    if (r2 != HSK_OK) return r2;
  }
  k->set_expect[set] = k->ring_seq | 0x80000000u;
  k->set_slot[set] = slot;
  // A device frame may still be in the making on the context's stream (an upload or a conversion kernel the caller
  // enqueued on the stream it handed over with hsk_set_stream): the second stream is ordered behind it.  The record
  // costs the main queue nothing, the wait sits on the second stream only.  (Host frames come from the context's own
  // pinned staging ring, already complete.)
  if (e == hipSuccess && kind == hipMemcpyDeviceToDevice && !k->own_stream) {
    e = hipEventRecord(k->ev_src, k->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(k->pstream, k->ev_src, 0);
  }
  const auto tp0 = std::chrono::steady_clock::now();
  if (e == hipSuccess) e = hipMemcpyAsync(k->B().d_raw, depth_dev, (size_t)w * h * 2, kind, k->pstream);
  if (e == hipSuccess) e = stage_color(k, set, k->pstream);
  if (e == hipSuccess) {
    enqueue_preprocess(k, k->pstream);
    e = hipEventRecord(k->ev_pre[set], k->pstream);
  }
  const auto tp1 = std::chrono::steady_clock::now();
  // The frame's own work needs the preprocessing.  A hipStreamWaitEvent on the main stream would be the obvious form,
  // but a cross-stream wait costs ~19 us of stalled queue at every frame boundary even when the event fired long ago
  // (2330 -> 2440 frames/s without it).  The host waits instead: it is a frame ahead of the GPU, the preprocessing takes
  // ~60 us, and kernels enqueued after the host has seen it complete need no device-side dependency.
  if (e == hipSuccess) e = hipEventSynchronize(k->ev_pre[set]);
  const auto tp2 = std::chrono::steady_clock::now();
  if (e == hipSuccess) {
    // Eager launches, on purpose: the host runs a frame ahead here, so their launch cost is hidden, while replaying
    // the frame from a hipGraph left ~8 us more idle GPU between consecutive frames (2330 vs 2285 frames/s measured).
    // The graph stays on the synchronous path, where the launch cost is exposed.
    if (k->cfg.use_graph == 2 && k->own_stream) {
      // (the chain's arguments depend on the buffer set only: the kernels read the pose from the tracker state, the ICP's
      // iteration index restarts with every frame, the ring slot comes through the pinned fifo)
      if (!k->pgexec[set]) {
        e = hipStreamBeginCapture(k->stream, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
          enqueue_tracked_rest(k);
          e = hipStreamEndCapture(k->stream, &k->pgraph[set]);
        }
        if (e == hipSuccess) e = hipGraphInstantiate(&k->pgexec[set], k->pgraph[set], nullptr, nullptr, 0);
      } else {
        k->weights_pending = true;  // (what enqueue_integrate notes on the host side)
        k->vol_epoch += 1;
      }
      if (e == hipSuccess) e = hipGraphLaunch(k->pgexec[set], k->stream);
    } else {
      enqueue_tracked_rest(k);
    }
  }
  {
    const auto tp3 = std::chrono::steady_clock::now();
    k->submit_us[1] += std::chrono::duration<double, std::micro>(tp1 - tp0).count();
    k->submit_us[2] += std::chrono::duration<double, std::micro>(tp2 - tp1).count();
    k->submit_us[3] += std::chrono::duration<double, std::micro>(tp3 - tp2).count();
    k->submit_n += 1;
  }
  k->set_used[set] = true;
  k->cur = 0;
  HIPCHK(k, e);
  k->ring_kind[slot] = 0;
  k->ring_count += 1;
  return HSK_OK;
}

extern "C" int hsk_wait_frame(hsk_ctx* k, float pose_out[16], int* tracked) {
  if (!k) return HSK_ERR_ARG;
  if (k->ring_count == 0) return fail(k, HSK_ERR_STATE, "no frame in flight");
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const int slot = k->ring_head;
  {
    const int rw = wait_slot(k, slot, true);  // (the pose: the frame's volume work may still be running)
    if (rw != HSK_OK) return rw;
  }
  const TrackState& st = k->h_ring[slot];
  k->ring_head = (k->ring_head + 1) % (HSK_MAX_IN_FLIGHT + 1);
  k->ring_count -= 1;
  if (pose_out) rt_to_pose16(st.R, st.t, pose_out);
  if (k->ring_kind[slot] == 1) {  // completed synchronously at submission
    if (tracked) *tracked = st.lost ? 0 : 1;
    return HSK_OK;
  }
  // a lost or dropped frame reports the restarted scan's pose, or under HSK_LOSS_HOLD the last tracked pose: the previous pose
  // of its slot (a lost frame started with previous pose <- pose, a dropped one left the state alone)
  const bool hold = k->loss_policy == HSK_LOSS_HOLD;
  if (k->ring_kind[slot] == 2) {  // was in flight behind a lost frame; the reset (or the hold) has already happened
    if (tracked) *tracked = 0;
    if (pose_out) rt_to_pose16(hold ? st.Rp : k->init_R, hold ? st.tp : k->init_t, pose_out);
    return HSK_OK;
  }
  if (st.lost) {
    // the volume is reset lazily: at the next submission, or now if nothing else is in flight
    k->pending_reset = true;
    if (tracked) *tracked = 0;
    if (pose_out) rt_to_pose16(hold ? st.Rp : k->init_R, hold ? st.tp : k->init_t, pose_out);
    if (k->ring_count == 0) {
      int r = after_loss(k);
      if (r != HSK_OK) return r;
    }
    return HSK_OK;
  }
  k->frame += 1;
  if (tracked) *tracked = 1;
  return HSK_OK;
}

// The recorded-stream frame feed: what the host loop around takeDepthSnapshot (HoniHelper.hs:20-36, Main.hs:1285-1290)
// becomes when the frames come from a file.  One frame is always in flight ahead of the one being collected, so the
// file read + the copy into the pinned staging ring + the upload of frame i + 1 run under frame i's GPU work.
extern "C" int hsk_track_stream(hsk_ctx* k, hsk_depth_stream* s, int first, int count, float* poses_out, int* tracked_out) {
  if (!k) return HSK_ERR_ARG;
  if (!s) return fail(k, HSK_ERR_ARG, "stream is null");
  int w = 0, h = 0, n = 0;
  if (hsk_stream_info(s, &w, &h, &n, nullptr) != HSK_OK) return fail(k, HSK_ERR_ARG, "not a stream opened for reading");
  if (w != k->cfg.width || h != k->cfg.height) return fail(k, HSK_ERR_ARG, "the stream's frame size does not match the context");
  if (first < 0 || count < 0 || first > n || count > n - first) return fail(k, HSK_ERR_ARG, "frame range outside the stream");
  if (int ri = require_idle(k)) return ri;
  uint16_t* buf = (uint16_t*)malloc((size_t)w * h * 2);
  if (!buf) return fail(k, HSK_ERR_STATE, "out of host memory");
  // `next`: the frame to submit next; `collected`: results handed out so far (frames first .. first + collected - 1).
  // A frame that reports tracking LOST (a pipelined frame, kind 0, with tracked = 0) leaves its successor -- already in
  // flight -- dropped on the device: that result is collected and thrown away, and the successor goes in again as the
  // first frame of the restarted scan, which is what hsk_process_frame makes of it.
  int next = 0, collected = 0, r = HSK_OK;
  auto collect = [&](bool* lost_verdict) -> int {
    float pose[16];
    int tr = 0;
    const bool pipelined = k->ring_kind[k->ring_head] == 0;
    const int rc = hsk_wait_frame(k, pose, &tr);
    if (rc != HSK_OK) return rc;
    if (poses_out) memcpy(poses_out + (size_t)16 * collected, pose, sizeof(pose));
    if (tracked_out) tracked_out[collected] = tr;
    collected += 1;
    *lost_verdict = pipelined && !tr;
    return HSK_OK;
  };
  auto after_collect = [&](bool lost) -> int {
    if (!lost) return HSK_OK;
    if (k->ring_count > 0) {  // the frames behind the lost one: dropped on the device; the reset, then their results discarded
      const int rr = reset_behind_lost_frame(k, true);
      if (rr != HSK_OK) return rr;
    }
    while (k->ring_count > 0) {
      const int rc = hsk_wait_frame(k, nullptr, nullptr);
      if (rc != HSK_OK) return rc;
    }
    next = collected;  // ... and fed again, the first of them restarting the scan
    return HSK_OK;
  };
  while (r == HSK_OK && collected < count) {
    bool lost = false;
    if (next < count) {
      if (hsk_stream_read(s, first + next, buf) != HSK_OK) {
        r = fail(k, HSK_ERR_STATE, "reading a frame from the stream failed");
        break;
      }
      r = hsk_submit_frame(k, buf, w, h);  // copies the frame before it returns
      next += 1;
      if (r == HSK_OK && k->ring_count > 1) {
        r = collect(&lost);
        if (r == HSK_OK) r = after_collect(lost);
      }
    } else {
      r = collect(&lost);
      if (r == HSK_OK) r = after_collect(lost);
    }
  }
  free(buf);
  return r;
}

// ------------------------------------------------------------------------------------------------------
// stage-level entry points
// ------------------------------------------------------------------------------------------------------
int set_pose_internal(hsk_ctx* k, const float pose[16]) {
  int r = download_state(k);
  if (r != HSK_OK) return r;
  pose16_to_rt(pose, k->h_st->R, k->h_st->t);
  k->h_st->lost = 0;
  return upload_state(k);
}

extern "C" int hsk_get_pose(hsk_ctx* k, float pose[16]) {
  if (!k || !pose) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  int r = download_state(k);
  if (r != HSK_OK) return r;
  rt_to_pose16(k->h_st->R, k->h_st->t, pose);
  return HSK_OK;
}
extern "C" int hsk_set_pose(hsk_ctx* k, const float pose[16]) {
  if (!k || !pose) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  return set_pose_internal(k, pose);
}

extern "C" int hsk_integrate(hsk_ctx* k, const uint16_t* depth, int w, int h, const float pose[16]) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  if (!pose) return fail(k, HSK_ERR_ARG, "pose is null");
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  r = set_pose_internal(k, pose);
  if (r != HSK_OK) return r;
  r = stage_depth_host(k, depth);
  if (r != HSK_OK) return r;
  enqueue_scaled_depth(k);
  enqueue_integrate(k);
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

extern "C" int hsk_count_updates(hsk_ctx* k, const uint16_t* depth, int w, int h, const float pose[16], uint64_t* n_upd) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  if (!pose || !n_upd) return fail(k, HSK_ERR_ARG, "null argument");
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  r = set_pose_internal(k, pose);
  if (r != HSK_OK) return r;
  r = stage_depth_host(k, depth);
  if (r != HSK_OK) return r;
  enqueue_scaled_depth(k);
  HIPCHK(k, hipMemsetAsync(k->d_counter, 0, 8, k->stream));
  launch_integrate(k->stream, k->d_vol, k->B().d_scaled, k->d_st, k->vp, w, h, k->lv[0].in, true, k->d_counter, k->d_flags,
                   k->B().d_tmax, k->d_zint, k->d_queue);
  unsigned long long c = 0;
  HIPCHK(k, hipMemcpyAsync(&c, k->d_counter, 8, hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  *n_upd = c;
  return HSK_OK;
}

extern "C" int hsk_raycast(hsk_ctx* k, const float pose[16], float* vmap, float* nmap, int32_t* keys) {
  if (!k || !pose || !vmap || !nmap) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  int r = set_pose_internal(k, pose);
  if (r != HSK_OK) return r;
  const size_t P = (size_t)k->lv[0].W * k->lv[0].H;
  launch_raycast(k->stream, k->d_vol, k->d_st, k->vp, k->lv[0].W, k->lv[0].H, k->lv[0].in, k->d_vmod[0], k->d_nmod[0],
                 k->d_keys, k->d_flags);
  launch_resize_maps2(k->stream, k->d_vmod[0], k->d_nmod[0], k->lv[0].W, k->lv[0].H, k->d_vmod[1], k->d_nmod[1], k->d_vmod[2],
                      k->d_nmod[2], k->d_st);
  HIPCHK(k, hipMemcpyAsync(vmap, k->d_vmod[0], P * 12, hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipMemcpyAsync(nmap, k->d_nmod[0], P * 12, hipMemcpyDeviceToHost, k->stream));
  if (keys) HIPCHK(k, hipMemcpyAsync(keys, k->d_keys, P * 4, hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

extern "C" int hsk_preprocess(hsk_ctx* k, const uint16_t* depth, int w, int h) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  return preprocess_frame(k, depth, w, h);
}
int preprocess_frame(hsk_ctx* k, const uint16_t* depth, int w, int h) {
  (void)w;
  (void)h;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  int r = stage_depth_host(k, depth);
  if (r != HSK_OK) return r;
  enqueue_preprocess(k, k->stream);
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

extern "C" int hsk_icp_accumulate(hsk_ctx* k, int level, const float pose_est[16], int row0, int row1, double out27[27]) {
  if (!k || !pose_est || !out27) return HSK_ERR_ARG;
  if (level < 0 || level >= HSK_NLEVELS) return fail(k, HSK_ERR_ARG, "level out of range");
  if (row0 < 0 || row1 > k->lv[level].H || row0 >= row1) return fail(k, HSK_ERR_ARG, "row range out of bounds");
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  // estimate goes to (R,t); the previous pose (Rp,tp) is left as the tracker stored it
  int r = download_state(k);
  if (r != HSK_OK) return r;
  TrackState saved = *k->h_st;
  // the model maps were raycast from the last stored pose: that is the "previous" camera of A.5
  memcpy(k->h_st->Rp, saved.R, sizeof(saved.R));
  memcpy(k->h_st->tp, saved.t, sizeof(saved.t));
  pose16_to_rt(pose_est, k->h_st->R, k->h_st->t);
  k->h_st->lost = 0;
  r = upload_state(k);
  if (r != HSK_OK) return r;
  enqueue_icp_row_sums(k, level, row0, row1, k->d_sums);
  HIPCHK(k, hipMemcpyAsync(out27, k->d_sums, 27 * sizeof(double), hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  *k->h_st = saved;
  return upload_state(k);
}

extern "C" int hsk_icp_solve(const double in27[27], float x6[6], int* ok) {
  if (!in27 || !x6 || !ok) return HSK_ERR_ARG;
  *ok = host_solve6(in27, x6) ? 1 : 0;
  if (!*ok)
    for (int i = 0; i < 6; ++i) x6[i] = 0.0f;
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// colour (RGB-D scans; opt-in: include/hskinfu.h "Colour", DESIGN.md "Colour")
// ------------------------------------------------------------------------------------------------------
void hsk_mark_group_slab(hsk_ctx* k) {  // (library-internal, not in the C ABI: hsk_ctx.h)
  if (k) k->group_slab = true;
}

// the captured frame chains hold the launches they were captured with: dropped, so that the next frame captures them again
static void drop_graphs(hsk_ctx* k) {
  if (k->gexec) (void)hipGraphExecDestroy(k->gexec);
  if (k->graph) (void)hipGraphDestroy(k->graph);
  k->gexec = nullptr;
  k->graph = nullptr;
  k->graph_ready = false;
  for (int i = 0; i < 2; ++i) {
    if (k->pgexec[i]) (void)hipGraphExecDestroy(k->pgexec[i]);
    if (k->pgraph[i]) (void)hipGraphDestroy(k->pgraph[i]);
    k->pgexec[i] = nullptr;
    k->pgraph[i] = nullptr;
  }
}

extern "C" int hsk_enable_color(hsk_ctx* k, int max_weight, float band_m) {
  if (!k) return HSK_ERR_ARG;
  if (max_weight < 0 || max_weight > 255) return fail(k, HSK_ERR_ARG, "hsk_enable_color: max_weight must lie in 0..255 (0: 64)");
  if (!(band_m == band_m)) return fail(k, HSK_ERR_ARG, "hsk_enable_color: band_m is NaN");
  if (k->group_slab)
    return fail(k, HSK_ERR_STATE, "hsk_enable_color: colour is not available for the slabs of a group");
  if (int ri = require_idle(k)) return ri;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  float m = k->vp.cell[0] > k->vp.cell[1] ? k->vp.cell[0] : k->vp.cell[1];
  m = m > k->vp.cell[2] ? m : k->vp.cell[2];
  float band = band_m > 0.0f ? band_m : 2.0f * m;
  if (band > k->vp.tau) band = k->vp.tau;  // every voxel coloured is one the frame's integrate updates
  if (!k->d_color) {
    const size_t P0 = (size_t)k->cfg.width * k->cfg.height;
    const size_t bytes = (size_t)k->vp.X * k->vp.Y * (size_t)k->vp.nzs * 4;
    hipError_t e = hipMalloc((void**)&k->d_color, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&k->d_has_color, 2 * sizeof(int));
    for (auto& b : k->ib)
      if (e == hipSuccess) e = hipMalloc((void**)&b.d_rgb, P0 * 3);
    if (e == hipSuccess) e = hipHostMalloc((void**)&k->h_rgb_stage, P0 * 3, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(k->d_color, 0, bytes, k->stream);
    if (e == hipSuccess) e = hipMemsetAsync(k->d_has_color, 0, 2 * sizeof(int), k->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
    if (e != hipSuccess) {  // (nothing half made is left behind: colour stays off)
      auto F = [](void* p) {
        if (p) (void)hipFree(p);
      };
      F(k->d_color);
      F(k->d_has_color);
      for (auto& b : k->ib) {
        F(b.d_rgb);
        b.d_rgb = nullptr;
      }
      if (k->h_rgb_stage) (void)hipHostFree(k->h_rgb_stage);
      k->d_color = nullptr;
      k->d_has_color = nullptr;
      k->h_rgb_stage = nullptr;
      HIPCHK(k, e);
    }
    k->color_bytes = bytes;
  }
  k->color_max_w = max_weight == 0 ? 64 : max_weight;
  k->color_band = band;
  drop_graphs(k);
  return HSK_OK;
}

static int check_rgb(hsk_ctx* k, const uint8_t* rgb) {
  if (int rc = require_color(k)) return rc;
  if (!rgb) return fail(k, HSK_ERR_ARG, "rgb pointer is null");
  memcpy(k->h_rgb_stage, rgb, (size_t)k->cfg.width * k->cfg.height * 3);  // (the caller's buffer may be gone when this returns)
  k->rgb_src = k->h_rgb_stage;
  return HSK_OK;
}

extern "C" int hsk_process_frame_rgbd(hsk_ctx* k, const uint16_t* depth, const uint8_t* rgb, int w, int h, float pose_out[16], int* tracked) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  if (int ri = require_idle(k)) return ri;
  r = check_rgb(k, rgb);
  if (r != HSK_OK) return r;
  r = hsk_process_frame(k, depth, w, h, pose_out, tracked);
  k->rgb_src = nullptr;
  return r;
}

extern "C" int hsk_submit_frame_rgbd(hsk_ctx* k, const uint16_t* depth, const uint8_t* rgb, int w, int h) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  if (k->ring_count >= HSK_MAX_IN_FLIGHT) return fail(k, HSK_ERR_STATE, "too many frames in flight: call hsk_wait_frame first");
  const auto t0 = std::chrono::steady_clock::now();
  r = check_rgb(k, rgb);
  if (r != HSK_OK) return r;
  k->submit_us[0] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  r = hsk_submit_frame(k, depth, w, h);
  k->rgb_src = nullptr;
  return r;
}

extern "C" int hsk_integrate_color(hsk_ctx* k, const uint16_t* depth, const uint8_t* rgb, int w, int h, const float pose[16]) {
  int r = check_dims(k, depth, w, h);
  if (r != HSK_OK) return r;
  if (!pose) return fail(k, HSK_ERR_ARG, "pose is null");
  if (int ri = require_idle(k)) return ri;
  r = check_rgb(k, rgb);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  leave_slab_bookkeeping(k);
  r = set_pose_internal(k, pose);
  if (r == HSK_OK) r = stage_depth_host(k, depth);
  if (r != HSK_OK) {
    k->rgb_src = nullptr;
    return r;
  }
  enqueue_scaled_depth(k);
  const hipError_t e = stage_color(k, k->cur, k->stream);
  k->rgb_src = nullptr;
  HIPCHK(k, e);
  enqueue_color(k);
  k->pack.drop();  // (the colour changed without the TSDF: the volume image's pass is void)
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// profiling
// ------------------------------------------------------------------------------------------------------
extern "C" int hsk_set_profiling(hsk_ctx* k, int on) {
  if (!k) return HSK_ERR_ARG;
  k->prof = on != 0;
  k->prof_levels = on == 2;
  return HSK_OK;
}
extern "C" int hsk_stage_ms(hsk_ctx* k, double sum_ms[HSK_NSTAGES], uint64_t* n_frames, int reset) {
  if (!k) return HSK_ERR_ARG;
  if (sum_ms)
    for (int i = 0; i < HSK_NSTAGES; ++i) sum_ms[i] = k->stage_ms[i];
  if (n_frames) *n_frames = k->prof_frames;
  if (reset) {
    for (int i = 0; i < HSK_NSTAGES; ++i) k->stage_ms[i] = 0.0;
    for (int i = 0; i < HSK_NLEVELS; ++i) k->icp_level_ms[i] = 0.0;
    k->prof_frames = 0;
  }
  return HSK_OK;
}
// host microseconds the pipelined submissions have spent, by phase, and how many there were (reset != 0: counted from now on)
extern "C" int hsk_submit_host_us(hsk_ctx* k, double sum_us[4], uint64_t* n_submissions, int reset) {
  if (!k) return HSK_ERR_ARG;
  if (sum_us)
    for (int i = 0; i < 4; ++i) sum_us[i] = k->submit_us[i];
  if (n_submissions) *n_submissions = k->submit_n;
  if (reset) {
    for (auto& v : k->submit_us) v = 0.0;
    k->submit_n = 0;
  }
  return HSK_OK;
}
extern "C" int hsk_icp_level_ms(hsk_ctx* k, double sum_ms[HSK_LEVELS]) {
  if (!k || !sum_ms) return HSK_ERR_ARG;
  for (int i = 0; i < HSK_NLEVELS; ++i) sum_ms[i] = k->icp_level_ms[i];
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// multi-GPU (z-slab) building blocks: enqueue-only, the host runs its collective between them
// ------------------------------------------------------------------------------------------------------
extern "C" int hsk_mgpu_frame_index(const hsk_ctx* k) { return k ? k->frame : -1; }

// Optional: enqueue the depth copy and the preprocessing of the NEXT frame on the second stream, into the buffer set
// the current frame does not use, so that they run under the current frame's ICP / integrate / raycast and collectives.
// The following hsk_mgpu_frame_begin with the same pointer picks the result up instead of preprocessing again.
extern "C" int hsk_mgpu_prefetch(hsk_ctx* k, const void* depth_dev, int w, int h) {
  int r = check_dims(k, depth_dev, w, h);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const int set = k->mgpu_set ^ 1;
  if (k->set_used[set]) HIPCHK(k, hipStreamWaitEvent(k->pstream, k->ev_free[set], 0));  // its previous frame has finished
  const int keep = k->cur;
  k->cur = set;
  // (No ordering against the context's stream: the point of the prefetch is to run beside the frame that stream is busy
  // with.  The contract -- include/hskinfu.h -- asks for a frame that is complete when this is called; it may live in
  // device memory or in pinned host memory, hence hipMemcpyDefault.)
  hipError_t e = hipMemcpyAsync(k->B().d_raw, depth_dev, (size_t)w * h * 2, hipMemcpyDefault, k->pstream);
  if (e == hipSuccess) {
    enqueue_preprocess(k, k->pstream);
    e = hipEventRecord(k->ev_pre[set], k->pstream);
  }
  k->cur = keep;
  HIPCHK(k, e);
  k->pf_ptr = depth_dev;
  k->pf_set = set;
  return HSK_OK;
}

extern "C" int hsk_mgpu_frame_begin(hsk_ctx* k, const void* depth_dev, int w, int h) {
  int r = check_dims(k, depth_dev, w, h);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  if (k->pending_reset) {  // a pipelined frame (hsk_mgpu_frame_end_async) lost tracking: restart the scan with this frame
    r = reset_behind_lost_frame(k);
    if (r != HSK_OK) return r;
  }
  if (k->pf_ptr == depth_dev && k->pf_set >= 0) {
    // preprocessed ahead of time by hsk_mgpu_prefetch: the frame works on that buffer set once the event has fired
    k->mgpu_set = k->pf_set;
    k->cur = k->mgpu_set;
    HIPCHK(k, hipStreamWaitEvent(k->stream, k->ev_pre[k->mgpu_set], 0));
  } else {
    k->cur = k->mgpu_set;  // same set as the previous frame: stream order protects it
    HIPCHK(k, hipMemcpyAsync(k->B().d_raw, depth_dev, (size_t)w * h * 2, hipMemcpyDefault, k->stream));
    enqueue_preprocess(k, k->stream);
  }
  k->pf_ptr = nullptr;
  k->pf_set = -1;
  if (k->frame == 0) {
    enqueue_integrate(k);
    for (int l = 0; l < HSK_NLEVELS; ++l)
      launch_transform_maps(k->stream, k->B().d_vcur[l], k->B().d_ncur[l], k->lv[l].W * k->lv[l].H, k->d_st, k->d_vmod[l],
                            k->d_nmod[l]);
  } else {
    launch_begin_frame(k->stream, k->d_st, nullptr);
  }
  return HSK_OK;
}

// hsk_mgpu_frame_begin + hsk_mgpu_icp_replicated + hsk_mgpu_integrate + hsk_mgpu_raycast_local as ONE call.  The part
// after the preprocessing (about 25 launches) is captured into a hipGraph per buffer set on first use: the z-slab host
// then issues five operations per frame (this, two collectives, resolve, frame end) and stops being launch-bound.
// keys_dev must be the same buffer on every call (it is part of the captured graph).
extern "C" int hsk_mgpu_frame_front(hsk_ctx* k, const void* depth_dev, int w, int h, void* keys_dev) {
  if (!keys_dev) return k ? fail(k, HSK_ERR_ARG, "keys buffer is null") : HSK_ERR_ARG;
  int r = hsk_mgpu_frame_begin(k, depth_dev, w, h);
  if (r != HSK_OK) return r;
  if (k->frame == 0) return HSK_OK;  // first frame: integrate + transformed maps only (frame_begin did it)
  const int set = k->cur;
  const size_t P0 = (size_t)k->lv[0].W * k->lv[0].H;
  auto body = [&]() {
    enqueue_icp(k);  // (k_begin_frame ran in frame_begin; the first fused iteration repeats its bookkeeping: idempotent)
    enqueue_integrate(k);
    launch_raycast(k->stream, k->d_vol, k->d_st, k->vp, k->lv[0].W, k->lv[0].H, k->lv[0].in, k->d_vmod[0], k->d_nmod[0], k->d_keys,
                   k->d_flags);
    (void)hipMemcpyAsync(keys_dev, k->d_keys, P0 * 4, hipMemcpyDeviceToDevice, k->stream);
  };
  if (!k->cfg.use_graph || k->stream == nullptr) {  // (the legacy default stream cannot be captured)
    body();
    HIPCHK(k, hipGetLastError());
    return HSK_OK;
  }
  if (k->sgraph_keys != keys_dev) {  // a different keys buffer: the captured graphs are stale
    for (int i = 0; i < 2; ++i) {
      if (k->sgexec[i]) (void)hipGraphExecDestroy(k->sgexec[i]);
      if (k->sgraph[i]) (void)hipGraphDestroy(k->sgraph[i]);
      k->sgexec[i] = nullptr;
      k->sgraph[i] = nullptr;
    }
    k->sgraph_keys = keys_dev;
  }
  if (!k->sgexec[set]) {
    HIPCHK(k, hipStreamBeginCapture(k->stream, hipStreamCaptureModeThreadLocal));
    body();
    HIPCHK(k, hipStreamEndCapture(k->stream, &k->sgraph[set]));
    HIPCHK(k, hipGraphInstantiate(&k->sgexec[set], k->sgraph[set], nullptr, nullptr, 0));
  }
  HIPCHK(k, hipGraphLaunch(k->sgexec[set], k->stream));
  k->weights_pending = true;
  k->vol_epoch += 1;
  return HSK_OK;
}

extern "C" int hsk_mgpu_icp_accumulate(hsk_ctx* k, int level, int row0, int row1, void* sums27_dev) {
  if (!k || !sums27_dev || level < 0 || level >= HSK_NLEVELS) return HSK_ERR_ARG;
  if (row0 < 0 || row1 > k->lv[level].H || row0 > row1) return fail(k, HSK_ERR_ARG, "row range out of bounds");
  if (row0 == row1) {
    HIPCHK(k, hipMemsetAsync(sums27_dev, 0, 27 * sizeof(double), k->stream));
    return HSK_OK;
  }
  enqueue_icp_row_sums(k, level, row0, row1, (double*)sums27_dev);
  return HSK_OK;
}

extern "C" int hsk_mgpu_icp_update(hsk_ctx* k, const void* sums27_dev) {
  if (!k || !sums27_dev) return HSK_ERR_ARG;
  launch_icp_update(k->stream, (const double*)sums27_dev, k->d_st);
  return HSK_OK;
}

extern "C" int hsk_mgpu_icp_replicated(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  if (k->frame == 0) return fail(k, HSK_ERR_STATE, "no model maps yet: the first frame has no ICP");
  enqueue_icp(k);  // the first fused iteration seeds itself from the tracker state (k_begin_frame already ran: idempotent)
  return HSK_OK;
}

extern "C" int hsk_mgpu_integrate(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  enqueue_integrate(k);
  return HSK_OK;
}

extern "C" int hsk_mgpu_raycast_local(hsk_ctx* k, void* keys_dev) {
  if (!k || !keys_dev) return HSK_ERR_ARG;
  launch_raycast(k->stream, k->d_vol, k->d_st, k->vp, k->lv[0].W, k->lv[0].H, k->lv[0].in, k->d_vmod[0], k->d_nmod[0],
                 k->d_keys, k->d_flags);
  HIPCHK(k, hipMemcpyAsync(keys_dev, k->d_keys, (size_t)k->lv[0].W * k->lv[0].H * 4, hipMemcpyDeviceToDevice, k->stream));
  return HSK_OK;
}

extern "C" int hsk_mgpu_raycast_resolve(hsk_ctx* k, const void* keys_min_dev, void* maps_bits_dev) {
  if (!k || !keys_min_dev || !maps_bits_dev) return HSK_ERR_ARG;
  launch_resolve(k->stream, k->d_keys, (const int*)keys_min_dev, k->d_vmod[0], k->d_nmod[0], (int*)maps_bits_dev,
                 k->lv[0].W * k->lv[0].H);
  return HSK_OK;
}

// direct exchange: this slab's winning pixels straight into every device's composite buffer (dest_bits[d]: int32[6 P],
// device-accessible from this context's device -- local, peer-enabled or IPC-mapped memory)
extern "C" int hsk_mgpu_raycast_push(hsk_ctx* k, const void* keys_min_dev, void* const* dest_bits, int n_dest) {
  if (!k || !keys_min_dev || !dest_bits || n_dest < 1 || n_dest > HSK_PUSH_MAX) return HSK_ERR_ARG;
  PushDests d;
  d.n = n_dest;
  for (int i = 0; i < HSK_PUSH_MAX; ++i) d.p[i] = i < n_dest ? (int*)dest_bits[i] : nullptr;
  launch_resolve_push(k->stream, k->d_keys, (const int*)keys_min_dev, k->d_vmod[0], k->d_nmod[0], d, k->lv[0].W * k->lv[0].H);
  return HSK_OK;
}

// 1 when the next frame starts (or restarts) the scan: frame 0, or tracking was lost by a pipelined frame.  Such a frame
// has no ICP and no composite: hsk_mgpu_frame_begin / hsk_mgpu_frame_front, then the synchronous hsk_mgpu_frame_end.
extern "C" int hsk_mgpu_restart_pending(const hsk_ctx* k) { return k ? (k->frame == 0 || k->pending_reset) : -1; }

// Pipelined end of a tracked slab frame: adopt the composite, rebuild the model pyramid, and queue the pose read-back
// instead of waiting for it -- the host goes on to enqueue the next frame; hsk_wait_frame returns the results in order
// (at most HSK_MAX_IN_FLIGHT outstanding).  Loss semantics are those of hsk_submit_frame_dev: frames already enqueued
// behind a lost one are dropped on the device and report tracked = 0.
extern "C" int hsk_mgpu_frame_end_async(hsk_ctx* k, const void* keys_min_dev, const void* maps_bits_dev) {
  if (!k) return HSK_ERR_ARG;
  if (k->frame == 0 || k->pending_reset) return fail(k, HSK_ERR_STATE, "the first frame of a scan ends with hsk_mgpu_frame_end");
  if (!keys_min_dev || !maps_bits_dev) return fail(k, HSK_ERR_ARG, "composite buffers are null");
  if (k->ring_count >= HSK_MAX_IN_FLIGHT) return fail(k, HSK_ERR_STATE, "too many frames in flight: call hsk_wait_frame first");
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  // the frame's last kernel reports the tracker state into the ring slot assigned here (no copy node, no event record
  // for the pose: see hsk_submit_frame_dev)
  const int slot = (k->ring_head + k->ring_count) % (HSK_MAX_IN_FLIGHT + 1);
  k->h_slot_fifo[k->ring_seq % HSK_RING_FIFO] = slot;
  k->ring_seq += 1;
  k->ring_expect[slot] = k->ring_seq | 0x80000000u;
  ((volatile TrackState*)&k->h_ring[slot])->ring_mark = 0u;
  ((volatile TrackState*)&k->h_ring[slot])->pose_mark = 0u;
  const RingOut ring = {k->d_ring_view, k->d_fifo_view, k->d_ring_seq};
  // (round 6: adopt, the model pyramid and the report in ONE launch -- they were two, with level 0 written and read back between them)
  launch_adopt_pyramid(k->stream, (const int*)keys_min_dev, (const int*)maps_bits_dev, k->lv[0].W, k->lv[0].H, k->d_vmod[0], k->d_nmod[0],
                       k->d_vmod[1], k->d_nmod[1], k->d_vmod[2], k->d_nmod[2], k->d_st, &ring);
  HIPCHK(k, hipEventRecord(k->ev_free[k->cur], k->stream));  // the prefetch of the frame after next waits on it (second stream)
  k->set_used[k->cur] = true;
  k->ring_kind[slot] = 0;
  k->ring_count += 1;
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

extern "C" int hsk_mgpu_frame_end(hsk_ctx* k, const void* keys_min_dev, const void* maps_bits_dev, float pose_out[16],
                                  int* tracked) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const bool first = (k->frame == 0);
  if (!first) {
    if (int ri = require_idle(k)) return ri;
    if (!keys_min_dev || !maps_bits_dev) return fail(k, HSK_ERR_ARG, "composite buffers are null");
    launch_adopt_pyramid(k->stream, (const int*)keys_min_dev, (const int*)maps_bits_dev, k->lv[0].W, k->lv[0].H, k->d_vmod[0], k->d_nmod[0],
                         k->d_vmod[1], k->d_nmod[1], k->d_vmod[2], k->d_nmod[2], k->d_st, nullptr);
  }
  // the frame's image buffers are free again once everything enqueued so far has run
  HIPCHK(k, hipEventRecord(k->ev_free[k->cur], k->stream));
  k->set_used[k->cur] = true;  // k->cur keeps naming this frame's set: downloads of its images read the right buffers
  int r = download_state(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipGetLastError());
  if (first) {
    k->frame = 1;
    return hand_back(k, pose_out, tracked, 0);
  }
  return end_tracked_frame(k, pose_out, tracked);
}
