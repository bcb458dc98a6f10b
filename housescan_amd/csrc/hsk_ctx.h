// hsk_ctx.h -- library-internal, not installed: the context behind the C ABI (include/hskinfu.h) and the host helpers that the
// ABI's four files share -- hskinfu_api.hip (context, frames), api_readout.hip (what reaches the caller), api_volume.hip (what
// replaces or serialises the volume), api_align.hip (registration against the volume).  hskinfu_group.hip takes
// hsk_mark_group_slab from here.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_launch.h"
#include "hsk_volume_image.h"

// image-space buffers of one frame; two sets so that the asynchronous path can preprocess frame k+1 on a second
// stream while frame k is still being tracked / fused / raycast
struct ImgBufs {
  uint16_t* d_raw = nullptr;
  uint16_t* d_dep[HSK_NLEVELS] = {};
  float* d_scaled = nullptr;
  float* d_vcur[HSK_NLEVELS] = {};
  float* d_ncur[HSK_NLEVELS] = {};
  float* d_tmax = nullptr;  // tile tables of the scaled depth (see launch_tile_max)
  unsigned char* d_rgb = nullptr;  // the frame's colour image (RGB8), only once colour is enabled (hsk_enable_color)
};

// a number no other context of the process ever had (a diff names the context it was made with; an address can come back)
inline uint64_t next_ctx_serial() {
  static std::atomic<uint64_t> n{0};
  return n.fetch_add(1) + 1;
}

// A pass over the whole volume whose result stays on the device while the volume stands: the scratch, an optional second
// table buffer that only grows, the vol_epoch it was made at (0: nothing is held; vol_epoch starts at 1) and the key it was made
// for, as bytes.  A build drops what is held before it writes the scratch and stamps it once the result has been read back; an
// error in between leaves nothing held.  (The bodies follow HIPCHK, below.)
struct hsk_ctx;
struct HeldPass {
  void* buf = nullptr;
  size_t bytes = 0;
  void* tab = nullptr;
  size_t tab_bytes = 0;
  uint64_t epoch = 0;
  std::vector<unsigned char> key;
  inline bool stands(const hsk_ctx* k) const;
  bool stands_for(const hsk_ctx* k, const void* kp, size_t n) const { return stands(k) && key.size() == n && (n == 0 || memcmp(key.data(), kp, n) == 0); }
  void drop() { epoch = 0; }
  inline int grow(hsk_ctx* k, size_t want);      // a scratch that has to be made again drops what it held
  inline int grow_tab(hsk_ctx* k, size_t want);  // (the table is filled and read back within one call: nothing held lives in it)
  inline void stamp(const hsk_ctx* k, const void* kp = nullptr, size_t n = 0);
  inline int release(hsk_ctx* k);  // frees both buffers behind what the stream still holds
  // HSK_ERR_STATE "<who><what>" unless it stands
  inline int require(hsk_ctx* k, const char* who, const char* what) const;
};

struct hsk_ctx {
  hsk_config cfg;
  uint64_t serial = next_ctx_serial();
  hipStream_t stream = nullptr;
  bool own_stream = false;
  VolParams vp;
  ImgLevel lv[HSK_NLEVELS];
  float init_R[9], init_t[3];
  // device memory (all sized once at create; nothing is allocated on the frame path)
  void* d_vol = nullptr;
  size_t vol_bytes = 0;
  ImgBufs ib[2];
  int cur = 0;  // set the enqueue_* helpers work on (0 everywhere except inside the overlapped async submission)
  ImgBufs& B() { return ib[cur]; }
  float* d_vmod[HSK_NLEVELS] = {};
  float* d_nmod[HSK_NLEVELS] = {};
  TrackState* d_st = nullptr;
  TrackState* h_st = nullptr;  // pinned
  double* d_partials = nullptr;  // per-block ICP sums of the stage-level accumulate (launch_icp_accumulate)
  void* d_icp_pose = nullptr;     // two IcpPose slots
  double* d_sums = nullptr;
  float h_ws[169] = {};  // bilateral spatial weights (host copy: passed to the kernel by value)
  float* d_wc = nullptr;
  int* d_keys = nullptr;
  unsigned* d_flags = nullptr;       // bitfield, one bit per brick: ever held a negative TSDF
  unsigned char* d_uni = nullptr;    // lane-block summaries (integrate.hip: hsk_uniform_code), one byte per 4x1x4 voxels
  size_t uni_bytes = 0;
  bool weights_pending = false;      // an integrate has been enqueued since the summaries' weights were last written back
  size_t flags_bytes = 0;
  unsigned* d_queue = nullptr;       // integrate pass A -> pass B: count (4 words) + uncertain lane-block ids
  CubeTable* d_cube_tab = nullptr;   // marching-cubes table (hsk_extract_mesh_cubes; filled on first use)
  int2* d_zint = nullptr;            // per lane column: stored-plane range inside the padded frustum
  uint16_t* h_stage = nullptr;  // pinned staging for the incoming depth frame (HSK_MAX_IN_FLIGHT + 1 frames, used in turn)
  unsigned stage_turn = 0;
  unsigned long long* d_counter = nullptr;
  unsigned* d_rowcnt = nullptr;
  unsigned long long* d_rowoff = nullptr;
  // read-out (round 5): what the volume looked like when a product was last counted (a size query followed by the fill
  // finds the rows' counts and offsets in place), a grow-only device buffer for the product, and two pinned staging
  // buffers through which products and the volume reach the caller's pageable memory (lazily allocated)
  uint64_t vol_epoch = 1;       // counted up by everything that changes the volume
  int ro_kind = 0;              // 1 cloud, 2 tetrahedra mesh, 3 cubes mesh, 4 indexed mesh: whose counts d_rowcnt / d_rowoff hold
  uint64_t ro_epoch = 0;
  unsigned long long ro_totals[2] = {0, 0};  // its items; of the indexed mesh the vertices, then the faces
  void* d_out = nullptr;
  size_t out_bytes = 0;
  void* h_pin[2] = {nullptr, nullptr};
  size_t pin_bytes = 0;
  hipEvent_t ev_pin[2] = {};
  int frame = 0;
  std::string err;
  // asynchronous submission ring (hsk_submit_frame_dev / hsk_wait_frame)
  TrackState* h_ring = nullptr;  // pinned, HSK_MAX_IN_FLIGHT + 1 slots
  int* h_slot_fifo = nullptr;    // pinned: ring slot of each pipelined frame, read by the frame's last kernel (RingOut)
  unsigned* d_ring_seq = nullptr;  // device: pipelined frames that have reported
  unsigned ring_seq = 0;         // host mirror: pipelined frames submitted
  unsigned ring_expect[HSK_MAX_IN_FLIGHT + 1] = {};  // mark the frame in each slot will write
  unsigned set_expect[2] = {0, 0};                     // ... and the one that last used each image buffer set
  int set_slot[2] = {-1, -1};
  TrackState* d_ring_view = nullptr;  // device-side addresses of h_ring / h_slot_fifo
  int* d_fifo_view = nullptr;
  hipEvent_t ring_ev[HSK_MAX_IN_FLIGHT + 1] = {};
  int ring_kind[HSK_MAX_IN_FLIGHT + 1] = {};  // 0 tracked-frame candidate, 1 first frame (already complete)
  int ring_head = 0, ring_count = 0;
  bool pending_reset = false;
  int loss_policy = HSK_LOSS_RESET;  // what a lost frame does to the scan (hsk_set_loss_policy; hskinfu_api.hip: after_loss)
  // overlapped preprocessing: stream, per-set events (preprocess done / set free again), per-set graphs of the rest
  hipStream_t pstream = nullptr;
  hipEvent_t ev_pre[2] = {}, ev_free[2] = {};
  hipEvent_t ev_src = nullptr;  // orders the second stream behind the caller's (adopted) stream before a depth copy

  bool set_used[2] = {false, false};
  int async_set = 1;
  const void* pf_ptr = nullptr;   // hsk_mgpu_prefetch: depth pointer whose preprocessing is already enqueued ...
  int pf_set = -1;                // ... into this buffer set (on pstream, ev_pre[pf_set] recorded)
  int mgpu_set = 0;               // buffer set of the slab frame in progress
  hipGraph_t sgraph[2] = {};       // slab frame front (ICP + integrate + local raycast) per buffer set
  hipGraphExec_t sgexec[2] = {};
  void* sgraph_keys = nullptr;     // the keys buffer baked into those graphs
  // hipGraph of the steady-state frame
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  bool graph_ready = false;
  // use_graph = 2: the main-stream chain of a PIPELINED frame (19 ICP launches + 3 integrate + raycast) as one graph per
  // image-buffer set -- the host's cost of a frame is then one launch where it was 23 (what limits several rooms on one GPU)
  hipGraph_t pgraph[2] = {};
  hipGraphExec_t pgexec[2] = {};
  // profiling
  bool prof = false;
  bool prof_levels = false;  // profiling level 2: also an event at every ICP level (they cost about 4 us each)
  hipEvent_t ev[HSK_NSTAGES + 1] = {};
  hipEvent_t ev_icp[HSK_NLEVELS + 1] = {};  // profiling: start of each ICP level (coarsest first) and the end of the last
  double icp_level_ms[HSK_NLEVELS] = {};    // ... summed per level, index = level (0 = finest)
  double stage_ms[HSK_NSTAGES] = {};
  // host time of the pipelined submissions, by phase (hsk_submit_host_us): staging copy, copy + preprocessing enqueue, the
  // wait for the preprocessing, the main-stream chain's enqueue; and the submissions counted
  double submit_us[4] = {};
  unsigned long long submit_n = 0;
  uint64_t prof_frames = 0;
  // colour (hsk_enable_color; all null until then): the (r, g, b, w) volume, row-major; per image-buffer set a device flag "this
  // frame has colour", written when the frame is submitted (the captured graphs read it, with the set's d_rgb); one pinned
  // staging image (its upload has completed before a submission returns, as the depth frame's has)
  unsigned* d_color = nullptr;
  size_t color_bytes = 0;
  int* d_has_color = nullptr;
  unsigned char* h_rgb_stage = nullptr;
  const unsigned char* rgb_src = nullptr;  // the colour of the frame being submitted (h_rgb_stage), null: a depth-only frame
  int color_max_w = 0;
  bool group_slab = false;  // a slab of a group (hsk_group_create*): no colour
  float color_band = 0.0f;
  // the passes held over the volume, each with its scratch (HeldPass; hsk_destroy frees them through `passes`):
  // mi: the indexed mesh's scratch (extract.hip mesh_index_layout), made on first use; only a buffer -- its counts are ro_kind 4's
  // pack: the volume image's class and offset pass (pack.hip: 64 B of counters, the two class tables, the two size / offset
  //   tables, the scan's block sums), keyed by the colour flag; pk_counts its counters
  // comp: the labelling (components.hip comp_layout: counters, row tables, one parent per volume word); tab = the roots
  //   ascending, eight words per component, the survivors of a keep_largest prune (region_tab)
  // fill: the last fill's scratch (fill.hip fill_layout), its mask at fill_mask
  // diff: diff_layout's counters, class words, byte volumes and labelling scratch; tab = the regions' roots, records and class
  //   counts.  Key: cur's serial and cur's vol_epoch (two uint64: hsk_adopt_diff reads them back), then the zero-padded parameters
  // split: split_layout's scratch; tab = the objects' roots and records.  Key: the zero-padded parameters, then the planes
  //   (hsk_remove_objects reads both back)
  // clear: clear_layout's counters, field and intermediates.  Key: the 20 device-relevant parameter bytes (clear_key_of)
  // reach: reach_layout's counters, field, tile flags and worklists.  Key: the clearance key, min_d2, max_cost, then the seed
  //   voxels (those inside the grid, in the caller's order)
  // part: part_layout's scratch; tab = the dense door table of the last build or floor call.  Key: the clearance key and the four
  //   partition parameters
  // simp: the simplified mesh's count pass (simp_layout of the cluster size asked for); tab = what is proportional to the output,
  //   per output vertex its cluster's number and its 20 sums (164 B).  Key: the shift
  HeldPass mi, pack, comp, fill, diff, split, clear, reach, part, simp;
  HeldPass* const passes[10] = {&mi, &pack, &comp, &fill, &diff, &split, &clear, &reach, &part, &simp};
  // scene views (hsk_render_view), made on first use: the free camera's block and the counter slots in device memory, and their
  // pinned host side (the camera on its way in, the counts on their way out)
  void* d_view = nullptr;
  void* h_view = nullptr;
  // volume fusion (hsk_fuse_volume), made on first use as a destination and only grown: 64 B of counters, then the source's
  // brick table (fuse.hip)
  void* d_fuse = nullptr;
  size_t fuse_bytes = 0;
  // the scratch of every call that works on a cloud (align_scratch -> CloudScratch), made on first use and only grown: the
  // alignment's accumulators (align.hip: HSK_ALIGN_ACC_WORDS words), then the cloud's six planes, then what the call carves for
  // itself -- RelocScratch (api_reloc.hip), PlaneScratch (api_planes.hip), LevelScratch (api_level.hip) or SplatScratch
  // (api_splat.hip: the z-buffer, a frame, the views' counters) or NormalScratch (api_normals.hip: the cell table, the points in
  // cell order, the outputs); h_align: the
  // accumulators' pinned host side
  void* d_align = nullptr;
  size_t align_bytes = 0;
  unsigned long long* h_align = nullptr;
  unsigned pk_counts[16] = {};  // the counters of the volume image's pass (pack)
  // surface components (hsk_label_components): comp_recs the records of what `comp` holds, in their order
  uint64_t comp_inside = 0;  // the voxels of all components
  std::vector<hsk_component> comp_recs;
  // hole filling (hsk_fill_holes): where in fill's scratch the last fill's mask lies
  const unsigned char* fill_mask = nullptr;
  // volume differencing (hsk_diff_volume): diff_recs the kept regions' records in their order, diff_stats the call's stats --
  // hsk_diff_volume answers a call with the same cur and parameters from them
  std::vector<hsk_diff_region> diff_recs;
  hsk_diff_stats diff_stats = {};
  // the scene split (hsk_split_scene): split_recs the kept objects' records in their order, split_stats the call's stats --
  // hsk_split_scene answers a call with the same planes and parameters from them
  std::vector<hsk_object> split_recs;
  hsk_split_stats split_stats = {};
  // the clearance field (hsk_build_clearance): its counters
  unsigned long long clear_counts[3] = {0, 0, 0};
  // the reach field (hsk_build_reach): reach_q its geometry and costs (the path trace's), reach_counts its counters,
  // reach_rounds its rounds
  ReachGeom reach_q = {};
  unsigned long long reach_counts[4] = {0, 0, 0, 0};
  uint32_t reach_rounds = 0;
  unsigned long long reach_tiles = 0;  // the tiles relaxed over all rounds of the last hsk_build_reach that built (hsk_reach_tiles_relaxed)
  // the room partition (hsk_build_partition): part_q its geometry, part_recs and part_doors its records in their order,
  // part_counts = passable, cores, kept cores, assigned
  PartGeom part_q = {};
  std::vector<hsk_room> part_recs;
  std::vector<hsk_door> part_doors;
  unsigned long long part_counts[4] = {0, 0, 0, 0};
  uint32_t part_rounds = 0;
  unsigned long long part_tiles = 0, part_first = 0;  // of the last build that built: tiles relaxed over all rounds, tiles of the first worklist
  // the simplified mesh (hsk_extract_mesh_simplified): simp_totals the faces, vertices and clusters of simp's count pass -- a
  // size query followed by the fill counts once, as the other products do
  unsigned long long simp_totals[3] = {0, 0, 0};
  // the keyframe store (hsk_enable_keyframes; hsk_keytex_point.h: KeyStore), one allocation made there and freed by
  // hsk_release_keyframes: key_cap slots of key_slot_bytes(key_w, key_h), key_n of them taken; key_rec = the host's copy of the
  // taken slots' records, 16 floats each (hsk_get_keyframe).  Nothing the tracker reads; hsk_reset leaves it alone
  void* d_key = nullptr;
  int key_cap = 0, key_w = 0, key_h = 0, key_n = 0;
  std::vector<float> key_rec;
};

#define HIPCHK(k, call)                                                                        \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      char buf_[512];                                                                          \
      snprintf(buf_, sizeof(buf_), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      (k)->err = buf_;                                                                         \
      return HSK_ERR_HIP;                                                                      \
    }                                                                                          \
  } while (0)

// the truncation distance of a configuration (hsk_create's tau): trunc_dist_m, but at least 2.1 times the largest cell
inline float config_tau(const hsk_config* c) {
  float m = c->vol_size_m[0] / (float)c->vol_x;
  const float cy = c->vol_size_m[1] / (float)c->vol_y, cz = c->vol_size_m[2] / (float)c->vol_z;
  m = m > cy ? m : cy;
  m = m > cz ? m : cz;
  const float lo = 2.1f * m;
  return c->trunc_dist_m > lo ? c->trunc_dist_m : lo;
}

// ---- hskinfu_api.hip ----
std::string& create_error();  // the thread's message of the calls that have no context (hsk_last_error(NULL))
int fail(hsk_ctx* k, int code, const char* msg);
void pose16_to_rt(const float m[16], float R[9], float t[3]);
void rt_to_pose16(const float R[9], const float t[3], float m[16]);
void flush_weights(hsk_ctx* k);
int upload_state(hsk_ctx* k);
int download_state(hsk_ctx* k);
void leave_slab_bookkeeping(hsk_ctx* k);
int set_pose_internal(hsk_ctx* k, const float pose[16]);
void enqueue_raycast_and_resize(hsk_ctx* k, int* keys, bool report = false);
int preprocess_frame(hsk_ctx* k, const uint16_t* depth, int w, int h);  // hsk_preprocess behind its argument checks
void enqueue_integrate_staged(hsk_ctx* k);  // the scaled depth and the integrate of the frame in B().d_raw, at the device state's pose
void hsk_mark_group_slab(hsk_ctx* k);  // hsk_group_create* marks the contexts it makes as slabs, whatever planes they own
// the state a call needs, or its refusal (HSK_ERR_STATE): no frame in flight; colour enabled; a context that stores its whole
// volume ("<who>: not for a slab (<sentence>)").  `errs` takes the message: hsk_fuse_volume asks of its source, too, and reports
// in its destination.
int require_idle(const hsk_ctx* k, hsk_ctx* errs);
inline int require_idle(hsk_ctx* k) { return require_idle(k, k); }
int require_color(hsk_ctx* k);
int require_whole_volume(const hsk_ctx* k, hsk_ctx* errs, const char* who, const char* sentence = "a context that stores part of its volume");
// ---- api_volume.hip ----
// The volume's content was replaced: the brick bitfield and both summary levels are made again from the volume as it now is,
// behind whatever wrote it on the stream.  Enqueues only; the caller synchronises.
int volume_replaced(hsk_ctx* k);
// ---- products.cpp ----
uint32_t plane_lcg_next(uint64_t* state);  // hsk_detect_planes' generator: one step, the state in place
// ---- api_align.hip ----
int align_check(hsk_ctx* dst, const float src_to_dst[16], const hsk_align_params* params, hsk_align_params* p, const char* who);
// The scratch of a cloud of np points (d_align): the accumulators, the cloud's six planes `pitch` floats apart at `soa`, then
// `extra` bytes of the caller's at `extra` (256-byte aligned; a caller carves them with ProductLayout)
struct CloudScratch {
  unsigned pitch = 0;
  float* soa = nullptr;
  void* extra = nullptr;
};
int align_scratch(hsk_ctx* k, size_t np, size_t extra, CloudScratch* s);
// The caller's packed triples, every stride-th of them -- n points in all --, into the scratch's planes: six, or, normals null, the
// three of the positions.  *n_invalid (may be null; asks for normals): the points hsk_plane_point.h calls invalid.  HSK_ERR_STATE:
// "<who>: out of host memory for the cloud".  Returns with the copy done.
int cloud_upload(hsk_ctx* k, const float* xyz, const float* normals, size_t n, size_t stride, const CloudScratch& s, size_t* n_invalid,
                 const char* who);
// The volume's own cloud -- the n > 0 points cloud_count found -- in the planes of a scratch with `extra` bytes behind them: written
// by the cloud's second pass and gathered on the device.  Enqueues only.
int cloud_from_volume(hsk_ctx* k, size_t n, size_t extra, CloudScratch* s);
int align_run(hsk_ctx* k, const hsk_align_params& p, const float* d_soa, size_t np, unsigned pitch, const float src_to_dst[16], float m_out[16],
              hsk_align_stats* st);
// ---- api_reloc.hip ----
// every one of the n_poses matrices (16 floats each) is rigid (hsk_invert_rigid), or HSK_ERR_ARG: "<who>: pose <index> is not rigid ..."
int check_poses(hsk_ctx* k, const float* poses, size_t n_poses, const char* who);
// ---- api_components.hip ----
int ensure_grown(hsk_ctx* k, void** buf, size_t* have, size_t want);  // a device buffer of at least `want` bytes, its content not kept
inline bool HeldPass::stands(const hsk_ctx* k) const { return buf && epoch == k->vol_epoch; }
inline int HeldPass::grow(hsk_ctx* k, size_t want) {
  if (bytes < want) drop();
  return ensure_grown(k, &buf, &bytes, want);
}
inline int HeldPass::grow_tab(hsk_ctx* k, size_t want) { return ensure_grown(k, &tab, &tab_bytes, want); }
inline void HeldPass::stamp(const hsk_ctx* k, const void* kp, size_t n) {
  key.assign((const unsigned char*)kp, (const unsigned char*)kp + n);
  epoch = k->vol_epoch;
}
inline int HeldPass::release(hsk_ctx* k) {
  if (buf || tab) HIPCHK(k, hipStreamSynchronize(k->stream));
  for (void** b : {&buf, &tab})
    if (*b) {
      HIPCHK(k, hipFree(*b));
      *b = nullptr;
    }
  bytes = tab_bytes = 0;
  drop();
  return HSK_OK;
}
inline int HeldPass::require(hsk_ctx* k, const char* who, const char* what) const {
  return stands(k) ? HSK_OK : fail(k, HSK_ERR_STATE, (std::string(who) + what).c_str());
}
// The host's half of "labelled regions -> records" for a labelling in b (launch_comp_label has run): the root count is read and
// more than 2^24 refused with `too_many` (null: no refusal -- r->n says it, nothing else is done); the host vectors are sized
// (`no_memory` when they cannot be); pass's table is grown to roots, eight words a region, extra_words more a region and
// tail_bytes behind them (region_tab); launch_comp_records runs, then -- minor_cls not null -- the MINOR step on those class words
// (the regions below min_voxels stop being members), then -- extra not null -- the caller's record kernel, which writes the extra
// words; roots, table and extra words come back, and the stream has drained.  hsk_comp_point.h's comp_region_records turns them
// into the ABI's records.
struct RegionTab {
  size_t bytes;
  unsigned *roots, *table, *extra;
};
RegionTab region_tab(const HeldPass& pass, size_t n, size_t extra_bytes);
struct RegionRead {
  unsigned n = 0;
  std::vector<unsigned> roots, table, extra;
};
int region_read(hsk_ctx* k, const CompBufs& b, HeldPass* pass, size_t extra_words, size_t tail_bytes, const char* too_many, const char* no_memory,
                void* minor_cls, uint64_t min_voxels, const std::function<void(const RegionTab&, unsigned)>& extra, RegionRead* r);
// The tail of a call that writes the volume: the deferred weights are written back (the words that stay are to hold theirs), `launch`
// writes, volume_replaced follows it, and the stream drains.  The caller drops its own held pass.
int commit_volume_write(hsk_ctx* k, const std::function<void()>& launch);
// the held records into the caller's array, or their count: *n_out is the count; recs null: that is all; cap below it: `message`
template <class T>
int reply_records(hsk_ctx* k, const std::vector<T>& held, T* recs, size_t cap, size_t* n_out, const char* message) {
  *n_out = held.size();
  if (!recs) return HSK_OK;
  if (cap < held.size()) return fail(k, HSK_ERR_ARG, message);
  if (!held.empty()) memcpy(recs, held.data(), held.size() * sizeof(T));
  return HSK_OK;
}
// ---- api_clearance.hip ----
// the cells and the truncation distance of this context, or (k null) of hsk_default_config(256)
void context_cells(const hsk_ctx* k, float cell[3], float* tau);
// the arguments of an _at call, or HSK_ERR_ARG: "<who>: null argument" (n > 0 points without xyz or out), "<who>: more than 2^20
// points", "<who>: radius must lie in 0..<max_radius>" (max_radius negative: the call takes no radius)
int points_check(hsk_ctx* k, const char* who, const void* xyz, const void* out, size_t n, int radius, int max_radius);
// ---- api_clearance.hip ----
// the parameters a clearance call works with (NULL: the defaults), checked -> the kernels' block; the field of the volume as it
// stands, in clear's scratch (*reused: nothing had to be launched)
int clear_check(hsk_ctx* k, const hsk_clearance_params* params, const char* who, hsk_clearance_params* p, ClearGeom* q);
// the state a pass over a whole volume needs of k, reported in `errs`: require_whole_volume's and require_idle's refusals, and a
// volume lin can number (HSK_ERR_ARG: "<who>: the volume has more than 2^31 voxels")
int volume_state_check(hsk_ctx* k, hsk_ctx* errs, const char* who);
int clear_build(hsk_ctx* k, const hsk_clearance_params& p, const ClearGeom& q, bool* reused);
void clear_key_of(const hsk_clearance_params& p, uint32_t key[5]);
// the box a read works on (NULL: the whole volume) in *b and its voxels in *n, or HSK_ERR_ARG: "<who>: the box must satisfy ..."
int clear_box_check(hsk_ctx* k, const hsk_voxel_box* box, const char* who, hsk_voxel_box* b, size_t* n);
// a floor map's grid, (u, v, 1) with u the lower-numbered of the two axes that remain: their numbers and lengths, and the weights
// permuted to (u, v, axis); the axis and the band lo <= p < hi are checked first ("<who>: axis must be ...", "<who>: the band ...")
struct FloorGrid {
  int au, av;
  unsigned nu, nv, w[3];
};
int clear_floor_grid(hsk_ctx* k, const ClearGeom& q, int axis, int lo, int hi, const char* who, FloorGrid* f);
// the tail of a box download: the n voxels of the checked box b of a row-major device field (elem_bytes 1 or 4 a voxel) into out.
// n == 0: nothing; the whole volume: one copy; else through the product buffer
int download_rows(hsk_ctx* k, const void* field, size_t elem_bytes, const hsk_voxel_box& b, size_t n, void* out);
// n > 0 points (packed triples) go to the product buffer, launch(device points, device words, device bytes) gathers a word a point
// and -- bytes not null -- a byte a point, the n words come back into out (may be null) and the n bytes into bytes
int gather_points(hsk_ctx* k, const float* xyz, size_t n, uint32_t* out, const std::function<void(const float*, unsigned*, unsigned char*)>& launch,
                  uint8_t* bytes = nullptr);
// ---- api_reach.hip ----
// The rounds of a tile relaxation: while the current worklist holds tiles -- n_active at first, in list 0 --, launch_round(cur, its
// length) relaxes them and fills the other list, whose length the host then reads from lengths[cur ^ 1] on the device.  *rounds and
// *tiles: the rounds run and the tiles relaxed.  HSK_ERR_STATE after HSK_REACH_MAX_ROUNDS: "<what> did not settle within ..."
int relax_rounds(hsk_ctx* k, const std::function<hipError_t(int, unsigned)>& launch_round, const unsigned long long* lengths, unsigned long long n_active,
                 const char* what, uint32_t* rounds, unsigned long long* tiles);
// ---- api_texture.hip ----
// hsk_bake_texture (kb null) and hsk_bake_texture_keyframes behind their own checks: the layout, the upload, the launch and the
// way back.  kb: the store and the rule's parameters, the source plane (may be null) and the call's second info (may be null)
struct KeyStore;
struct KeyArgs;
struct KeyBake {
  const KeyStore* ks;
  const KeyArgs* ka;
  uint8_t* source;
  hsk_keytex_info* kinfo;
};
int texture_bake(hsk_ctx* k, const char* who, const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces,
                 const hsk_texture_params* params, uint8_t* rgb, uint8_t* normal_rgb, uint8_t* mask, size_t cap_texels, float* uv,
                 hsk_texture_chart* charts, hsk_texture_info* info, const KeyBake* kb);
// ---- api_readout.hip ----
int ensure_pinned(hsk_ctx* k);
void parallel_memcpy(void* dst, const void* src, size_t bytes);
int copy_out(hsk_ctx* k, void* dst, const void* src_dev, size_t bytes);
int ensure_product_bytes(hsk_ctx* k, size_t want, bool headroom = true);
int read_u64(hsk_ctx* k, unsigned long long* dst, const unsigned long long* src_dev, int n = 1);
// the cloud's count pass (shared with hsk_extract_cloud / hsk_extract_cloud_attrs) and, behind it, all n > 0 points with their
// normals (packed triples) written into the product buffer and left there
int cloud_count(hsk_ctx* k, size_t* total);
int cloud_attrs_on_device(hsk_ctx* k, size_t n, const float** d_xyz, const float** d_normals);
// the product buffer carved into the arrays of one product, each 256-byte aligned: take() -> the next array's offset
struct ProductLayout {
  size_t bytes = 0;
  size_t take(size_t n) {
    const size_t at = bytes;
    bytes += (n + 255) & ~(size_t)255;
    return at;
  }
};
// The arrays of one product in the product buffer.  add(host pointer or null, bytes, keep) in order -> the array's number; an
// array that is neither handed out (a host pointer) nor kept for a device consumer (keep) takes no space.  place() sizes the
// buffer once; dev<T>(i) is array i's device pointer (null when absent); copy_out() brings the arrays that have a host pointer to
// the caller through the pinned pair, in that order, and stops at the first error.
struct ProductArrays {
  ProductLayout lay;
  int n = 0;
  void* host[5];
  size_t at[5], len[5];
  char* base = nullptr;
  int add(void* h, size_t bytes, bool keep = false) {
    host[n] = h;
    len[n] = (h || keep) ? bytes : 0;
    at[n] = lay.take(len[n]);
    return n++;
  }
  int place(hsk_ctx* k) {
    const int r = ensure_product_bytes(k, lay.bytes);
    base = (char*)k->d_out;
    return r;
  }
  template <class T>
  T* dev(int i) const { return len[i] ? (T*)(base + at[i]) : nullptr; }
  int copy_out(hsk_ctx* k) const {
    int r = HSK_OK;
    for (int i = 0; i < n && r == HSK_OK; ++i)
      if (host[i] && len[i]) r = ::copy_out(k, host[i], base + at[i], len[i]);
    return r;
  }
};
