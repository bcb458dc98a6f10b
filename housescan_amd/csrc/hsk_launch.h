// hsk_launch.h -- launcher prototypes shared between the kernel translation units and the C-ABI layer.
#pragma once
#include "hsk_dev.h"
#include "hsk_icp_dev.h"

// what the *_layout functions below carve a pass's scratch with: take(n) -> the next array of n bytes, 256-byte aligned, of the
// device buffer at `base` (null: the sizes only); `bytes`: what has been taken
struct ScratchCarve {
  void* base;
  size_t bytes = 0;
  char* take(size_t n) {
    char* p = base ? (char*)base + bytes : nullptr;
    bytes += (n + 255) & ~(size_t)255;
    return p;
  }
};

// volume
void launch_integrate(hipStream_t s, void* vol, const float* scaled, const TrackState* st, const VolParams& vp, int W,
                      int H, Intr in, bool count_only, unsigned long long* counter, unsigned* flags,
                      const float* tmax, int2* zint, unsigned* queue, const IcpFinal* icp_final = nullptr,
                      unsigned char* uni = nullptr, const RingOut* early = nullptr);
size_t uniform_bytes(const VolParams& vp);  // lane-block summaries (integrate.hip: hsk_uniform_code)
size_t uniform_lane_bytes(const VolParams& vp);  // ... of which the lane-block bytes; the wave-chunk bytes of the coarse level follow
void launch_rebuild_uniform(hipStream_t s, const void* vol, const VolParams& vp, unsigned char* uni);
void launch_materialize(hipStream_t s, void* vol, const VolParams& vp, unsigned char* uni);  // before anything reads weights
size_t integrate_queue_words(const VolParams& vp);
size_t integrate_queue_counter_words();  // the head of the queue buffer that holds the counters ...
unsigned long long integrate_queue_entries(const unsigned* counter_words);  // ... and their sum, from a host copy of it
unsigned long long integrate_queue_light_entries(const unsigned* counter_words);  // ... and of the light class (free space over holes)
size_t integrate_cflag_offset_bytes(const VolParams& vp);  // the coarse level's verdict bytes inside the zint buffer ...
size_t integrate_chunk_count(const VolParams& vp);         // ... one per wave-chunk
size_t integrate_zint_entries(const VolParams& vp);  // column z ranges + workgroup z ranges (launch_integrate's zint)
void launch_tile_max(hipStream_t s, const float* scaled, int W, int H, float* tmax);
void launch_tile_fine(hipStream_t s, const float* scaled, int W, int H, float* tiles);
void launch_tile_tables(hipStream_t s, int W, int H, float* tiles);  // the window forms + the sparse table, from the raw tables
size_t tile_table_bytes(int W, int H);  // allocation of `tiles` (launch_tile_max + launch_tile_fine fill it)
void launch_rebuild_flags(hipStream_t s, const void* vol, const VolParams& vp, unsigned* flags);
// stored planes [zz0, zz0 + nz) of the volume (64-B blocks, hsk_dev.h: hsk_vox_index) to / from a row-major device array
void launch_vol_to_linear(hipStream_t s, const void* vol, const VolParams& vp, int zz0, int nz, void* lin);
void launch_vol_from_linear(hipStream_t s, void* vol, const VolParams& vp, int zz0, int nz, const void* lin);
void launch_raycast(hipStream_t s, const void* vol, const TrackState* st, const VolParams& vp, int W, int H, Intr in,
                    float* vmap, float* nmap, int* keys, const unsigned* flags, const MapPyramid* pyramid = nullptr,
                    const RingOut* ring = nullptr);
bool raycast_can_fuse_pyramid(const VolParams& vp, int W, int H);
// scene views (view.hip).  The camera of a view lives in device memory: a ViewCam block the host fills by a copy -- or the
// TrackState itself, which begins with the same twelve floats (`follow`: the tracker's pose as the stream has it by then)
struct ViewCam {
  float R[9], t[3];   // cam->world
};
// one view: the march of launch_raycast for a whole (unsharded) volume from `cam`, shaded by `mode` (HSK_VIEW_*); rgb (3 B per
// pixel), depth (millimetres), vmap, nmap (3 planes each) may each be null; counts: HSK_VIEW_COUNT_SLOTS slots of 16 words, a wave
// adds its hits to word 0 and its hits without colour to word 1 of its tile's slot
#define HSK_VIEW_COUNT_SLOTS 64
void launch_render_view(hipStream_t s, const void* vol, const unsigned* colv, const ViewCam* cam, const VolParams& vp, int W, int H,
                        Intr in, const unsigned* flags, int mode, const float light[3], int light_in_camera,
                        const unsigned char background[3], unsigned char* rgb, unsigned short* depth, float* vmap, float* nmap,
                        unsigned long long* counts);
int view_warm();      // loads view.hip's code object (hsk_prepare_readout); a hipError_t
// section views (section.hip): launch_render_view's arguments, and what makes a section of a view -- the projection (HSK_PROJ_*),
// the clip planes (keep a x + b y + c z + d >= 0, world coordinates), the kind of light and the colour of a cut pixel; counts: a
// wave adds its shown hits to word 0, those without colour to word 1 and its cut pixels to word 2 of its tile's slot
struct SectionPlane {
  float a, b, c, d;
};
struct SectionClip {
  int projection, n_clip;
  SectionPlane plane[4];
};
void launch_render_section(hipStream_t s, const void* vol, const unsigned* colv, const ViewCam* cam, const VolParams& vp, int W, int H,
                           Intr in, const unsigned* flags, int mode, const float light[3], int light_in_camera, int light_directional,
                           const unsigned char background[3], const unsigned char cut_rgb[3], const SectionClip& clip,
                           unsigned char* rgb, unsigned short* depth, float* vmap, float* nmap, unsigned long long* counts);
int section_warm();   // loads section.hip's code object (hsk_prepare_readout); a hipError_t
void launch_resolve(hipStream_t s, const int* keys_local, const int* keys_min, const float* vmap, const float* nmap,
                    int* bits, int P);
// the end of a z-slab frame in ONE launch: k_adopt + k_resize_maps2 (+ the report into the host ring) fused (kernels_image.hip)
void launch_adopt_pyramid(hipStream_t s, const int* keys_min, const int* bits, int W, int H, float* v0, float* n0, float* v1, float* n1,
                          float* v2, float* n2, const TrackState* st, const RingOut* ring);
void launch_resolve_push(hipStream_t s, const int* keys_local, const int* keys_min, const float* vmap, const float* nmap,
                         const PushDests& dst, int P);
int extract_warm();   // loads extract.hip's code object (hsk_prepare_readout); a hipError_t
// the products' two passes (extract.hip): without an output buffer the count pass (the rows' counts and offsets, the total),
// with one the write pass behind it
void launch_extract(hipStream_t s, const void* vol, const VolParams& vp, unsigned* row_count,
                    unsigned long long* row_offset, unsigned long long* total, float* xyz, unsigned long long cap,
                    const unsigned* flags);
size_t hsk_scan_scratch_entries(int nrows);  // entries of a row_offset buffer for nrows rows (the offsets, then the scan's block sums)
// the cloud's write pass with normals and colour (either may be null), behind launch_extract's count pass (extract.hip)
void launch_extract_attrs(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const unsigned* row_count,
                          const unsigned long long* row_offset, float* xyz, float* normals, unsigned char* rgb,
                          unsigned long long cap, unsigned long long* n_uncolored, const unsigned* flags);
// colour volume (color.hip): one frame's colour into the row-major (r, g, b, w) words `col`, behind the frame's integrate
void launch_color_integrate(hipStream_t s, unsigned* col, const TrackState* st, const int* has_color, const float* scaled,
                            const unsigned char* rgb, const float* tiles, const VolParams& vp, int W, int H, Intr in, float band,
                            int max_w);
// volume fusion (fuse.hip): the source's brick table -- one bit per 8^3 brick, "holds an observed voxel", fuse_table_words
// words zeroed by the caller -- then the sweep of the destination footprint `box` (x0 x1 y0 y1 z0 z1, half-open, not empty);
// (A, b) maps destination to source coordinates; colour is merged when both colour volumes are given; counts: [0] voxels
// fused, [1] voxels coloured, [2] chunks swept (zeroed by the caller); *chunks_total: the chunks of the footprint
size_t fuse_table_words(const VolParams& sv);
void launch_fuse_bricks(hipStream_t s, const void* src_vol, const VolParams& sv, unsigned* tab);
void launch_fuse_sweep(hipStream_t s, const void* src_vol, const unsigned* src_col, void* dst_vol, unsigned* dst_col, const VolParams& sv,
                       const VolParams& dv, const float A[9], const float b[3], const int box[6], const unsigned* tab, int max_w,
                       unsigned long long* counts, unsigned long long* chunks_total);

// volume alignment (align.hip): one iteration's sums over n points -- six planes of `pitch` floats each at
// `soa` (x, y, z, nx, ny, nz in source coordinates) -- moved by (R, t) and probed in the destination volume.  acc:
// HSK_ALIGN_ACC_WORDS 64-bit words zeroed by the caller: HSK_ALIGN_SHARDS rows of 32, in each the 28 sums as integers in
// units of 2^-26 (two's complement) and, in word 28, the contributing points
#define HSK_ALIGN_SHARDS 16
#define HSK_ALIGN_ACC_WORDS (HSK_ALIGN_SHARDS * 32)
struct AlignPose {
  float R[9], t[3];
};
void launch_align_iter(hipStream_t s, const void* dst_vol, const VolParams& dv, const float* soa, unsigned n, unsigned pitch,
                       const AlignPose& m, int probes, float cos_gate, unsigned long long* acc);

// pose scoring (reloc.hip): the n points of the planes x, y, z at `soa` (`pitch` floats apart) under each of
// n_poses poses (12 floats each: R row-major, then t).  partial: n_poses x reloc_slabs(n, n_poses) x 8 64-bit words of scratch;
// scores: n_poses records, written whole (nothing needs zeroing).  Nothing is launched with n == 0 or n_poses == 0.
#define HSK_RELOC_MAX_SLABS 32
struct hsk_pose_score;
unsigned reloc_slabs(unsigned n, unsigned n_poses);
void launch_reloc_score(hipStream_t s, const void* dst_vol, const VolParams& dv, const float* soa, unsigned n, unsigned pitch,
                        const float* poses12, unsigned n_poses, unsigned long long* partial, hsk_pose_score* scores);
// every stride-th of the P pixels of a vertex map and its normal map (three planes each), np = ceil(P / stride) of them, as
// the alignment's six planes; a normal that faces away from the camera is negated
void launch_reloc_gather(hipStream_t s, const float* vmap, const float* nmap, unsigned P, unsigned stride, unsigned np, unsigned pitch,
                         float* soa);

// scan coverage (cover.hip).  rays: the probe's rays (hsk_cover_point.h: CoverProbe) under each of n_poses
// poses (12 floats each: R row-major, then t) add their classes and gain to scores[pose] -- ZEROED by the caller -- and store the
// pose's eye_state; with any of cls / depth / gain (W x H each, n_poses == 1) the rays' own values too.  census: the counts of
// the box a CoverSweep describes (cover_sweep: inside the grid, not empty) -> out10 = hsk_coverage's ten words; partial:
// cover_census_blocks x 10 words of scratch.
struct hsk_view_score;
struct CoverProbe;
struct CoverSweep {
  int X, Y, Z;                       // the grid (a whole volume: every plane stored)
  int c0, ncols, by0, nby, bz0, nbz;  // the sweep: vector columns [c0, c0 + ncols), brick rows and brick layers likewise
  int lo[3], hi[3];                  // the box
};
void launch_cover_rays(hipStream_t s, const void* vol, const VolParams& vp, const CoverProbe& pr, const float* poses12, unsigned n_poses,
                       hsk_view_score* scores, unsigned char* cls, unsigned short* depth, unsigned short* gain);
CoverSweep cover_sweep(const VolParams& vp, const int lo[3], const int hi[3]);
unsigned cover_census_blocks(const CoverSweep& g);
void launch_cover_census(hipStream_t s, const void* vol, const CoverSweep& g, unsigned long long* partial, unsigned long long* out10);
int cover_warm();     // loads cover.hip's code object (hsk_prepare_readout); a hipError_t

// what the passes over a WHOLE volume share (volume_sweep.hip; hsk_vol_sweep.h the device text).  A row-major byte volume of zeros
// and ones dilated by the Chebyshev radius r <= 8, an axis a launch: x a -> b, y b -> a, z a -> b -- the result is in b, a is
// overwritten.  The n > 0 elements (elem_bytes 1 or 4 each) of the box lo <= (x, y, z) < hi of a row-major field, row-major.
void launch_mask_dilate3(hipStream_t s, const VolParams& vp, unsigned char* a, unsigned char* b, int r);
void launch_box_rows(hipStream_t s, const void* field, size_t elem_bytes, const VolParams& vp, const int lo[3], const int hi[3], size_t n, void* out);
int sweep_warm();     // loads volume_sweep.hip's code object (hsk_prepare_readout); a hipError_t

// surface components (components.hip) of a WHOLE volume.  The scratch, carved out of one device buffer by
// comp_layout: `rows` = one word per grid row (y, z) and one more, the rows' root counts, then -- launch_pack_scan in place -- their
// first root's index; `parent` = one word per volume word, a voxel's at the voxel's own place (hsk_vox_index).
struct CompBufs {
  unsigned* counts;   // 16 words: [0..7] launch_pack_scan's ([4]: the roots)
  unsigned* rows;     // Y * Z + 1 words
  unsigned* bsum;     // the scan's block sums
  unsigned* parent;   // hsk_vol_words
};
size_t comp_layout(const VolParams& vp, void* base /* null: the size only */, CompBufs* b);
// label: parent[v] = the root of v's component for every INSIDE voxel, 0xFFFFFFFF elsewhere; rows' counts -> offsets; the number
// of roots in counts[4]
void launch_comp_label(hipStream_t s, const void* vol, const VolParams& vp, const CompBufs& b);
// behind it, with n > 0 roots: roots[0, n) ascending; table: 8 words per root -- voxels, lo (3), hi (3, exclusive), 0
void launch_comp_records(hipStream_t s, const VolParams& vp, const CompBufs& b, unsigned n, unsigned* roots, unsigned* table);
// the voxels of the components with fewer than min_voxels voxels or -- n_keep > 0 -- whose root is not among keep[0, n_keep)
// (ascending) get the fill word (fill_free: the weight kept, the TSDF +1; else 0) and the colour word 0 (col may be null)
void launch_comp_prune(hipStream_t s, void* vol, unsigned* col, const VolParams& vp, const unsigned* parent, const unsigned* roots,
                       const unsigned* table, unsigned n, unsigned min_voxels, const unsigned* keep, unsigned n_keep, bool fill_free);
int comp_warm();      // loads components.hip's code object (hsk_prepare_readout); a hipError_t

// the clearance field (clearance.hip) of a WHOLE volume: what the kernels take of the grid and the parameters
// (the reaches computed once on the host), and the scratch, carved out of one device buffer by clear_layout -- 2.5 times the
// volume's bytes: the field and the y pass's sums (uint32 a voxel each), the x pass's distances (uint16), all row-major, x fastest
struct ClearGeom {
  unsigned X, Y, Z, Zg, nw;   // the grid; its plane groups; the 64-bit mask words of a row
  unsigned w[3], R[3];        // the axis weights and reaches
  unsigned max_d2, flags;
};
struct ClearBufs {
  unsigned long long* stats;  // 8 words: [0] obstacles, [1] FAR voxels, [2] the largest value that is not FAR
  unsigned* field;
  unsigned* tmp;
  unsigned short* dx;
};
size_t clear_layout(const VolParams& vp, void* base /* null: the size only */, ClearBufs* b);
void launch_clear_build(hipStream_t s, const void* vol, const ClearGeom& q, const ClearBufs& b);
// the floor map of the band lo <= p < hi along `axis`: a, b = two arrays of one word per column; the map ends in a
void launch_clear_floor(hipStream_t s, const void* vol, const VolParams& vp, const ClearGeom& q, int axis, int lo, int hi, unsigned* a, unsigned* b);
void launch_clear_gather(hipStream_t s, const unsigned* field, const VolParams& vp, const float* xyz, unsigned n, unsigned* out);

// the reach field (reach.hip) of any X Y Z grid of clearance values -- the volume's field, or a floor map with
// Z = 1: the grid, its tiles (hsk_reach_point.h: REACH_TILE_*), the two bounds and the 27 move costs; and the scratch, carved out
// of one device buffer by reach_layout -- the uint32 field, row-major as the clearance field, and per tile two flag words and
// two worklist words
struct ReachGeom {
  unsigned X, Y, Z, ntx, nty, ntz;
  unsigned min_d2, max_cost;
  unsigned cost[27];
};
struct ReachBufs {
  unsigned long long* counters;  // 8 words: [0] passable, [1] reached, [2] ~ the largest value, [3] seeds used, [4], [5] the worklists' lengths
  unsigned* field;
  unsigned* flags[2];            // a word per tile: on the worklist of the same number
  unsigned* list[2];
};
void reach_geom(unsigned X, unsigned Y, unsigned Z, const unsigned w[3], unsigned min_d2, unsigned max_cost, ReachGeom* q);
size_t reach_layout(const ReachGeom& q, void* base /* null: the size only */, ReachBufs* b);
// init: counters and flags cleared, BLOCKED / UNREACHED from the clearance values d2; seed: n_seeds > 0 voxels (linear indices inside
// the grid) -> worklist 0; round: relaxes the n_active > 0 tiles of worklist `cur` and fills the other, whose length is zeroed first;
// stats: counters [1] and [2] of the finished field ([2] as the complement of the largest value, all ones when none).  init and
// round clear device words first and return the first error of their calls
hipError_t launch_reach_init(hipStream_t s, const unsigned* d2, const ReachGeom& q, const ReachBufs& b);
void launch_reach_seed(hipStream_t s, const ReachGeom& q, const ReachBufs& b, const unsigned* seeds, unsigned n_seeds);
hipError_t launch_reach_round(hipStream_t s, const ReachGeom& q, const ReachBufs& b, int cur, unsigned n_active);
void launch_reach_stats(hipStream_t s, const ReachGeom& q, const ReachBufs& b);
// the path from the voxel `goal` back to a seed: out = its first `cap` voxels (x, y, z each) from the goal on; result[0] = its
// length (0: the goal holds no value), result[1] = 1 when the walk met a voxel without a move of the path rule
void launch_reach_path(hipStream_t s, const unsigned* field, const ReachGeom& q, unsigned goal, unsigned long long cap, int* out,
                       unsigned long long* result);

// the room partition (partition.hip) of any X Y Z grid of clearance values -- the volume's field, or a floor
// map with Z = 1: the grid, the reach field's tiles, the thresholds, the axis weights (the point lookup's) and the 27 move costs;
// and the scratch, carved out of one device buffer by part_layout -- 12 bytes a voxel: the 64-bit keys (G << 32 | label) and the
// uint32 parents of the core labelling, both row-major as the clearance field; per tile two flag words and two worklist words;
// the kept roots as the device found them and in ascending order, the rank (room id) of each, 16 words of sums per room
#define PART_REC_WORDS 16   // per room: n_voxels, n_core_voxels, sum x y z, ~lo x y z, hi x y z (inclusive), max_d2, max_g (hsk_part_recs)
#define PART_DOOR_WORDS 8   // per pair of rooms, 64 bytes: sum2 x y z, then as uint32 n_faces x y z, ~lo x y z, hi x y z (inclusive), max_d2
struct PartGeom {
  unsigned X, Y, Z, ntx, nty, ntz;
  unsigned core_d2, min_d2, min_core, max_cost;
  unsigned w[3];
  unsigned cost[27];
};
struct PartBufs {
  unsigned long long* counters;  // 16 words: [0] passable, [1] cores, [2] kept cores, [4], [5] the worklists' lengths
  unsigned long long* keys;
  unsigned* parent;
  unsigned* flags[2];
  unsigned* list[2];
  unsigned* roots_found;         // 1024: the kept roots in the order the device met them
  unsigned* roots;               // 1024: ascending
  unsigned* rank;                // 1024: the room id of roots[i]
  unsigned long long* recs;      // 1024 x PART_REC_WORDS
};
void part_geom(unsigned X, unsigned Y, unsigned Z, const unsigned w[3], unsigned core_d2, unsigned min_d2, unsigned min_core, unsigned max_cost,
               PartGeom* q);
size_t part_layout(const PartGeom& q, void* base /* null: the size only */, PartBufs* b);
// label: counters cleared; the 6-connected components of the core voxels of d2, parent[v] = the smallest lin of v's core (COMP_NONE:
// no core voxel); the voxels of every core counted and the cores with at least min_core voxels put into roots_found (the first
// 1024 of them; counters [1] and [2] count them all).  init: with n_kept <= 1024 ascending roots in b.roots, every voxel's key --
// (0, label) in a kept core, UNASSIGNED or BLOCKED -- and worklist 0: the tiles that hold an UNASSIGNED voxel.  round: relaxes the
// n_active > 0 tiles of worklist `cur` and fills the other, whose length is zeroed first.  records / doors: with b.rank filled, the
// sums per room (b.recs, zeroed first) and per pair of rooms (table: n_kept^2 x PART_DOOR_WORDS words, zeroed first).  Those that
// clear device words first return the first error of their calls.
hipError_t launch_part_label(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b);
hipError_t launch_part_init(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b, unsigned n_kept);
hipError_t launch_part_round(hipStream_t s, const PartGeom& q, const PartBufs& b, int cur, unsigned n_active);
hipError_t launch_part_records(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b, unsigned n_kept);
hipError_t launch_part_doors(hipStream_t s, const unsigned* d2, const PartGeom& q, const PartBufs& b, unsigned n_kept, unsigned long long* table);
// a box of the field (not empty), row-major: the room ids (UNASSIGNED / BLOCKED where a voxel holds none), or the costs G
void launch_part_box(hipStream_t s, const PartGeom& q, const PartBufs& b, unsigned n_kept, const int lo[3], const int hi[3], bool cost, unsigned* out);
// the room ids of n points: the voxel as hsk_clearance_at finds it, then hsk_part_point.h's search with `radius`
void launch_part_gather(hipStream_t s, const PartGeom& q, const PartBufs& b, unsigned n_kept, const VolParams& vp, const float* xyz, unsigned n, int radius,
                        unsigned* out);

// A 256-point sweep over the n points of a cloud in the alignment's scratch (planes.hip's, level.hip's) runs cloud_sweep_blocks(n)
// blocks, each of which leaves up to 16 integer words in partial[block][16]; launch_cloud_fold (planes.hip: k_cloud_fold) folds the
// first n_words of the n_blocks rows into out -- their sums, or, box, signed words of which 0..2 are minima and the others maxima.
#define HSK_CLOUD_MAX_BLOCKS 1024
unsigned cloud_sweep_blocks(unsigned n);
void launch_cloud_fold(hipStream_t s, const unsigned long long* partial, unsigned n_blocks, unsigned n_words, bool box, unsigned long long* out);

// oriented plane detection (planes.hip) over the n points of the six planes at `soa` (`pitch` floats apart);
// labels: n ints, < 0 = unlabelled (launch_plane_score alone takes null: every valid point is open).  Every sum is an integer.
// seed: hyp[j] = the plane of point seeds[j] (< n), four NaNs when that point is invalid or labelled.  score: counts[j] = the
// inliers of hyp[j], j < n_hyp <= HSK_PLANE_MAX_HYP; partial: plane_score_blocks(n) x n_hyp words.  moments: sums10 = the
// inliers' count, sum of q (3), sum of q_a q_b (xx xy xz yy yz zz), q = rint(x 4096); label: the inliers get `index`, out2 = their
// count and the sum of rint(|s| 65536); both with partial: cloud_sweep_blocks(n) x 16 words.  Nothing is launched with n == 0.
#define HSK_PLANE_MAX_HYP 4096
#define HSK_PLANE_MAX_BLOCKS 1024
unsigned plane_score_blocks(unsigned n);
void launch_plane_seed(hipStream_t s, const float* soa, const int* labels, const unsigned* seeds, unsigned n_hyp, unsigned pitch, float* hyp);
void launch_plane_score(hipStream_t s, const float* soa, const int* labels, const float* hyp, unsigned n, unsigned pitch, unsigned n_hyp,
                        float dist_m, float cos_min, unsigned* partial, unsigned* counts);
void launch_plane_moments(hipStream_t s, const float* soa, const int* labels, const float abcd[4], unsigned n, unsigned pitch, float dist_m,
                          float cos_min, unsigned long long* partial, unsigned long long* sums10);
void launch_plane_label(hipStream_t s, const float* soa, int* labels, const float abcd[4], int index, unsigned n, unsigned pitch, float dist_m,
                        float cos_min, unsigned long long* partial, unsigned long long* out2);
void launch_plane_unlabel(hipStream_t s, int* labels, int index, unsigned n);
// a cloud with normals as two arrays of packed triples (the product buffer's) -> the six planes
void launch_plane_gather(hipStream_t s, const float* xyz, const float* normals, unsigned n, unsigned pitch, float* soa);

// the upright-frame estimate (level.hip) over the n points of the six planes at `soa` (`pitch` floats apart), their
// normals weighted by w.  Every sum is an integer.  hist: HSK_LEVEL_HIST_BINS counts and one more word, the valid points -- ZEROED by
// the caller.  sums: sums15 = per axis a < n_axes the supporters' count and the three sums of sign(N . A) N (words 4 a ..), then --
// wall set -- the wall points of W[0], their count and the two fourth-power sums against W[1], W[2] (words 12 ..); partial:
// cloud_sweep_blocks(n) x 16 words.  extents: box6 = the min (3) then max (3) of P . R_k over the valid points as signed 64-bit words
// (INT32_MAX / INT32_MIN when there is none); classes set: the two height histograms, HSK_LEVEL_H_BINS bins a class, the floor class
// first -- h_count, h_sum ZEROED by the caller.  Nothing is launched with n == 0.
struct LevelWeights {
  float w[3];
};
struct LevelAxes {
  int A[3][3], W[3][3];      // integer axes: |A|^2 <= HSK_UPRIGHT_AXIS_MAX2
  long long aa[3], waa;      // |A_a|^2, |W_0|^2
  double cone2, wall2;       // the squared cosine of the cone, the squared sine of the wall test
  int n_axes, wall;
};
struct LevelFrame {
  int R[3][3];
  long long raa;             // |R_1|^2
  double cone2;
  int classes;
};
void launch_level_hist(hipStream_t s, const float* soa, unsigned n, unsigned pitch, const LevelWeights& w, unsigned* hist);
void launch_level_sums(hipStream_t s, const float* soa, unsigned n, unsigned pitch, const LevelWeights& w, const LevelAxes& ax,
                       unsigned long long* partial, unsigned long long* sums15);
void launch_level_extents(hipStream_t s, const float* soa, unsigned n, unsigned pitch, const LevelWeights& w, const LevelFrame& fr,
                          unsigned long long* partial, unsigned long long* box6, unsigned* h_count, unsigned long long* h_sum);
int level_warm();     // loads level.hip's code object (hsk_prepare_readout); a hipError_t

// sparse volume image (pack.hip): bricks of 8^3 voxels, pack_bricks of them, a class byte and a record size
// (in 4-byte words) each.  launch_pack_scan turns the sizes into offsets in place (an exclusive scan; bsum: pack_scan_blocks
// words of scratch) and leaves in counts[0..3] the bricks per class, in counts[4] the payload's length in words (8 words).
// gather / scatter move the records of every non-ZERO brick between the volume (color: the row-major colour volume) and the
// payload; the scatter expects a zeroed volume.
size_t pack_bricks(const VolParams& vp);
size_t pack_scan_blocks(size_t n_bricks);
void launch_pack_classify(hipStream_t s, const void* vol, const VolParams& vp, unsigned char* cls, unsigned* size);
void launch_pack_classify_color(hipStream_t s, const unsigned* col, const VolParams& vp, unsigned char* cls, unsigned* size);
void launch_pack_sizes(hipStream_t s, const unsigned char* cls, size_t n_bricks, unsigned* size);
void launch_pack_scan(hipStream_t s, unsigned* size, size_t n_bricks, unsigned* bsum, unsigned* counts);
void launch_pack_gather(hipStream_t s, const void* vol, bool color, const VolParams& vp, const unsigned char* cls, const unsigned* off,
                        void* payload);
void launch_pack_scatter(hipStream_t s, void* vol, bool color, const VolParams& vp, const unsigned char* cls, const unsigned* off,
                         const void* payload);

// image
void launch_bilateral_scale(hipStream_t s, const uint16_t* src, int W, int H, Intr in, const float* ws, const float* wc,
                            uint16_t* dst, float* scaled, float* tiles);
void launch_scale_depth(hipStream_t s, const uint16_t* src, int W, int H, Intr in, float* scaled);
// pyrDown x 2 and the vertex / normal maps of all three levels in one launch (depth[0] is read, depth[1], depth[2] written)
void launch_pyramid_maps(hipStream_t s, uint16_t* const* depth, const ImgLevel* lv, float* const* vmap, float* const* nmap);
void launch_transform_maps(hipStream_t s, const float* vs, const float* ns, int P, const TrackState* st, float* vd,
                           float* nd);
void launch_resize_maps2(hipStream_t s, const float* v0, const float* n0, int W, int H, float* v1, float* n1, float* v2,
                         float* n2, const TrackState* st,
                         const RingOut* ring = nullptr);
int icp_num_blocks(int W, int rows);
void launch_icp_accumulate(hipStream_t s, const float* vcur, const float* ncur, const float* vprev, const float* nprev,
                           int W, int H, Intr in, const TrackState* st, float dist_thresh, float angle_thresh, int row0,
                           int row1, double* partials);
void launch_icp_reduce(hipStream_t s, const double* partials, int nblocks, double* out27);
void launch_icp_update(hipStream_t s, const double* sums27, TrackState* st);
void launch_begin_frame(hipStream_t s, TrackState* st, void* icp_pose_buf);
size_t icp_pose_bytes();
void launch_icp_fused(hipStream_t s, float* const* vcur, float* const* ncur, float* const* vmod, float* const* nmod,
                      const ImgLevel* lv, const int* iters, TrackState* st, float dist_thresh, float angle_thresh,
                      void* pose_buf, IcpFinal* defer_final = nullptr, hipEvent_t* level_events = nullptr);
bool host_solve6(const double* in27, float* x6);
void host_pose_update(float* R, float* t, const float* x6);
void hsk_build_tet_table(TetTable* tt);
int hsk_build_cube_table(CubeTable* ct);  // marching cubes; returns the most triangles of a case (HSK_MC_MAXT)
int hsk_mesh_z_end(const VolParams& vp);
void launch_extract_mesh(hipStream_t s, const void* vol, const VolParams& vp, const TetTable& tt, unsigned* row_count,
                         unsigned long long* row_offset, unsigned long long* total, float* tri, unsigned long long cap, const unsigned* flags);
void launch_extract_mesh_mc(hipStream_t s, const void* vol, const VolParams& vp, const CubeTable* ct_dev, unsigned* row_count,
                            unsigned long long* row_offset, unsigned long long* total, float* tri, unsigned long long cap, const unsigned* flags);
// the indexed marching-cubes mesh (extract.hip): its scratch, carved out of one device buffer by mesh_index_layout
struct MeshIndexBufs {
  int rows;                     // grid rows: Y x (hsk_mesh_z_end - zo0 + 1) planes (0 when the context emits no cube)
  int nseg;                     // 64-voxel segments per row; a row's edge bits are 3 nseg words
  unsigned long long* totals;   // [0] vertices, [1] faces, [2] uncoloured vertices
  unsigned long long* bits;     // rows x 3 nseg words: bit 3 x + axis of row (y, z) = the edge from (x, y, z) has a vertex
  unsigned long long* voff;     // rows (+ the scan's block sums): the rows' first vertex
  unsigned* vcount;             // rows: vertices per row
  unsigned short* segbase;      // rows x nseg: vertices of the row before each segment
};
size_t mesh_index_layout(const VolParams& vp, void* base /* null: the size only */, MeshIndexBufs* b);
// count pass (faces' row counts into row_count / row_offset, as launch_extract_mesh_mc's count pass), then the write passes
void launch_mesh_index_count(hipStream_t s, const void* vol, const VolParams& vp, const CubeTable* ct_dev, unsigned* row_count,
                             unsigned long long* row_offset, const MeshIndexBufs& mb, const unsigned* flags);
void launch_mesh_index_write(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const CubeTable* ct_dev,
                             const unsigned* row_count, const unsigned long long* row_offset, const MeshIndexBufs& mb, float* xyz,
                             float* normals, unsigned char* rgb, unsigned long long* n_uncolored, int* faces, const unsigned* flags);
// the exclusive scan of n row counts (extract.hip): off[i] = the items before row i, *total their sum; off has room for
// hsk_scan_scratch_entries(n) entries
void launch_scan_rows(hipStream_t s, const unsigned* cnt, unsigned long long* off, int n, unsigned long long* total);
// the simplified mesh (simplify.hip): its fixed scratch for clusters of 2^s voxels, carved out of one device buffer by simp_layout
struct SimpBufs {
  int s;                        // log2 of the cluster's edge in voxels
  int CX, CY, CZ;               // clusters per axis (the last one partial where a dim is no multiple of the edge)
  int crows, cseg;              // cluster rows CY x CZ; 64-cluster segments per row
  int frows;                    // cube rows (Y - 1) x (Z - 1): the indexed mesh's face rows
  unsigned long long* totals;   // [0] faces out, [1] vertices out, [2] clusters that hold a vertex, [4 .. 7] vertices by rank, [8] clamped, [9] uncoloured
  unsigned char* ref;           // a byte per cluster: referenced by a surviving face; after the rows pass 0x80 | rank in its segment
  unsigned* cl_cnt;             // cluster rows: referenced clusters
  unsigned long long* cl_off;   // ... and the row's first output vertex (+ the scan's block sums)
  unsigned* tc_cnt;             // cluster rows: clusters that hold a vertex
  unsigned long long* tc_off;
  unsigned short* segbase;      // cluster rows x cseg: referenced clusters of the row before each segment
  unsigned* sf_cnt;             // cube rows: surviving faces
  unsigned long long* sf_off;   // ... and the row's first face (+ the scan's block sums)
};
size_t simp_layout(const VolParams& vp, int s, void* base /* null: the size only */, SimpBufs* b);
void launch_simp_count(hipStream_t s, const void* vol, const VolParams& vp, const CubeTable* ct_dev, const unsigned* tri_count,
                       const MeshIndexBufs& mb, const SimpBufs& sb);
void launch_simp_write(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const CubeTable* ct_dev,
                       const unsigned* tri_count, const MeshIndexBufs& mb, const SimpBufs& sb, unsigned n_out, unsigned* list, long long* sums,
                       int mode, double floor_rel, float* xyz, float* normals, unsigned char* rgb, int* faces);
int simplify_warm();

// hole filling (fill.hip) of a WHOLE volume.  The scratch, carved out of one device buffer by fill_layout:
// two state buffers of one int16 per volume word, a voxel's at the voxel's own place (hsk_vox_index) -- together as large as the
// volume --, and per 16 x 16 x 8 tile 256 bytes of FREE bits and three bytes.  Iteration `it` (1-based) reads state[(it - 1) & 1]
// and writes state[it & 1]; with `fin` the buffer of the final states, the other one holds row-major bytes: the mask in its first
// half, the keep rule's bytes in its second.
#define FILL_COUNTS 16   // counts[0] n_unseen, [1] n_reached, [2] n_written, [3] n_written_negative, [4] tile visits; behind
                         // them 256 words: [it] the states iteration `it` changed
struct FillBufs {
  unsigned* counts;
  unsigned char* tile_free;  // a byte per thread of a tile's workgroup: its eight voxels' FREE bits
  unsigned char* cand;       // a byte per tile: it holds a FREE voxel
  unsigned char* flag[2];    // a byte per tile: its states changed in the iteration that wrote this buffer
  short* state[2];
  unsigned n_tiles;
};
size_t fill_layout(const VolParams& vp, void* base /* null: the size only */, FillBufs* b);
inline unsigned char* fill_mask_bytes(const VolParams& vp, const FillBufs& b, int fin) { return (unsigned char*)b.state[fin ^ 1]; }
inline unsigned char* fill_keep_bytes(const VolParams& vp, const FillBufs& b, int fin) { return (unsigned char*)b.state[fin ^ 1] + hsk_vol_words(vp); }
// the states, bits and bytes of the volume as it stands for the box lo <= (x, y, z) < hi; the counters zeroed, counts[0] set
void launch_fill_init(hipStream_t s, const void* vol, const VolParams& vp, const int lo[3], const int hi[3], const FillBufs& b);
void launch_fill_round(hipStream_t s, const VolParams& vp, const FillBufs& b, int it);
// HSK_FILL_SURFACE's bytes from the final states: within Chebyshev distance `band` of a crossing voxel
void launch_fill_keep(hipStream_t s, const VolParams& vp, const FillBufs& b, int fin, int band);
// the mask and counts[1 .. 3]; keep_all: HSK_FILL_ALL (launch_fill_keep's bytes are not read)
void launch_fill_count(hipStream_t s, const void* vol, const VolParams& vp, const int lo[3], const int hi[3], const FillBufs& b, int fin, bool keep_all);
// the masked voxels' words: (fill_weight << 16) | (value & 0xffff)
void launch_fill_commit(hipStream_t s, void* vol, const VolParams& vp, const FillBufs& b, int fin, int fill_weight);
int fill_warm();      // loads fill.hip's code object (hsk_prepare_readout); a hipError_t

// volume differencing (diff.hip) of two WHOLE volumes on one grid.  The scratch, carved out of one device
// buffer by diff_layout: the counters, the class words (one per volume word, in the volume's layout: hsk_diff_point.h), two byte
// volumes (row-major) for the adopt set, and a labelling scratch of its own (comp_layout: never the one hsk_label_components holds)
#define DIFF_COUNTS 16  // [0..6] the classes before the MINOR step, [8] the adopt targets, [9] the adopt set
struct DiffBufs {
  unsigned* counts;
  unsigned* cls;           // hsk_vol_words
  unsigned char* mask[2];  // X Y Z bytes each
  CompBufs comp;
};
size_t diff_layout(const VolParams& vp, void* base /* null: the size only */, DiffBufs* b);
// the class words of (ref, cur) and counts[0..6]
void launch_diff_classify(hipStream_t s, const void* ref, const void* cur, const VolParams& vp, const DiffBufs& b, int thresh, int min_weight);
// behind the labelling and the MINOR step: av[2 i], av[2 i + 1] = the APPEARED and VANISHED voxels of region roots[i] (0, 0 for a
// region that was not kept)
void launch_diff_records(hipStream_t s, const VolParams& vp, const DiffBufs& b, unsigned n, const unsigned* roots, unsigned* av);
// the n > 0 voxels of a box, row-major: class bytes and (region may be null) labels
void launch_diff_box(hipStream_t s, const VolParams& vp, const DiffBufs& b, const int lo[3], const int hi[3], size_t n, unsigned char* cls,
                     unsigned* region);
// hsk_diff_at's choice for n > 0 points
void launch_diff_gather(hipStream_t s, const VolParams& vp, const DiffBufs& b, const float* xyz, unsigned n, int radius, unsigned* region,
                        unsigned char* cls);
// the adopt set's halo in mask[1] and its counts: counts[8] the targets, counts[9] the set; nothing but the scratch is written
void launch_diff_halo(hipStream_t s, const void* cur, const VolParams& vp, const DiffBufs& b, int which, int halo);
// the masked copy: cur's words into ref and, ref_col not null, cur's colour words (cur_col null: the colour word 0)
void launch_diff_adopt(hipStream_t s, void* ref, const void* cur, unsigned* ref_col, const unsigned* cur_col, const VolParams& vp, const DiffBufs& b);
int diff_warm();      // loads diff.hip's code object (hsk_prepare_readout); a hipError_t

// the scene split (split.hip) of a WHOLE volume.  The scratch, carved out of one device buffer by split_layout:
// the counters, the planes as the host converted them, the removal's selected objects, the class words (one per volume word, in the
// volume's layout: hsk_split_point.h), two byte volumes (row-major) for the removal, and a labelling scratch of its own
// (comp_layout: never the one hsk_label_components holds)
#define SPLIT_COUNTS 16  // [1..5] the classes before the MINOR step, [6] edge-rule voxels, [7] voxels with G = 0, [8] the removal's
                         // targets, [9] its written and [10] its restored voxels
// an object's record on the device, SPLIT_REC_WORDS words: three 64-bit sums of x, y, z; the contacts by kind; the 64-bit plane
// mask; the heights, as ~key and key with key = height ^ 0x80000000 (both only ever raised from 0)
#define SPLIT_REC_WORDS 16
#define SPLIT_REC_CONTACT 6
#define SPLIT_REC_MASK 10
#define SPLIT_REC_HLO 12
#define SPLIT_REC_HHI 13
struct SplitPlaneQ;
struct SplitRule;
struct SplitSelected;
struct SplitBufs {
  unsigned* counts;
  SplitPlaneQ* planes;     // SPLIT_MAX_PLANES
  SplitSelected* sel;      // SPLIT_MAX_SELECTED
  unsigned* cls;           // hsk_vol_words
  unsigned char* mask[2];  // X Y Z bytes each
  CompBufs comp;
};
size_t split_layout(const VolParams& vp, void* base /* null: the size only */, SplitBufs* b);
// the class words of the volume for the planes in b.planes, and counts[1..7]
void launch_split_classify(hipStream_t s, const void* vol, const VolParams& vp, const SplitBufs& b, const SplitRule& r);
// behind the labelling and the MINOR step: the records of the kept objects among roots[0, n) (zeros for the others)
void launch_split_records(hipStream_t s, const VolParams& vp, const SplitBufs& b, unsigned n, const unsigned* roots, unsigned* rec, int floor_plane);
// the n > 0 voxels of a box, row-major: class bytes and (may be null) plane bytes and labels
void launch_split_box(hipStream_t s, const VolParams& vp, const SplitBufs& b, const int lo[3], const int hi[3], size_t n, unsigned char* cls,
                      unsigned char* plane, unsigned* object);
// hsk_split_at's choice for n > 0 points
void launch_split_gather(hipStream_t s, const VolParams& vp, const SplitBufs& b, const float* xyz, unsigned n, int radius, unsigned char* cls,
                         unsigned char* plane, unsigned* object);
// the removal of the n_sel objects in b.sel (uni: the union of their grown boxes): the halo in mask[1] and counts[8..10]; nothing
// but the scratch is written
void launch_split_halo(hipStream_t s, const void* vol, const VolParams& vp, const SplitBufs& b, unsigned n_sel, const int uni_lo[3], const int uni_hi[3],
                       const SplitRule& r, int mode, int halo, int fill_weight);
// the masked write of rules 1 and 2 (col not null: a written voxel's colour word becomes 0)
void launch_split_restore(hipStream_t s, void* vol, unsigned* col, const VolParams& vp, const SplitBufs& b, unsigned n_sel, const int uni_lo[3],
                          const int uni_hi[3], const SplitRule& r, int mode, int fill_weight);
int split_warm();     // loads split.hip's code object (hsk_prepare_readout); a hipError_t

// baked textures (texture.hip) from a WHOLE volume: a wave per 8 x 8 tile of the ta.W x ta.H atlas bakes its
// texels by hsk_texture_point.h's rule into rgb, nrm (3 bytes a texel) and mask (1), each of which may be null and all of which
// the caller has cleared; counts: HSK_VIEW_COUNT_SLOTS slots of 16 words, a wave adds its texels by mask bit to words 0 .. 4 of
// one of them (cleared likewise)
struct TexArgs;
struct TexBlock;
void launch_bake_texture(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const TexArgs& ta, const unsigned* tiles,
                         const TexBlock* blocks, const int* faces, const float* vertices, unsigned char* rgb, unsigned char* nrm,
                         unsigned char* mask, unsigned long long* counts);
int texture_warm();   // loads texture.hip's code object (hsk_prepare_readout); a hipError_t

// keyframe textures (keytex.hip): launch_bake_texture with the colour from the keyframes of ks by
// hsk_keytex_point.h's rule, and the source plane (1 byte a texel, may be null, cleared by the caller like the others -- to
// HSK_KEYTEX_NONE); a wave adds its texels by mask bit to words 0 .. 5 of its slot, its pairs seen and occluded to words 6 and 7
struct KeyStore;
struct KeyArgs;
void launch_bake_keytex(hipStream_t s, const void* vol, const unsigned* colv, const VolParams& vp, const TexArgs& ta, const KeyStore& ks,
                        const KeyArgs& ka, const unsigned* tiles, const TexBlock* blocks, const int* faces, const float* vertices,
                        unsigned char* rgb, unsigned char* nrm, unsigned char* mask, unsigned char* source, unsigned long long* counts);
int keytex_warm();    // loads keytex.hip's code object (hsk_prepare_readout); a hipError_t

// cloud import (splat.hip): the n points of a cloud in the alignment scratch's planes (the normals' three only
// with_normals) offered to a view's z-buffer by hsk_splat_point.h's rule -- zbuf: cam.w x cam.h words, all ones before the first
// offer; counts: SPLAT_COUNT_WORDS words of the view, zeroed by the caller: the points by SPLAT_* class, then the pixels that got
// a depth.  resolve: the z-buffer as the 16-bit frame (all ones -> 0), counted, and all ones again.  pose: the view's pose into
// the tracker state, lost cleared (hsk_set_pose's effect).  Nothing is launched for n == 0.
#define SPLAT_COUNT_WORDS 8
struct SplatCam;
struct SplatPose;
struct SplatArgs;
void launch_splat_points(hipStream_t s, const float* soa, unsigned n, unsigned pitch, bool with_normals, const SplatCam& cam, const SplatPose& pose,
                         const SplatArgs& args, unsigned* zbuf, unsigned* counts);
void launch_splat_resolve(hipStream_t s, unsigned* zbuf, unsigned n_pixels, unsigned short* frame, unsigned* counts);
void launch_splat_pose(hipStream_t s, TrackState* st, const SplatPose& pose);
int splat_warm();     // loads splat.hip's code object (hsk_prepare_readout); a hipError_t

// cloud normals (normals.hip): a fixed-radius neighbour search over the n <= 2^24 points of a cloud in the
// alignment scratch's planes (the positions' three), and hsk_normal_point.h's solve at every point.
// NormalIndex: the cell table -- mask + 1 slots, a power of two and at least 2 n; keys all ones, counts, cursor and words zeroed by
// the caller -- and the points in cell order: sq, three planes `pitch` ints apart (the cloud's pitch) of q, and sidx, their
// original indices.  words: [0 .. 4] the points by NORMAL_* class, [5] the sum of the reported neighbour counts, then
#define NORMAL_W_CELLS 6   // the occupied cells
#define NORMAL_W_ERROR 7   // not 0: a probe ran out of its bound, or a range left the cloud -- the call fails
#define NORMAL_W_VALID 8   // the valid points (the scan's total)
#define NORMAL_WORDS 16
struct NormalIndex {
  unsigned long long* keys;
  unsigned* counts;
  unsigned long long* off;  // hsk_scan_scratch_entries(mask + 1) entries: a cell's first place in cell order
  unsigned* cursor;
  unsigned* slot;           // n: a point's slot in the table, all ones for an invalid point
  int* sq;
  unsigned* sidx;
  unsigned long long* words;
  unsigned mask;
};
struct NormalArgs {
  unsigned min_neighbours, max_neighbours, n_viewpoints;
  float line_rel;
};
// the call's outputs on the device: normals 3 n floats (packed triples), the others n each
struct NormalOut {
  float* normals;
  float* curvature;
  unsigned* neighbours;
  unsigned char* cls;
};
// index: the table, the scan, the points in cell order -- and the invalid points' outputs.  gather: every valid point's sums,
// solve and outputs.  viewpoints: 3 floats each on the device, args.n_viewpoints of them.  Nothing is launched for n == 0.
void launch_normal_index(hipStream_t s, const float* soa, unsigned n, unsigned pitch, int r_q, const NormalIndex& ix, const NormalOut& out);
void launch_normal_gather(hipStream_t s, const float* soa, unsigned n, unsigned pitch, int r_q, const NormalArgs& args, const float* viewpoints,
                          const NormalIndex& ix, const NormalOut& out);
int normals_warm();   // loads normals.hip's code object (hsk_prepare_readout); a hipError_t
