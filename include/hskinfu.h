/*
 * hskinfu.h -- C ABI of the MI355X-native KinectFusion core for HouseScan.
 *
 * The reference program (nh2/housescan) holds no KinectFusion code and no FFI; it exchanges FILES with an
 * external PCL KinFu fork (/root/reference/README.md:13-14).  This header defines the seam the north_star
 * asks for: a thin C ABI the Haskell host loop would bind with `foreign import ccall`.  Each entry point
 * cites the reference interface whose data shape it honours or whose role it replaces:
 *
 *   depth frames in   : `takeDepthSnapshot :: IO (Either String (Vector Word16, (Int, Int)))`
 *                       housescan/HoniHelper.hs:20-36 -- row-major uint16, i = y*w + x (Main.hs:1297-1300),
 *                       0 = invalid (Main.hs:1297); errors are values, never exceptions (HoniHelper.hs:39-42).
 *   clouds out        : `Cloud { cloudPoints :: Vector Vec3 }` packed float32 xyz, 12 B/point
 *                       housescan/Main.hs:117-121, :641, :792; consumed by addPointCloud Main.hs:806.
 *   poses / transforms: 16 floats row-major, LEFT-multiplicative (p' = M p) -- the form HouseScan exports
 *                       in roomProjectionToString / roomProjectionToXfFormat, Main.hs:2271-2302.
 *   products on disk  : cloud_downsampled.pcd, cloud_bin.pcd (Main.hs:1740, :1334-1345, :2437).
 *
 * Conventions: every call returns HSK_OK (0) or a negative error code; the message is available from
 * hsk_last_error (maps to Haskell `Left String`).  Tracking loss is NOT an error: *tracked = 0 and the
 * volume is reset.  A context is not re-entrant; distinct contexts are independent and
 * may be driven from different OS threads.  The library never retains caller pointers past the call.
 * No torch / C++ types cross this boundary.
 */
#ifndef HSKINFU_H
#define HSKINFU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSK_OK 0
#define HSK_ERR_ARG (-1)
#define HSK_ERR_HIP (-2)
#define HSK_ERR_STATE (-3)
#define HSK_ERR_NOGPU (-4)
#define HSK_ERR_TIMEOUT (-5) /* a pipelined frame did not report within HSK_FRAME_TIMEOUT_S seconds (environment, default 20) */

#define HSK_LEVELS 3
#define HSK_KEY_NONE 0x7fffffff

typedef struct hsk_ctx hsk_ctx; /* opaque; one per volume / room */

typedef struct {
  int vol_x, vol_y, vol_z;      /* voxels, e.g. 256 / 512 / 1024; vol_x and vol_y multiples of 8.  Large volumes want
                                   multiples of 16 or more (best: powers of two): the brick bitfield of the stored planes
                                   -- one bit per 8^3 voxels, per 16^3 .. 64^3 only while vol_x and vol_y are multiples of
                                   that edge and the field is longer than 4 KiB -- is staged in LDS by the raycast, and
                                   hsk_create refuses (HSK_ERR_ARG) a volume whose field exceeds 64 KiB or, if that is
                                   less, what the runtime reports as the shared memory of a block of the device:
                                   648^3 is refused (66560 B), 656^3 and 1024^3 are not                   */
  float vol_size_m[3];          /* metric extent, default 3 x 3 x 3                                    */
  float trunc_dist_m;           /* default 0.03; clamped to >= 2.1 * max cell                           */
  int width, height;            /* depth image, default 640 x 480 (the shape HoniHelper.hs:34-36 returns) */
  float fx, fy, cx, cy;         /* default 525, 525, 319.5, 239.5                                       */
  int icp_iters[HSK_LEVELS];    /* level 0 (finest) .. 2, default {10, 5, 4}; run coarsest first        */
  float icp_dist_thresh_m;      /* 0.10                                                                 */
  float icp_angle_thresh_sin;   /* sin(20 deg)                                                          */
  float integrate_move_thresh;  /* 0 => integrate every frame                                           */
  float init_pose[16];          /* row-major cam->world; default R = I, t = (1.5, 1.5, -0.3)            */
  int device_id;                /* HIP device ordinal                                                   */
  /* z-slab sharding (multi-GPU): this context stores planes [own_z0 - halo, own_z1 + halo) clipped to the
   * volume and OWNS raycast steps whose far sample lies in [own_z0, own_z1).  Single device: 0, vol_z, 0. */
  int own_z0, own_z1, halo;
  int use_graph;                /* 1 = replay synchronous frames from one hipGraph; 0 (default) = eager;
                                   2 = the main-stream chain of PIPELINED frames (hsk_submit_frame*) from one hipGraph per
                                   image-buffer set: 23 launches become one -- for hosts that scan several rooms at once */
} hsk_config;

/* identity of the sources this library was built from (first 16 hex digits of their sha256; "+exp" appended when it
 * was built with other than the default compiler flags) */
const char* hsk_build_id(void);

/* fills *c with the defaults above for an n^3 volume */
void hsk_default_config(hsk_config* c, int n);

int hsk_create(const hsk_config* c, hsk_ctx** out);
void hsk_destroy(hsk_ctx* k);
int hsk_reset(hsk_ctx* k);
const char* hsk_last_error(const hsk_ctx* k); /* k may be NULL: last create error */

/* Whole tracker step.  `depth` is caller-owned row-major uint16 millimetres (HoniHelper.hs:20; index
 * convention Main.hs:1298-1300), read-only, may be freed on return.  pose_out: row-major,
 * left-multiplicative cam->world (Main.hs:2278-2284). */
int hsk_process_frame(hsk_ctx* k, const uint16_t* depth, int w, int h, float pose_out[16], int* tracked);
/* Same, the depth frame already resident in device memory (HBM) */
int hsk_process_frame_dev(hsk_ctx* k, const void* depth_dev, int w, int h, float pose_out[16], int* tracked);

/* Asynchronous form of the tracker step (throughput): hsk_submit_frame_dev enqueues a frame and returns at once,
 * hsk_wait_frame returns the pose of the OLDEST submitted frame (FIFO).  Up to HSK_MAX_IN_FLIGHT frames may be
 * outstanding, so the GPU runs frame k+1 while the host reads frame k's pose.  After a tracking loss the frames
 * already in flight are dropped (tracked = 0) and the volume is reset before the next submission.  The depth copy
 * and preprocessing of a submitted frame run on a second stream, overlapped with the previous frame; depth_dev must
 * therefore stay valid until hsk_wait_frame has returned that frame.  Its CONTENTS may still be in the making on a
 * stream the context has adopted through hsk_set_stream (an upload or a conversion kernel enqueued there): the second
 * stream is ordered behind everything enqueued on the adopted stream at the time of the call.  Work on any other
 * stream (and any work when the context runs on its own stream) must have completed before the call.
 * WHAT "WAITED" MEANS: hsk_wait_frame returns as soon as the frame's POSE and verdict are final -- when its ICP has ended.
 * The frame's integrate and raycast may still be running on hsk_stream() at that point.  Every call of this library is
 * ordered behind them on that stream, so callers that only use the library see nothing of it; a caller that takes
 * "waited" for "the GPU is idle" or "the volume is current" -- to stop a clock, or to touch the volume or the model maps
 * from another stream -- must call hsk_synchronize() first.  A frame that does not report within HSK_FRAME_TIMEOUT_S
 * seconds (environment, default 20) makes hsk_wait_frame -- and the synchronous hsk_process_frame[_dev], which go through
 * it -- return HSK_ERR_TIMEOUT. */
#define HSK_MAX_IN_FLIGHT 3
int hsk_submit_frame_dev(hsk_ctx* k, const void* depth_dev, int w, int h);
int hsk_submit_frame(hsk_ctx* k, const uint16_t* depth, int w, int h); /* host frame; copied before the call returns */
int hsk_wait_frame(hsk_ctx* k, float pose_out[16], int* tracked);

/* Stage-level entry points: exist so parity tests and rocprof can isolate each kernel. */
int hsk_integrate(hsk_ctx* k, const uint16_t* depth, int w, int h, const float pose[16]);
int hsk_raycast(hsk_ctx* k, const float pose[16], float* vmap /* 3*h*w SoA */, float* nmap, int32_t* keys /* may be NULL */);
int hsk_preprocess(hsk_ctx* k, const uint16_t* depth, int w, int h); /* bilateral, pyramid, vertex/normal maps */
/* 27 sums for pose estimate `pose_est` against the stored model maps and previous pose, rows [row0,row1) */
int hsk_icp_accumulate(hsk_ctx* k, int level, const float pose_est[16], int row0, int row1, double out27[27]);
int hsk_icp_solve(const double in27[27], float x6[6], int* ok);       /* host mirror of the device solve */
int hsk_count_updates(hsk_ctx* k, const uint16_t* depth, int w, int h, const float pose[16], uint64_t* n_upd);

int hsk_download_tsdf(hsk_ctx* k, int16_t* tsdf_weight_pairs /* 2 * X*Y*stored_planes, x fastest */);
int hsk_upload_tsdf(hsk_ctx* k, const int16_t* tsdf_weight_pairs);
/* The weights of deep free space are kept in side tables (one byte per 16 voxels, one per 2048) and written back into the
 * volume when something is about to read them: hsk_download_tsdf does it itself.  (The products -- hsk_extract_cloud,
 * hsk_extract_mesh[_cubes] -- ask of a weight only whether it is zero, which no deferred weight is, and do not.)  This call
 * does only that write-back (enqueued; no host synchronisation) -- it changes nothing any call returns, and exists so
 * that the deferred work can be timed on its own (bench.py: readout_ms). */
int hsk_flush_weights(hsk_ctx* k);
int hsk_stored_planes(const hsk_ctx* k, int* z0, int* nz);
int hsk_get_pose(hsk_ctx* k, float pose[16]);
int hsk_set_pose(hsk_ctx* k, const float pose[16]);
/* kind: 0 current vertex, 1 current normal, 2 model vertex, 3 model normal; out = 3*(h>>level)*(w>>level) floats */
int hsk_download_map(hsk_ctx* k, int kind, int level, float* out);
int hsk_upload_map(hsk_ctx* k, int kind, int level, const float* in);
int hsk_download_depth_level(hsk_ctx* k, int level, uint16_t* out); /* filtered pyramid */
int hsk_download_scaled_depth(hsk_ctx* k, float* out);

/* Everything a read-out allocates on its first use -- the pinned staging pair (2 x 32 MiB, or a plane of the volume if that is
 * more), the row tables of the count pass, the marching-cubes table, a product buffer of `product_bytes` (0: 48 MiB, a scan's
 * cloud and cubes mesh at 512^3) -- made NOW.  A host that shows a cloud from its GL thread (addPointCloud, Main.hs:806)
 * calls this once from the worker thread that created the context: the first hsk_extract_* then costs what every later
 * one does (it was 7 ms against 0.7).  Optional; idempotent; the buffers still grow on demand. */
int hsk_prepare_readout(hsk_ctx* k, size_t product_bytes);
/* the product buffer's size in bytes as it stands (0: not made yet, or k NULL): it only grows, by a quarter more than what is asked
 * for, so a call that leaves it unchanged has allocated none of it */
size_t hsk_product_capacity(const hsk_ctx* k);
/* TSDF zero-crossing cloud: packed float32 xyz (the layout of Cloud.cloudPoints, Main.hs:120) in voxel order. */
int hsk_extract_cloud(hsk_ctx* k, float* xyz, size_t cap_points, size_t* n_points);
/* TSDF zero level set as a triangle soup, 9 floats per triangle, marching tetrahedra (6 Kuhn tetrahedra per cube),
 * deterministic voxel order, normals towards free space.  Edge vertices shared by neighbouring cubes are bit-identical,
 * so hsk_write_ply_mesh can weld them by exact comparison.  Two-call protocol like hsk_extract_cloud. */
int hsk_extract_mesh(hsk_ctx* k, float* tri_xyz, size_t cap_triangles, size_t* n_triangles);
/* the same level set by MARCHING CUBES, the form the .ply of upstream's KinFu export has (/root/reference/README.md:16-17):
 * about half the triangles.  PCL's 256-case table is not in the reference; this one is generated (segments between cut
 * edges face by face, ambiguous faces cut one inside corner off each, loops fanned from their lowest edge) and has the
 * classic table's counts (820 triangles, at most 5 per cube); same validity rule, vertices and order as hsk_extract_mesh */
int hsk_extract_mesh_cubes(hsk_ctx* k, float* tri_xyz, size_t cap_triangles, size_t* n_triangles);

/* ---- Colour (RGB-D scans; opt-in).  A context that never calls hsk_enable_color runs exactly as without this section.
 * The colour volume holds one uint8 (r, g, b, w) quadruple per stored voxel -- 4 B per voxel, 512 MiB at 512^3, allocated
 * and zeroed by hsk_enable_color, nothing before.  Host arrays are row-major like hsk_download_tsdf's:
 * rgbw[stored_plane][y][x][4].  A frame's colour image is RGB8, 3 bytes per pixel, registered to the depth grid, row-major
 * (i = y*w + x) with the depth frame's w x h.  Each frame that integrates its TSDF also colours: voxel (x, y, z), projected
 * with the integrate's own arithmetic onto pixel (u, v) with scaled depth D_s != 0 and -band < D_s - dist < band, takes
 *     c' = (c w + p + ((w + 1) >> 1)) / (w + 1)  per channel (integers, truncating),  w' = min(w + 1, max_weight).
 * Lost frames and frames dropped in flight behind one colour nothing; hsk_reset and the reset after a tracking loss zero the
 * colour volume with the TSDF; frames submitted through the depth-only calls (hsk_process_frame, hsk_submit_frame,
 * hsk_track_stream, ...) leave colour untouched.  Not for the slabs of a group, nor for the *_dev frame calls. */
/* max_weight 1..255 (0: 64); band_m <= 0: 2 x the largest cell; the band is clamped to the truncation distance.  No frame may
 * be in flight.  A second call keeps the volume and changes the parameters.  HSK_ERR_STATE on a slab of a group. */
int hsk_enable_color(hsk_ctx* k, int max_weight, float band_m);
/* hsk_process_frame / hsk_submit_frame with the frame's colour image; both images are copied before the call returns.
 * HSK_ERR_STATE without hsk_enable_color. */
int hsk_process_frame_rgbd(hsk_ctx* k, const uint16_t* depth, const uint8_t* rgb, int w, int h, float pose_out[16], int* tracked);
int hsk_submit_frame_rgbd(hsk_ctx* k, const uint16_t* depth, const uint8_t* rgb, int w, int h);
/* stage level: the colour update of one frame at `pose` (the TSDF is untouched) */
int hsk_integrate_color(hsk_ctx* k, const uint16_t* depth, const uint8_t* rgb, int w, int h, const float pose[16]);
int hsk_download_color(hsk_ctx* k, uint8_t* rgbw /* 4 * X*Y*stored_planes */);
int hsk_upload_color(hsk_ctx* k, const uint8_t* rgbw);
/* hsk_extract_cloud with attributes: xyz, the count and the order are bit-identical to hsk_extract_cloud's (same two-call
 * protocol).  normals (3 floats per point): the raycast's normal at the point (central differences of the trilinear TSDF),
 * NaN x 3 where floor(p / cell) is not within (1, dims - 2) on every axis.  rgb (3 bytes per point): the colour of the
 * crossing's voxel with the smaller |tsdf|, or of the other one when that has colour weight 0; (0, 0, 0) when both have,
 * counted in *n_uncolored.  normals, rgb and n_uncolored may be NULL; rgb != NULL needs hsk_enable_color (HSK_ERR_STATE). */
int hsk_extract_cloud_attrs(hsk_ctx* k, float* xyz, float* normals, uint8_t* rgb, size_t cap_points, size_t* n_points,
                            size_t* n_uncolored);
/* hsk_extract_mesh_cubes' surface as an indexed mesh, welded on the device by edge identity.
 *   faces: one per triangle of hsk_extract_mesh_cubes on the same context, in its order (cube voxel order, then table order),
 *     corners in the soup's order: vertices[faces] equals the soup bit for bit, and the winding (normals towards free space) stays.
 *   vertices: one per cube edge that a face uses -- an edge that is cut (one end < 0, the other >= 0) and lies on at least one
 *     valid cube (all 8 weights non-zero) that this context emits.  Ordered by the edge's lower corner in voxel order (plane, row,
 *     x), then by axis (x, y, z); at pa + (Fa / (Fa - Fb)) (pb - pa), a the lower corner (the soup's arithmetic).  Distinct edges
 *     stay distinct vertices even where their coordinates coincide: on a grid point whose stored TSDF is exactly 0, and (at fine
 *     cells, 1024^3) where an extreme ratio of the two TSDF values moves a vertex by less than half an ulp from its end.  So
 *     *n_vertices >= hsk_weld_triangles' count on the soup, equal when neither occurs.
 *   normals (3 floats per vertex, may be NULL): hsk_extract_cloud_attrs' rule at the vertex -- central differences of the
 *     trilinear TSDF, one cell either side, scaled by 1 / |n|; NaN x 3 outside the (1, dims - 2) interior.
 *   rgb (3 bytes per vertex, may be NULL): hsk_extract_cloud_attrs' selection rule on the edge's two voxels -- the smaller |tsdf|
 *     (the lower corner on a tie), the other when that has colour weight 0, (0, 0, 0) and one count in *n_uncolored when both
 *     have.  Needs hsk_enable_color (HSK_ERR_STATE), so not on the slabs of a group.  n_uncolored may be NULL (0 without rgb).
 *   protocol: with every array NULL only the counts (the count pass is kept for the next call while the volume is unchanged).
 *     Any subset of the arrays may be asked for; each is written whole or not at all: a cap below its total (cap_vertices for
 *     vertices, normals and rgb) returns HSK_ERR_ARG with the counts set and nothing written.  More than INT32_MAX vertices:
 *     HSK_ERR_STATE.  No flush of the deferred weights is needed (as for the other products).  On a slab of a group: the cubes
 *     hsk_extract_mesh_cubes covers there; vertices on a plane two slabs share appear in both slabs' meshes.
 *   memory, made on first use and kept: R = Y x (planes of the emitted cubes + 1) grid rows, S = ceil(X / 64) segments per row:
 *     24 S + 2 S + 12 B per row (edge bits: 3 bits per voxel; per-segment bases; count and offset) + 8 B per 1024 rows + at
 *     most 1.3 KiB of alignment; at 512^3 55.0 MiB.  The arrays come back through the product buffer (12 B per vertex for each of vertices and normals,
 *     3 for rgb, 12 per face; it only grows), the faces' row tables are the ones every product shares. */
int hsk_extract_mesh_indexed(hsk_ctx* k, float* vertices /* 3 per vertex */, float* normals /* 3 per vertex, may be NULL */,
                             uint8_t* rgb /* 3 per vertex, may be NULL */, size_t cap_vertices, size_t* n_vertices,
                             int32_t* faces /* 3 per face */, size_t cap_faces, size_t* n_faces, size_t* n_uncolored);

/* ---- Simplified mesh: hsk_extract_mesh_indexed's surface reduced on the device by quadric vertex clustering (Lindstrom's
 * out-of-core simplification, SIGGRAPH 2000; DESIGN.md 3.17 the kernels, 8k the rule).  The volume is cut into cells of
 * c = cluster_voxels voxels; all vertices of the indexed mesh whose cube edge STARTS in a cell (the edge's lower corner g, in voxel
 * indices: cluster (gx / c, gy / c, gz / c) -- an integer identity, not floor of the float position) become one vertex, placed
 * by the quadric of the triangles that touch the cell; a face survives when its three vertices lie in three different clusters.
 *   vertices: the clusters that a surviving face references, in ascending cluster order (plane, row, x).  A blob that lies wholly
 *     inside one cluster yields nothing.  Positions are first quantised to 1/256 voxel -- 256 g off the edge's axis, 256 g +
 *     (512 |Fa| + D) / (2 D) on it, D = |Fb - Fa| of the two stored int16 values, in integers -- and every sum of a cluster is a
 *     64-bit integer relative to the centre of its cell: the count n and sum p of its vertices; over the input triangles with a
 *     vertex in the cluster, each once per cluster, N = (p1 - p0) x (p2 - p0) (twice the area times the normal, towards free
 *     space), dN = N . p0: sum N, sum N N^T, sum N dN.  |sum N dN| < 2^61.4 at c = 16 (hsk_simplify_point.h states and asserts
 *     the arithmetic): no cluster size is refused.  The vertex, in binary64 in a fixed order (hsk_cluster_vertex is the same
 *     text on the host): xbar = sum p / n; HSK_SIMPLIFY_MEAN: x = xbar.  HSK_SIMPLIFY_QUADRIC: A = sum N N^T is diagonalised by
 *     8 cyclic Jacobi sweeps and x = xbar + sum over the eigenvalues lambda_i > sv_floor * lambda_max of v_i (v_i . (sum N dN -
 *     A xbar)) / lambda_i; the vertex's rank is the number of eigenvalues kept (1 on a flat wall, 2 on an edge, 3 at a corner).
 *     x is clamped to the cell grown by one voxel on every side, taken to metres as the soup's vertices are ((voxel + 0.5) *
 *     cell) and rounded once to float.  With anisotropic cells the error that is minimised is the GRID's (distances measured in
 *     voxels), not the metric one.
 *   normals (may be NULL): sum N taken to metric space (each component over its axis's cell), scaled to length 1 in binary64;
 *     NaN x 3 where sum N = 0.
 *   rgb (may be NULL; needs hsk_enable_color, HSK_ERR_STATE): per channel (sum + n_c / 2) / n_c over the n_c vertices of the
 *     cluster that hsk_extract_mesh_indexed's selection rule gives a colour; (0, 0, 0) and one count in n_uncolored where n_c = 0.
 *   faces: the surviving faces in the indexed mesh's order, corners in its order (the winding stays), as indices into vertices.
 *     Faces that name the same three clusters are NOT merged: identifying vertices and dropping the faces with a repeated vertex
 *     commutes with the boundary operator, so a closed input stays closed -- every directed edge (a, b) occurs as often as
 *     (b, a) -- exactly; merging duplicates would break that count.
 *   protocol: hsk_extract_mesh_indexed's.  With every array NULL only the counts and stats; any subset of the arrays may be asked
 *     for; each is written whole or not at all: a cap below its total returns HSK_ERR_ARG with the counts (and the count fields
 *     of stats) set and nothing written.  No flush of the deferred weights; nothing the tracker reads is written, the volume
 *     stays bit for bit; enqueued on hsk_stream() behind the frames submitted so far.  The indexed mesh's count pass is shared
 *     (whichever product asks first pays for it; it is voided by whatever changes the volume), and the clustering's own count
 *     pass is kept likewise for the cluster size last asked for.  params NULL: the defaults.
 *   HSK_ERR_ARG: cluster_voxels outside {0, 2, 4, 8, 16}, an unknown mode, an sv_floor that is negative, non-finite or >= 1.
 *   HSK_ERR_STATE: a slab of a group or any context that stores part of its volume (clusters would straddle the slabs); rgb
 *     without colour; more than INT32_MAX input vertices.
 *   memory, made on first use and kept, beside the indexed mesh's: one byte per cluster of the grid, 24 B + 2 B per 64 clusters
 *     for every cluster row, 12 B per cube row (of the largest cluster grid asked for so far); and 164 B per OUTPUT vertex (its
 *     cluster's number and 20 sums), grown by a quarter more when it has to grow.  At 512^3: 21.0 MiB at c = 2 (16 MiB of it the
 *     cluster bytes), 5.4 MiB at c = 4, 3.3 MiB at c = 8, 3.0 MiB at c = 16, and 15.6 MiB per 100 000 output vertices. */
#define HSK_SIMPLIFY_QUADRIC 0
#define HSK_SIMPLIFY_MEAN 1
typedef struct hsk_simplify_params {
  int32_t cluster_voxels;  /* c: 2, 4, 8 or 16; 0: the default, 4                                                              */
  int32_t mode;            /* HSK_SIMPLIFY_QUADRIC (the default) or HSK_SIMPLIFY_MEAN                                          */
  float sv_floor;          /* eigenvalues up to sv_floor * the largest are dropped; 0: the default, 1e-3 (Lindstrom's value)   */
} hsk_simplify_params;     /* 12 bytes */
typedef struct hsk_simplify_stats {
  uint64_t n_in_vertices, n_in_faces;    /* the indexed mesh                                                                   */
  uint64_t n_clusters;                   /* clusters that hold an input vertex                                                  */
  uint64_t n_out_vertices, n_out_faces;
  uint64_t n_faces_collapsed;            /* input faces with two corners in one cluster: n_in_faces - n_out_faces               */
  uint64_t n_rank[4];                    /* output vertices by the rank of their solve, 0 .. 3 (HSK_SIMPLIFY_MEAN: all rank 0)  */
  uint64_t n_clamped;                    /* output vertices the clamp moved                                                     */
  uint64_t n_uncolored;                  /* output vertices without a coloured input vertex (0 without rgb)                     */
} hsk_simplify_stats;      /* 96 bytes; n_rank, n_clamped and n_uncolored are set by a call that succeeds with n_out_vertices > 0 */
/* cluster_voxels = 4, mode = HSK_SIMPLIFY_QUADRIC, sv_floor = 1e-3; k may be NULL (the defaults do not depend on the volume) */
void hsk_default_simplify_params(const hsk_ctx* k, hsk_simplify_params* p);
int hsk_extract_mesh_simplified(hsk_ctx* k, const hsk_simplify_params* params, float* vertices /* 3 per vertex */,
                                float* normals /* 3 per vertex, may be NULL */, uint8_t* rgb /* 3 per vertex, may be NULL */,
                                size_t cap_vertices, size_t* n_vertices, int32_t* faces /* 3 per face */, size_t cap_faces,
                                size_t* n_faces, hsk_simplify_stats* stats /* may be NULL */);
/* The host mirror of the device solve, as hsk_plane_refit is for the planes: a cluster's representative vertex from its 16 sums
 * -- n, sum p (3), sum N (3), sum N N^T (xx, xy, xz, yy, yz, zz), sum N dN (3), positions in 1/256 voxel relative to the centre
 * of the cluster's cell -- as xyz_voxels relative to that centre, in voxels, with the rank of the solve and whether the clamp
 * moved it.  Host only, needs no device.  HSK_ERR_ARG: a NULL pointer, n <= 0, or what hsk_extract_mesh_simplified refuses of
 * cluster_voxels, mode and sv_floor (0: the defaults). */
int hsk_cluster_vertex(const int64_t sums[16], int cluster_voxels, int mode, float sv_floor, double xyz_voxels[3], int* rank,
                       int* clamped);

/* ---- Baked textures: a colour atlas for any indexed triangle mesh in volume coordinates -- hsk_extract_mesh_simplified's, or one
 * that never came from this library -- at the colour volume's own density, sampled on the device (DESIGN.md 3.25 the kernel, 8s
 * the rule in full; hsk_texture_point.h is its text, for host and device alike).
 *   layout (hsk_texture_layout; host only, integers and binary64 in a fixed order): a face is SKIPPED -- no chart, uv 0, counted in
 *     n_faces_skipped -- when an index is out of range or repeated, a coordinate is not finite, or L2 = 0, L2 the largest squared
 *     edge length ((dx dx + dy dy) + dz dz of the coordinates' exact binary64 differences).  T = L2 (tpm tpm); the face's block
 *     side s is the smallest of 8, 16, 32, 64 with (s - 5)^2 >= T, else 64.  Edge k joins corners k and k + 1 mod 3; r is the
 *     corner opposite the longest edge (the lowest on a tie) and chart corner j holds face corner (j + r) mod 3, so r sits at the
 *     chart's right angle.  The faces of one size, in ascending index, pair up two to a block of s x s texels (half A, then half
 *     B; an odd last face leaves B empty); blocks are placed largest size first at a running offset counted in 8 x 8-texel tiles
 *     that grows by (s / 8)^2 per block: offset >> 6 numbers a 64 x 64 super-tile, row-major across the width W, and the low 6
 *     bits are a Morton code inside it (x the even bits), so every block is aligned to its size.  H = 64 ceil(super-tiles / (W /
 *     64)); H > 16384 is refused (HSK_ERR_ARG) with the needed H in info.height, so that a caller can lower the density.
 *     Inside a block, texel (i, j) has its centre at (i + 1/2, j + 1/2); half A owns the texels with i + j <= s - 2, half B the
 *     rest; A's chart corners are (1, 1), (s - 4, 1), (1, s - 4), B's the point mirror (s - x, s - y): a bilinear look-up anywhere
 *     inside a face's uv triangle touches only texels that the face owns.  uv: u = x / W, v = 1 - y / H (row 0 of the images is
 *     the top), formed in binary64 and rounded once, in the face's corner order.
 *   texel: an unowned texel (no block, or the empty half B) is (0, 0, 0) with mask 0.  Otherwise (x, y) is the texel's centre
 *     in its block (mirrored in half B), u = (x - 1) / (s - 5), v = (y - 1) / (s - 5), P0 = (c0 + u (c1 - c0)) + v (c2 - c0) with
 *     the chart's corners -- ALSO for owned texels outside the triangle, which are not dilated from neighbours but baked at the
 *     extrapolated point.  P0 is projected onto the TSDF's zero level set by up to n_iter Newton steps P <- P - (F / g.g) g, F the
 *     trilinear sample (hsk_sample.h) and g its gradient; it has succeeded once |F| <= f_tol, and fails when a sample leaves the
 *     volume's shell or has a never-observed tap, g.g is not > 0, |P - P0|^2 is not <= max_offset^2, or the steps run out; a
 *     failed texel stays at P0.  At the final point: rgb = the trilinear mean of the eight colour voxels around it over those that
 *     have a colour, min(255, (int)(c + 0.5)) per channel ((0, 0, 0) where their weights sum to 0 or the point is outside the
 *     shell); normal_rgb = g / |g| encoded as HSK_VIEW_NORMALS does ((0, 0, 0) without a valid sample).
 *   mask: HSK_TEXEL_OWNED | _INSIDE (all three barycentrics >= 0) | _PROJECTED | _COLORED | _NORMAL; info counts each -- the last
 *     five counts only in a call that bakes (asks for rgb, normal_rgb or mask).
 *   protocol: every output may be NULL; with all NULL the info only, which is how a caller sizes rgb / normal_rgb (3 W H bytes)
 *     and mask (W H).  Each output is written whole or not at all: cap_texels < W H with rgb, normal_rgb or mask asked for is
 *     HSK_ERR_ARG with info set and nothing written.  The read-outs' contract: enqueued on hsk_stream() behind the frames
 *     submitted so far, nothing the tracker reads is written, the volume stays bit for bit, no flush of the deferred weights (a
 *     weight is only asked whether it is zero); the mesh, the block records and the tile table go up in one copy into the
 *     product buffer, the images come back through the pinned pair; a later call of the same size allocates nothing.
 *   HSK_ERR_ARG: a NULL mesh with n > 0; more than INT32_MAX vertices or faces; texels_per_metre negative or not finite,
 *     atlas_width no multiple of 64 in 64 .. 16384 (0: 1024), n_iter outside 0 .. 16, f_tol or max_offset_m negative or not
 *     finite; the cap; the H overflow.
 *   HSK_ERR_STATE: rgb without hsk_enable_color (normal_rgb and mask need none); a slab of a group or any context that stores
 *     part of its volume. */
#define HSK_TEXEL_OWNED 1
#define HSK_TEXEL_INSIDE 2
#define HSK_TEXEL_PROJECTED 4
#define HSK_TEXEL_COLORED 8
#define HSK_TEXEL_NORMAL 16
typedef struct hsk_texture_params {
  float texels_per_metre;  /* 0: the default, 1 / the smallest cell -- one texel per voxel                                     */
  int32_t atlas_width;     /* W: a multiple of 64 in 64 .. 16384; 0: the default, 1024                                         */
  int32_t n_iter;          /* Newton steps at most, 0 .. 16 (hsk_default_texture_params: 4); taken as it is                   */
  float f_tol;             /* |F| <= f_tol is on the surface, in units of tau (hsk_default_texture_params: 0.01); as it is     */
  float max_offset_m;      /* how far the projection may move a texel's point; 0: the default, 4 x the largest cell           */
} hsk_texture_params;      /* 20 bytes */
typedef struct hsk_texture_chart {
  int32_t x0, y0;          /* the block's first texel                                                                          */
  int32_t s;               /* its side                                                                                         */
  int32_t half_rot;        /* half (0: A, 1: B) | rotation r << 8                                                              */
} hsk_texture_chart;       /* 16 bytes; all four -1 for a skipped face */
typedef struct hsk_texture_info {
  uint64_t width, height;                    /* W, H (the H the mesh needs, also where it is refused)                          */
  uint64_t n_faces_charted, n_faces_skipped;
  uint64_t n_blocks[4];                      /* blocks of side 8, 16, 32, 64                                                   */
  uint64_t n_owned, n_inside, n_projected, n_colored, n_normal;  /* texels by mask bit (a call that bakes)                     */
} hsk_texture_info;        /* 104 bytes */
/* texels_per_metre = atlas_width = 0 and max_offset_m = 0 (the defaults above), n_iter = 4, f_tol = 0.01; k may be NULL */
void hsk_default_texture_params(const hsk_ctx* k, hsk_texture_params* p);
/* The layout alone: host only, needs no device and no context (errors: hsk_last_error(NULL)).  texels_per_metre must be > 0 here
 * (there is no volume to take the default from); atlas_width 0: 1024.  uv (6 per face), charts (one per face) and info may each
 * be NULL. */
int hsk_texture_layout(const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces, float texels_per_metre,
                       int atlas_width, float* uv, hsk_texture_chart* charts, hsk_texture_info* info);
int hsk_bake_texture(hsk_ctx* k, const float* vertices /* 3 per vertex */, size_t n_vertices, const int32_t* faces /* 3 per face */,
                     size_t n_faces, const hsk_texture_params* params /* NULL: the defaults */, uint8_t* rgb /* 3 W H */,
                     uint8_t* normal_rgb /* 3 W H */, uint8_t* mask /* W H */, size_t cap_texels, float* uv /* 6 per face */,
                     hsk_texture_chart* charts /* one per face */, hsk_texture_info* info);

/* ---- Keyframe textures: the atlas of "Baked textures" with its colour from photographs instead of the colour volume (DESIGN.md
 * 3.26 the kernel, 8t the rule in full; hsk_keytex_point.h is its text, for host and device alike).  A colour voxel is a running
 * mean over every frame that saw it and no sharper than a voxel; a keyframe is one colour frame kept whole with its depth image
 * and its pose.  The bake projects every texel's point into every keyframe, tests it against the keyframe's depth, and takes the
 * colour of the keyframe that sees it best.  rgb needs NO hsk_enable_color: a depth-only scan can have a picture.
 *   the store: one device allocation of cap slots made by hsk_enable_keyframes and by nothing later; a slot is a 64-byte record
 *     (the 12 pose floats that matter, fx fy cx cy), the colour image packed to one 32-bit word a pixel (R | G << 8 | B << 16) and
 *     the depth image as uint16: 64 + 6 w h bytes rounded up to 256 (hsk_keyframe_count: bytes).  All keyframes share one size.
 *     A second hsk_enable_keyframes with the same cap, w, h keeps the store and its contents; with others it is HSK_ERR_STATE
 *     until hsk_release_keyframes.  The store does not depend on the volume: hsk_reset and the reset after a tracking loss leave
 *     it alone.  THE CALLER clears it (hsk_clear_keyframes) when the volume's frame is no longer the keyframes' frame -- after a
 *     reset that starts a new scan, a hsk_set_pose into another frame, a volume replaced by an upload, a fusion or a levelled copy.
 *   hsk_add_keyframe: both images are copied before it returns; the copy is enqueued on hsk_stream() behind the frames submitted
 *     so far and writes nothing the tracker reads, so it is legal between hsk_submit_frame and hsk_wait_frame.  depth_mm is in the
 *     sensor's unit, millimetres, 0 = invalid: either the frame's own depth image, or hsk_render_view's depth_mm at the same pose
 *     -- the model's clean depth, which has no sensor noise and no holes the scan has closed.  pose: camera-to-world, row-major, in
 *     the volume's frame (a caller who moves the volume pre-multiplies); only its upper three rows are kept.  intr: fx fy cx cy,
 *     NULL = the context's camera.  *index (may be NULL): the slot taken.  A full store is HSK_ERR_STATE with nothing written; a
 *     size that is not the store's, a NULL image, a pose entry that is not finite, fx or fy not finite or not positive, cx or cy
 *     not finite: HSK_ERR_ARG.
 *   hsk_keyframe_wanted: the host's selection rule, no context, binary64 in a fixed order.  1 when n = 0; else 1 when EVERY
 *     stored pose i differs from `pose` by more than min_translation_m in position (the root of (dx dx + dy dy) + dz dz) OR by
 *     more than min_angle_rad in rotation (acos of (trace(Ri^T R) - 1) / 2 clamped to [-1, 1], the trace summed row by row); else
 *     0.  HSK_ERR_ARG: a threshold negative or not finite, pose NULL, poses NULL with n > 0.
 *   the bake (hsk_bake_texture_keyframes): the layout, uv, charts, normal_rgb, the texel's point and the mask bits OWNED, INSIDE,
 *     PROJECTED and NORMAL are hsk_bake_texture's bit for bit, with its protocol (all NULL: the info only; each output written
 *     whole or not at all; enqueued on hsk_stream(); nothing the tracker reads is written; no flush; a later call of the same size
 *     allocates nothing) and its refusals.  A texel with HSK_TEXEL_NORMAL is looked up in keyframes k = 0 .. n - 1 in ascending
 *     order, binary32, one rounding per written operator.  q = the texel's final point, nh = its gradient over its length, R, t
 *     the keyframe's pose:
 *       1. d = q - t; x_c, y_c, z_c = dot3(d, column 0, 1, 2 of R), dot3(a, b) = (a0 b0 + a1 b1) + a2 b2; z_min_m <= z_c <= z_max_m.
 *       2. r2 = dot3(d, d); c = -dot3(nh, d) / sqrtf(r2); c >= cos_min.
 *       3. u = fx (x_c / z_c) + cx, v likewise (pixel centres at integers); border_px <= u <= (float)(w - 1) - border_px, v against
 *          h; iu = min((int)u, w - 2), a = u - (float)iu, likewise iv, b.
 *       4. every tap (iu + i, iv + j), i, j in 0, 1, has depth D != 0 and fabsf(z_c - (float)D * 0.001f) <= occlusion_tol_m; one
 *          failing tap fails the keyframe for this texel (which also rejects depth edges, holes and whatever walked past the
 *          lens).  (texel, keyframe) pairs that reach this step count in n_pairs_seen, those that fail it in n_pairs_occluded.
 *       5. per channel top = c00 + a (c10 - c00), bot = c01 + a (c11 - c01), val = top + b (bot - top); the weight w_k = c / r2.
 *     HSK_KEYTEX_BEST: the keyframe of the largest w_k, the lowest index on a tie; rgb = min(255, (int)(val + 0.5f)).
 *     HSK_KEYTEX_BLEND: over the passing keyframes with w_k >= blend_floor * w_max, in ascending k, sw += w_k, s += w_k val;
 *       rgb = min(255, (int)(s / sw + 0.5f)) (sw = 0, every weight 0: the best keyframe's val).
 *     source (W H bytes): the index of w_max in both modes, HSK_KEYTEX_NONE where no keyframe passes.
 *     A keyed texel has HSK_TEXEL_KEYFRAME.  A texel no keyframe passes: with fallback_volume != 0 on a context with colour it
 *     takes hsk_bake_texture's colour and HSK_TEXEL_COLORED where the colour volume has one (n_fallback); otherwise it is
 *     (0, 0, 0) (n_uncolored, owned texels only).  HSK_TEXEL_COLORED is therefore set only where the colour volume coloured the
 *     texel, and n_keyed + n_fallback + n_uncolored = n_owned.  With an empty store every texel falls back: the images are
 *     hsk_bake_texture's.
 *   The defaults (hsk_default_keytex_params) are stated CHOICES, not measurements: BEST, z_min_m 0.3, z_max_m 4.0, cos_min 0.2,
 *     border_px 4, occlusion_tol_m 3 x the largest cell (k NULL: 0.03), blend_floor 0.5, fallback_volume 1.
 *   HSK_ERR_ARG (the bake): what hsk_bake_texture refuses; an unknown mode; a parameter negative or not finite; z_min_m > z_max_m;
 *     cos_min > 1; blend_floor > 1.  HSK_ERR_STATE: no store; a slab of a group or a context that stores part of its volume
 *     (every call here that takes a context; hsk_keyframe_count, hsk_clear_keyframes and hsk_release_keyframes never
 *     refuse). */
#define HSK_TEXEL_KEYFRAME 32      /* the texel's colour comes from a keyframe */
#define HSK_KEYTEX_BEST  0
#define HSK_KEYTEX_BLEND 1
#define HSK_KEYTEX_NONE  255       /* source plane: no keyframe */
typedef struct hsk_keytex_params {
  int32_t mode;                    /* HSK_KEYTEX_*                                                                             */
  float z_min_m, z_max_m;          /* the range of z_c in which a keyframe is trusted                                          */
  float cos_min;                   /* the smallest cosine between the texel's normal and the direction to the camera           */
  float border_px;                 /* the image margin a pixel must keep                                                       */
  float occlusion_tol_m;           /* how far a tap's depth may lie from the texel's                                           */
  float blend_floor;               /* HSK_KEYTEX_BLEND: the share of the best weight a keyframe needs, 0 .. 1                  */
  int32_t fallback_volume;         /* != 0: texels no keyframe passes take the colour volume's colour, where there is one      */
} hsk_keytex_params;               /* 32 bytes */
typedef struct hsk_keytex_info {
  uint64_t n_keyframes;            /* the store's keyframes at the call                                                        */
  uint64_t n_keyed, n_fallback, n_uncolored;   /* owned texels by where their colour comes from (a call that bakes)            */
  uint64_t n_pairs_seen, n_pairs_occluded;     /* (texel, keyframe) pairs at step 4, and those that failed it                  */
} hsk_keytex_info;                 /* 48 bytes */
int hsk_enable_keyframes(hsk_ctx* k, int cap /* 1 .. 255 */, int w, int h /* 2 .. 4096 each */);
int hsk_add_keyframe(hsk_ctx* k, const uint16_t* depth_mm, const uint8_t* rgb, int w, int h, const float pose[16],
                     const float intr[4] /* fx fy cx cy; NULL: the context's camera */, int* index /* may be NULL */);
/* every output may be NULL; without a store all are 0 */
int hsk_keyframe_count(const hsk_ctx* k, int* n, int* cap, int* w, int* h, uint64_t* bytes);
/* what went in: the pose with the last row 0 0 0 1.  HSK_ERR_ARG: an index outside 0 .. n - 1; HSK_ERR_STATE: no store */
int hsk_get_keyframe(hsk_ctx* k, int index, float pose[16], float intr[4], uint16_t* depth_mm /* may be NULL */,
                     uint8_t* rgb /* may be NULL */);
int hsk_clear_keyframes(hsk_ctx* k);     /* n = 0, the memory kept */
int hsk_release_keyframes(hsk_ctx* k);   /* the memory freed; hsk_destroy does it too */
int hsk_keyframe_wanted(const float* poses /* 16 per keyframe */, size_t n, const float pose[16], float min_translation_m,
                        float min_angle_rad);   /* host only, no context */
void hsk_default_keytex_params(const hsk_ctx* k /* may be NULL */, hsk_keytex_params* p);
int hsk_bake_texture_keyframes(hsk_ctx* k, const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces,
                               const hsk_texture_params* tp /* NULL: the defaults */, const hsk_keytex_params* kp /* NULL: the defaults */,
                               uint8_t* rgb /* 3 W H */, uint8_t* normal_rgb /* 3 W H */, uint8_t* mask /* W H */, uint8_t* source /* W H */,
                               size_t cap_texels, float* uv, hsk_texture_chart* charts, hsk_texture_info* info, hsk_keytex_info* kinfo);

/* ---- Scene views: what has been fused so far, as an image from any camera (upstream's generateImage / generateDepth and its
 * colour view; DESIGN.md 3.8 the kernel, 8b the rule).  One call marches the TSDF from a virtual pinhole camera, shades the
 * hits on the device and hands back small images.  It is enqueued on hsk_stream() behind every frame submitted so far and
 * waits for its own result only: it neither consumes nor delays a hsk_wait_frame result, and it writes NOTHING the tracker
 * reads (not the tracker state, the model maps, the step keys, the image-buffer sets or the ring), so it is legal in the
 * middle of a pipelined scan -- unlike hsk_raycast, which overwrites the tracker's pose and model maps.  No flush of the
 * deferred weights is needed (a march reads TSDF values only).  The images come back through the product buffer and the
 * pinned staging pair (hsk_prepare_readout covers the first-use costs); nothing is allocated on a later call of the same size. */
#define HSK_VIEW_LAMBERT   0  /* grey: one point light, upstream's generateImage (ambient 50, diffuse 205, no specular)  */
#define HSK_VIEW_NORMALS   1  /* the world normal as a colour: (n * 0.5 + 0.5) * 255 per channel; no normal: background  */
#define HSK_VIEW_COLOR     2  /* the colour volume, unlit (needs hsk_enable_color: HSK_ERR_STATE)                        */
#define HSK_VIEW_COLOR_LIT 3  /* the colour volume times the Lambert term                                                */
typedef struct {
  int width, height;     /* 1..4096 each, any value                                                                    */
  float fx, fy, cx, cy;  /* fx, fy finite and positive                                                                 */
  float pose[16];        /* row-major cam->world, as everywhere on this ABI; ignored when follow != 0                  */
  int follow;            /* 1: the tracker's current pose, read on the device, so the host need not know it: the pose
                            of the last frame enqueued before this call (after a tracking loss: what hsk_get_pose gives) */
  int mode;              /* HSK_VIEW_*                                                                                 */
  float light[3];        /* point light; light_in_camera != 0: in camera coordinates (it moves with the camera)        */
  int light_in_camera;
  uint8_t background[3]; /* every pixel without a hit                                                                  */
} hsk_view;
/* the context's sensor camera, follow = 1, HSK_VIEW_LAMBERT, the light at the camera ((0, 0, 0) in camera coordinates), black
 * background, the identity as pose.  k == NULL: the camera of hsk_default_config; v == NULL: nothing */
void hsk_default_view(const hsk_ctx* k, hsk_view* v);
/* Every output may be NULL.  rgb: 3 bytes per pixel, row-major; depth_mm: the hit's z along the optical axis in millimetres
 * (the sensor's own unit: a rendered depth image can be fed back as a frame), 0 without a hit or outside 1..65535; vmap, nmap:
 * the raycast's world vertex and normal maps for this camera, 3 planes of h*w floats each, NaN = no hit / no normal, bit for
 * bit what hsk_raycast gives for the same camera and pose; *n_hit: pixels with a hit; *n_uncolored: hits whose voxel has
 * colour weight 0 (colour modes; they come out (0, 0, 0)).  The colour of a hit is that of the voxel containing the vertex
 * (nearest voxel, no filtering).  HSK_ERR_ARG: NULL context or view, a size outside 1..4096, fx or fy not finite and
 * positive, an unknown mode; HSK_ERR_STATE: a colour mode without hsk_enable_color, a slab of a group or any context
 * that stores part of the volume (a slab owns only its own march steps). */
int hsk_render_view(hsk_ctx* k, const hsk_view* v, uint8_t* rgb /* 3*w*h */, uint16_t* depth_mm /* w*h */, float* vmap /* 3*h*w SoA */,
                    float* nmap /* 3*h*w SoA */, size_t* n_hit, size_t* n_uncolored);
/* binary Netpbm files of a view: P6 (8-bit RGB) and P5 with maxval 65535 (16-bit, most significant byte first).  w, h in
 * 1..4096; HSK_ERR_ARG for a NULL pointer or a size outside that, HSK_ERR_STATE for an I/O failure */
int hsk_write_ppm(const char* path, const uint8_t* rgb, int w, int h);
int hsk_write_pgm16(const char* path, const uint16_t* depth_mm, int w, int h);

/* ---- Section views: floor plans, elevations and "dollhouse" views (DESIGN.md 3.9 the kernel, 8c the rule).  A room is
 * scanned from inside, so a camera outside it meets the back of a wall or ceiling first and sees nothing.  A section is a
 * scene view whose rays may be parallel (an orthographic camera) and start on clip planes inside the volume: what the planes
 * cut away is not shown, and where a plane cuts through the material of a wall (a negative TSDF) the pixel gets cut_rgb, so
 * walls show as outlines.  With HSK_PROJ_PINHOLE, no planes and a point light hsk_render_section gives hsk_render_view's
 * outputs byte for byte. */
#define HSK_PROJ_PINHOLE 0
#define HSK_PROJ_ORTHO   1   /* parallel rays along the camera's z axis; view.fx, view.fy are PIXELS PER METRE */
#define HSK_MAX_CLIP     4
typedef struct {
  hsk_view view;                /* size, fx, fy, cx, cy, pose, follow, mode, light, light_in_camera, background: as for hsk_render_view */
  int projection;               /* HSK_PROJ_* */
  int light_directional;        /* 0: view.light is a point (8b step 4); 1: a direction TOWARDS the light */
  int n_clip;                   /* 0..HSK_MAX_CLIP */
  float clip[HSK_MAX_CLIP][4];  /* keep a x + b y + c z + d >= 0, in the volume's (world) coordinates */
  uint8_t cut_rgb[3];           /* colour of a pixel whose ray starts on a clip plane inside a negative TSDF */
} hsk_section;
/* hsk_default_view's values, HSK_PROJ_PINHOLE, a point light, no planes, cut_rgb (255, 96, 0).  s == NULL: nothing */
void hsk_default_section(const hsk_ctx* k, hsk_section* s);
/* Outputs, enqueue and ordering contract as hsk_render_view's (legal between submit and wait of pipelined frames; writes nothing
 * the tracker reads; no flush; product buffer and pinned pair; nothing allocated on a later call of the same size).  A pixel is
 * CUT (its ray starts on a clip plane, inside the volume's box, in a voxel with a negative TSDF: cut_rgb, the depth of that
 * point), else a HIT (the march's vertex, if it satisfies every plane), else background.  An orthographic camera's depth_mm is
 * the distance from the camera's plane: a top-down depth image is a height map.  vmap, nmap: NaN except on shown hits;
 * *n_hit, *n_cut: the pixels shown as each; *n_uncolored: as hsk_render_view's, over shown hits.  The march does not stop at a
 * far-side plane; a hit beyond one is not shown.  HSK_ERR_ARG: what hsk_render_view refuses, an unknown projection, n_clip
 * outside 0..HSK_MAX_CLIP, a plane with a non-finite number or a = b = c = 0; HSK_ERR_STATE: as hsk_render_view. */
int hsk_render_section(hsk_ctx* k, const hsk_section* s, uint8_t* rgb /* 3*w*h */, uint16_t* depth_mm /* w*h */,
                       float* vmap /* 3*h*w SoA */, float* nmap /* 3*h*w SoA */, size_t* n_hit, size_t* n_cut, size_t* n_uncolored);
/* host only: a section given in HOUSE coordinates, in the frame of a room placed in the house by the rigid .xf matrix
 * room_xf = M (room -> house, row-major, p_house = M p_room): pose M^-1 pose, each plane (a b c d) M, a world-space point
 * light M^-1 l, a world-space direction R_M^T l; camera-space lights and everything else copied.  Computed in binary64,
 * rounded once.  `room` may be `house`.  HSK_ERR_ARG: a NULL pointer, follow != 0, M's last row not (0 0 0 1),
 * max |R_M^T R_M - I| > 1e-4 (not rigid).  Rigid maps keep the distance from the camera's plane or centre, so the depths of
 * the rooms' sections made from one house section compare: hsk_composite_views. */
int hsk_section_in_room(const hsk_section* house, const float room_xf[16], hsk_section* room);
/* host only: n >= 1 views of one size into one image.  Per pixel the view with the smallest non-zero depth wins (the lowest
 * index on a tie): its rgb, depth and index are written; a pixel without a depth in any view gets background, 0 and -1.
 * Every output may be NULL; rgb may be NULL when out_rgb is.  HSK_ERR_ARG: n < 1, w or h outside 1..4096, depth_mm or one
 * of its entries NULL, rgb (or an entry) or background NULL while out_rgb is given. */
int hsk_composite_views(int n, const uint8_t* const* rgb, const uint16_t* const* depth_mm, int w, int h,
                        const uint8_t background[3], uint8_t* out_rgb, uint16_t* out_depth_mm, int32_t* out_index);

/* ---- Volume fusion: one volume resampled through a rigid transform into another and merged by weight, on the device
 * (DESIGN.md 3.10 the kernels, 8d the rule).  With it a "house" context is an ordinary hsk_ctx -- a larger vol_size_m, non-cubic
 * dims -- into which every room is fused by its .xf; every product (clouds, meshes, views, sections) and hsk_integrate then
 * work on the house unchanged, and a second scan session of a room merges into the first. */
typedef struct {
  uint64_t n_fused;      /* destination voxels that took a sample (rule step 3)                    */
  uint64_t n_colored;    /* of those, voxels whose colour was merged (step 4)                       */
  uint64_t chunks_total; /* destination work units inside the footprint                             */
  uint64_t chunks_swept; /* ... of which were swept voxel by voxel (the others left on the skip test) */
  int32_t  box[6];       /* the destination footprint swept: x0 x1 y0 y1 z0 z1, half-open, voxels   */
} hsk_fuse_stats;

/* dst <- dst (+) resample(src) under src_to_dst (row-major, p_dst = M p_src, rigid).  stats may be NULL.
 * Destination voxel (x, y, z), centre pd, is sampled at ps = M^-1 pd (hsk_invert_rigid) with the raycast's trilinear sample Fs
 * and the smallest weight Ws of its eight taps; a sample on the source's outer shell or with Ws == 0 leaves the voxel alone,
 * else raw' = round((raw_d W_d + q Ws) / (W_d + Ws)) with q = rint(Fs * 32767), W' = min(W_d + Ws, 128); the colour of the
 * source voxel containing ps is merged likewise, by the colour weights.  Stored TSDF values are in units of the truncation
 * distance, so the two EFFECTIVE truncation distances (trunc_dist_m after the 2.1-cell clamp) must be bit-equal; cells, dims
 * and sizes may differ in every other way.
 * Synchronous: returns when the destination is complete and the counts are on the host.  The source is read only (its deferred
 * free-space weights are written back first, which changes nothing it returns).  The destination's deferred weights are
 * written back before the merge; behind it its brick bitfield and summaries are rebuilt (as by hsk_upload_tsdf), so every later
 * product, integrate or raycast sees a consistent volume.  The destination's tracker pose and model maps are NOT touched: a
 * host that goes on scanning against the fused volume calls hsk_resume_scan(dst, pose) first, which sets them and makes the next
 * frame a tracked one (hsk_raycast sets them too, but leaves a context that has seen no frame at its first-frame step).
 * Colour is merged iff both contexts have called hsk_enable_color; otherwise the destination's colour volume, if any, is
 * untouched and n_colored = 0.  An empty footprint: HSK_OK, zero counts, nothing launched.
 * HSK_ERR_ARG: a NULL context, src == dst, a matrix hsk_invert_rigid refuses, unequal truncation distances, contexts on
 * different devices; HSK_ERR_STATE: a frame in flight in either context, a slab of a group or any context that stores part of
 * its volume (hsk_render_view's cases). */
int hsk_fuse_volume(hsk_ctx* dst, hsk_ctx* src, const float src_to_dst[16], hsk_fuse_stats* stats);

/* host only: the inverse of a rigid matrix, computed in binary64 from the binary32 entries and rounded once
 * (R^T, -R^T t; last row 0 0 0 1).  The rigidity test and HSK_ERR_ARG are hsk_section_in_room's. */
int hsk_invert_rigid(const float m[16], float inv[16]);

/* host only: the half-open destination voxel box that can receive a sample.  It is the image of the source volume's
 * interior under M, padded by one destination cell and clipped to the destination.  Empty: x1 <= x0, HSK_OK. */
int hsk_fuse_footprint(const int src_dims[3], const float src_size_m[3], const int dst_dims[3], const float dst_size_m[3],
                       const float src_to_dst[16], int32_t box[6]);

/* ---- Volume files: a scanned volume (TSDF + colour) as a lossless sparse image, made and consumed on the device, so that a
 * room outlives its process: saved behind a scan, loaded later to be fused into a house, merged with a second session or
 * scanned further (DESIGN.md 3.11 the kernels, 8e the format "HSKV" version 1).  The volume is cut into bricks of 8 x 8 x 8
 * voxels; a brick is stored as nothing (every word 0), one word (all words equal), its tsdf and 512 weight bytes (free
 * space: one tsdf, weights below 256) or its 512 words; only the packed bytes cross the host link. */
typedef struct {
  uint32_t version, header_bytes;  /* 1, 256                                                                         */
  uint32_t flags;                  /* bit 0: the image holds colour                                                  */
  int32_t dims[3];                 /* vol_x, vol_y, vol_z                                                            */
  int32_t z0, nz;                  /* the stored planes (hsk_stored_planes); whole volumes only: 0, vol_z            */
  float size_m[3];
  float trunc_dist_m;              /* as configured                                                                  */
  float trunc_eff_m;               /* as used: after the 2.1-cell clamp; stored TSDF values are in units of it       */
  int32_t width, height;           /* the depth camera                                                               */
  float fx, fy, cx, cy;
  float pose[16];                  /* the tracker pose when the image was made (hsk_get_pose)                        */
  int32_t frame;                   /* frames the scan had taken since its (re)start                                  */
  int32_t color_max_weight;        /* hsk_enable_color's parameters as in effect (0, 0 without colour)               */
  float color_band_m;
  uint64_t n_bricks;               /* (vol_x / 8) (vol_y / 8) ceil(nz / 8)                                           */
  uint64_t tsdf_bricks[4];         /* per class: ZERO, UNIFORM, SPLIT, RAW                                           */
  uint64_t color_bricks[2];        /* ZERO, RAW (0, 0 without colour)                                                */
  uint64_t tsdf_table_bytes, tsdf_payload_bytes, color_table_bytes, color_payload_bytes;
  uint64_t total_bytes;            /* header + the four sections = the image                                         */
  int32_t pass_reused;             /* hsk_pack_volume only (not in the image): 1 when the call found the class and offset pass
                                      of an earlier call in place */
} hsk_volume_info;

/* The image of the context's volume.  Two-call protocol like the products': with buf == NULL only *n_bytes and *info (may be
 * NULL) are set, and the class and offset pass is kept for the next call while the volume is unchanged; a cap_bytes below the
 * total returns HSK_ERR_ARG with the counts set and nothing written.  The deferred free-space weights are written back first
 * (as by hsk_download_tsdf: the image holds weights).  Colour is packed iff the context has called hsk_enable_color.
 * Synchronous.  The bytes come back through the product buffer and the pinned staging pair; device memory: the packed size
 * plus 10 bytes per brick of tables, never a second copy of the volume.  HSK_ERR_STATE: a frame in flight, a slab of a group
 * or any context that stores part of its volume (hsk_render_view's cases). */
int hsk_pack_volume(hsk_ctx* k, void* buf, size_t cap_bytes, size_t* n_bytes, hsk_volume_info* info);
/* Replaces the context's volume as a whole by the image's.  The image is validated on the host first (hsk_volume_image_info's
 * rules: HSK_ERR_ARG and an untouched context); dims, stored planes, size_m and the effective truncation distance must then
 * equal the context's bit for bit (HSK_ERR_ARG).  The payload goes up in batches through the pinned pair, the bricks are
 * written on the device, the brick bitfield and the summaries are rebuilt (as by hsk_upload_tsdf).  Colour: image and context
 * both have it: taken; only the context: its colour volume is zeroed; only the image: skipped.  The tracker pose and the model
 * maps are NOT touched (hsk_resume_scan does that).  State errors as hsk_pack_volume's. */
int hsk_unpack_volume(hsk_ctx* k, const void* buf, size_t n_bytes);
/* the image as a file, byte for byte.  Save writes `path`.tmp and renames it into place; an I/O failure is HSK_ERR_STATE */
int hsk_save_volume(hsk_ctx* k, const char* path, hsk_volume_info* info /* may be NULL */);
int hsk_load_volume(hsk_ctx* k, const char* path);
/* host only: the header of an image, after validating the image: magic, version, header size; a self-consistent header
 * (dims, planes, brick count, section lengths, total); every class byte legal; the header's brick counts and section lengths
 * those that follow from the class tables; the total equal to n_bytes.  HSK_ERR_ARG with a message (hsk_last_error(NULL))
 * otherwise.  There is no payload checksum.  The file form reads the header and the class tables only. */
int hsk_volume_image_info(const void* buf, size_t n_bytes, hsk_volume_info* info);
int hsk_volume_file_info(const char* path, hsk_volume_info* info);
/* host only: hsk_default_config with the image's dims, size_m, configured trunc_dist_m and camera, its pose as init_pose: a
 * context created from *c accepts the image */
int hsk_config_from_volume(const hsk_volume_info* info, hsk_config* c);
/* Puts the tracker where it stands after a tracked frame at `pose`: the pose is set, the model maps of all three levels are
 * made by the raycast of the volume as it is (hsk_raycast's device work without the downloads), the lost flag and any pending
 * reset are cleared, and the context counts as having seen a frame -- so the next frame, through any of the frame calls, is
 * tracked by ICP against the volume, whoever grew it (hsk_unpack_volume, hsk_load_volume, hsk_fuse_volume, hsk_upload_tsdf).
 * HSK_ERR_STATE: a frame in flight, a slab of a group. */
int hsk_resume_scan(hsk_ctx* k, const float pose[16]);

/* ---- Volume alignment: a cloud with normals, or another volume, registered against this volume's TSDF on the device
 * (DESIGN.md 3.12 the kernel, 8f the rule).  It makes or improves the rigid matrix that hsk_fuse_volume and hsk_resume_scan take:
 * stitch -> align -> fuse for the rooms of a house, load -> align -> fuse / resume for a second session of a room.
 * Every source point p (unit normal n towards free space) is moved by the current M and looked up in the destination's TSDF
 * at p and at `probes` steps of the truncation distance tau to either side along n: a TSDF holds distance only within tau of
 * a surface, the probes widen the basin to (probes + 1) tau.  The probe with the smallest |F| whose TSDF gradient agrees with
 * n (cosine >= cos_gate) gives the point its row of a point-to-plane system; the 27 + 1 sums are exact (the ICP's 2^-26
 * quantisation, integer accumulation), the 6 x 6 solve and the pose update are the tracker's (hsk_icp_solve), taken about
 * the volume's centre.  Far probes can find OTHER surfaces (a prototype of the rule ended 11 mm off with 5 probes on the scene
 * of DESIGN.md 8f; the exact rule did not repeat that, it took 5 iterations instead of 4): the default is 3, whose basin of
 * 4 tau already exceeds the wall stitch's 5 cm at every resolution, at 7 look-ups per point instead of 11.
 * What the statuses do NOT say: the points of one wall alone do not make the solve fail -- rounding keeps the 6 x 6 system
 * regular -- and may even end CONVERGED, with the motion along the wall left wherever it was (15 mm off on that scene).  Give it
 * points whose normals span the three directions. */
#define HSK_ALIGN_CONVERGED 0   /* the last step was below eps_rot and eps_trans_m: out is the refined matrix              */
#define HSK_ALIGN_MAX_ITERS 1   /* max_iters steps without that: DO NOT TRUST out                                          */
#define HSK_ALIGN_FEW 2         /* fewer than min_points points found a valid probe: out is the last matrix formed         */
#define HSK_ALIGN_DEGENERATE 3  /* the 6 x 6 system was singular: out is the last matrix formed                            */
#define HSK_ALIGN_DIVERGED 4    /* the steps' sum passed max_rot or max_shift_m: out is src_to_dst, bit for bit            */
#define HSK_ALIGN_MAX_ITERS_CAP 64
#define HSK_ALIGN_DIRECT (-1)   /* `probes`: none to either side, the point itself only (0 means the default)              */
typedef struct {
  int max_iters;        /* 1..64                                                             default 30             */
  int probes;           /* to either side, 1..8; HSK_ALIGN_DIRECT: none                      default 3              */
  float cos_gate;       /* least cosine between n and the TSDF gradient, (0, 1]              default 0.5            */
  uint32_t max_points;  /* the cloud is taken with the stride ceil(n / max_points); <= 2^20  default 262144         */
  uint32_t min_points;  /*                                                                   default 256            */
  float eps_rot;        /* radians: largest |angle| of a step that counts as converged       default 1e-5           */
  float eps_trans_m;    /* metres, likewise                                                  default 1e-5           */
  float max_rot;        /* radians: sum over the steps of their largest |angle|              default 0.2            */
  float max_shift_m;    /* metres, likewise                                                  default 2 (probes + 1) tau */
} hsk_align_params;     /* a 0 in a field means its default                                                         */
typedef struct {
  int status;                                /* HSK_ALIGN_*                                                          */
  int iterations;                            /* iterations taken, 1..max_iters                                       */
  uint32_t n_points, stride;                 /* points used (of every `stride` one, from the first)                  */
  uint32_t n_used[HSK_ALIGN_MAX_ITERS_CAP];  /* per iteration: points with a valid probe                             */
  float rms_m[HSK_ALIGN_MAX_ITERS_CAP];      /* per iteration: root mean square of their residuals (0 without a point) */
  float x_last[6];                           /* the last solved step (alpha, beta, gamma, tx, ty, tz)                */
  double sums_last[28];                      /* the last iteration's sums: the solve's 27, then the residuals' squares */
} hsk_align_stats;

/* the defaults of the table above, as values (max_shift_m from dst's truncation distance; 0 with dst NULL) */
void hsk_default_align_params(const hsk_ctx* dst, hsk_align_params* p);
/* n points xyz (3 floats each) with unit normals towards free space (3 floats each; NaN normals are allowed, such points never
 * contribute), in source coordinates; src_to_dst the rough matrix (row-major, p_dst = M p_src, rigid); out the refined one.
 * params NULL: the defaults; stats may be NULL.  Synchronous.  The points go up once, into a scratch buffer that dst owns
 * (made on first use, only grown); an iteration is one kernel launch on dst's stream and a read-back of 4 KiB.  dst's deferred
 * free-space weights are written back first (the rule reads weights); nothing else of dst is written: not the volume, the
 * brick flags, the tracker pose, the model maps or the cached count passes.  Every HSK_ALIGN_* status returns HSK_OK: the
 * status is a value, like tracked = 0.  n = 0 is not an error (HSK_ALIGN_FEW).
 * HSK_ERR_ARG (out untouched): a NULL context, xyz (with n > 0), normals (with n > 0) or out; a matrix hsk_invert_rigid refuses;
 * a parameter outside its range; half the diagonal of dst's box above 8 m or (probes + 1) tau above 8 m (the sums' exactness).
 * HSK_ERR_STATE (out untouched): a frame in flight, a slab of a group or any context that stores part of its volume
 * (hsk_render_view's cases). */
int hsk_align_cloud(hsk_ctx* dst, const float* xyz, const float* normals, size_t n, const float src_to_dst[16],
                    const hsk_align_params* params, float out[16], hsk_align_stats* stats);
/* src's hsk_extract_cloud_attrs product (xyz and normals) handed to hsk_align_cloud: the result is that of making the two
 * calls yourself, bit for bit.  The cloud passes through host memory.  Only dst's TSDF is sampled, so -- unlike the fuse --
 * the two truncation distances need not be equal.  Errors as hsk_align_cloud's, the state errors also for src; a NULL src or src == dst:
 * HSK_ERR_ARG. */
int hsk_align_volume(hsk_ctx* dst, hsk_ctx* src, const float src_to_dst[16], const hsk_align_params* params, float out[16],
                     hsk_align_stats* stats);
/* host only: one iteration's solve and pose update about `centre`: x6 = hsk_icp_solve(sums27); with (R, t) = m the tracker's
 * pose update is applied to (R, t - centre) and centre added back.  A singular system: *ok = 0, x6 zeros, m_next = m. */
int hsk_align_step(const double sums27[27], const float m[16], const float centre[3], float m_next[16], float x6[6], int* ok);

/* ---- Loss hold and relocalisation: keep the volume when tracking is lost, and find a frame's pose in it (DESIGN.md 3.13 the
 * kernel, 8g the rule).  The host loop: hsk_set_loss_policy(k, HSK_LOSS_HOLD) once; a frame reports
 * tracked = 0 and the volume stays; hsk_pose_lattice around the last pose -> hsk_relocalize with the next frame ->
 * hsk_resume_scan(k, pose_out) -> frames are tracked again.  The search is LOCAL: the host supplies the candidate poses; a
 * whole-room search is a host loop over lattices, not a promise (views of a bare wall are ambiguous in a box). */
#define HSK_LOSS_RESET 0 /* a lost frame restarts the scan: the volume is wiped, the pose is the initial pose (the default) */
#define HSK_LOSS_HOLD 1  /* a lost frame is dropped: nothing but its verdict changes                                       */
/* Under HSK_LOSS_HOLD a frame that loses tracking reports tracked = 0 and the pose of the last tracked frame; the volume, the
 * colour volume, the model maps and the frame count stay as they were; frames in flight behind it are dropped on the device (as
 * under RESET) and report tracked = 0 and that same pose; the next frame submitted is tracked by ICP from the last tracked pose
 * against the unchanged model maps.  hsk_reset still resets; hsk_track_stream stays frame for frame what hsk_process_frame
 * gives under the same policy.  HSK_ERR_ARG: a NULL context, an unknown policy; HSK_ERR_STATE: a frame in flight, a slab of a
 * group (a group handles a loss itself). */
int hsk_set_loss_policy(hsk_ctx* k, int policy);
int hsk_get_loss_policy(const hsk_ctx* k); /* -1 for NULL */

/* How a cloud lies in the volume under one pose.  Every point falls in exactly one of the six counts. */
typedef struct hsk_pose_score {
  uint32_t n_near;    /* |F| < 1 at the moved point: on a surface the volume holds                                  */
  uint32_t n_free;    /* F >= 1: a measured point in space the volume saw empty                                     */
  uint32_t n_behind;  /* F <= -1                                                                                    */
  uint32_t n_unseen;  /* one of the sample's eight voxels was never observed                                        */
  uint32_t n_outside; /* outside the volume, or in its outer shell of voxels                                        */
  uint32_t n_skipped; /* a NaN coordinate (an invalid pixel of a vertex map)                                        */
  uint64_t sum_abs;   /* over the near points: rint(|F| * 65536), added as integers                                 */
} hsk_pose_score;     /* 32 bytes */
/* n points xyz (3 floats each, camera coordinates) under each of n_poses poses (16 floats each, row-major, p_dst = M p):
 * out[j] is pose j's score.  The moved point is sampled once with the raycast's trilinear sample; no normals, no gradient.
 * Synchronous.  The cloud goes up once, into the scratch buffer of hsk_align_cloud (only grown: a later call of the same size
 * allocates nothing); dst's deferred free-space weights are written back first, nothing else of dst is written.
 * n <= 2^20, n_poses <= 65536; n = 0 or n_poses = 0: HSK_OK (the scores are zeros).  HSK_ERR_ARG (out untouched): a NULL
 * context, xyz (n > 0), poses or out (n_poses > 0); a count above its limit; a pose hsk_invert_rigid refuses (the message names
 * its index).  HSK_ERR_STATE: hsk_align_cloud's cases. */
int hsk_score_cloud(hsk_ctx* dst, const float* xyz, size_t n, const float* poses, size_t n_poses, hsk_pose_score* out);
/* host only: order[] = the indices 0..n-1 by key = n_near - n_free - n_behind (signed), larger first; ties to the smaller
 * sum_abs, then to the lower index.  HSK_ERR_ARG: a NULL pointer with n > 0. */
int hsk_rank_scores(const hsk_pose_score* s, size_t n, uint32_t* order);

#define HSK_RELOC_FOUND 0
#define HSK_RELOC_NONE 1      /* no refined candidate was accepted: pose_out is the best-scored candidate, unrefined; DO NOT TRUST it */
#define HSK_RELOC_EMPTY 2     /* the frame's level has no valid pixel, or n_poses == 0: pose_out is the identity            */
#define HSK_RELOC_FINEST (-1) /* `level`: level 0 (0 means the default)                                                   */
#define HSK_RELOC_MAX_REFINE 16
typedef struct {
  int level;              /* pyramid level whose maps are scored and refined: 1, 2 or HSK_RELOC_FINEST   default 2       */
  int n_refine;           /* best-ranked candidates refined, 1..16                                       default 4       */
  float accept_fraction;  /* least n_used(last iteration) / n_valid, (0, 1]                              default 0.5     */
  float accept_rms_m;     /* largest rms of the last iteration                                           default tau / 4 */
  hsk_align_params align; /* zeros: hsk_align_cloud's defaults                                                           */
} hsk_reloc_params;       /* a 0 in a field means its default                                                            */
typedef struct {
  int status;             /* HSK_RELOC_*                                                                                 */
  uint32_t n_valid;       /* pixels of the level with a vertex                                                           */
  uint32_t n_candidates;  /* n_poses                                                                                     */
  int32_t best;           /* index (into poses) of the candidate the result was refined from; NONE: the best-scored; EMPTY: -1 */
  int32_t n_refined;      /* entries of the arrays below: min(n_refine, n_poses)                                         */
  int32_t candidate[HSK_RELOC_MAX_REFINE];     /* by rank: index into poses (-1 beyond n_refined)                        */
  hsk_pose_score score[HSK_RELOC_MAX_REFINE];  /* ... its score                                                          */
  int32_t align_status[HSK_RELOC_MAX_REFINE];  /* ... its refinement's HSK_ALIGN_* status                                */
  int32_t iterations[HSK_RELOC_MAX_REFINE];
  uint32_t n_used[HSK_RELOC_MAX_REFINE];       /* ... of its last iteration                                              */
  float rms_m[HSK_RELOC_MAX_REFINE];
} hsk_reloc_stats;
/* the defaults as values (accept_rms_m and align.max_shift_m from k's truncation distance; 0 with k NULL) */
void hsk_default_reloc_params(const hsk_ctx* k, hsk_reloc_params* p);
/* Finds the camera pose of one depth frame among the candidates.  Defined by composition, bit for bit: the frame is
 * preprocessed as by hsk_preprocess; the cloud is ALL pixels of the level's vertex map in row-major order (invalid pixels are
 * NaN: skipped by the score, never a term of the alignment), the normals are the normal map's, each negated when n . v > 0;
 * the candidates are scored (hsk_score_cloud) and ranked (hsk_rank_scores); each of the first n_refine is refined by
 * hsk_align_cloud(k, cloud, normals, n, candidate, &params->align, ..); a refinement is ACCEPTED when its status is
 * HSK_ALIGN_CONVERGED, n_used[last] >= accept_fraction * n_valid and rms_m[last] <= accept_rms_m; the winner is the accepted
 * one with the largest n_used[last], then the smallest rms, then the earlier rank.  On the device the cloud never leaves it:
 * the read-backs are the scores and 4 KiB per alignment iteration.
 * It overwrites the image buffers of set 0 (as hsk_preprocess does) and nothing else: not the volume (the deferred weights
 * are written back), the tracker pose, the model maps, the flags, the frame count or the cached count passes.  The host then
 * calls hsk_resume_scan(k, pose_out) and, if it wants the frame in the volume, hsk_integrate(depth, pose_out).
 * params NULL: the defaults; stats may be NULL.  Every HSK_RELOC_* status returns HSK_OK.  Errors: hsk_score_cloud's and
 * hsk_align_cloud's; a frame size that is not the context's, a level or n_refine outside its range, accept_fraction outside
 * (0, 1] or a negative or non-finite accept_rms_m: HSK_ERR_ARG. */
int hsk_relocalize(hsk_ctx* k, const uint16_t* depth, int w, int h, const float* poses, size_t n_poses,
                   const hsk_reloc_params* params, float pose_out[16], hsk_reloc_stats* stats);
/* host only: the candidate lattice pose = centre . T(i step_m, j step_m, k step_m) . Ry(a step_rad) . Rx(b step_rad) for
 * i, j, k in [-n_trans, n_trans] and a, b in [-n_rot, n_rot] -- offsets in the camera's own frame -- computed in binary64 and
 * rounded once; i slowest, then j, k, a, and b fastest; (2 n_trans + 1)^3 (2 n_rot + 1)^2 poses, of which the one with all
 * offsets 0 is `centre` bit for bit.  Two calls: poses == NULL sets *n only.  HSK_ERR_ARG: a NULL centre or n, a negative
 * count, a non-finite step, more than 65536 poses, cap below the count (with *n set). */
int hsk_pose_lattice(const float centre[16], float step_m, int n_trans, float step_rad, int n_rot, float* poses, size_t cap, size_t* n);

/* ---- Oriented plane detection on the device: a room's planes from points with normals, a caller's cloud or the context's own
 * volume (DESIGN.md 3.14 the kernels, 8h the rule; tests/planes_twin.py restates the rule in numpy).  With a normal at every
 * point one point is a plane hypothesis, and the two faces of one wall -- 3 cm apart, normals opposed -- are two planes, which
 * the unoriented host detector (hsk_detect_planes) cannot tell apart.  Every device sum is an integer: the result is the same
 * bits whatever the launch shape.  A plane's normal points as its points' normals do: into the room.
 * A point is VALID iff its six numbers are finite and |x|, |y|, |z| <= 64; it is an INLIER of (a, b, c, d) iff it is valid,
 * unlabelled, |((a x + b y) + c z) + d| <= dist_m and (a nx + b ny) + c nz >= cos_min (binary32, no contraction). */
typedef struct hsk_plane_params {
  float dist_m;           /* largest |distance| of an inlier, (0, 1]                                     default 0.02       */
  float cos_min;          /* least n_plane . n_point of an inlier, [-1, 1]                               default cos 30 deg */
  float min_fraction;     /* a plane needs max(3, floor(min_fraction n)) inliers; finite, >= 0           default 0.03       */
  int32_t max_planes;     /* 1..64                                                                       default 12         */
  int32_t n_hypotheses;   /* seed points tried per round, 1..4096                                        default 512        */
  int32_t refits;         /* refits of a round's best hypothesis on its inliers, 0..8                    default 2          */
  uint64_t seed;          /* of the 64-bit LCG that draws the seed points               default 0x9E3779B97F4A7C15          */
} hsk_plane_params;       /* 32 bytes; every field is taken as it stands (no "0 = default")                                 */
void hsk_default_plane_params(hsk_plane_params* p);
typedef struct hsk_plane_record {
  float abcd[4];          /* a x + b y + c z + d = 0, (a, b, c) a unit normal (the seed point's as stored when refits = 0)  */
  uint32_t n_inliers;     /* the points labelled with this plane                                                            */
  uint32_t pad;           /* 0                                                                                              */
  uint64_t sum_abs;       /* over them: rint(|distance| * 65536), added as integers (mean residual = sum_abs / 65536 / n)   */
} hsk_plane_record;       /* 32 bytes */
#define HSK_PLANE_MAX_POINTS ((size_t)1 << 24)
#define HSK_PLANE_MAX_PLANES 64
#define HSK_PLANE_MAX_HYPOTHESES 4096
#define HSK_PLANE_MAX_REFITS 8
/* The planes of n points xyz with normals (3 floats each), in detection order.  Round by round while fewer than max_planes are
 * found: n_hypotheses seed points i = next() % n (hsk_detect_planes' generator, running on across rounds) each make the
 * plane (its normal, d = -((a x + b y) + c z)) -- none when the point is invalid or labelled; every hypothesis is scored
 * against every point, the largest count wins (ties: the first) and the detection ends when it is below the least count; the
 * winner is refitted `refits` times on its inliers (hsk_plane_refit on their integer moments); its inliers are labelled -- or,
 * when the refits left fewer than the least count, nothing is and the detection ends.
 * params NULL: the defaults.  planes: cap records (at most max_planes are written); labels (may be NULL): n ints, the plane of
 * each point or -1; *n_invalid (may be NULL): the invalid points.  Synchronous.  The context supplies the device, the stream
 * and the scratch (hsk_align_cloud's, only grown): its volume is not read and nothing of it is written, so any idle context
 * will do.  n = 0: HSK_OK, no planes.  HSK_ERR_ARG: a NULL context, xyz or normals (n > 0), planes or n_planes; n > 2^24; a
 * parameter outside its range; cap < max_planes.  HSK_ERR_STATE: a frame in flight. */
int hsk_detect_planes_oriented(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const hsk_plane_params* params,
                               hsk_plane_record* planes, size_t cap, size_t* n_planes, int32_t* labels, size_t* n_invalid);
/* The same on the context's own cloud -- hsk_extract_cloud_attrs' points and normals, in that order, which never leave the
 * device -- so the labels are in that cloud's order: extract it (before or after; the count pass is shared) to use them.
 * Two calls as for the products: planes == NULL and labels == NULL set *n_points only; otherwise cap as above and, with labels,
 * cap_labels >= *n_points (HSK_ERR_ARG with *n_points set when it is not).  Nothing the tracker reads is written, and the
 * cached count pass stays valid.  HSK_ERR_STATE: a frame in flight; a slab of a group or a context that stores part of its
 * volume (as hsk_render_view); HSK_ERR_ARG also: a cloud of more than 2^24 points. */
int hsk_detect_planes_volume(hsk_ctx* k, const hsk_plane_params* params, hsk_plane_record* planes, size_t cap, size_t* n_planes,
                             int32_t* labels, size_t cap_labels, size_t* n_points);
/* The scoring stage alone: counts[j] = the inliers of planes_abcd[4 j ..] among the n points; labels (may be NULL: every valid
 * point is unlabelled): n ints, a point with a label >= 0 counts for no plane.  n_planes <= 4096, n <= 2^24, dist_m in (0, 1],
 * cos_min in [-1, 1]; n = 0: zeros.  Errors as hsk_detect_planes_oriented's. */
int hsk_score_planes(hsk_ctx* k, const float* xyz, const float* normals, const int32_t* labels, size_t n, const float* planes_abcd,
                     size_t n_planes, float dist_m, float cos_min, uint32_t* counts);
/* host only: one refit.  sums10 = the inliers' count m, the sums of q_x, q_y, q_z and of q_x q_x, q_x q_y, q_x q_z, q_y q_y,
 * q_y q_z, q_z q_z with q = rint(coordinate * 4096) (|q| <= 2^18, m <= 2^24).  C_ab = (double)(m S_ab - S_a S_b) / ((double)m
 * (double)m), the numerator exact; the normal is C's eigenvector of the smallest eigenvalue (hsk_detect_planes' Jacobi) divided
 * by its length, negated when its binary64 dot product with prev_abcd's normal is negative; d = -(n . mean), mean =
 * ((double)S_a / (double)m) / 4096; the four numbers rounded to binary32 once.  *ok = 0 and out_abcd = prev_abcd: m < 3, or a
 * length below 1e-12.  HSK_ERR_ARG: a NULL pointer, m < 0 or > 2^24, a sum outside +-2^62. */
int hsk_plane_refit(const int64_t sums10[10], const float prev_abcd[4], float out_abcd[4], int* ok);

/* ---- Upright frame: level a scan.  The volume's frame is the first camera's; a hand-held scan that starts looking down puts the
 * room into the volume tilted, and every floor form (hsk_clearance_floor, hsk_reach_floor, hsk_partition_floor) and floor plan
 * wants the up axis to be one of the volume's axes.  This estimates the scan's upright (Manhattan) frame from its oriented points
 * -- the up direction from floor and ceiling together, the two wall directions from all walls at once, the floor and ceiling
 * heights and the content's box -- on the device, in a handful of streaming passes with integer sums: the result is the same bits
 * whatever the launch shape (DESIGN.md 3.21 the kernels, 8o the rule; tests/level_twin.py restates the rule in numpy).
 * hsk_level_config turns it into the configuration of a levelled, wall-aligned volume of minimal size and the matrix that
 * hsk_fuse_volume, hsk_transform_cloud and hsk_write_xf take. */
#define HSK_UPRIGHT_NO_YAW 1u          /* params.flags: level only, row 0 is the volume's +X projected                          */
#define HSK_UPRIGHT_UP 1u              /* found: the up direction ...                                                           */
#define HSK_UPRIGHT_YAW 2u             /* ... the walls' direction ...                                                          */
#define HSK_UPRIGHT_FLOOR 4u           /* ... floor_m ...                                                                       */
#define HSK_UPRIGHT_CEILING 8u         /* ... ceiling_m                                                                         */
#define HSK_UPRIGHT_MAX_POINTS ((size_t)1 << 24)
#define HSK_UPRIGHT_MAX_REFITS 8
#define HSK_UPRIGHT_HIST_BINS 1536     /* the cube map of normals: 6 faces x 16 x 16                                            */
#define HSK_UPRIGHT_HEIGHT_BINS 16384  /* the height histograms: 1/64 m a bin, bin 8192 begins at 0                             */
#define HSK_UPRIGHT_AXIS_MAX2 16810000 /* the largest |A|^2 of an integer axis A = rint(a 4096): 4100^2                         */
typedef struct hsk_upright_params {
  float up_hint[3];       /* roughly up, in the volume's frame; finite, not zero        default (0, -1, 0): image y points down */
  float max_tilt_cos;     /* up lies within this cone about the hint, [-1, 1]                            default cos 45 deg */
  float cone_cos;         /* a point supports an axis when its normal lies within this cone, (0, 1]      default cos 10 deg */
  float wall_sin;         /* a wall point's normal lies within this angle of the horizon, [0, 1]         default sin 15 deg */
  float min_fraction;     /* an axis needs max(3, floor(min_fraction n)) supporters; finite, >= 0        default 0.02       */
  int32_t refits;         /* 0..8                                                                        default 3          */
  uint32_t flags;         /* HSK_UPRIGHT_NO_YAW                                                          default 0          */
} hsk_upright_params;     /* 36 bytes; every field is taken as it stands (no "0 = default")                                 */
void hsk_default_upright_params(hsk_upright_params* p);
typedef struct hsk_upright {
  float level[16];        /* row-major, a pure rotation, p_level = L p_volume: row 1 (the levelled +Y) is DOWN, row 0 the wall
                             direction nearest the volume's +X, row 2 = row 0 x row 1.  The identity unless UP was found       */
  float floor_m, ceiling_m; /* the levelled y of the floor and of the ceiling (floor_m > ceiling_m: y points down)            */
  float box_lo[3], box_hi[3]; /* the valid points' box in the levelled frame                                                 */
  uint32_t n_points, n_invalid; /* the cloud; of it, the points with a number not finite, |x| > 64, |n_k| > 2 or N = 0        */
  uint32_t n_axis[3];     /* the supporters of the three rows in the last refit (refits = 0: [1] is the seed's support)       */
  uint32_t n_walls;       /* the wall points the yaw was taken from                                                          */
  uint32_t found;         /* HSK_UPRIGHT_UP | _YAW | _FLOOR | _CEILING                                                        */
  uint32_t pad;           /* 0                                                                                                */
} hsk_upright;            /* 128 bytes */
/* The upright frame of the context's own cloud and normals (hsk_extract_cloud_attrs' points), which never leave the device; the
 * normals are weighted by the cells (w_k = c_min / c_k: the raycast's normals are differences over one cell per axis).  params
 * NULL: the defaults.  An empty cloud: HSK_OK, nothing found.  Nothing the tracker reads is written, and the cached count pass
 * stays valid.  HSK_ERR_ARG: a NULL context or out; a parameter outside its range; a cloud of more than 2^24 points.
 * HSK_ERR_STATE: as hsk_detect_planes_volume (a frame in flight, a slab of a group, a context that stores part of its volume). */
int hsk_estimate_upright(hsk_ctx* k, const hsk_upright_params* params, hsk_upright* out);
/* The same on a caller's n points with normals (3 floats each), through the alignment scratch.  cell_weights: the three w_k, each
 * in (0, 1]; NULL: 1, 1, 1 (true normals).  n = 0: HSK_OK, nothing found.  HSK_ERR_ARG also: NULL xyz or normals with n > 0,
 * n > 2^24, a weight outside (0, 1].  HSK_ERR_STATE: a frame in flight. */
int hsk_estimate_upright_oriented(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const float cell_weights[3],
                                  const hsk_upright_params* params, hsk_upright* out);
/* The device stages alone, for integer axes A = rint(a 4096) the caller gives (|A|^2 <= HSK_UPRIGHT_AXIS_MAX2, not zero); every
 * output may be NULL and its stage is then not run:
 *   hist: the cube-map histogram, HSK_UPRIGHT_HIST_BINS counts; n_valid: the valid points (either or both);
 *   axis_sums: for each of the n_axes <= 3 axes (3 ints each) the count of its supporters and the three sums of sign(N . A) N;
 *   wall_sums: for wall_axes = (up, e1, e2) the count of up's wall points and the two fourth-power sums;
 *   box: for frame = three rows R, the min (3) and max (3) of t_k = P . R_k over the valid points (zeros when there is none), in
 *   units of 2^-22 m; height_counts and height_sums (both or neither): 2 x HSK_UPRIGHT_HEIGHT_BINS, the floor class then the ceiling
 *   class -- the supporters of R_1 whose normal points against it, then along it: per bin the count and the sum of t_1.
 * cone_cos and wall_sin as in hsk_upright_params.  Errors as hsk_estimate_upright_oriented's; n = 0: zeros. */
int hsk_upright_sums(hsk_ctx* k, const float* xyz, const float* normals, size_t n, const float cell_weights[3], float cone_cos,
                     float wall_sin, uint32_t* hist, uint32_t* n_valid, const int32_t* axes, int n_axes, int64_t* axis_sums,
                     const int32_t* wall_axes, int64_t* wall_sums, const int32_t* frame, int32_t* box, uint32_t* height_counts,
                     int64_t* height_sums);
/* host only: the steps between the device stages, in binary64 with + - x / and sqrt only.  `least`:
 * the least count max(3, floor(min_fraction n)).  HSK_ERR_ARG: a NULL pointer, a hint that is zero or not finite.
 *   seed: the 2 x 2 block of histogram bins of the largest support (its four counts plus their antipodes') among those whose shared
 *   corner lies within max_tilt_cos of the hint -> the corner's direction, the support, *found = the support reaches `least`;
 *   axis: sums4 = (count, S) -> S / |S| in the hint's hemisphere, *ok = 0 when S = 0;
 *   basis: (e1, e2) of the plane across `up`;  yaw: wall3 = (count, re, im) -> x, *found = 0 and the plain x without it;
 *   frame: one refit of (up, x), in place, from the three rows' sums12;  rows: the three rows (x, -up, x x -up);
 *   heights: floor_m, ceiling_m and the bits HSK_UPRIGHT_FLOOR | HSK_UPRIGHT_CEILING from the two height histograms. */
int hsk_upright_solve_seed(const uint32_t* hist, const float up_hint[3], float max_tilt_cos, uint64_t least, double axis[3],
                           uint64_t* support, int* found);
int hsk_upright_solve_axis(const int64_t sums4[4], const float up_hint[3], double axis[3], int* ok);
int hsk_upright_solve_basis(const double up[3], double e1[3], double e2[3]);
int hsk_upright_solve_yaw(const int64_t wall3[3], uint64_t least, const double up[3], double x[3], int* found);
int hsk_upright_solve_frame(const int64_t sums12[12], uint64_t least, const float up_hint[3], int yaw, double up[3], double x[3]);
int hsk_upright_solve_rows(const double up[3], const double x[3], double rows9[9], int32_t axes9[9]);
int hsk_upright_solve_heights(const uint32_t* height_counts, const int64_t* height_sums, uint64_t least, double* floor_m,
                              double* ceiling_m, uint32_t* found);
/* host only: the configuration of the levelled destination of `src` and the matrix hsk_fuse_volume(dst, src, M) takes.  One
 * isotropic cell, the source's largest; the extent is up's box plus margin_m on every side (negative: the effective truncation
 * distance plus two cells), every dim rounded up to a multiple of 8; M = T L with the translation that puts box_lo - margin at
 * the origin.  Camera, ICP and device fields are the source's; init_pose = M x the source's current pose (what
 * hsk_resume_scan(dst, .) wants); trunc_dist_m = the source's effective truncation distance, and each vol_size_m[k] is the
 * largest binary32 not above dims_k c whose quotient by dims_k does not exceed c, so the two effective distances are bit-equal.
 * HSK_ERR_ARG: a NULL pointer, UP not found, a margin that is not finite, a box that is not finite or gives a dim above 4096. */
int hsk_level_config(hsk_ctx* src, const hsk_upright* up, float margin_m, hsk_config* cfg, float src_to_dst[16]);

/* ---- Scan coverage: what the volume has never observed, and where the camera should go to see it (DESIGN.md 3.15 the kernels,
 * 8i the rule; tests/cover_twin.py restates the rule in numpy).  A voxel is UNSEEN when its weight is 0, FREE when it was
 * observed with a positive TSDF, SOLID when it was observed with a TSDF <= 0.  The host loop: hsk_coverage_census (is anything
 * open, and on which side) -> hsk_pose_lattice around the current pose -> hsk_score_views -> hsk_rank_views -> show
 * hsk_render_coverage of the best view to the operator.  Every device sum is an integer: the same bits whatever the launch shape.
 * The three device calls behave like hsk_render_view: enqueued on hsk_stream() behind every frame submitted so far, waiting
 * only for their own result, writing nothing the tracker reads -- legal between submit and wait of pipelined frames.  Results
 * come through the product buffer and the pinned staging pair; nothing is allocated on a later call of the same size
 * (hsk_prepare_readout covers the first).  HSK_ERR_STATE: a slab of a group, or any context that stores part of its volume
 * (hsk_render_view's cases). */
typedef struct hsk_voxel_box {
  int lo[3], hi[3];       /* the voxels lo <= (x, y, z) < hi                                                                  */
} hsk_voxel_box;
typedef struct hsk_coverage {
  uint64_t n_unseen, n_free, n_solid;   /* the box's voxels by state                                                          */
  uint64_t n_frontier;    /* FREE voxels of the box with at least one of their six face neighbours UNSEEN; the neighbour lies
                             inside the grid, it may lie outside the box                                                       */
  uint64_t faces[6];      /* the pairs (FREE voxel of the box, UNSEEN neighbour) by direction: -x, +x, -y, +y, -z, +z           */
} hsk_coverage;           /* 80 bytes */
/* A probe is a virtual depth camera.  Pixel (u, v) looks along (dx, dy, 1), dx = ((float)u - cx) / fx, dy = ((float)v - cy) / fy;
 * sample i = 0 .. n - 1 of its ray lies at optical-axis depth z = near_m + (float)i * step_m -- a depth sensor's own notion of
 * range -- at the camera point (dx z, dy z, z); n = min(4096, floor((far_m - near_m) / step_m) + 1) in binary64.  A sample is
 * INSIDE iff its voxel (floor(p / cell), unclamped) lies in the grid.  The ray walks its samples in order and ends in one class:
 *   OUTSIDE   no sample was inside
 *   BLIND     the first inside sample is not FREE: the camera would sit in unknown or solid space
 *   HIT       after >= 1 FREE sample, the first non-FREE inside sample is SOLID
 *   FRONTIER  ... is UNSEEN; the ray goes on, and its gain is the number of UNSEEN inside samples from that one onward, up to
 *             the first SOLID sample, the first outside sample or the last sample
 *   OPEN      every inside sample is FREE, up to the last sample or to the first outside sample behind an inside one
 * The deciding sample of a HIT or FRONTIER ray is that first non-FREE one; its depth is rint(z * 1000) millimetres when within
 * 1..65535, else 0 (and 0 for the other classes).
 * step_m: keep it at or below half the truncation distance (the default).  The band of SOLID voxels behind a surface is one
 * truncation distance thick; a longer step can carry a ray from FREE straight into the UNSEEN space behind a wall and report a
 * frontier that is not there. */
typedef struct hsk_probe {
  int width, height;      /* 1..4096 each                                                                                      */
  float fx, fy, cx, cy;   /* fx, fy finite and positive                                                                        */
  float near_m, far_m;    /* 0 <= near_m <= far_m, finite                                                                      */
  float step_m;           /* finite and positive                                                                               */
} hsk_probe;
#define HSK_RAY_HIT 0
#define HSK_RAY_FRONTIER 1
#define HSK_RAY_OPEN 2
#define HSK_RAY_BLIND 3
#define HSK_RAY_OUTSIDE 4
#define HSK_EYE_FREE 0
#define HSK_EYE_UNSEEN 1
#define HSK_EYE_SOLID 2
#define HSK_EYE_OUTSIDE 3
typedef struct hsk_view_score {
  uint32_t n_hit, n_frontier, n_open, n_blind, n_outside;   /* the rays by class: they sum to width * height                  */
  uint32_t eye_state;     /* HSK_EYE_*: the voxel that holds the camera centre (OUTSIDE: none does)                            */
  uint64_t gain;          /* the sum of the rays' gains                                                                        */
} hsk_view_score;         /* 32 bytes */
#define HSK_COVER_MAX_POSES ((size_t)65536)
/* the context's camera at a quarter of its resolution (pyramid level 2), near_m = 0.4, far_m = 3.5, step_m = half the context's
 * truncation distance; k NULL: hsk_default_config(256)'s camera and truncation distance */
void hsk_default_probe(const hsk_ctx* k, hsk_probe* p);
/* The census of the box (NULL: the whole volume).  HSK_ERR_ARG (out untouched): a NULL context or out; lo < 0, hi > the volume's
 * dims or hi < lo on an axis.  An empty box (hi == lo on an axis) is legal and counts nothing. */
int hsk_coverage_census(hsk_ctx* k, const hsk_voxel_box* box, hsk_coverage* out);
/* One hsk_view_score per pose (n_poses matrices of 16 floats, row-major, camera -> world; at most 65536) for the probe (NULL:
 * hsk_default_probe's).  n_poses = 0: HSK_OK.  HSK_ERR_ARG (out untouched): a NULL context, poses or out; a probe field outside
 * its range; more than 65536 poses; a pose hsk_invert_rigid refuses (the message names its index). */
int hsk_score_views(hsk_ctx* k, const hsk_probe* probe, const float* poses, size_t n_poses, hsk_view_score* out);
/* One pose, per pixel (row-major, any of the three may be NULL): cls = HSK_RAY_*, depth_mm of the deciding sample, gain (saturated
 * at 65535); score (may be NULL): what hsk_score_views gives for this pose.  Errors as hsk_score_views'. */
int hsk_render_coverage(hsk_ctx* k, const hsk_probe* probe, const float pose[16], uint8_t* cls /* w*h */, uint16_t* depth_mm /* w*h */,
                        uint16_t* gain /* w*h */, hsk_view_score* score);
/* host only: order[0..n) = the indices by larger gain first; ties to the larger n_frontier, then to the lower index; the poses
 * whose eye_state is not HSK_EYE_FREE -- viewpoints nobody can stand in -- behind all others, in the same order among themselves */
int hsk_rank_views(const hsk_view_score* s, size_t n, uint32_t* order);

/* ---- Cloud import: a point cloud rendered into the depth images of virtual cameras and fused like a sensor's frames (DESIGN.md
 * 3.27 the kernels, 8u the rule; tests/splat_twin.py restates the rule in numpy).  The way INTO the volume chain for data that
 * are no depth stream: a room directory's cloud_bin.pcd (hsh_read_pcd_xyz), another scanner's cloud, this library's own
 * exports once their volume is gone.  xyz alone suffices, and free space is carved as a sensor carves it -- so clearance, reach,
 * partition and coverage, which take never-observed space for an obstacle, work on the result.  The host loop: hsk_pose_lattice
 * (centre, 0, 0, step_rad, n_rot) for a fan of views from one standpoint -> hsk_import_cloud -> hsk_coverage_census,
 * hsk_score_views, hsk_rank_views for where the next virtual camera should stand -> hsk_import_cloud again.
 *   The camera is the context's own (width, height, fx, fy, cx, cy); pose is camera -> world, rigid.  Per point p:
 *   1. a coordinate that is not finite: skipped (n_invalid)
 *   2. p_c = R^T (p - t), z = p_c.z; z outside [near_m, far_m]: skipped (n_clipped)
 *   3. HSK_SPLAT_SURFEL, the point's normal n finite and not zero: n . p_c >= 0 faces away -- skipped (n_backfacing); this is what
 *      keeps the far face of a thin wall out of a view.  Any other normal makes the point a DISC point
 *   4. the footprint: the integer pixels u0 - ru <= u <= u0 + ru, v0 - rv <= v <= v0 + rv inside the image, (u0, v0) = (fx x / z +
 *      cx, fy y / z + cy), ru = fx half_m / z and rv = fy half_m / z each clamped to [min_half_px, max_half_px], half_m = 0.5
 *      point_size_m cover.  No pixel: skipped (n_outside); min_half_px >= 0.5, so a point inside the image owns at least one
 *   5. every pixel of the footprint is offered a depth in millimetres, rounded as hsk_render_view's depth image rounds and kept to
 *      1..65535 -- DISC: the point's z; SURFEL: the depth at which the pixel's ray ((u - cx) / fx, (v - cy) / fy, 1) meets the
 *      point's tangent plane, clamped to z +- 2 half_m (n_splatted counts the points that reach this step)
 *   A pixel's value is the smallest depth offered to it, 0 if none was: the image does not depend on the order of the points.
 *   point_size_m is a property of the CLOUD -- the leaf size of a downsampled cloud, the spacing of neighbouring points of one
 * surface --, not of the camera or the volume; its default, the context's largest cell, is right for a cloud this library
 * extracted from such a volume.  cover must be >= sqrt(2) for a regular grid of that spacing in any in-plane rotation to be
 * watertight under square footprints (default 1.5).
 *   Colour is out of scope: neither an rgb field of the cloud nor a winner-index image is taken. */
#define HSK_SPLAT_DISC 0
#define HSK_SPLAT_SURFEL 1
#define HSK_SPLAT_MAX_POINTS ((size_t)1 << 24)
#define HSK_SPLAT_MAX_POSES ((size_t)65536)
typedef struct hsk_splat_params {   /* a 0 in a field means its default */
  int mode;               /* HSK_SPLAT_DISC (default), HSK_SPLAT_SURFEL (needs normals)                                        */
  float point_size_m;     /* finite, > 0; default: the context's largest cell (without a context 3 / 512)                      */
  float cover;            /* finite, >= 1; default 1.5                                                                         */
  float min_half_px;      /* >= 0.5; default 0.5                                                                               */
  float max_half_px;      /* min_half_px .. 64; default 8                                                                      */
  float near_m, far_m;    /* 0 < near_m <= far_m <= 65.535; defaults 0.1 and 8                                                 */
} hsk_splat_params;       /* 28 bytes */
typedef struct hsk_splat_stats {
  uint32_t n_invalid, n_clipped, n_backfacing, n_outside, n_splatted;   /* the points by what became of them: they sum to n     */
  uint32_t n_pixels;      /* the pixels of the image that are not 0                                                            */
} hsk_splat_stats;        /* 24 bytes */
/* the defaults as values (k NULL: point_size_m = 3 / 512) */
void hsk_default_splat_params(const hsk_ctx* k /* may be NULL */, hsk_splat_params* p);
/* One view: the cloud (n <= 2^24 packed xyz triples; normals likewise or NULL: DISC only) as the depth image of the context's camera
 * at `pose`.  Writes nothing of the context but scratch -- pose, volume (the deferred weights are not even flushed), model maps and
 * image buffers stay bit for bit -- and is legal between submit and wait of pipelined frames.  n = 0: HSK_OK, the image all 0.
 * The cloud goes up once per call; nothing is allocated on a later call of the same size.
 * HSK_ERR_ARG (outputs untouched): a NULL context, pose or depth_out; xyz NULL with n > 0; n > 2^24; SURFEL without normals; a
 * parameter that is not finite or outside its range; a pose hsk_invert_rigid refuses.  HSK_ERR_STATE: a slab of a group, or any
 * context that stores part of its volume. */
int hsk_splat_cloud(hsk_ctx* k, const float* xyz, const float* normals /* NULL: DISC only */, size_t n, const float pose[16],
                    const hsk_splat_params* params /* NULL: the defaults */, uint16_t* depth_out /* width * height of the context */,
                    hsk_splat_stats* stats /* may be NULL */);
/* Defined by composition, bit for bit: for j ascending, hsk_integrate(k, hsk_splat_cloud's image of poses[j], width, height,
 * poses[j]).  The cloud goes up once, the frames never leave the device, the host waits once at the end, and the views' counters
 * come back in one copy.  Leaves the pose at poses[n_poses - 1], as the composition does; follow with hsk_resume_scan(k, that pose)
 * to track a live sensor on in the imported volume.  n_poses = 0: HSK_OK and nothing changes; n = 0: the views are empty frames,
 * which change no voxel.
 * HSK_ERR_ARG (context and per_view untouched): hsk_splat_cloud's cases; poses NULL with n_poses > 0; n_poses > 65536; a pose
 * hsk_invert_rigid refuses (the message names its index).  HSK_ERR_STATE: frames in flight; a slab of a group, or any context that
 * stores part of its volume. */
int hsk_import_cloud(hsk_ctx* k, const float* xyz, const float* normals /* NULL: DISC only */, size_t n, const float* poses /* 16 per view */,
                     size_t n_poses, const hsk_splat_params* params, hsk_splat_stats* per_view /* n_poses of them, may be NULL */);

/* ---- Cloud normals: oriented normals and curvature of a cloud that has none, on the device (DESIGN.md 3.28 the kernels, 8v the
 * rule; tests/normals_twin.py restates the rule in numpy).  What a room directory's cloud_bin.pcd or another scanner's cloud needs
 * before HSK_SPLAT_SURFEL, hsk_detect_planes_oriented, hsk_estimate_upright_oriented and hsk_align_cloud can take it.  A fixed-radius
 * neighbourhood on the 1 / 4096 m grid of the plane moments, integer sums, a binary64 solve: the result is the same bits whatever
 * the launch shape, and permuting the cloud permutes the outputs and changes no bit.  Per point p:
 *   1. a coordinate that is not finite or beyond +-64 m: HSK_NORMAL_INVALID.  q = rint(4096 coordinate)
 *   2. its neighbours: every valid point j with |q_j - q_p|^2 <= r_q^2 in integers, r_q = rint(4096 radius_m) -- the boundary, the
 *      point itself and every duplicate included.  m of them
 *   3. m < min_neighbours: HSK_NORMAL_SPARSE; m > max_neighbours: HSK_NORMAL_CROWDED, reported as max_neighbours + 1 -- the cost of a
 *      call is the sum of m, and a dense cloud wants hsk_voxel_downsample or a smaller radius first
 *   4. the covariance m S_ab - S_a S_b of the neighbours' q - q_p, exact in 64 bits; its eigenvalues e0 <= e1 <= e2 by eight cyclic
 *      Jacobi sweeps in binary64.  Not e1 > line_rel e2: HSK_NORMAL_DEGENERATE (a collinear or coincident neighbourhood)
 *   5. the normal: the eigenvector of e0 at length 1, turned towards the nearest of the viewpoints (the lowest index on a tie; one
 *      standpoint per room makes each face of a shared wall turn to its own room); without viewpoints, or when the viewpoint lies
 *      in the tangent plane, so that its component of largest magnitude is positive (the lowest index on a tie)
 *   6. curvature = max(e0, 0) / (e0 + e1 + e2), the surface variation: 0 on a plane, at most 1 / 3
 * Every class but HSK_NORMAL_OK has the normal (0, 0, 0) and the curvature 0; INVALID has the neighbour count 0.
 *   Out of scope: colour, k-nearest neighbourhoods (a cap on WHICH neighbours count would depend on their order), normals
 * propagated without a standpoint, outlier filters (threshold neighbours_out). */
#define HSK_NORMAL_OK 0
#define HSK_NORMAL_INVALID 1
#define HSK_NORMAL_SPARSE 2
#define HSK_NORMAL_CROWDED 3
#define HSK_NORMAL_DEGENERATE 4
#define HSK_NORMAL_MAX_POINTS ((size_t)1 << 24)
#define HSK_NORMAL_MAX_VIEWPOINTS 256
typedef struct hsk_normal_params {   /* a 0 in a field means its default */
  float radius_m;           /* 1 / 1024 .. 0.25; default: 3 x the context's largest cell, clamped to that range (no context: 9 / 512) */
  uint32_t min_neighbours;  /* >= 3; default 8                                                                                  */
  uint32_t max_neighbours;  /* min_neighbours .. 2^20; default 4096                                                             */
  float line_rel;           /* finite, 0 < line_rel <= 1; default 1e-3                                                          */
  uint32_t flags;           /* 0                                                                                                */
  uint32_t pad;
} hsk_normal_params;        /* 24 bytes */
typedef struct hsk_normal_stats {
  uint32_t n_ok, n_invalid, n_sparse, n_crowded, n_degenerate;   /* the points by class: they sum to n                          */
  uint32_t n_cells;         /* the occupied cells of the search grid (edge r_q)                                                 */
  uint64_t n_pairs;         /* the sum of the reported neighbour counts: the work done                                          */
} hsk_normal_stats;         /* 32 bytes */
/* the defaults as values (k NULL: radius_m = 9 / 512) -- stated choices, not measurements */
void hsk_default_normal_params(const hsk_ctx* k /* may be NULL */, hsk_normal_params* p);
/* The normals of the cloud (n <= 2^24 packed xyz triples), synchronous; any idle context will do, its volume is not read.  Writes
 * nothing of the context but scratch: pose, volume, deferred weights, model maps and image buffers stay bit for bit.  The cloud goes
 * up once; nothing is allocated on a later call of the same size.  n = 0: HSK_OK, zero stats.  With CROWDED points the call still
 * returns HSK_OK, and hsk_last_error says how many and what to do.
 * HSK_ERR_ARG (outputs untouched): a NULL context or normals_out; xyz NULL with n > 0; n > 2^24; viewpoints NULL with n_viewpoints > 0;
 * n_viewpoints > 256; a viewpoint that is not finite; a parameter that is not finite or outside its range; flags != 0.
 * HSK_ERR_STATE: frames in flight; a slab of a group, or any context that stores part of its volume. */
int hsk_estimate_normals(hsk_ctx* k, const float* xyz, size_t n, const float* viewpoints /* 3 each, may be NULL */, size_t n_viewpoints,
                         const hsk_normal_params* params /* NULL: the defaults */, float* normals_out /* 3 n */,
                         float* curvature_out /* n, may be NULL */, uint32_t* neighbours_out /* n, may be NULL */,
                         uint8_t* class_out /* n, may be NULL */, hsk_normal_stats* stats /* may be NULL */);
/* host only: one point's solve from its ten sums -- m, S_x S_y S_z, S_xx S_xy S_xz S_yy S_yz S_zz of the neighbours' q - q_p -- as the
 * device does it (steps 4 to 6): *class_out HSK_NORMAL_OK or HSK_NORMAL_DEGENERATE.  HSK_ERR_ARG: a NULL pointer, m outside 1 .. 2^20,
 * a sum beyond what m neighbours within 1024 grid steps can make, viewpoints NULL with n_viewpoints > 0, n_viewpoints > 256, a
 * point or viewpoint that is not finite, a line_rel outside (0, 1]. */
int hsk_normal_solve(const int64_t sums10[10], const float point[3], const float* viewpoints, size_t n_viewpoints, float line_rel,
                     float normal_out[3], float* curvature_out, int* class_out);

/* ---- Surface components: the volume's pieces, labelled on the device, and the call that erases the small ones (DESIGN.md 3.16
 * the kernels, 8j the rule; tests/components_twin.py restates the rule in numpy).  All integers.  A voxel is INSIDE when it was
 * observed (weight != 0) with a NEGATIVE TSDF -- the voxels that can be the negative end of a zero crossing, so everything the
 * read-outs show hangs on one of them (not the coverage rule's SOLID, which also takes a TSDF of 0).  Two INSIDE voxels are
 * adjacent when they differ by 1 on exactly one axis (6-neighbourhood; diagonal contact does not connect: the band behind a
 * surface is at least 2.1 cells thick, so a surface is 6-connected).  With lin(x, y, z) = (z vol_y + y) vol_x + x, the label of an
 * INSIDE voxel is the smallest lin of its component (its root), that of every other voxel HSK_COMPONENT_NONE: integers that no
 * schedule can change.  Records are ordered by n_voxels descending, ties to the smaller root; a component's rank is its place
 * in that order.  No flush of the deferred weights is needed to label (no deferred weight is 0 in the volume's own copy, and
 * TSDF values are always current); the labelling stays on the device and is reused until the volume changes.  Its scratch --
 * one 32-bit parent per stored voxel, as large as the volume itself -- is made by the first call that labels, NOT by
 * hsk_prepare_readout (which only loads the kernels): a context that never labels does not pay for it.
 * HSK_ERR_STATE: frames in flight, a slab of a group, or any context that stores part of its volume.  HSK_ERR_ARG: a NULL
 * context or output, a volume of more than 2^31 voxels, and what each call lists.  A refused call writes nothing. */
#define HSK_COMPONENT_NONE 0xffffffffu
#define HSK_COMPONENT_MAX ((size_t)1 << 24)
typedef struct hsk_component {
  int32_t root[3];        /* x, y, z of the root                                                                                */
  int32_t pad;
  uint64_t n_voxels;
  int32_t lo[3], hi[3];   /* the voxel bounding box, hi exclusive                                                               */
} hsk_component;          /* 48 bytes */
typedef struct hsk_component_stats {
  uint64_t n_components, n_inside, largest;   /* the components, their voxels, the voxels of the first record                  */
  int32_t labels_reused;  /* 1: the labelling of an earlier call was still valid                                                */
  int32_t pad;
} hsk_component_stats;    /* 32 bytes */
#define HSK_PRUNE_UNSEEN 0   /* a pruned voxel becomes word 0: never observed                                                   */
#define HSK_PRUNE_FREE 1     /* ... becomes (weight << 16) | 0x7fff: observed free space, its weight kept                       */
typedef struct hsk_prune_params {
  uint64_t min_voxels;    /* a component with fewer voxels is pruned                                                            */
  int32_t keep_largest;   /* > 0: so is every component of rank >= keep_largest; 0: no limit; at most 4096                     */
  int32_t fill;           /* HSK_PRUNE_UNSEEN (the default: a pruned blob may have been a real small object, and "never
                             observed" is the honest state -- the coverage census then shows a frontier round it) or HSK_PRUNE_FREE */
} hsk_prune_params;       /* 16 bytes */
typedef struct hsk_prune_stats {
  uint64_t n_components, n_pruned, n_pruned_voxels, n_kept_voxels;
} hsk_prune_stats;        /* 32 bytes */
/* min_voxels = the voxels of a cube of edge 4 tau, ceil((4 tau)^3 / (cell_x cell_y cell_z)) computed in binary64 from the
 * context's binary32 truncation distance and cells (k NULL: hsk_default_config(256)'s): anything whose inside is smaller than a
 * 12 cm cube at the default tau of 3 cm.  A stated choice, not a measurement -- set another value where it does not fit.
 * keep_largest = 0, fill = HSK_PRUNE_UNSEEN. */
void hsk_default_prune_params(const hsk_ctx* k, hsk_prune_params* p);
/* Labels the volume (or finds the labelling of an earlier call still valid) and gives the records in their order.  recs NULL:
 * the counts only (*n_components, stats).  HSK_ERR_ARG with *n_components and stats set and no record written: cap below the
 * count; more than 2^24 components (a volume of noise; hsk_prune_components shares the limit; such a labelling is not kept:
 * every call labels again).  stats may be NULL. */
int hsk_label_components(hsk_ctx* k, hsk_component* recs, size_t cap, size_t* n_components, hsk_component_stats* stats);
/* the dense label volume: vol_x * vol_y * vol_z labels, row-major, x fastest; labels first when no valid labelling is held */
int hsk_download_components(hsk_ctx* k, uint32_t* labels);
/* Prunes the components with n_voxels < min_voxels or, with keep_largest > 0, of rank >= keep_largest (params NULL: the
 * defaults): every voxel of theirs gets the fill word and, where the context has colour, the colour word 0.  Every other word of
 * the volume and of the colour volume stays as it is bit for bit (the deferred weights written back).  When nothing is pruned
 * nothing is written and cached passes stay valid.  The pose and the model maps are not touched (as by hsk_unpack_volume): a
 * scan may go on.  stats may be NULL.  HSK_ERR_ARG: keep_largest outside 0..4096, an unknown fill. */
int hsk_prune_components(hsk_ctx* k, const hsk_prune_params* params, hsk_prune_stats* stats);

/* ---- Hole filling: close a scan's gaps by volumetric diffusion, on the device (DESIGN.md 3.22 the kernels, 8p the rule;
 * tests/fill_twin.py restates the rule in numpy; after Davis, Marschner, Garr and Levoy, "Filling holes in complex surfaces using
 * volumetric diffusion", 3DPVT 2002).  The counterpart of hsk_prune_components: prune turns small observed blobs into "never
 * observed", fill turns small never-observed gaps into surface.  All integers.
 * STATES.  A voxel (z < vol_z) is a SOURCE iff its weight is non-zero; its value is its raw TSDF, a raw of -32768 counting as
 * -32767 in every sum and test (the word itself is never rewritten).  Every other voxel starts UNKNOWN.  No flush of the deferred
 * weights is needed to read (no deferred weight is 0 in the volume's own copy).
 * ONE ITERATION is a Jacobi step: every new state comes from the previous iteration's states.  A source never changes; a
 * non-source voxel outside the box never changes (it stays UNKNOWN).  For a non-source voxel v inside the box, K = the KNOWN
 * voxels (sources and filled ones) among v itself and its six face neighbours inside the grid, n = |K|: n = 0, v stays UNKNOWN;
 * otherwise v is FILLED with the value (2 U + n) div (2 n) - 32768, U the sum of value + 32768 over K -- the mean, half rounded
 * up.  A filled voxel is computed again in every iteration: the field relaxes.  `iterations` of them run; iterations_run is the
 * number of the first one that changed no state, or `iterations`.
 * A CROSSING, on the final states, in hsk_extract_cloud's words: two face-adjacent KNOWN voxels, neither at 32767, one value > 0
 * and the other < 0; both are crossing voxels (sources or filled ones, inside the box or outside it).
 * KEEP.  HSK_FILL_SURFACE: a FILLED voxel is written iff a crossing voxel lies within Chebyshev distance `band` of it (2: the cells
 * of the crossing and the neighbours a normal's central difference reads).  HSK_FILL_ALL: every FILLED voxel is written.  The
 * diffusion front also runs `iterations` voxels into every wall's never-observed interior; those voxels make no crossing, carry
 * no information, would bridge the two faces of a thin wall for hsk_label_components and bloat hsk_pack_volume: hence the default.
 * A written voxel's word is (fill_weight << 16) | (value & 0xffff) -- with the default weight 1 the first real observation counts
 * half.  Every other word of the volume and every word of the colour volume stays bit for bit (the deferred weights written
 * back, as by hsk_prune_components).  When nothing is to be written nothing is written and cached passes stay valid.  The pose
 * and the model maps are not touched: a scan may go on.
 * KNOWN PROPERTY: where a scan simply ends (a frustum's edge) the surface is continued outward by up to `iterations` voxels, as
 * Davis et al. describe; the box is the remedy.
 * The scratch -- two int16 states per stored voxel, together as large as the volume -- is made by the first call that fills, NOT
 * by hsk_prepare_readout (which only loads the kernels).
 * HSK_ERR_STATE: frames in flight, a slab of a group, or any context that stores part of its volume.  HSK_ERR_ARG: a NULL
 * context, a volume of more than 2^31 voxels, iterations outside 1..255, an unknown keep, band outside 0..8, fill_weight
 * outside 1..128, a box with lo < 0, hi > the volume's dims or hi < lo on an axis (an empty box is legal and fills nothing).  A
 * refused call writes nothing. */
#define HSK_FILL_SURFACE 0
#define HSK_FILL_ALL 1
typedef struct hsk_fill_params {
  int32_t iterations, keep, band, fill_weight;
} hsk_fill_params;        /* 16 bytes */
typedef struct hsk_fill_stats {
  uint64_t n_unseen;            /* non-source voxels of the box before the call                                                */
  uint64_t n_reached;           /* FILLED after the last iteration                                                             */
  uint64_t n_written;           /* written to the volume                                                                       */
  uint64_t n_written_negative;  /* ... with a value < 0                                                                        */
  uint64_t tile_visits;         /* 16 x 16 x 8 tiles worked on, summed over the iterations: implementation-defined, reported,
                                   never compared                                                                              */
  int32_t iterations_run, pad;
} hsk_fill_stats;         /* 48 bytes */
/* iterations = clamp(ceil(0.15 / the smallest cell), 1, 255) in binary64 from the context's binary32 cells (k NULL:
 * hsk_default_config(256)'s) -- gaps up to about 30 cm across close; a stated choice, not a measurement --, keep =
 * HSK_FILL_SURFACE, band = 2, fill_weight = 1 */
void hsk_default_fill_params(const hsk_ctx* k, hsk_fill_params* p);
/* Fills the box (NULL: the whole volume) by the rule above (params NULL: the defaults).  stats may be NULL. */
int hsk_fill_holes(hsk_ctx* k, const hsk_fill_params* params, const hsk_voxel_box* box, hsk_fill_stats* stats);
/* One byte per voxel of the box (NULL: the whole volume), row-major, x fastest: 1, the last hsk_fill_holes wrote this voxel; 0, it
 * did not -- what lets a caller paint filled surface differently or put the words back.  Valid while the volume is as that fill
 * left it (a fill that wrote nothing holds an all-zero mask); otherwise HSK_ERR_STATE "hsk_download_fill_mask: no fill is held for
 * the volume as it stands". */
int hsk_download_fill_mask(hsk_ctx* k, const hsk_voxel_box* box, uint8_t* mask);

/* ---- Volume differencing: what changed between two scans of the same place, and the call that adopts it (DESIGN.md 3.23 the
 * kernels, 8q the rule; tests/diff_twin.py restates the rule in numpy).  hsk_fuse_volume merges two sessions by a weighted mean:
 * a chair that was moved becomes two half-weight ghosts.  hsk_diff_volume says where the scene changed; hsk_adopt_diff takes the
 * newer scan's words there, so that a following hsk_fuse_volume merges without ghosts.  All integers.
 * INPUTS.  `ref` is the older scan -- the result lives in it, on its grid --, `cur` the newer one.  Both are whole volumes on the
 * SAME GRID: equal dims, size_m bit-equal, effective truncation distance bit-equal, same device.  A cur in another frame or at
 * another resolution is resampled first: create an empty context with ref's configuration and hsk_fuse_volume(empty, cur,
 * cur_to_ref) -- into an empty destination the fusion rule gives exactly the sampled word; this rule samples nothing.  Both
 * contexts' deferred free-space weights are written back first, as hsk_fuse_volume does.
 * PER VOXEL (z < vol_z), with the words (raw_a, W_a) of ref and (raw_b, W_b) of cur: r = max(raw, -32767) -- a raw of -32768
 * counts as -32767; the word is never rewritten --; a voxel is observed in a volume iff W >= min_weight; d = r_b - r_a:
 *   HSK_DIFF_UNSEEN    observed in neither            HSK_DIFF_ONLY_REF  in ref only          HSK_DIFF_ONLY_CUR  in cur only
 *   HSK_DIFF_SAME      in both, -thresh < d < thresh
 *   HSK_DIFF_APPEARED  in both, d <= -thresh (matter came nearer: something is there now)
 *   HSK_DIFF_VANISHED  in both, d >= thresh
 *   HSK_DIFF_MINOR     APPEARED or VANISHED, but in a region below min_voxels
 * REGIONS.  CHANGED = APPEARED + VANISHED, before the MINOR step.  Two CHANGED voxels are adjacent when they differ by 1 on
 * exactly one axis (the components' 6-neighbourhood); a region is a connected component of CHANGED whatever the mix of its two
 * classes -- a thing pushed 10 cm is one region with both counts --, its label the smallest lin(x, y, z) = (z vol_y + y) vol_x + x
 * among its voxels.  A region with n_voxels >= min_voxels is KEPT; every voxel of any other region gets the class MINOR.  Records
 * exist for kept regions only, ordered by n_voxels descending, ties to the smaller root.  More than HSK_COMPONENT_MAX regions in
 * all: HSK_ERR_ARG, nothing held.
 * DEFAULTS: thresh = 16384, half the truncation distance; min_weight = 1; min_voxels = hsk_default_prune_params' value, the
 * voxels of a cube of edge 4 tau.  Stated choices, not measurements -- set other values where they do not fit.  Ranges: thresh
 * 1..65534, min_weight 1..128, min_voxels >= 1.
 * KNOWN PROPERTY: the TSDF's slope is one tau per tau, so a residual misalignment of delta along a surface normal moves the values
 * by delta / tau.  At the default thresh a static wall stays SAME up to delta < tau / 2 (with tau = 2.1 cells: shifts of 0.5, 1.0
 * and 1.04 cells give no CHANGED voxel, 1.1 cells flood the wall); beyond that the whole wall becomes one large region.  The
 * remedy is a better matrix (hsk_align_volume) or a larger thresh.
 * ADOPT.  T = the voxels of kept regions whose class `which` selects (a mask of HSK_ADOPT_APPEARED and HSK_ADOPT_VANISHED; the
 * default is both).  The adopt set S = every voxel with W_b != 0 within Chebyshev distance `halo` (0..8, default 2: the cells of
 * the crossing and the neighbours a normal's central difference reads; clipped at the grid) of a voxel of T.  Every voxel of S
 * gets cur's word as it is, raw and weight; when both contexts have colour also cur's colour word; when only ref has colour the
 * colour word 0 (prune's convention).  Every other word of ref, every other colour word and all of cur stay bit for bit.  When S
 * is empty nothing is written and cached passes stay valid; otherwise the write follows hsk_prune_components' order and the held
 * diff is no longer valid.  The pose and the model maps are not touched.
 * KNOWN PROPERTY: the inside of a vanished object, which ref never observed, stays never-observed beyond the halo.  A following
 * hsk_fuse_volume(ref, cur) takes it from cur (where the destination's weight is 0 the fusion rule is a copy), or hsk_fill_holes
 * closes it.  With halo >= 1 ref's zero crossings become cur's and ref equals cur on every voxel both observe; with halo = 0
 * neither holds (the voxels next to a region keep ref's values), though differencing again finds no CHANGED voxel either way.
 * VALIDITY.  The diff is held in ref for (ref's volume, cur's identity, cur's volume).  hsk_download_diff and hsk_diff_at need
 * ref unchanged since, hsk_adopt_diff both unchanged and cur to be the context the diff was made with; otherwise HSK_ERR_STATE
 * "<call>: no diff is held for the volume as it stands" (for the volumes as they stand).
 * The scratch -- 2.5 times the volume's bytes: the class words, a labelling of its own (never hsk_label_components', whose
 * labels_reused keeps its meaning) and two byte volumes for the adopt set -- is made by the first call that diffs, NOT by
 * hsk_prepare_readout (which only loads the kernels), and freed by hsk_release_diff or hsk_destroy.
 * hsk_download_diff and hsk_diff_at work through the grow-only product buffer of the read-outs: a whole-volume download with
 * labels grows it to 5 bytes a voxel (671 MB at 512^3), which stays allocated beside the scratch until hsk_destroy.
 * HSK_ERR_ARG: a NULL argument, ref == cur, unequal grids or truncation distances ("... resample cur first: hsk_fuse_volume into
 * an empty context of ref's configuration"), another device, more than 2^31 voxels, a parameter out of range.  HSK_ERR_STATE:
 * frames in flight in either context, a slab of a group or a context that stores part of its volume, no valid diff held.  A
 * refused call writes nothing. */
#define HSK_DIFF_UNSEEN 0
#define HSK_DIFF_ONLY_REF 1
#define HSK_DIFF_ONLY_CUR 2
#define HSK_DIFF_SAME 3
#define HSK_DIFF_APPEARED 4
#define HSK_DIFF_VANISHED 5
#define HSK_DIFF_MINOR 6
#define HSK_ADOPT_APPEARED 1
#define HSK_ADOPT_VANISHED 2
typedef struct hsk_diff_params {
  int32_t thresh, min_weight;
  uint64_t min_voxels;
} hsk_diff_params;        /* 16 bytes */
typedef struct hsk_diff_region {
  int32_t root[3], pad;   /* x, y, z of the root                                                                                */
  uint64_t n_voxels, n_appeared, n_vanished;
  int32_t lo[3], hi[3];   /* the voxel bounding box, hi exclusive                                                               */
} hsk_diff_region;        /* 64 bytes */
typedef struct hsk_diff_stats {
  uint64_t n_class[7];    /* the voxels by final class: APPEARED and VANISHED of kept regions only, the others' under MINOR     */
  uint64_t n_regions;     /* kept                                                                                               */
  uint64_t n_minor_regions, largest;   /* the regions below min_voxels; the voxels of the first record                         */
} hsk_diff_stats;         /* 80 bytes */
typedef struct hsk_adopt_params {
  int32_t which, halo;
} hsk_adopt_params;       /* 8 bytes */
typedef struct hsk_adopt_stats {
  uint64_t n_targets;     /* |T|                                                                                                */
  uint64_t n_adopted;     /* |S|                                                                                                */
  uint64_t n_colored;     /* the voxels of S that got cur's colour word (both contexts have colour; else 0)                    */
} hsk_adopt_stats;        /* 24 bytes */
/* the defaults described above for the context's cells and truncation distance; k NULL: hsk_default_config(256)'s */
void hsk_default_diff_params(const hsk_ctx* k, hsk_diff_params* p);
/* Diffs cur against ref (params NULL: the defaults), holds the result in ref and gives the records in their order.  recs NULL: the
 * counts only (*n_regions, stats).  HSK_ERR_ARG with *n_regions and stats set and no record written: cap below the count (the
 * diff is held all the same).  stats may be NULL.  While both volumes stand, a further call with the same cur and the same
 * parameters launches nothing and gives the held records and stats: the size query followed by the fill diffs once. */
int hsk_diff_volume(hsk_ctx* ref, hsk_ctx* cur, const hsk_diff_params* params, hsk_diff_region* recs, size_t cap, size_t* n_regions,
                    hsk_diff_stats* stats);
/* The voxels of the box (NULL: the whole volume), row-major, x fastest: cls = one HSK_DIFF_* byte each; region (may be NULL) =
 * the region's root lin for APPEARED and VANISHED voxels, HSK_COMPONENT_NONE elsewhere, MINOR included.  HSK_ERR_ARG: lo < 0,
 * hi > the volume's dims or hi < lo on an axis.  An empty box writes nothing. */
int hsk_download_diff(hsk_ctx* ref, const hsk_voxel_box* box, uint8_t* cls, uint32_t* region);
/* The diff at n <= 2^20 world points (x, y, z triples) -- what tints a cloud or a mesh: a surface point of a new object lies
 * inside its APPEARED shell.  A point's voxel is found as hsk_clearance_at finds it; a point outside the grid gives
 * HSK_DIFF_UNSEEN and HSK_COMPONENT_NONE.  Candidates are the voxels within Chebyshev `radius` (0..4) of that voxel whose class
 * is APPEARED or VANISHED; the result is the candidate with the smallest (dx^2 + dy^2 + dz^2, lin), its class and its region;
 * with no candidate the own voxel's class and HSK_COMPONENT_NONE.  region may be NULL. */
int hsk_diff_at(hsk_ctx* ref, const float* xyz, size_t n, int radius, uint8_t* cls, uint32_t* region);
/* Adopts cur's words by the rule above (params NULL: which = both, halo = 2).  stats may be NULL.  HSK_ERR_ARG: which outside
 * 1..3, halo outside 0..8. */
int hsk_adopt_diff(hsk_ctx* ref, hsk_ctx* cur, const hsk_adopt_params* params, hsk_adopt_stats* stats);
/* frees the held diff and its scratch (the next hsk_diff_volume makes it again); HSK_ERR_ARG: a NULL context */
int hsk_release_diff(hsk_ctx* ref);

/* ---- Scene split: structure, objects, and the room without them (DESIGN.md 3.24 the kernels, 8r the rule; tests/split_twin.py
 * restates the rule in numpy).  Every product of the building -- planes, the cuboid, floor plans, clearance, reach, rooms -- is
 * bent by the furniture in the scan.  hsk_split_scene says which INSIDE voxels belong to given planes (the structure) and groups
 * the others into objects; hsk_remove_objects takes objects out and rewrites what they hid from the planes they touched.  All
 * device arithmetic is in integers or in the fixed binary64 products named below: the same bits whatever the launch shape.
 * PLANES.  n_planes in 0..64 of hsk_split_plane: abcd as hsk_plane_record's (the normal points into the room), kind one of
 * HSK_KIND_*.  HSK_ERR_ARG: a number not finite, a normal's length outside [0.5, 2], |d| > 64, an unknown kind.  The host converts
 * once, in binary64 from the binary32 inputs, with rint; c_j are the context's binary32 cells, tau its effective truncation
 * distance, c_min the smallest cell:  Q_j = rint(a_j c_j 2^29), Q_d = rint(d 2^30), N_j = rint(a_j 4096), front = rint(dist_m 2^30),
 * back = rint(back_m 2^30), tauq = rint(tau 2^30), w_j = rint(4096 c_min / c_j).  The signed distance of voxel (x, y, z) -- its
 * centre lies at (index + 1/2) cell -- to plane k, in units of 2^-30 m, int64:
 *   s_k = Q_x (2 x + 1) + Q_y (2 y + 1) + Q_z (2 z + 1) + Q_d
 * VOXELS (the whole grid, z < vol_z).  INSIDE: weight != 0 and raw < 0 (the components' rule).  Values r = max(raw, -32767); a voxel
 * is observed iff its weight != 0.  A voxel that is not INSIDE has the class HSK_SPLIT_NONE.
 * GRADIENT of an INSIDE voxel, per axis j, from its two neighbours on that axis (outside the grid counts as unobserved): both
 * observed g_j = r(+1) - r(-1); only +1 observed g_j = 2 (r(+1) - r(0)); only -1 observed g_j = 2 (r(0) - r(-1)); neither 0.
 * G_j = g_j w_j, int64.
 * AGAINST PLANE k.  NEAR: -back <= s_k <= front.  ALIGNED: G = 0, or dot = sum G_j N_kj > 0 and (double)dot (double)dot >=
 * cos2 ((double)|G|^2 (double)|N_k|^2), cos2 = (double)cos_min (double)cos_min; |G|^2 and |N_k|^2 are int64 sums, converted once;
 * every product is binary64 with no contraction.
 * CLASS.  m = the planes NEAR, q = the planes NEAR and ALIGNED.  q >= 1: the voxel's plane is the one of least (|s_k|, k) among
 * those q, its class that plane's kind.  q = 0 and m >= 2: the same among the m planes -- the EDGE RULE: at a floor-wall or
 * wall-wall edge the gradient is diagonal and agrees with neither plane; without the rule every room edge is a strip of OBJECT
 * that chains the furniture together.  Otherwise the class is HSK_SPLIT_OBJECT and the plane 0xff.
 * OBJECTS: the 6-connected components of the OBJECT voxels, labelled by their smallest lin = (z vol_y + y) vol_x + x.  An object
 * with n_voxels >= min_voxels is KEPT; every voxel of any other object gets the class HSK_SPLIT_MINOR.  Records exist for kept
 * objects only, ordered by n_voxels descending, ties to the smaller root.  More than HSK_COMPONENT_MAX objects in all:
 * HSK_ERR_ARG, nothing held.
 * DEFAULTS (stated choices, not measurements): dist_m = 0.04, back_m = tau + 0.04, cos_min = cos 30 deg, min_voxels =
 * hsk_default_prune_params' value.  Ranges: dist_m in (0, 1], back_m in (0, 2], cos_min in [0, 1], min_voxels >= 1.
 * VALIDITY.  The split is held in the context for (its volume, the planes' bytes, the parameters' bytes): the same call again
 * launches nothing (stats.reused = 1), so a size query followed by the fill splits once.  hsk_download_split, hsk_split_at and
 * hsk_remove_objects need the volume unchanged since; otherwise HSK_ERR_STATE "<call>: no split is held for the volume as it
 * stands".  The scratch -- 2.5 times the volume's bytes: the class words, a labelling of its own (never hsk_label_components')
 * and two byte volumes -- is made by the first call that splits, NOT by hsk_prepare_readout (which only loads the kernels), and
 * freed by hsk_release_split or hsk_destroy.
 * REMOVAL.  roots: the labels of up to 256 kept objects (a label named twice counts once); NULL: all kept (more than 256 kept:
 * HSK_ERR_ARG).  T = the voxels of the selected objects; H = the voxels within Chebyshev `halo` of T; B_o = object o's box grown
 * by halo and clipped; A(v) = the OR of plane_mask(o) over the selected o with v in B_o.  Per voxel v, in this order:
 *   1. mode = HSK_REMOVE_RESTORE, A(v) != 0, v in some B_o, and (v in H or weight(v) = 0): the word becomes P(v): s = the least
 *      s_k(v) over k in A(v); s < -tauq: word 0; else sc = min(s, tauq), raw = floor((65534 sc + tauq) / (2 tauq)) in int64, the
 *      word (fill_weight << 16) | (raw & 0xffff) -- what an ideal scan of those planes would hold.  Every voxel of H is
 *      rewritten, structure included.
 *   2. otherwise, v in T, or v in H and observed and not INSIDE: word 0.
 *   3. otherwise unchanged.
 * A written voxel (rule 1 or 2) gets the colour word 0; every other word and colour word stays bit for bit.  When no voxel would
 * be written nothing is, and cached passes stay valid; otherwise the write follows hsk_prune_components' order (deferred weights
 * written back, the volume's epoch counted up) and the held split is no longer valid.  The pose and the model maps are not
 * touched.  Defaults: HSK_REMOVE_RESTORE, halo = clamp(ceil(tau / c_min) + 1, 1, 8), fill_weight = 1.
 * KNOWN PROPERTIES: the unobserved interior and shadow inside a removed object's grown box become the empty room, including space
 * nobody saw.  An object without contact (plane_mask = 0) is simply erased.
 * HSK_ERR_ARG: a NULL argument, more than 2^31 voxels, a parameter out of range, a root that is no kept object's label.
 * HSK_ERR_STATE: frames in flight, a slab of a group or a context that stores part of its volume, no valid split held.  A refused
 * call writes nothing. */
#define HSK_SPLIT_NONE 0
#define HSK_SPLIT_FLOOR 1
#define HSK_SPLIT_CEILING 2
#define HSK_SPLIT_WALL 3
#define HSK_SPLIT_OTHER 4
#define HSK_SPLIT_OBJECT 5
#define HSK_SPLIT_MINOR 6
#define HSK_KIND_FLOOR 1
#define HSK_KIND_CEILING 2
#define HSK_KIND_WALL 3
#define HSK_KIND_OTHER 4
#define HSK_REMOVE_ERASE 0
#define HSK_REMOVE_RESTORE 1
#define HSK_SPLIT_MAX_PLANES 64
#define HSK_REMOVE_MAX_OBJECTS 256
typedef struct hsk_split_plane {
  float abcd[4];
  int32_t kind, pad;
} hsk_split_plane;        /* 24 bytes */
typedef struct hsk_split_params {
  float dist_m, back_m, cos_min;
  int32_t pad;
  uint64_t min_voxels;
} hsk_split_params;       /* 24 bytes */
typedef struct hsk_object {
  int32_t root[3], pad;   /* x, y, z of the root                                                                                */
  uint64_t n_voxels;
  uint64_t sum[3];        /* the sums of the voxels' x, y, z (centroid = sum / n_voxels + 1/2, in cells)                        */
  int32_t lo[3], hi[3];   /* the voxel bounding box, hi exclusive                                                               */
  uint32_t contact[4];    /* [kind - 1]: the object's voxels with at least one 6-neighbour of class FLOOR, CEILING, WALL, OTHER */
  uint64_t plane_mask;    /* bit k: some voxel of the object has a 6-neighbour whose plane is k                                 */
  int32_t height_lo, height_hi; /* the least and the largest s_f >> 14 (arithmetic; units of 2^-16 m) over the object's voxels,
                             f the first plane of kind FLOOR in the list; both 0 when there is none                             */
} hsk_object;             /* 104 bytes */
typedef struct hsk_split_stats {
  uint64_t n_class[7];    /* the voxels by final class                                                                          */
  uint64_t n_objects;     /* kept                                                                                               */
  uint64_t n_minor_objects, largest;   /* the objects below min_voxels; the voxels of the first record                         */
  uint64_t n_edge;        /* voxels classed by the edge rule                                                                    */
  uint64_t n_no_normal;   /* INSIDE voxels with G = 0                                                                           */
  uint32_t reused, pad;   /* 1: answered from the held split                                                                    */
} hsk_split_stats;        /* 104 bytes */
typedef struct hsk_remove_params {
  int32_t mode, halo, fill_weight;   /* HSK_REMOVE_*; 0..8; 1..128 */
} hsk_remove_params;      /* 12 bytes */
typedef struct hsk_remove_stats {
  uint64_t n_objects;     /* selected                                                                                           */
  uint64_t n_targets;     /* |T|                                                                                                */
  uint64_t n_written;     /* the voxels rule 1 or 2 applies to                                                                  */
  uint64_t n_restored;    /* of them, those whose new word is not 0                                                             */
  uint64_t n_colored;     /* the colour words set to 0 (n_written with colour enabled, else 0)                                  */
} hsk_remove_stats;       /* 40 bytes */
/* the defaults described above for the context's cells and truncation distance; k NULL: hsk_default_config(256)'s */
void hsk_default_split_params(const hsk_ctx* k, hsk_split_params* p);
void hsk_default_remove_params(const hsk_ctx* k, hsk_remove_params* p);
/* host only, binary64: planes[i].kind from the normal and the up direction: t = n . u / (|n| |u|); FLOOR iff t >= level_cos,
 * CEILING iff t <= -level_cos, WALL iff |t| <= wall_sin, else OTHER.  up is minus row 1 of hsk_upright.level.  The defaults
 * are cos 15 deg and sin 15 deg.  HSK_ERR_ARG: a NULL pointer (n > 0), a number not finite, a zero normal or up, a threshold
 * outside [0, 1]. */
int hsk_split_plane_kinds(hsk_split_plane* planes, size_t n, const float up[3], float level_cos, float wall_sin);
/* Classifies, labels and tabulates (params NULL: the defaults), holds the result in the context and gives the kept objects'
 * records in their order.  recs NULL: the counts only (*n_objects, stats).  HSK_ERR_ARG with *n_objects and stats set and no
 * record written: cap below the count (the split is held all the same).  stats may be NULL. */
int hsk_split_scene(hsk_ctx* k, const hsk_split_plane* planes, size_t n_planes, const hsk_split_params* params, hsk_object* recs, size_t cap,
                    size_t* n_objects, hsk_split_stats* stats);
/* The voxels of the box (NULL: the whole volume), row-major, x fastest: cls = one HSK_SPLIT_* byte each; plane (may be NULL) = the
 * plane's index for the four structure classes, 0xff elsewhere; object (may be NULL) = the object's root lin for OBJECT voxels,
 * HSK_COMPONENT_NONE elsewhere, MINOR included.  An empty box writes nothing. */
int hsk_download_split(hsk_ctx* k, const hsk_voxel_box* box, uint8_t* cls, uint8_t* plane, uint32_t* object);
/* The split at n <= 2^20 world points (x, y, z triples) -- what tints a cloud or a mesh by class.  A point's voxel is found as
 * hsk_clearance_at finds it.  Candidates are the voxels within Chebyshev `radius` (0..4) of that voxel whose class is not NONE;
 * the result is the candidate with the smallest (dx^2 + dy^2 + dz^2, lin): its class, plane and object; with no candidate, or
 * outside the grid, HSK_SPLIT_NONE, 0xff and HSK_COMPONENT_NONE.  plane and object may be NULL. */
int hsk_split_at(hsk_ctx* k, const float* xyz, size_t n, int radius, uint8_t* cls, uint8_t* plane, uint32_t* object);
/* Removes objects by the rule above (params NULL: the defaults).  stats may be NULL. */
int hsk_remove_objects(hsk_ctx* k, const uint32_t* roots, size_t n, const hsk_remove_params* params, hsk_remove_stats* stats);
/* frees the held split and its scratch (the next hsk_split_scene makes it again); HSK_ERR_ARG: a NULL context */
int hsk_release_split(hsk_ctx* k);

/* ---- Clearance field: how much room there is -- the exact distance from every voxel to the nearest obstacle, on the device
 * (DESIGN.md 3.18 the kernels, 8l the rule; tests/clearance_twin.py restates the rule in numpy).  All integers.  A voxel is an
 * OBSTACLE when it is the coverage rule's SOLID (observed with a TSDF <= 0); with the flag HSK_CLEAR_UNKNOWN so is every UNSEEN
 * voxel (weight 0) and everything outside the grid.  The field's value at voxel v is
 *     D(v) = min over obstacles o of  weight[0] dx^2 + weight[1] dy^2 + weight[2] dz^2      (dx, dy, dz: voxel index differences)
 * and with HSK_CLEAR_UNKNOWN also over the three border terms weight[k] min(v_k + 1, dim_k - v_k)^2; an obstacle has D = 0; a
 * D above max_d2, or no obstacle at all, is reported as HSK_CLEARANCE_FAR.  Metres are sqrt(D) * unit_m; the device never reads
 * unit_m.  The per-axis reach floor(sqrt(max_d2 / weight[k])) (binary64) must not exceed HSK_CLEAR_MAX_REACH = 255 voxels: a
 * stated choice that bounds every loop of the kernels and keeps every sum below 2^27.
 * The default weights make the metric that of the cells: (1, 1, 1) with unit_m = the cell when the three cells are bit-equal,
 * else weight[k] = rint(16 (cell_k / cell_min)^2) (binary64; at most 1024) with unit_m = cell_min / 4.  The rounding of a weight
 * bends the metric along its axis by at most 1/32 of the weight (a relative error of at most 1/64 in a distance along that axis,
 * and less than that in any other direction).  max_d2 = min(ceil((1 / unit_m)^2), 255^2 min weight): one metre.
 * No flush of the deferred weights is needed (the rule asks of a weight only whether it is zero, of the TSDF its sign).  The
 * field stays on the device and is reused while the volume and the 20 device-relevant parameter bytes (all but unit_m) stand;
 * its scratch -- 2.5 times the volume's bytes: the uint32 field, one uint32 and one uint16 intermediate per voxel -- is made by
 * the first call that builds, NOT by hsk_prepare_readout, and freed by hsk_release_clearance or hsk_destroy.  Nothing the tracker
 * reads is written.  HSK_ERR_STATE: frames in flight, a slab of a group, or any context that stores part of its volume.
 * HSK_ERR_ARG: a NULL context or output, a weight outside 1..1024, a reach above 255, unknown flag bits, a volume of more than
 * 2^31 voxels, and what each call lists.  A refused call writes nothing. */
#define HSK_CLEAR_UNKNOWN 1u
#define HSK_CLEAR_MAX_REACH 255
#define HSK_CLEARANCE_FAR 0xffffffffu
#define HSK_CLEARANCE_OUTSIDE 0xfffffffeu
#define HSK_CLEAR_MAX_POINTS ((size_t)1 << 20)
typedef struct hsk_clearance_params {
  uint32_t weight[3];     /* 1..1024 each                                                                                       */
  uint32_t max_d2;        /* the largest value reported                                                                         */
  uint32_t flags;         /* 0 or HSK_CLEAR_UNKNOWN                                                                             */
  float unit_m;           /* metres = sqrt(d2) * unit_m; host side only                                                         */
} hsk_clearance_params;   /* 24 bytes */
typedef struct hsk_clearance_stats {
  uint64_t n_obstacle;    /* obstacle voxels (of the floor map: obstacle columns)                                               */
  uint64_t n_far;         /* voxels (columns) reported as HSK_CLEARANCE_FAR                                                     */
  uint64_t scratch_bytes; /* the device memory the field holds                                                                  */
  uint32_t max_d2_seen;   /* the largest value that is not HSK_CLEARANCE_FAR (0: none)                                          */
  int32_t reused;         /* 1: the field of an earlier call was still valid                                                    */
} hsk_clearance_stats;    /* 32 bytes */
/* the defaults described above for the context's cells; k NULL: hsk_default_config(256)'s */
void hsk_default_clearance_params(const hsk_ctx* k, hsk_clearance_params* p);
/* host only: the d2 of a distance in metres, ceil((metres / unit_m)^2) in binary64, saturating at 0xffffffff; 0 for metres <= 0;
 * 0xffffffff for a NULL p, a NaN, or a unit_m that is not finite and positive */
uint32_t hsk_clearance_d2(const hsk_clearance_params* p, float metres);
/* builds the field (or finds the one of an earlier call still valid; params NULL: the defaults); stats may be NULL */
int hsk_build_clearance(hsk_ctx* k, const hsk_clearance_params* params, hsk_clearance_stats* stats);
/* the voxels of the box (NULL: the whole volume), row-major, x fastest; builds first when no valid field is held.  HSK_ERR_ARG:
 * lo < 0, hi > the volume's dims or hi < lo on an axis.  An empty box writes nothing. */
int hsk_download_clearance(hsk_ctx* k, const hsk_clearance_params* params, const hsk_voxel_box* box, uint32_t* d2);
/* the field at the voxels of n <= 2^20 world points (x, y, z triples): the voxel is floor(p / cell), unclamped; a point outside
 * the grid, or with a NaN, gives HSK_CLEARANCE_OUTSIDE; builds first when no valid field is held */
int hsk_clearance_at(hsk_ctx* k, const hsk_clearance_params* params, const float* xyz, size_t n, uint32_t* d2);
/* The floor map: for the up axis `axis` (0 x, 1 y, 2 z) and its planes lo <= p < hi, a column is an obstacle when any voxel of
 * its band is; the map is the same transform in 2-D over the two remaining axes with their weights (border terms on those two
 * only), one uint32 per column, row-major, the lower-numbered remaining axis fastest.  An empty band (hi == lo) has no obstacle
 * columns.  Not cached (stats->reused = 0); stats may be NULL.  HSK_ERR_ARG: axis outside 0..2, lo < 0, hi > the axis, hi < lo. */
int hsk_clearance_floor(hsk_ctx* k, const hsk_clearance_params* params, int axis, int lo, int hi, uint32_t* map, hsk_clearance_stats* stats);
/* frees the field and its scratch (the next call that needs it builds again); HSK_ERR_ARG: a NULL context */
int hsk_release_clearance(hsk_ctx* k);
/* host only: hsk_rank_views' order, with the poses whose eye_state is not HSK_EYE_FREE, whose eye_d2 (hsk_clearance_at of the
 * camera centres) is below min_d2 or is HSK_CLEARANCE_OUTSIDE behind all others, in the same order among themselves;
 * HSK_CLEARANCE_FAR counts as clear */
int hsk_rank_views_clear(const hsk_view_score* s, const uint32_t* eye_d2, uint32_t min_d2, size_t n, uint32_t* order);

/* ---- Reach field: whether a place can be walked to, and how far the walk is -- a geodesic distance field over the scanned free
 * space, on the device (DESIGN.md 3.19 the kernels, 8m the rule; tests/reach_twin.py restates the rule in numpy).  All integers.
 * Let D be the clearance field above for the clearance parameters given.  A voxel is PASSABLE when D >= min_d2 (HSK_CLEARANCE_FAR
 * passes; 1 <= min_d2 <= max_d2, so an obstacle never is).  The MOVES are the 26 neighbours d in {-1, 0, 1}^3; a move between v
 * and v + d is allowed only when every voxel of the box the two span (2, 4 or 8) lies in the grid and is passable: no path slips
 * diagonally between two obstacles that touch by an edge or a corner.  A move COSTS c(d) = rint(16 sqrt(weight[0] dx^2 + weight[1]
 * dy^2 + weight[2] dz^2)) (binary64), so metres are G unit_m / 16.  The field's value G(v) is the least sum of costs over the
 * chains of allowed moves from any seed voxel to v: 0 at a passable seed; HSK_REACH_UNREACHED where no chain of at most max_cost
 * arrives; HSK_REACH_BLOCKED where v is not passable.  It is the least fixpoint of G(v) = min(G(v), G(u) + c) and does not depend on
 * the order of the work.
 * This is a 26-neighbour CHAMFER metric, not the Euclidean geodesic: across open space it overestimates a straight walk by up to
 * sqrt(1 + (sqrt2 - 1)^2 + (sqrt3 - sqrt2)^2) - 1 = 12.8 % (8.2 % in a plane), reached in the direction (1, sqrt2 - 1, sqrt3 -
 * sqrt2), and is exact along the 26 directions themselves up to the rounding of the costs.
 * SEEDS are up to 4096 world points, mapped to voxels as hsk_clearance_at maps its points; a seed outside the grid, with a NaN, or
 * on a voxel that is not passable is ignored (n_seeds_used counts the others, duplicates each).
 * The field stays on the device and is reused while the volume, the 20 device-relevant clearance bytes, min_d2, max_cost and the
 * seeds' voxels (those inside the grid, in the caller's order) stand.  Its scratch -- the uint32 field and four words per tile of
 * 32 x 8 x 8 voxels -- is made by the first build, NOT by hsk_prepare_readout, and freed by hsk_release_reach or hsk_destroy.
 * Nothing the tracker reads is written.  Errors as the clearance calls have them; HSK_ERR_ARG as well for more than 4096 seeds,
 * flags != 0, min_d2 outside 1..max_d2, max_cost above HSK_REACH_MAX_COST.  A refused call writes nothing.  The rounds of a build
 * are driven by the host and end when a round lowers nothing, or with HSK_ERR_STATE and no field kept after HSK_REACH_MAX_ROUNDS. */
#define HSK_REACH_UNREACHED 0xffffffffu
#define HSK_REACH_OUTSIDE 0xfffffffeu
#define HSK_REACH_BLOCKED 0xfffffffdu
#define HSK_REACH_MAX_COST 0xf0000000u
#define HSK_REACH_MAX_SEEDS 4096
#define HSK_REACH_MAX_ROUNDS 65536
typedef struct hsk_reach_params {
  uint32_t min_d2;        /* a voxel is passable when its clearance is at least this; 1..max_d2                                */
  uint32_t max_cost;      /* values above it are not propagated; at most HSK_REACH_MAX_COST                                    */
  uint32_t flags;         /* 0                                                                                                  */
  uint32_t pad;
} hsk_reach_params;       /* 16 bytes */
typedef struct hsk_reach_stats {
  uint64_t n_passable;    /* passable voxels (of the floor map: columns)                                                       */
  uint64_t n_reached;     /* voxels that hold a value                                                                          */
  uint64_t scratch_bytes; /* the device memory the field holds                                                                 */
  uint32_t max_cost_seen; /* the largest value (0: none)                                                                       */
  uint32_t n_rounds;      /* rounds of tile relaxations launched (0: reused, or no usable seed)                                */
  uint32_t n_seeds_used;  /* seeds on a passable voxel of the grid                                                             */
  int32_t reused;         /* 1: the field of an earlier call was still valid                                                   */
} hsk_reach_stats;        /* 40 bytes */
/* min_d2 = hsk_clearance_d2(cp, 0.3f) -- a person's half width, a stated choice -- clamped to cp's max_d2; max_cost =
 * HSK_REACH_MAX_COST.  cp NULL: the context's default clearance parameters */
void hsk_default_reach_params(const hsk_ctx* k, const hsk_clearance_params* cp, hsk_reach_params* p);
/* builds the clearance field (or reuses it), then the reach field (or finds the one of an earlier call still valid: reused = 1,
 * nothing launched); cp, params NULL: the defaults; stats may be NULL */
int hsk_build_reach(hsk_ctx* k, const hsk_clearance_params* cp, const hsk_reach_params* params, const float* seeds_xyz, size_t n_seeds,
                    hsk_reach_stats* stats);
/* The three reads of the field held.  HSK_ERR_STATE when none is valid for the volume as it stands: there are no seeds to build
 * from.  download: the voxels of the box (NULL: the whole volume), row-major, x fastest.  at: the field at the voxels of n <= 2^20
 * world points, HSK_REACH_OUTSIDE outside the grid or with a NaN. */
int hsk_download_reach(hsk_ctx* k, const hsk_voxel_box* box, uint32_t* g);
int hsk_reach_at(hsk_ctx* k, const float* xyz, size_t n, uint32_t* g);
/* The path to the voxel of goal_xyz, from the seed to the goal, x y z each: from the goal, step to v + d for the smallest move
 * index m = (dz + 1) 9 + (dy + 1) 3 + (dx + 1) whose move is allowed and has G(v + d) + c(d) == G(v), until G == 0.  A goal that
 * holds no value gives *n = 0 and HSK_OK.  cap (in voxels) too small: HSK_ERR_ARG with *n = the length needed, nothing written. */
int hsk_reach_path(hsk_ctx* k, const float goal_xyz[3], int32_t* voxels_xyz, size_t cap, size_t* n);
/* The floor form -- where a person can walk: the same rule, by the same kernels, on hsk_clearance_floor's map of the band
 * lo <= p < hi along `axis`: one plane deep, so only the 8 in-plane moves occur, with the weights of the two remaining axes; the
 * seeds are projected by dropping the up axis (that coordinate does not count).  map: one uint32 per column, the lower-numbered
 * remaining axis fastest.  Not cached. */
int hsk_reach_floor(hsk_ctx* k, const hsk_clearance_params* cp, int axis, int lo, int hi, const hsk_reach_params* params, const float* seeds_xyz,
                    size_t n_seeds, uint32_t* map, hsk_reach_stats* stats);
int hsk_release_reach(hsk_ctx* k);
/* of the last hsk_build_reach that built: the tiles relaxed over all its rounds, and the tiles of the grid (either may be NULL) */
int hsk_reach_tiles_relaxed(const hsk_ctx* k, uint64_t* tiles_relaxed, uint64_t* tiles);
/* host only: hsk_rank_views' order, with the poses whose eye_g (hsk_reach_at of the camera centres) is HSK_REACH_UNREACHED,
 * HSK_REACH_BLOCKED, HSK_REACH_OUTSIDE or above max_g behind all others, in the same order among themselves */
int hsk_rank_views_reach(const hsk_view_score* s, const uint32_t* eye_g, uint32_t max_g, size_t n, uint32_t* order);
/* host only: g unit_m / 16; NaN for the three markers */
float hsk_reach_metres(const hsk_clearance_params* p, uint32_t g);

/* ---- Room partition: where one room ends and the next begins -- the scanned free space split into rooms and doors, on the device
 * (DESIGN.md 3.20 the kernels, 8n the rule; tests/partition_twin.py restates the rule in numpy).  All integers.  Let D be the
 * clearance field for the clearance parameters given and lin(x, y, z) = (z Y + y) X + x.
 * CORES.  A voxel is a core voxel when D >= core_d2 (HSK_CLEARANCE_FAR passes).  The cores are the 6-connected components of the
 * core voxels; a core's label is the smallest lin among its voxels.  A core of fewer than min_core_voxels voxels is dropped: its
 * voxels are ordinary passable voxels.  At most HSK_PARTITION_MAX_ROOMS cores may be kept.
 * SPREADING.  A voxel is passable when D >= min_d2, 1 <= min_d2 <= core_d2 <= max_d2.  The moves, the box rule and the costs are
 * the reach field's.  A voxel's key is K(v) = (G, L): the lexicographically least (sum of costs, label of the core the chain
 * starts in) over the chains of allowed moves from any voxel of a kept core to v, chains above max_cost not propagated; a kept
 * core voxel holds (0, its label).  K is the least fixpoint of K(v) = min(K(v), K(u) + (c, 0)) and does not depend on the order
 * of the work; G alone is the reach field seeded at every kept core voxel.
 * ROOMS.  A room is the set of voxels that share an L.  The records are ordered by n_voxels descending, ties to the smaller root;
 * a room's id is its rank.  A passable voxel that no chain reaches reports HSK_ROOM_UNASSIGNED, a voxel that is not passable
 * HSK_ROOM_BLOCKED.
 * DOORS.  A face is a pair of 6-adjacent voxels that hold two different rooms a < b; there is one record per pair of rooms with a
 * face, ordered by (a, b).  A door's max_d2 -- the largest min(D(u), D(u')) over its faces -- is an UPPER estimate of the squared
 * half width of the passage.  The interface between two rooms is the geodesic bisector of their two cores: it lies in the
 * doorway only as far as the two cores are equally far from it.
 * The partition stays on the device and is reused while the volume, the 20 device-relevant clearance bytes and the partition
 * parameters stand.  Its scratch -- 12 bytes a voxel, four words per tile of 32 x 8 x 8 voxels, 64 bytes per pair of rooms -- is
 * made by the first build and freed by hsk_release_partition or hsk_destroy.  Nothing the tracker reads is written.  Errors as
 * the reach calls have them; HSK_ERR_ARG as well for flags != 0, thresholds out of order, more than 1024 kept cores, radius
 * outside 0..4, a cap too small.  A refused call writes nothing but what it lists. */
#define HSK_PARTITION_MAX_ROOMS 1024
#define HSK_PARTITION_MAX_RADIUS 4
#define HSK_ROOM_UNASSIGNED 0xffffffffu
#define HSK_ROOM_OUTSIDE 0xfffffffeu
#define HSK_ROOM_BLOCKED 0xfffffffdu
#define HSK_ROOM_NONE 0xfffffffcu
typedef struct hsk_partition_params {
  uint32_t core_d2;         /* a voxel is a core voxel when its clearance is at least this; min_d2..max_d2                       */
  uint32_t min_d2;          /* a voxel is passable when its clearance is at least this; 1..core_d2                               */
  uint32_t min_core_voxels; /* a core of fewer voxels is dropped                                                                  */
  uint32_t max_cost;        /* chains above it are not propagated; at most HSK_REACH_MAX_COST                                    */
  uint32_t flags;           /* 0                                                                                                  */
  uint32_t pad;
} hsk_partition_params;     /* 24 bytes */
typedef struct hsk_room {
  uint64_t n_voxels;        /* voxels (of the floor form: columns) that hold this room                                           */
  uint64_t n_core_voxels;   /* of them, voxels of its core (G == 0)                                                              */
  uint64_t sum[3];          /* sums of x, y, z over its voxels: the centroid is sum / n_voxels (+ 0.5, in voxels)                */
  uint32_t root[3];         /* the voxel whose lin is the room's label                                                           */
  uint32_t lo[3], hi[3];    /* its voxels' box, hi exclusive                                                                     */
  uint32_t max_d2;          /* the largest clearance in the room (HSK_CLEARANCE_FAR counts as the largest)                       */
  uint32_t max_g;           /* the largest G in the room                                                                         */
  uint32_t pad;
} hsk_room;                 /* 88 bytes */
typedef struct hsk_door {
  uint64_t sum2[3];         /* sums over the faces of twice the face centre, a voxel's centre being at its index: 2 u + e_axis   */
  uint32_t a, b;            /* the two rooms' ids, a < b                                                                         */
  uint32_t n_faces[3];      /* faces by the axis they cross                                                                      */
  uint32_t lo[3], hi[3];    /* the box of the faces' lower voxels, hi exclusive                                                  */
  uint32_t max_d2;          /* the largest min(D(u), D(u')) over the faces: an upper estimate of the squared half width          */
} hsk_door;                 /* 72 bytes */
typedef struct hsk_partition_stats {
  uint64_t n_cores;         /* cores before dropping                                                                             */
  uint64_t n_passable;      /* passable voxels (of the floor form: columns)                                                      */
  uint64_t n_assigned;      /* voxels that hold a room                                                                           */
  uint64_t scratch_bytes;   /* the device memory the partition holds                                                             */
  uint64_t n_dropped;       /* cores dropped for their size                                                                      */
  uint32_t n_rooms;         /* cores kept                                                                                        */
  uint32_t n_doors;
  uint32_t n_rounds;        /* rounds of tile relaxations launched (0: reused)                                                   */
  int32_t reused;           /* 1: the partition of an earlier call was still valid                                               */
} hsk_partition_stats;      /* 56 bytes */
/* core_d2 = hsk_clearance_d2(cp, 0.5f), clamped to cp's max_d2: wider than an interior door's half width, so anything narrower
 * than 1 m has no core of its own and joins a neighbour -- a stated choice, not a measurement; min_d2 = 1: every voxel that is no
 * obstacle gets a room; min_core_voxels = the voxels of a cube of edge 0.25 m (binary64, as hsk_default_prune_params computes its
 * cube); max_cost = HSK_REACH_MAX_COST.  cp NULL: the context's default clearance parameters */
void hsk_default_partition_params(const hsk_ctx* k, const hsk_clearance_params* cp, hsk_partition_params* p);
/* builds the clearance field (or reuses it), then the partition (or finds the one of an earlier call still valid: reused = 1,
 * nothing launched); cp, params NULL: the defaults; stats may be NULL.  recs NULL: counts only; else the records of all rooms in
 * their order, cap of them at least: a cap too small gives HSK_ERR_ARG with *n_rooms = the count needed and nothing else written
 * (the partition is held all the same).  More than HSK_PARTITION_MAX_ROOMS kept cores: HSK_ERR_ARG with the stats set (n_cores,
 * n_rooms = the kept cores, n_dropped; all else zero) and nothing held. */
int hsk_build_partition(hsk_ctx* k, const hsk_clearance_params* cp, const hsk_partition_params* params, hsk_room* recs, size_t cap, size_t* n_rooms,
                        hsk_partition_stats* stats);
/* The reads of the partition held.  HSK_ERR_STATE when none is valid for the volume as it stands.  doors: the records in their
 * order (doors NULL: the count only; a cap too small: HSK_ERR_ARG with *n_doors = the count needed).  download: the room ids of
 * the voxels of the box (NULL: the whole volume), row-major, x fastest; download_cost: their G, which is the reach field's value
 * with HSK_REACH_UNREACHED and HSK_REACH_BLOCKED.  at: the room of n <= 2^20 world points -- the voxel of a point as
 * hsk_clearance_at finds it; among the voxels within |dx|, |dy|, |dz| <= radius (0..4) of it that hold a room, the one that
 * minimises (weight[0] dx^2 + weight[1] dy^2 + weight[2] dz^2, lin); HSK_ROOM_OUTSIDE for a point outside the grid or with a NaN,
 * HSK_ROOM_NONE when there is no such voxel.  With a radius above 0 a surface point, which sits in an obstacle voxel, gets the room
 * whose air it borders. */
int hsk_partition_doors(hsk_ctx* k, hsk_door* doors, size_t cap, size_t* n_doors);
int hsk_download_partition(hsk_ctx* k, const hsk_voxel_box* box, uint32_t* ids);
int hsk_download_partition_cost(hsk_ctx* k, const hsk_voxel_box* box, uint32_t* g);
int hsk_partition_at(hsk_ctx* k, const float* xyz, size_t n, int radius, uint32_t* ids);
/* The floor form: the same rule, by the same kernels, on hsk_clearance_floor's map of the band lo <= p < hi along `axis`: one
 * plane deep, so the cores are 4-connected and only the 8 in-plane moves occur, with the weights of the two remaining axes.  map:
 * one room id per column, the lower-numbered remaining axis fastest (a record's x, y are the map's u, v; z is 0).  recs, doors:
 * as above, either may be NULL with its cap 0 (n_rooms, n_doors may then be NULL too); a cap too small: HSK_ERR_ARG with both
 * counts set and nothing else written.  Not cached. */
int hsk_partition_floor(hsk_ctx* k, const hsk_clearance_params* cp, int axis, int lo, int hi, const hsk_partition_params* params, uint32_t* map,
                        hsk_room* recs, size_t rec_cap, size_t* n_rooms, hsk_door* doors, size_t door_cap, size_t* n_doors, hsk_partition_stats* stats);
int hsk_release_partition(hsk_ctx* k);
/* of the last hsk_build_partition that built: the tiles relaxed over all its rounds, the tiles of the first worklist and the tiles
 * of the grid (any may be NULL) */
int hsk_partition_tiles_relaxed(const hsk_ctx* k, uint64_t* tiles_relaxed, uint64_t* first_tiles, uint64_t* tiles);
/* host only: the caller's remedy for a room that got two cores (an L-shaped one).  map[i], i < n_rooms: the smallest id of room
 * i's class under the union of all pairs (a, b) whose door has max_d2 >= merge_d2.  Touches nothing on the device.  HSK_ERR_ARG:
 * a NULL argument where one is needed, a door whose rooms are not below n_rooms */
int hsk_merge_rooms(const hsk_door* doors, size_t n_doors, size_t n_rooms, uint32_t merge_d2, uint32_t* map);

/* Multi-GPU (z-slab) building blocks; device pointers so that the host's collective (RCCL through
 * torch.distributed) can run on them without a host round trip.  All work is enqueued on hsk_stream(). */
int hsk_mgpu_frame_begin(hsk_ctx* k, const void* depth_dev, int w, int h); /* preprocess + (frame 0) transform */
/* optional: enqueue the copy + preprocessing of the NEXT frame on a second stream, under the current frame's work; the
 * next hsk_mgpu_frame_begin with the same pointer picks it up.  depth_dev: device memory or pinned host memory holding
 * a COMPLETE frame (host-synchronised: this call orders against no stream); its contents must not change until that
 * hsk_mgpu_frame_begin has been enqueued */
int hsk_mgpu_prefetch(hsk_ctx* k, const void* depth_dev, int w, int h);
/* frame_begin + icp_replicated + integrate + raycast_local in one call; everything after the preprocessing is replayed
 * from a hipGraph (config use_graph).  keys_dev: int32[h*w], the SAME buffer on every call */
int hsk_mgpu_frame_front(hsk_ctx* k, const void* depth_dev, int w, int h, void* keys_dev);
int hsk_mgpu_icp_accumulate(hsk_ctx* k, int level, int row0, int row1, void* sums27_dev /* double[27] */);
int hsk_mgpu_icp_update(hsk_ctx* k, const void* sums27_dev);                /* solve + pose update on device */
int hsk_mgpu_icp_replicated(hsk_ctx* k); /* the whole 19-iteration ICP on this rank's (composited) maps, fused kernels */
int hsk_mgpu_integrate(hsk_ctx* k);
int hsk_mgpu_raycast_local(hsk_ctx* k, void* keys_dev /* int32[h*w] */);    /* slab-local march */
int hsk_mgpu_raycast_resolve(hsk_ctx* k, const void* keys_min_dev, void* maps_bits_dev /* int32[6*h*w] */);
/* direct exchange (no collective): where this slab won the pixel (keys_min == its own key, a hit), the bit patterns of its
 * vertex / normal go straight into each of the n_dest (<= 16) composite buffers dest_bits[d] (int32[6*h*w], memory this
 * context's device can write: its own, a peer's with access enabled, or an IPC-mapped one); nothing is written elsewhere */
int hsk_mgpu_raycast_push(hsk_ctx* k, const void* keys_min_dev, void* const* dest_bits, int n_dest);
int hsk_mgpu_frame_end(hsk_ctx* k, const void* keys_min_dev, const void* maps_bits_dev, float pose_out[16], int* tracked);
int hsk_mgpu_frame_index(const hsk_ctx* k);
/* pipelined form of the frame end: queues the pose read-back instead of waiting; collect with hsk_wait_frame (in order,
 * at most HSK_MAX_IN_FLIGHT outstanding).  hsk_mgpu_restart_pending() == 1: the next frame (re)starts the scan and must
 * end with the synchronous hsk_mgpu_frame_end (frame 0, or a pipelined frame lost tracking). */
int hsk_mgpu_frame_end_async(hsk_ctx* k, const void* keys_min_dev, const void* maps_bits_dev);
int hsk_mgpu_restart_pending(const hsk_ctx* k);

/* ---- ONE volume sharded as z-slabs over several GPUs, behind one frame call (SURVEY.md 8(b) n_devices / device_ids,
 * 8(e); BASELINE.json configs[3]).  The host keeps feeding whole depth frames (HoniHelper.hs:20, the loop that would
 * replace Main.hs:1285-1290); slab s of n owns planes [s Z / n, (s + 1) Z / n) plus a redundantly integrated halo, and
 * the per-frame exchanges -- MIN of the raycast's step keys, SUM of the winning vertex / normal bit patterns, optionally
 * the 27 ICP sums of every iteration -- run inside the library: a kernel between slabs that share a device,
 * ncclAllReduce (RCCL over xGMI, loaded at run time) between devices.  Results are bit-identical to a single context.
 * A group is not re-entrant; it is driven from one host thread. */
typedef struct hsk_group hsk_group;
#define HSK_GROUP_FORCE_RCCL 1     /* run the collectives through RCCL even when the group has a single device / rank */
#define HSK_GROUP_ICP_ALLREDUCE 2  /* row-shard the ICP over the slabs and all-reduce its 27 sums every iteration
                                      (default: every slab runs the whole ICP on the composited maps, no collective) */
#define HSK_GROUP_DIRECT 4         /* the per-frame composites as a ONE-HOP exchange over peer-mapped memory instead of
                                      two all-reduces: every slab stores its step keys into a slot of every device's
                                      gather buffer, each device takes the MIN locally, the winner of a pixel stores its
                                      vertex / normal bits into every device's composite (24 B per won pixel and peer
                                      instead of a 7.4 MB all-reduce); stream wait / write-value operations on a shared
                                      flag page order the steps -- no RCCL, no spinning kernel.  Single process: peer
                                      access between the devices; rank form: hipIpc memory handles and a POSIX shared-
                                      memory page named after comm_id (one node).  Not with HSK_GROUP_ICP_ALLREDUCE. */
#define HSK_GROUP_PROFILE 8        /* HSK_GROUP_DIRECT: HIP events round the slab work and the exchange of every frame
                                      (hsk_group_exchange_ms) */
/* single process: slab s lives on device_ids[s] (a device may be named several times); the distinct devices form one
 * communicator.  c->device_id, own_z0, own_z1, halo and use_graph are set by the library. */
int hsk_group_create(const hsk_config* c, int n_slabs, const int* device_ids, int flags, hsk_group** out);
/* one process per GPU (c->device_id): rank r of `world` owns slab r.  comm_id: the 128 bytes hsk_group_unique_id() gave
 * ONE of the ranks, handed to all of them by the host's own means (ignored when world == 1) */
int hsk_group_unique_id(void* id128);
int hsk_group_create_rank(const hsk_config* c, int rank, int world, const void* comm_id, int flags, hsk_group** out);
void hsk_group_destroy(hsk_group* g);
const char* hsk_group_last_error(const hsk_group* g); /* g may be NULL: last create error */
int hsk_group_reset(hsk_group* g);
/* the tracker step of hsk_process_frame, on the sharded volume */
int hsk_group_process_frame(hsk_group* g, const uint16_t* depth, int w, int h, float pose_out[16], int* tracked);
/* pipelined form (as hsk_submit_frame / hsk_wait_frame): the frame and its collectives are enqueued, the pose collected
 * later, in order, at most HSK_MAX_IN_FLIGHT outstanding; the first frame of a (re)started scan completes at submission.
 * After a tracking loss the frames already in flight behind the lost one are dropped (tracked = 0); the submission
 * that follows restarts the scan, its result is handed out behind theirs.
 * A failure in the MIDDLE of a frame (some slabs or devices have taken it, others not) poisons the group: every later
 * call returns HSK_ERR_STATE until hsk_group_reset succeeds (single process) or the group is destroyed (several ranks,
 * RCCL or direct form: the peers may be left in a collective or waiting for a flag).  A peer rank that dies or hangs
 * shows as HSK_ERR_TIMEOUT from hsk_group_wait_frame on every other rank after HSK_FRAME_TIMEOUT_S seconds (environment
 * variable, default 20) -- which poisons the group.  Poisoning lets this rank's own queues drain (direct form: the
 * flags its streams wait for are raised from the host; RCCL form: ncclCommAbort), so hsk_group_destroy returns.
 * STATUS: groups of several slabs on ONE device -- RCCL form, direct form, and the direct form between 2, 3 and 8 OS
 * processes sharing the device -- are tested bit-exact against a single context; groups over more than one DEVICE
 * (ncclCommInitAll / ncclCommInitRank with world > 1, the direct form over xGMI peer mappings) have never run on
 * hardware -- no multi-GPU box was available (tests/test_gpu_multi_device.py runs all three forms when one is, and
 * `bench.py --gpus N` checks every form it times against a single context: "matches_single_gpu"). */
int hsk_group_submit_frame(hsk_group* g, const uint16_t* depth, int w, int h);
/* depth_dev[d]: the frame in the memory of the d-th distinct device of this process (creation order), complete and
 * valid until the frame has been waited for */
int hsk_group_submit_frame_dev(hsk_group* g, const void* const* depth_dev, int w, int h);
int hsk_group_wait_frame(hsk_group* g, float pose_out[16], int* tracked);
/* HSK_GROUP_PROFILE: summed over n_frames tracked frames, on this process's first device: the exchange (waits for the peers
 * included) and the slab's own work before it (ICP + integrate + slab-local raycast) */
int hsk_group_exchange_ms(hsk_group* g, double* sum_ms, double* front_sum_ms, unsigned long long* n_frames);
int hsk_group_n_slabs(const hsk_group* g);            /* slabs held by this process */
/* how many ranks / devices the group's exchange really spans: ncclCommCount of its communicator (RCCL forms), the ranks
 * attached to the shared flag page (direct form between processes), the distinct devices of a single-process group */
int hsk_group_ranks_seen(hsk_group* g, int* n_ranks);
hsk_ctx* hsk_group_slab(hsk_group* g, int i);         /* for hsk_download_map, hsk_extract_cloud, ... on one slab */
/* the planes this process owns, at their place in a full 2 * X * Y * Z array (other planes are left untouched) */
int hsk_group_download_tsdf(hsk_group* g, int16_t* full_tsdf_weight_pairs);

/* streams / profiling */
void* hsk_stream(hsk_ctx* k);                 /* hipStream_t the context launches on */
int hsk_set_stream(hsk_ctx* k, void* stream); /* adopt the caller's hipStream_t (e.g. torch's current stream) */
int hsk_synchronize(hsk_ctx* k);
#define HSK_STAGE_PRE 0
#define HSK_STAGE_ICP 1
#define HSK_STAGE_INTEGRATE 2
#define HSK_STAGE_RAYCAST 3
#define HSK_NSTAGES 4
int hsk_set_profiling(hsk_ctx* k, int on);    /* 1: record HIP events around each stage of process_frame; 2: also at every ICP level */
int hsk_stage_ms(hsk_ctx* k, double sum_ms[HSK_NSTAGES], uint64_t* n_frames, int reset);
/* while profiling at level 2: time of the ICP iterations of each pyramid level, summed over the same frames as hsk_stage_ms (read it
 * before resetting that); index = level, 0 = finest.  Divide by frames x icp_iters[level] for the time of an iteration. */
int hsk_icp_level_ms(hsk_ctx* k, double sum_ms[HSK_LEVELS]);
/* lane-blocks (4 x 1 x 4 voxels) the last integrate's classification pass could not settle and handed to its per-voxel
 * pass (a measure of the classification's slack: bench.py reports it beside V_upd); synchronises the context's stream */
/* host microseconds the pipelined submissions (hsk_submit_frame[_dev|_rgbd]) have spent so far, by phase: [0] the copy of a host frame
   into the pinned staging ring, [1] enqueueing the upload and the preprocessing on the second stream, [2] waiting for that
   preprocessing, [3] enqueueing the frame's main-stream chain; n_submissions: how many.  reset != 0: counted afresh from now. */
int hsk_submit_host_us(hsk_ctx* k, double sum_us[4], uint64_t* n_submissions, int reset);
int hsk_integrate_queue_entries(hsk_ctx* k, uint64_t* n_entries);
/* ... and the lane-blocks of the last integrate's LIGHT class: free space with holes in the depth image under it (each voxel is
   rewritten with F = 1 or left alone according to whether its pixel has depth); not counted by hsk_integrate_queue_entries */
int hsk_integrate_light_entries(hsk_ctx* k, uint64_t* n_entries);
/* the coarse level of the last integrate (one verdict per wave-chunk of 16 x 16 voxels x the pass-A chunk of planes):
 * counts[0] = chunks pass A had to classify lane-block by lane-block ("mixed"), [1] = chunks settled as a whole (outside the
 * frustum, wholly occluded, or wholly free space with the observation recorded in the chunk's byte), [2] = wholly free
 * chunks whose byte could not take it (pass A works them), [3] = chunks currently marked quiet; synchronises the stream */
int hsk_integrate_coarse_counts(hsk_ctx* k, uint64_t counts[4]);
int hsk_bilateral_tables(float ws[169], float wc[512]);
/* Exhaustive self-test, on the GPU itself, of the exact-arithmetic shortcuts the kernels use for the specification's
 * correctly rounded 1/x, sqrt(x) and a/n (hardware approximation + one fused correction step; hsk_dev.h): every binary32
 * value, every (a, n) pair of the domain.  counts: [0] 1/x values checked, [1] wrong, [2] wrong without the correction
 * (shows that the comparison bites), [3..5] the same for sqrt, [6] a/n pairs checked, [7] wrong.  About 0.3 s. */
int hsk_selftest_exact_ops(int device_id, uint64_t counts[8]);

/* Deterministic synthetic depth stream; host-only, no GPU needed. */
int hsk_synth_pose(int frame, float pose[16]);
int hsk_synth_render(const float pose[16], int w, int h, float fx, float fy, float cx, float cy, uint16_t* depth);
/* closed box rooms with furniture for the room-stitching configurations (BASELINE configs[0], [4]); variant 0..3 */
int hsk_synth_room_extents(int variant, float extents[6] /* x0 x1 y0 y1 z0 z1 */);
int hsk_synth_room_pose(int variant, int frame, int n_frames, float pose[16]); /* three turns from near the centre: level, up, down */
int hsk_synth_room_render(int variant, const float pose[16], int w, int h, float fx, float fy, float cx, float cy, uint16_t* depth);
/* The same scenes as a structured-light sensor returns them (housescan/HoniHelper.hs:20-36: a real takeDepthSnapshot frame
   has its invalid pixels in contiguous regions): no return from grazing rays (|n.d| < 0.15), a 3-5 px shadow band on the
   far side of every depth discontinuity, nothing beyond range_cut_m (<= 0: 3.5 m), nothing from absorbing furniture when
   `absorbing` is set, and sigma_mm x (z / 1 m)^2 of Gaussian noise keyed by (seed, pixel).  scene < 0: the open scene of
   hsk_synth_render; 0..3: closed room `scene`.  hole_fraction (may be NULL): the share of pixels without depth. */
int hsk_synth_render_sensor(int scene, const float pose[16], int w, int h, float fx, float fy, float cx, float cy, uint64_t seed,
                            float sigma_mm, float range_cut_m, int absorbing, uint16_t* depth, double* hole_fraction);
/* Synthetic colour for RGB-D tests: hsk_synth_color_at is a smooth colour of the world position (per channel
 * 128 + 100 sin(2 pi p_i / 1.2 m), rounded: 28..228), the same for every scene.  hsk_synth_render_rgb gives every pixel the
 * colour of the nearest hit the depth renders use, and (0, 0, 0) exactly where the clean depth render (hsk_synth_render,
 * hsk_synth_room_render) is 0.  scene < 0: the open scene; 0..3: closed room `scene`.  rgb: 3 * w * h bytes. */
int hsk_synth_color_at(int scene, const float p[3], uint8_t rgb[3]);
int hsk_synth_render_rgb(int scene, const float pose[16], int w, int h, float fx, float fy, float cx, float cy, uint8_t* rgb);

/* Products on the file seam (Main.hs:1740, :1320-1345): binary PCD with float32 x y z */
int hsk_write_pcd_xyz(const char* path, const float* xyz, size_t n_points);
/* binary little-endian .ply mesh (the file plyxform / pcl tools take, README.md:16-17): vertices welded by exact
 * coordinates, faces as uchar-count + int indices; zero-area triangles are dropped.  Returns counts when non-NULL. */
int hsk_write_ply_mesh(const char* path, const float* tri_xyz, size_t n_triangles, size_t* n_vertices_out, size_t* n_faces_out);
/* the same welding without a file: indices[3 * n_triangles] into vertices (cap_vertices x 3); degenerate triangles keep index triples with repeats */
int hsk_weld_triangles(const float* tri_xyz, size_t n_triangles, float* vertices, size_t cap_vertices, size_t* n_vertices, int32_t* indices);
/* binary little-endian PLY 1.0 of an indexed mesh (hsk_extract_mesh_indexed): element vertex with float x y z, then float nx ny
 * nz when normals != NULL, then uchar red green blue when rgb != NULL, interleaved per vertex without padding (NaN normal
 * components written as 0); element face with property list uchar int vertex_indices, 13 B per face, every face as given.
 * The property names are the ones Meshlab reads; whether plyxform carries the normals through is unverified.  An index
 * outside [0, n_vertices): HSK_ERR_ARG and no file; an I/O failure: HSK_ERR_STATE; an empty mesh is valid. */
int hsk_write_ply_indexed(const char* path, const float* vertices, const float* normals, const uint8_t* rgb, size_t n_vertices,
                          const int32_t* faces, size_t n_faces);
/* hsk_write_ply_indexed's file for a textured mesh (hsk_bake_texture): a "comment TextureFile <texture_file>" line names the
 * atlas, the vertices carry no colour, and every face record is followed by a uchar 6 and the face's six floats u0 v0 u1 v1 u2 v2
 * (property list uchar float texcoord, 38 B per face) -- the form Meshlab reads.  normals may be NULL.  HSK_ERR_ARG also for a
 * NULL or empty texture_file, one with a line break in it, or uv NULL with n_faces > 0. */
int hsk_write_ply_textured(const char* path, const float* vertices, const float* normals, size_t n_vertices, const int32_t* faces,
                           size_t n_faces, const float* uv /* 6 per face */, const char* texture_file);
/* 8-bit RGB PNG of a w x h image, rows top to bottom (hsk_bake_texture's rgb and normal_rgb as they are): IHDR, one IDAT, IEND.
 * The zlib stream holds stored (uncompressed) deflate blocks of up to 65535 bytes, so the file is 3 w h + h bytes and a little
 * more, and nothing but crc32 and adler32 is computed.  HSK_ERR_ARG: a NULL pointer, w or h <= 0, an image whose stream would
 * not fit one chunk (2^31 bytes); an I/O failure: HSK_ERR_STATE.  hsk_write_ppm writes the same pixels as a PPM. */
int hsk_write_png_rgb(const char* path, const uint8_t* rgb, int w, int h);
int hsk_voxel_downsample(const float* xyz, size_t n, float leaf_m, float* out, size_t cap, size_t* n_out);
/* the same leaves, xyz bit-identical to hsk_voxel_downsample's and in the same order, with the rounded mean colour and the
 * renormalised mean of the non-NaN normals of each leaf (NaN x 3 when it has none).  rgb / normals (inputs) may be NULL,
 * and the matching output is then not written. */
int hsk_voxel_downsample_attrs(const float* xyz, const uint8_t* rgb, const float* normals, size_t n, float leaf_m, float* out_xyz,
                               uint8_t* out_rgb, float* out_normals, size_t cap, size_t* n_out);
/* binary PCD v0.7, FIELDS x y z rgb normal_x normal_y normal_z curvature (SIZE 4, TYPE F, COUNT 1 each; 32 B per point):
 * rgb holds the bit pattern 0x00RRGGBB, curvature is 0, NaN normals are kept (normals may be NULL: NaN).  The form
 * HouseScan's loader falls back to for a coloured cloud (Main.hs:1325-1345); that pcd-loader's loadXyzRgbNormal accepts
 * exactly this layout is unverified here. */
int hsk_write_pcd_xyzrgbnormal(const char* path, const float* xyz, const uint8_t* rgb, const float* normals, size_t n);
/* Plane products loadRoom reads beside the cloud (Main.hs:1392-1404): planes.txt lines "a b c d" in PCL form
 * ax+by+cz+d=0 (planeEqsFromFile, Main.hs:1379-1389) and cloud_plane_hull<k>.pcd polygons (Main.hs:1395-1400).
 * Deterministic RANSAC + PCA refit; labels[i] = plane index of point i or -1. */
int hsk_detect_planes(const float* xyz, size_t n, float dist_thresh_m, float min_fraction, int max_planes, int iterations,
                      float* planes_abcd /* 4 * max_planes */, int* labels /* n, may be NULL */, int* n_planes);
int hsk_plane_hull(const float* xyz, size_t n, const int* labels, int plane, const float abcd[4], float* hull_xyz,
                   size_t cap, size_t* n_hull);
int hsk_write_planes_txt(const char* path, const float* planes_abcd, int n_planes);

/* Room placements coming back from HouseScan: row-major left-multiplicative 4x4, as the 4-line .xf file
 * (roomProjectionToXfFormat, Main.hs:2289-2302) or the one-line CSV (roomProjectionToString, Main.hs:2271-2284). */
int hsk_write_xf(const char* path, const float m[16]);
int hsk_read_xf(const char* path, float m[16]);              /* accepts both layouts */
int hsk_transform_cloud(const float* xyz, size_t n, const float m[16], float* out /* may alias xyz */);
/* normals by the rotation part of the same matrix (no translation, no renormalisation; hsk_transform_cloud's operation order
 * without the m[3] / m[7] / m[11] term; NaN stays NaN): a room's mesh moved by its .xf keeps correct normals */
int hsk_transform_normals(const float* n, size_t count, const float m[16], float* out /* may alias n */);

/* Recorded depth streams ("HSKD" raw container; frames in the layout of takeDepthSnapshot, HoniHelper.hs:20-36). */
typedef struct hsk_depth_stream hsk_depth_stream;
hsk_depth_stream* hsk_stream_create(const char* path, int w, int h, float fx, float fy, float cx, float cy);
hsk_depth_stream* hsk_stream_open(const char* path, int* w, int* h, int* n_frames, float intr[4]);
int hsk_stream_write(hsk_depth_stream* s, const uint16_t* depth);
int hsk_stream_read(hsk_depth_stream* s, int index, uint16_t* depth);
int hsk_stream_close(hsk_depth_stream* s);
int hsk_stream_info(const hsk_depth_stream* s, int* w, int* h, int* n_frames, float intr[4]);
/* The recorded-stream frame feed (BASELINE configs[2]: "scan from recorded stream"; the loop that replaces
 * Main.hs:1285-1290 around takeDepthSnapshot, HoniHelper.hs:20-36): frames [first, first + count) of `s` through the
 * tracker, pipelined -- frame i + 1 is read from the file and uploaded while frame i is on the GPU.  poses_out: 16 floats
 * per frame (row-major cam->world), tracked_out: one int per frame (either may be NULL).  The context must have no frame
 * in flight; results are exactly those of hsk_process_frame called with the same frames -- also behind a lost frame:
 * frame i + 1, in flight when frame i reports tracking lost, is dropped on the device, then read again and resubmitted
 * as the first frame of the restarted scan (as the reference-shaped host loop would feed it). */
int hsk_track_stream(hsk_ctx* k, hsk_depth_stream* s, int first, int count, float* poses_out, int* tracked_out);

#ifdef __cplusplus
}
#endif
#endif
