"""ctypes binding of libhskinfu.so (the C ABI declared in include/hskinfu.h).

The library is the product; there is NO fallback: if the shared object is missing the import fails loudly, and
`hsk_create` fails with HSK_ERR_NOGPU when no HIP device is present.
"""
import ctypes as C
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhskinfu.so")

HSK_LEVELS = 3
HSK_NSTAGES = 4
HSK_KEY_NONE = 0x7FFFFFFF


class HskConfig(C.Structure):
    """Mirror of `hsk_config` (include/hskinfu.h)."""

    _fields_ = [
        ("vol_x", C.c_int), ("vol_y", C.c_int), ("vol_z", C.c_int),
        ("vol_size_m", C.c_float * 3),
        ("trunc_dist_m", C.c_float),
        ("width", C.c_int), ("height", C.c_int),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("icp_iters", C.c_int * HSK_LEVELS),
        ("icp_dist_thresh_m", C.c_float),
        ("icp_angle_thresh_sin", C.c_float),
        ("integrate_move_thresh", C.c_float),
        ("init_pose", C.c_float * 16),
        ("device_id", C.c_int),
        ("own_z0", C.c_int), ("own_z1", C.c_int), ("halo", C.c_int),
        ("use_graph", C.c_int),
    ]


HSK_VIEW_LAMBERT, HSK_VIEW_NORMALS, HSK_VIEW_COLOR, HSK_VIEW_COLOR_LIT = 0, 1, 2, 3


class HskView(C.Structure):
    """Mirror of `hsk_view` (include/hskinfu.h)."""

    _fields_ = [
        ("width", C.c_int), ("height", C.c_int),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("pose", C.c_float * 16),
        ("follow", C.c_int),
        ("mode", C.c_int),
        ("light", C.c_float * 3),
        ("light_in_camera", C.c_int),
        ("background", C.c_uint8 * 3),
    ]


HSK_PROJ_PINHOLE, HSK_PROJ_ORTHO = 0, 1
HSK_MAX_CLIP = 4


class HskSection(C.Structure):
    """Mirror of `hsk_section` (include/hskinfu.h)."""

    _fields_ = [
        ("view", HskView),
        ("projection", C.c_int),
        ("light_directional", C.c_int),
        ("n_clip", C.c_int),
        ("clip", (C.c_float * 4) * HSK_MAX_CLIP),
        ("cut_rgb", C.c_uint8 * 3),
    ]


class HskFuseStats(C.Structure):
    """Mirror of `hsk_fuse_stats` (include/hskinfu.h)."""

    _fields_ = [
        ("n_fused", C.c_uint64), ("n_colored", C.c_uint64),
        ("chunks_total", C.c_uint64), ("chunks_swept", C.c_uint64),
        ("box", C.c_int32 * 6),
    ]


HSK_ALIGN_CONVERGED, HSK_ALIGN_MAX_ITERS, HSK_ALIGN_FEW, HSK_ALIGN_DEGENERATE, HSK_ALIGN_DIVERGED = 0, 1, 2, 3, 4
HSK_ALIGN_STATUS = ("converged", "max_iters", "few", "degenerate", "diverged")
HSK_ALIGN_MAX_ITERS_CAP = 64
HSK_ALIGN_DIRECT = -1


class HskAlignParams(C.Structure):
    """Mirror of `hsk_align_params` (include/hskinfu.h); a 0 in a field means its default."""

    _fields_ = [
        ("max_iters", C.c_int), ("probes", C.c_int),
        ("cos_gate", C.c_float),
        ("max_points", C.c_uint32), ("min_points", C.c_uint32),
        ("eps_rot", C.c_float), ("eps_trans_m", C.c_float), ("max_rot", C.c_float), ("max_shift_m", C.c_float),
    ]


class HskAlignStats(C.Structure):
    """Mirror of `hsk_align_stats` (include/hskinfu.h)."""

    _fields_ = [
        ("status", C.c_int), ("iterations", C.c_int),
        ("n_points", C.c_uint32), ("stride", C.c_uint32),
        ("n_used", C.c_uint32 * HSK_ALIGN_MAX_ITERS_CAP),
        ("rms_m", C.c_float * HSK_ALIGN_MAX_ITERS_CAP),
        ("x_last", C.c_float * 6),
        ("sums_last", C.c_double * 28),
    ]


HSK_LOSS_RESET, HSK_LOSS_HOLD = 0, 1
HSK_RELOC_FOUND, HSK_RELOC_NONE, HSK_RELOC_EMPTY = 0, 1, 2
HSK_RELOC_STATUS = ("found", "none", "empty")
HSK_RELOC_FINEST = -1
HSK_RELOC_MAX_REFINE = 16


class HskPoseScore(C.Structure):
    """Mirror of `hsk_pose_score` (include/hskinfu.h): 32 bytes."""

    _fields_ = [
        ("n_near", C.c_uint32), ("n_free", C.c_uint32), ("n_behind", C.c_uint32), ("n_unseen", C.c_uint32),
        ("n_outside", C.c_uint32), ("n_skipped", C.c_uint32),
        ("sum_abs", C.c_uint64),
    ]


class HskRelocParams(C.Structure):
    """Mirror of `hsk_reloc_params` (include/hskinfu.h); a 0 in a field means its default."""

    _fields_ = [
        ("level", C.c_int), ("n_refine", C.c_int),
        ("accept_fraction", C.c_float), ("accept_rms_m", C.c_float),
        ("align", HskAlignParams),
    ]


class HskRelocStats(C.Structure):
    """Mirror of `hsk_reloc_stats` (include/hskinfu.h)."""

    _fields_ = [
        ("status", C.c_int),
        ("n_valid", C.c_uint32), ("n_candidates", C.c_uint32),
        ("best", C.c_int32), ("n_refined", C.c_int32),
        ("candidate", C.c_int32 * HSK_RELOC_MAX_REFINE),
        ("score", HskPoseScore * HSK_RELOC_MAX_REFINE),
        ("align_status", C.c_int32 * HSK_RELOC_MAX_REFINE),
        ("iterations", C.c_int32 * HSK_RELOC_MAX_REFINE),
        ("n_used", C.c_uint32 * HSK_RELOC_MAX_REFINE),
        ("rms_m", C.c_float * HSK_RELOC_MAX_REFINE),
    ]


HSK_PLANE_MAX_POINTS, HSK_PLANE_MAX_PLANES, HSK_PLANE_MAX_HYPOTHESES, HSK_PLANE_MAX_REFITS = 1 << 24, 64, 4096, 8


class HskPlaneParams(C.Structure):
    """Mirror of `hsk_plane_params` (include/hskinfu.h): 32 bytes; every field is taken as it stands."""

    _fields_ = [
        ("dist_m", C.c_float), ("cos_min", C.c_float), ("min_fraction", C.c_float),
        ("max_planes", C.c_int32), ("n_hypotheses", C.c_int32), ("refits", C.c_int32),
        ("seed", C.c_uint64),
    ]


class HskPlaneRecord(C.Structure):
    """Mirror of `hsk_plane_record` (include/hskinfu.h): 32 bytes."""

    _fields_ = [
        ("abcd", C.c_float * 4),
        ("n_inliers", C.c_uint32), ("pad", C.c_uint32),
        ("sum_abs", C.c_uint64),
    ]


HSK_UPRIGHT_NO_YAW = 1
HSK_UPRIGHT_UP, HSK_UPRIGHT_YAW, HSK_UPRIGHT_FLOOR, HSK_UPRIGHT_CEILING = 1, 2, 4, 8
HSK_UPRIGHT_MAX_POINTS, HSK_UPRIGHT_MAX_REFITS, HSK_UPRIGHT_HIST_BINS, HSK_UPRIGHT_HEIGHT_BINS, HSK_UPRIGHT_AXIS_MAX2 = 1 << 24, 8, 1536, 16384, 16810000


class HskUprightParams(C.Structure):
    """Mirror of `hsk_upright_params` (include/hskinfu.h): 36 bytes; every field is taken as it stands."""

    _fields_ = [
        ("up_hint", C.c_float * 3), ("max_tilt_cos", C.c_float), ("cone_cos", C.c_float), ("wall_sin", C.c_float),
        ("min_fraction", C.c_float), ("refits", C.c_int32), ("flags", C.c_uint32),
    ]


class HskUpright(C.Structure):
    """Mirror of `hsk_upright` (include/hskinfu.h): 128 bytes."""

    _fields_ = [
        ("level", C.c_float * 16), ("floor_m", C.c_float), ("ceiling_m", C.c_float),
        ("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3),
        ("n_points", C.c_uint32), ("n_invalid", C.c_uint32), ("n_axis", C.c_uint32 * 3), ("n_walls", C.c_uint32),
        ("found", C.c_uint32), ("pad", C.c_uint32),
    ]


HSK_RAY_HIT, HSK_RAY_FRONTIER, HSK_RAY_OPEN, HSK_RAY_BLIND, HSK_RAY_OUTSIDE = 0, 1, 2, 3, 4
HSK_RAY_CLASS = ("hit", "frontier", "open", "blind", "outside")
HSK_EYE_FREE, HSK_EYE_UNSEEN, HSK_EYE_SOLID, HSK_EYE_OUTSIDE = 0, 1, 2, 3
HSK_COVER_MAX_POSES = 65536


class HskVoxelBox(C.Structure):
    """Mirror of `hsk_voxel_box` (include/hskinfu.h): the voxels lo <= (x, y, z) < hi."""

    _fields_ = [("lo", C.c_int * 3), ("hi", C.c_int * 3)]


class HskCoverage(C.Structure):
    """Mirror of `hsk_coverage` (include/hskinfu.h): 80 bytes."""

    _fields_ = [
        ("n_unseen", C.c_uint64), ("n_free", C.c_uint64), ("n_solid", C.c_uint64), ("n_frontier", C.c_uint64),
        ("faces", C.c_uint64 * 6),
    ]


class HskProbe(C.Structure):
    """Mirror of `hsk_probe` (include/hskinfu.h): a virtual depth camera and the samples along its rays."""

    _fields_ = [
        ("width", C.c_int), ("height", C.c_int),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("near_m", C.c_float), ("far_m", C.c_float), ("step_m", C.c_float),
    ]


class HskViewScore(C.Structure):
    """Mirror of `hsk_view_score` (include/hskinfu.h): 32 bytes."""

    _fields_ = [
        ("n_hit", C.c_uint32), ("n_frontier", C.c_uint32), ("n_open", C.c_uint32), ("n_blind", C.c_uint32), ("n_outside", C.c_uint32),
        ("eye_state", C.c_uint32),
        ("gain", C.c_uint64),
    ]


HSK_SPLAT_DISC, HSK_SPLAT_SURFEL = 0, 1
HSK_SPLAT_MAX_POINTS, HSK_SPLAT_MAX_POSES = 1 << 24, 65536


class HskSplatParams(C.Structure):
    """Mirror of `hsk_splat_params` (include/hskinfu.h): 28 bytes; a 0 in a field means its default."""

    _fields_ = [
        ("mode", C.c_int),
        ("point_size_m", C.c_float), ("cover", C.c_float), ("min_half_px", C.c_float), ("max_half_px", C.c_float),
        ("near_m", C.c_float), ("far_m", C.c_float),
    ]


class HskSplatStats(C.Structure):
    """Mirror of `hsk_splat_stats` (include/hskinfu.h): 24 bytes."""

    _fields_ = [
        ("n_invalid", C.c_uint32), ("n_clipped", C.c_uint32), ("n_backfacing", C.c_uint32), ("n_outside", C.c_uint32),
        ("n_splatted", C.c_uint32), ("n_pixels", C.c_uint32),
    ]


HSK_NORMAL_OK, HSK_NORMAL_INVALID, HSK_NORMAL_SPARSE, HSK_NORMAL_CROWDED, HSK_NORMAL_DEGENERATE = range(5)
HSK_NORMAL_MAX_POINTS, HSK_NORMAL_MAX_VIEWPOINTS = 1 << 24, 256


class HskNormalParams(C.Structure):
    """Mirror of `hsk_normal_params` (include/hskinfu.h): 24 bytes; a 0 in a field means its default."""

    _fields_ = [
        ("radius_m", C.c_float), ("min_neighbours", C.c_uint32), ("max_neighbours", C.c_uint32), ("line_rel", C.c_float),
        ("flags", C.c_uint32), ("pad", C.c_uint32),
    ]


class HskNormalStats(C.Structure):
    """Mirror of `hsk_normal_stats` (include/hskinfu.h): 32 bytes."""

    _fields_ = [
        ("n_ok", C.c_uint32), ("n_invalid", C.c_uint32), ("n_sparse", C.c_uint32), ("n_crowded", C.c_uint32), ("n_degenerate", C.c_uint32),
        ("n_cells", C.c_uint32),
        ("n_pairs", C.c_uint64),
    ]


HSK_COMPONENT_NONE = 0xFFFFFFFF
HSK_COMPONENT_MAX = 1 << 24
HSK_PRUNE_UNSEEN, HSK_PRUNE_FREE = 0, 1
HSK_FILL_SURFACE, HSK_FILL_ALL = 0, 1


class HskComponent(C.Structure):
    """Mirror of `hsk_component` (include/hskinfu.h): 48 bytes."""

    _fields_ = [
        ("root", C.c_int32 * 3), ("pad", C.c_int32),
        ("n_voxels", C.c_uint64),
        ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
    ]


class HskComponentStats(C.Structure):
    """Mirror of `hsk_component_stats` (include/hskinfu.h): 32 bytes."""

    _fields_ = [("n_components", C.c_uint64), ("n_inside", C.c_uint64), ("largest", C.c_uint64), ("labels_reused", C.c_int32), ("pad", C.c_int32)]


class HskPruneParams(C.Structure):
    """Mirror of `hsk_prune_params` (include/hskinfu.h): 16 bytes."""

    _fields_ = [("min_voxels", C.c_uint64), ("keep_largest", C.c_int32), ("fill", C.c_int32)]


class HskPruneStats(C.Structure):
    """Mirror of `hsk_prune_stats` (include/hskinfu.h): 32 bytes."""

    _fields_ = [("n_components", C.c_uint64), ("n_pruned", C.c_uint64), ("n_pruned_voxels", C.c_uint64), ("n_kept_voxels", C.c_uint64)]


class HskFillParams(C.Structure):
    """Mirror of `hsk_fill_params` (include/hskinfu.h): 16 bytes."""

    _fields_ = [("iterations", C.c_int32), ("keep", C.c_int32), ("band", C.c_int32), ("fill_weight", C.c_int32)]


class HskFillStats(C.Structure):
    """Mirror of `hsk_fill_stats` (include/hskinfu.h): 48 bytes."""

    _fields_ = [("n_unseen", C.c_uint64), ("n_reached", C.c_uint64), ("n_written", C.c_uint64), ("n_written_negative", C.c_uint64),
                ("tile_visits", C.c_uint64), ("iterations_run", C.c_int32), ("pad", C.c_int32)]


HSK_DIFF_UNSEEN, HSK_DIFF_ONLY_REF, HSK_DIFF_ONLY_CUR, HSK_DIFF_SAME, HSK_DIFF_APPEARED, HSK_DIFF_VANISHED, HSK_DIFF_MINOR = range(7)
HSK_ADOPT_APPEARED, HSK_ADOPT_VANISHED = 1, 2


class HskDiffParams(C.Structure):
    """Mirror of `hsk_diff_params` (include/hskinfu.h): 16 bytes."""

    _fields_ = [("thresh", C.c_int32), ("min_weight", C.c_int32), ("min_voxels", C.c_uint64)]


class HskDiffRegion(C.Structure):
    """Mirror of `hsk_diff_region` (include/hskinfu.h): 64 bytes."""

    _fields_ = [
        ("root", C.c_int32 * 3), ("pad", C.c_int32),
        ("n_voxels", C.c_uint64), ("n_appeared", C.c_uint64), ("n_vanished", C.c_uint64),
        ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
    ]


class HskDiffStats(C.Structure):
    """Mirror of `hsk_diff_stats` (include/hskinfu.h): 80 bytes."""

    _fields_ = [("n_class", C.c_uint64 * 7), ("n_regions", C.c_uint64), ("n_minor_regions", C.c_uint64), ("largest", C.c_uint64)]


class HskAdoptParams(C.Structure):
    """Mirror of `hsk_adopt_params` (include/hskinfu.h): 8 bytes."""

    _fields_ = [("which", C.c_int32), ("halo", C.c_int32)]


class HskAdoptStats(C.Structure):
    """Mirror of `hsk_adopt_stats` (include/hskinfu.h): 24 bytes."""

    _fields_ = [("n_targets", C.c_uint64), ("n_adopted", C.c_uint64), ("n_colored", C.c_uint64)]


HSK_SPLIT_NONE, HSK_SPLIT_FLOOR, HSK_SPLIT_CEILING, HSK_SPLIT_WALL, HSK_SPLIT_OTHER, HSK_SPLIT_OBJECT, HSK_SPLIT_MINOR = range(7)
HSK_KIND_FLOOR, HSK_KIND_CEILING, HSK_KIND_WALL, HSK_KIND_OTHER = 1, 2, 3, 4
HSK_REMOVE_ERASE, HSK_REMOVE_RESTORE = 0, 1
HSK_SPLIT_MAX_PLANES, HSK_REMOVE_MAX_OBJECTS = 64, 256


class HskSplitPlane(C.Structure):
    """Mirror of `hsk_split_plane` (include/hskinfu.h): 24 bytes."""

    _fields_ = [("abcd", C.c_float * 4), ("kind", C.c_int32), ("pad", C.c_int32)]


class HskSplitParams(C.Structure):
    """Mirror of `hsk_split_params` (include/hskinfu.h): 24 bytes."""

    _fields_ = [("dist_m", C.c_float), ("back_m", C.c_float), ("cos_min", C.c_float), ("pad", C.c_int32), ("min_voxels", C.c_uint64)]


class HskObject(C.Structure):
    """Mirror of `hsk_object` (include/hskinfu.h): 104 bytes."""

    _fields_ = [
        ("root", C.c_int32 * 3), ("pad", C.c_int32),
        ("n_voxels", C.c_uint64), ("sum", C.c_uint64 * 3),
        ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
        ("contact", C.c_uint32 * 4), ("plane_mask", C.c_uint64),
        ("height_lo", C.c_int32), ("height_hi", C.c_int32),
    ]


class HskSplitStats(C.Structure):
    """Mirror of `hsk_split_stats` (include/hskinfu.h): 104 bytes."""

    _fields_ = [("n_class", C.c_uint64 * 7), ("n_objects", C.c_uint64), ("n_minor_objects", C.c_uint64), ("largest", C.c_uint64),
                ("n_edge", C.c_uint64), ("n_no_normal", C.c_uint64), ("reused", C.c_uint32), ("pad", C.c_uint32)]


class HskRemoveParams(C.Structure):
    """Mirror of `hsk_remove_params` (include/hskinfu.h): 12 bytes."""

    _fields_ = [("mode", C.c_int32), ("halo", C.c_int32), ("fill_weight", C.c_int32)]


class HskRemoveStats(C.Structure):
    """Mirror of `hsk_remove_stats` (include/hskinfu.h): 40 bytes."""

    _fields_ = [("n_objects", C.c_uint64), ("n_targets", C.c_uint64), ("n_written", C.c_uint64), ("n_restored", C.c_uint64), ("n_colored", C.c_uint64)]


HSK_CLEAR_UNKNOWN = 1
HSK_CLEAR_MAX_REACH = 255
HSK_CLEARANCE_FAR, HSK_CLEARANCE_OUTSIDE = 0xFFFFFFFF, 0xFFFFFFFE
HSK_CLEAR_MAX_POINTS = 1 << 20


class HskClearanceParams(C.Structure):
    """Mirror of `hsk_clearance_params` (include/hskinfu.h): 24 bytes."""

    _fields_ = [("weight", C.c_uint32 * 3), ("max_d2", C.c_uint32), ("flags", C.c_uint32), ("unit_m", C.c_float)]


class HskClearanceStats(C.Structure):
    """Mirror of `hsk_clearance_stats` (include/hskinfu.h): 32 bytes."""

    _fields_ = [("n_obstacle", C.c_uint64), ("n_far", C.c_uint64), ("scratch_bytes", C.c_uint64), ("max_d2_seen", C.c_uint32), ("reused", C.c_int32)]


HSK_REACH_UNREACHED, HSK_REACH_OUTSIDE, HSK_REACH_BLOCKED = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
HSK_REACH_MAX_COST = 0xF0000000
HSK_REACH_MAX_SEEDS = 4096
HSK_REACH_MAX_ROUNDS = 65536


class HskReachParams(C.Structure):
    """Mirror of `hsk_reach_params` (include/hskinfu.h): 16 bytes."""

    _fields_ = [("min_d2", C.c_uint32), ("max_cost", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32)]


class HskReachStats(C.Structure):
    """Mirror of `hsk_reach_stats` (include/hskinfu.h): 40 bytes."""

    _fields_ = [("n_passable", C.c_uint64), ("n_reached", C.c_uint64), ("scratch_bytes", C.c_uint64), ("max_cost_seen", C.c_uint32),
                ("n_rounds", C.c_uint32), ("n_seeds_used", C.c_uint32), ("reused", C.c_int32)]


HSK_PARTITION_MAX_ROOMS = 1024
HSK_PARTITION_MAX_RADIUS = 4
HSK_ROOM_UNASSIGNED, HSK_ROOM_OUTSIDE, HSK_ROOM_BLOCKED, HSK_ROOM_NONE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC


class HskPartitionParams(C.Structure):
    """Mirror of `hsk_partition_params` (include/hskinfu.h): 24 bytes."""

    _fields_ = [("core_d2", C.c_uint32), ("min_d2", C.c_uint32), ("min_core_voxels", C.c_uint32), ("max_cost", C.c_uint32), ("flags", C.c_uint32),
                ("pad", C.c_uint32)]


class HskRoom(C.Structure):
    """Mirror of `hsk_room` (include/hskinfu.h): 88 bytes."""

    _fields_ = [("n_voxels", C.c_uint64), ("n_core_voxels", C.c_uint64), ("sum", C.c_uint64 * 3), ("root", C.c_uint32 * 3), ("lo", C.c_uint32 * 3),
                ("hi", C.c_uint32 * 3), ("max_d2", C.c_uint32), ("max_g", C.c_uint32), ("pad", C.c_uint32)]


class HskDoor(C.Structure):
    """Mirror of `hsk_door` (include/hskinfu.h): 72 bytes."""

    _fields_ = [("sum2", C.c_uint64 * 3), ("a", C.c_uint32), ("b", C.c_uint32), ("n_faces", C.c_uint32 * 3), ("lo", C.c_uint32 * 3),
                ("hi", C.c_uint32 * 3), ("max_d2", C.c_uint32)]


class HskPartitionStats(C.Structure):
    """Mirror of `hsk_partition_stats` (include/hskinfu.h): 56 bytes."""

    _fields_ = [("n_cores", C.c_uint64), ("n_passable", C.c_uint64), ("n_assigned", C.c_uint64), ("scratch_bytes", C.c_uint64), ("n_dropped", C.c_uint64),
                ("n_rooms", C.c_uint32), ("n_doors", C.c_uint32), ("n_rounds", C.c_uint32), ("reused", C.c_int32)]


HSK_SIMPLIFY_QUADRIC, HSK_SIMPLIFY_MEAN = 0, 1


class HskSimplifyParams(C.Structure):
    """Mirror of `hsk_simplify_params` (include/hskinfu.h): 12 bytes."""

    _fields_ = [("cluster_voxels", C.c_int32), ("mode", C.c_int32), ("sv_floor", C.c_float)]


class HskSimplifyStats(C.Structure):
    """Mirror of `hsk_simplify_stats` (include/hskinfu.h): 96 bytes."""

    _fields_ = [("n_in_vertices", C.c_uint64), ("n_in_faces", C.c_uint64), ("n_clusters", C.c_uint64), ("n_out_vertices", C.c_uint64),
                ("n_out_faces", C.c_uint64), ("n_faces_collapsed", C.c_uint64), ("n_rank", C.c_uint64 * 4), ("n_clamped", C.c_uint64),
                ("n_uncolored", C.c_uint64)]


HSK_TEXEL_OWNED, HSK_TEXEL_INSIDE, HSK_TEXEL_PROJECTED, HSK_TEXEL_COLORED, HSK_TEXEL_NORMAL = 1, 2, 4, 8, 16


class HskTextureParams(C.Structure):
    """Mirror of `hsk_texture_params` (include/hskinfu.h): 20 bytes."""

    _fields_ = [("texels_per_metre", C.c_float), ("atlas_width", C.c_int32), ("n_iter", C.c_int32), ("f_tol", C.c_float), ("max_offset_m", C.c_float)]


class HskTextureChart(C.Structure):
    """Mirror of `hsk_texture_chart` (include/hskinfu.h): 16 bytes."""

    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("s", C.c_int32), ("half_rot", C.c_int32)]


class HskTextureInfo(C.Structure):
    """Mirror of `hsk_texture_info` (include/hskinfu.h): 104 bytes."""

    _fields_ = [("width", C.c_uint64), ("height", C.c_uint64), ("n_faces_charted", C.c_uint64), ("n_faces_skipped", C.c_uint64),
                ("n_blocks", C.c_uint64 * 4), ("n_owned", C.c_uint64), ("n_inside", C.c_uint64), ("n_projected", C.c_uint64),
                ("n_colored", C.c_uint64), ("n_normal", C.c_uint64)]


HSK_TEXEL_KEYFRAME = 32
HSK_KEYTEX_BEST, HSK_KEYTEX_BLEND, HSK_KEYTEX_NONE = 0, 1, 255


class HskKeytexParams(C.Structure):
    """Mirror of `hsk_keytex_params` (include/hskinfu.h): 32 bytes."""

    _fields_ = [("mode", C.c_int32), ("z_min_m", C.c_float), ("z_max_m", C.c_float), ("cos_min", C.c_float), ("border_px", C.c_float),
                ("occlusion_tol_m", C.c_float), ("blend_floor", C.c_float), ("fallback_volume", C.c_int32)]


class HskKeytexInfo(C.Structure):
    """Mirror of `hsk_keytex_info` (include/hskinfu.h): 48 bytes."""

    _fields_ = [("n_keyframes", C.c_uint64), ("n_keyed", C.c_uint64), ("n_fallback", C.c_uint64), ("n_uncolored", C.c_uint64),
                ("n_pairs_seen", C.c_uint64), ("n_pairs_occluded", C.c_uint64)]


class HskVolumeInfo(C.Structure):
    """Mirror of `hsk_volume_info` (include/hskinfu.h): the header of a sparse volume image ("HSKV")."""

    _fields_ = [
        ("version", C.c_uint32), ("header_bytes", C.c_uint32), ("flags", C.c_uint32),
        ("dims", C.c_int32 * 3), ("z0", C.c_int32), ("nz", C.c_int32),
        ("size_m", C.c_float * 3),
        ("trunc_dist_m", C.c_float), ("trunc_eff_m", C.c_float),
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("pose", C.c_float * 16),
        ("frame", C.c_int32),
        ("color_max_weight", C.c_int32), ("color_band_m", C.c_float),
        ("n_bricks", C.c_uint64),
        ("tsdf_bricks", C.c_uint64 * 4), ("color_bricks", C.c_uint64 * 2),
        ("tsdf_table_bytes", C.c_uint64), ("tsdf_payload_bytes", C.c_uint64),
        ("color_table_bytes", C.c_uint64), ("color_payload_bytes", C.c_uint64),
        ("total_bytes", C.c_uint64),
        ("pass_reused", C.c_int32),
    ]


# every symbol include/hskinfu.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int)
SYMBOLS = {
    "hsk_build_id": (C.c_char_p, []),
    "hsk_default_config": (None, [C.POINTER(HskConfig), C.c_int]),
    "hsk_create": (C.c_int, [C.POINTER(HskConfig), C.POINTER(_P)]),
    "hsk_destroy": (None, [_P]),
    "hsk_reset": (C.c_int, [_P]),
    "hsk_last_error": (C.c_char_p, [_P]),
    "hsk_process_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, _F, _I]),
    "hsk_process_frame_dev": (C.c_int, [_P, _P, C.c_int, C.c_int, _F, _I]),
    "hsk_submit_frame_dev": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "hsk_submit_frame": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "hsk_wait_frame": (C.c_int, [_P, _F, _I]),
    "hsk_integrate": (C.c_int, [_P, _P, C.c_int, C.c_int, _F]),
    "hsk_raycast": (C.c_int, [_P, _F, _P, _P, _P]),
    "hsk_preprocess": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "hsk_icp_accumulate": (C.c_int, [_P, C.c_int, _F, C.c_int, C.c_int, _D]),
    "hsk_icp_solve": (C.c_int, [_D, _F, _I]),
    "hsk_count_updates": (C.c_int, [_P, _P, C.c_int, C.c_int, _F, C.POINTER(C.c_uint64)]),
    "hsk_download_tsdf": (C.c_int, [_P, _P]),
    "hsk_upload_tsdf": (C.c_int, [_P, _P]),
    "hsk_flush_weights": (C.c_int, [_P]),
    "hsk_prepare_readout": (C.c_int, [_P, C.c_size_t]),
    "hsk_stored_planes": (C.c_int, [_P, _I, _I]),
    "hsk_get_pose": (C.c_int, [_P, _F]),
    "hsk_set_pose": (C.c_int, [_P, _F]),
    "hsk_download_map": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "hsk_upload_map": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "hsk_download_depth_level": (C.c_int, [_P, C.c_int, _P]),
    "hsk_download_scaled_depth": (C.c_int, [_P, _P]),
    "hsk_extract_cloud": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_extract_mesh": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_extract_mesh_cubes": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_enable_color": (C.c_int, [_P, C.c_int, C.c_float]),
    "hsk_process_frame_rgbd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _F, _I]),
    "hsk_submit_frame_rgbd": (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    "hsk_integrate_color": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _F]),
    "hsk_download_color": (C.c_int, [_P, _P]),
    "hsk_upload_color": (C.c_int, [_P, _P]),
    "hsk_extract_cloud_attrs": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "hsk_extract_mesh_indexed": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P, C.c_size_t, C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_size_t)]),
    "hsk_default_simplify_params": (None, [_P, C.POINTER(HskSimplifyParams)]),
    "hsk_product_capacity": (C.c_size_t, [_P]),
    "hsk_default_texture_params": (None, [_P, C.POINTER(HskTextureParams)]),
    "hsk_texture_layout": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.c_float, C.c_int, _P, _P, C.POINTER(HskTextureInfo)]),
    "hsk_bake_texture": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(HskTextureParams), _P, _P, _P, C.c_size_t, _P, _P,
                                   C.POINTER(HskTextureInfo)]),
    "hsk_enable_keyframes": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "hsk_add_keyframe": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, _P, _P, C.POINTER(C.c_int)]),
    "hsk_keyframe_count": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "hsk_get_keyframe": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "hsk_clear_keyframes": (C.c_int, [_P]),
    "hsk_release_keyframes": (C.c_int, [_P]),
    "hsk_keyframe_wanted": (C.c_int, [_P, C.c_size_t, _P, C.c_float, C.c_float]),
    "hsk_default_keytex_params": (None, [_P, C.POINTER(HskKeytexParams)]),
    "hsk_bake_texture_keyframes": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(HskTextureParams), C.POINTER(HskKeytexParams), _P, _P, _P, _P,
                                             C.c_size_t, _P, _P, C.POINTER(HskTextureInfo), C.POINTER(HskKeytexInfo)]),
    "hsk_extract_mesh_simplified": (C.c_int, [_P, C.POINTER(HskSimplifyParams), _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P, C.c_size_t,
                                               C.POINTER(C.c_size_t), C.POINTER(HskSimplifyStats)]),
    "hsk_cluster_vertex": (C.c_int, [C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_float, _D, _I, _I]),
    "hsk_default_view": (None, [_P, C.POINTER(HskView)]),
    "hsk_render_view": (C.c_int, [_P, C.POINTER(HskView), _P, _P, _P, _P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "hsk_default_section": (None, [_P, C.POINTER(HskSection)]),
    "hsk_render_section": (C.c_int, [_P, C.POINTER(HskSection), _P, _P, _P, _P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_size_t)]),
    "hsk_section_in_room": (C.c_int, [C.POINTER(HskSection), _F, C.POINTER(HskSection)]),
    "hsk_composite_views": (C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_P), C.c_int, C.c_int, _P, _P, _P, _P]),
    "hsk_fuse_volume": (C.c_int, [_P, _P, _F, C.POINTER(HskFuseStats)]),
    "hsk_pack_volume": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HskVolumeInfo)]),
    "hsk_unpack_volume": (C.c_int, [_P, _P, C.c_size_t]),
    "hsk_save_volume": (C.c_int, [_P, C.c_char_p, C.POINTER(HskVolumeInfo)]),
    "hsk_load_volume": (C.c_int, [_P, C.c_char_p]),
    "hsk_volume_image_info": (C.c_int, [_P, C.c_size_t, C.POINTER(HskVolumeInfo)]),
    "hsk_volume_file_info": (C.c_int, [C.c_char_p, C.POINTER(HskVolumeInfo)]),
    "hsk_config_from_volume": (C.c_int, [C.POINTER(HskVolumeInfo), C.POINTER(HskConfig)]),
    "hsk_resume_scan": (C.c_int, [_P, _F]),
    "hsk_default_align_params": (None, [_P, C.POINTER(HskAlignParams)]),
    "hsk_align_cloud": (C.c_int, [_P, _P, _P, C.c_size_t, _F, C.POINTER(HskAlignParams), _F, C.POINTER(HskAlignStats)]),
    "hsk_align_volume": (C.c_int, [_P, _P, _F, C.POINTER(HskAlignParams), _F, C.POINTER(HskAlignStats)]),
    "hsk_align_step": (C.c_int, [_D, _F, _F, _F, _F, _I]),
    "hsk_set_loss_policy": (C.c_int, [_P, C.c_int]),
    "hsk_get_loss_policy": (C.c_int, [_P]),
    "hsk_score_cloud": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(HskPoseScore)]),
    "hsk_rank_scores": (C.c_int, [C.POINTER(HskPoseScore), C.c_size_t, C.POINTER(C.c_uint32)]),
    "hsk_default_reloc_params": (None, [_P, C.POINTER(HskRelocParams)]),
    "hsk_relocalize": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(HskRelocParams), _F, C.POINTER(HskRelocStats)]),
    "hsk_pose_lattice": (C.c_int, [_F, C.c_float, C.c_int, C.c_float, C.c_int, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_default_plane_params": (None, [C.POINTER(HskPlaneParams)]),
    "hsk_detect_planes_oriented": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(HskPlaneParams), C.POINTER(HskPlaneRecord), C.c_size_t,
                                             C.POINTER(C.c_size_t), _P, C.POINTER(C.c_size_t)]),
    "hsk_detect_planes_volume": (C.c_int, [_P, C.POINTER(HskPlaneParams), C.POINTER(HskPlaneRecord), C.c_size_t, C.POINTER(C.c_size_t), _P,
                                           C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_score_planes": (C.c_int, [_P, _P, _P, _P, C.c_size_t, _P, C.c_size_t, C.c_float, C.c_float, _P]),
    "hsk_plane_refit": (C.c_int, [C.POINTER(C.c_int64), _F, _F, _I]),
    "hsk_default_upright_params": (None, [C.POINTER(HskUprightParams)]),
    "hsk_estimate_upright": (C.c_int, [_P, C.POINTER(HskUprightParams), C.POINTER(HskUpright)]),
    "hsk_estimate_upright_oriented": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.POINTER(HskUprightParams), C.POINTER(HskUpright)]),
    "hsk_upright_sums": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_float, C.c_float, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "hsk_upright_solve_seed": (C.c_int, [_P, _P, C.c_float, C.c_uint64, _P, _P, _I]),
    "hsk_upright_solve_axis": (C.c_int, [_P, _P, _P, _I]),
    "hsk_upright_solve_basis": (C.c_int, [_P, _P, _P]),
    "hsk_upright_solve_yaw": (C.c_int, [_P, C.c_uint64, _P, _P, _I]),
    "hsk_upright_solve_frame": (C.c_int, [_P, C.c_uint64, _P, C.c_int, _P, _P]),
    "hsk_upright_solve_rows": (C.c_int, [_P, _P, _P, _P]),
    "hsk_upright_solve_heights": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P]),
    "hsk_level_config": (C.c_int, [_P, C.POINTER(HskUpright), C.c_float, _P, _F]),
    "hsk_default_probe": (None, [_P, C.POINTER(HskProbe)]),
    "hsk_coverage_census": (C.c_int, [_P, C.POINTER(HskVoxelBox), C.POINTER(HskCoverage)]),
    "hsk_score_views": (C.c_int, [_P, C.POINTER(HskProbe), _P, C.c_size_t, C.POINTER(HskViewScore)]),
    "hsk_render_coverage": (C.c_int, [_P, C.POINTER(HskProbe), _F, _P, _P, _P, C.POINTER(HskViewScore)]),
    "hsk_rank_views": (C.c_int, [C.POINTER(HskViewScore), C.c_size_t, C.POINTER(C.c_uint32)]),
    "hsk_default_splat_params": (None, [_P, C.POINTER(HskSplatParams)]),
    "hsk_splat_cloud": (C.c_int, [_P, _P, _P, C.c_size_t, _F, C.POINTER(HskSplatParams), _P, C.POINTER(HskSplatStats)]),
    "hsk_import_cloud": (C.c_int, [_P, _P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(HskSplatParams), C.POINTER(HskSplatStats)]),
    "hsk_default_normal_params": (None, [_P, C.POINTER(HskNormalParams)]),
    "hsk_estimate_normals": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t, C.POINTER(HskNormalParams), _P, _P, _P, _P, C.POINTER(HskNormalStats)]),
    "hsk_normal_solve": (C.c_int, [C.POINTER(C.c_int64), _F, _P, C.c_size_t, C.c_float, _F, _F, _I]),
    "hsk_default_prune_params": (None, [_P, C.POINTER(HskPruneParams)]),
    "hsk_label_components": (C.c_int, [_P, C.POINTER(HskComponent), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HskComponentStats)]),
    "hsk_download_components": (C.c_int, [_P, _P]),
    "hsk_prune_components": (C.c_int, [_P, C.POINTER(HskPruneParams), C.POINTER(HskPruneStats)]),
    "hsk_default_fill_params": (None, [_P, C.POINTER(HskFillParams)]),
    "hsk_fill_holes": (C.c_int, [_P, C.POINTER(HskFillParams), C.POINTER(HskVoxelBox), C.POINTER(HskFillStats)]),
    "hsk_download_fill_mask": (C.c_int, [_P, C.POINTER(HskVoxelBox), _P]),
    "hsk_default_diff_params": (None, [_P, C.POINTER(HskDiffParams)]),
    "hsk_diff_volume": (C.c_int, [_P, _P, C.POINTER(HskDiffParams), C.POINTER(HskDiffRegion), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HskDiffStats)]),
    "hsk_download_diff": (C.c_int, [_P, C.POINTER(HskVoxelBox), _P, _P]),
    "hsk_diff_at": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P]),
    "hsk_adopt_diff": (C.c_int, [_P, _P, C.POINTER(HskAdoptParams), C.POINTER(HskAdoptStats)]),
    "hsk_release_diff": (C.c_int, [_P]),
    "hsk_default_split_params": (None, [_P, C.POINTER(HskSplitParams)]),
    "hsk_default_remove_params": (None, [_P, C.POINTER(HskRemoveParams)]),
    "hsk_split_plane_kinds": (C.c_int, [C.POINTER(HskSplitPlane), C.c_size_t, C.POINTER(C.c_float), C.c_float, C.c_float]),
    "hsk_split_scene": (C.c_int, [_P, C.POINTER(HskSplitPlane), C.c_size_t, C.POINTER(HskSplitParams), C.POINTER(HskObject), C.c_size_t, C.POINTER(C.c_size_t),
                                  C.POINTER(HskSplitStats)]),
    "hsk_download_split": (C.c_int, [_P, C.POINTER(HskVoxelBox), _P, _P, _P]),
    "hsk_split_at": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P, _P, _P]),
    "hsk_remove_objects": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(HskRemoveParams), C.POINTER(HskRemoveStats)]),
    "hsk_release_split": (C.c_int, [_P]),
    "hsk_default_clearance_params": (None, [_P, C.POINTER(HskClearanceParams)]),
    "hsk_clearance_d2": (C.c_uint32, [C.POINTER(HskClearanceParams), C.c_float]),
    "hsk_build_clearance": (C.c_int, [_P, C.POINTER(HskClearanceParams), C.POINTER(HskClearanceStats)]),
    "hsk_download_clearance": (C.c_int, [_P, C.POINTER(HskClearanceParams), C.POINTER(HskVoxelBox), _P]),
    "hsk_clearance_at": (C.c_int, [_P, C.POINTER(HskClearanceParams), _P, C.c_size_t, _P]),
    "hsk_clearance_floor": (C.c_int, [_P, C.POINTER(HskClearanceParams), C.c_int, C.c_int, C.c_int, _P, C.POINTER(HskClearanceStats)]),
    "hsk_release_clearance": (C.c_int, [_P]),
    "hsk_rank_views_clear": (C.c_int, [C.POINTER(HskViewScore), C.POINTER(C.c_uint32), C.c_uint32, C.c_size_t, C.POINTER(C.c_uint32)]),
    "hsk_default_reach_params": (None, [_P, C.POINTER(HskClearanceParams), C.POINTER(HskReachParams)]),
    "hsk_build_reach": (C.c_int, [_P, C.POINTER(HskClearanceParams), C.POINTER(HskReachParams), _P, C.c_size_t, C.POINTER(HskReachStats)]),
    "hsk_download_reach": (C.c_int, [_P, C.POINTER(HskVoxelBox), _P]),
    "hsk_reach_at": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "hsk_reach_path": (C.c_int, [_P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_reach_floor": (C.c_int, [_P, C.POINTER(HskClearanceParams), C.c_int, C.c_int, C.c_int, C.POINTER(HskReachParams), _P, C.c_size_t, _P,
                                  C.POINTER(HskReachStats)]),
    "hsk_release_reach": (C.c_int, [_P]),
    "hsk_reach_tiles_relaxed": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hsk_rank_views_reach": (C.c_int, [C.POINTER(HskViewScore), C.POINTER(C.c_uint32), C.c_uint32, C.c_size_t, C.POINTER(C.c_uint32)]),
    "hsk_reach_metres": (C.c_float, [C.POINTER(HskClearanceParams), C.c_uint32]),
    "hsk_default_partition_params": (None, [_P, C.POINTER(HskClearanceParams), C.POINTER(HskPartitionParams)]),
    "hsk_build_partition": (C.c_int, [_P, C.POINTER(HskClearanceParams), C.POINTER(HskPartitionParams), _P, C.c_size_t, C.POINTER(C.c_size_t),
                                      C.POINTER(HskPartitionStats)]),
    "hsk_partition_doors": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_download_partition": (C.c_int, [_P, C.POINTER(HskVoxelBox), _P]),
    "hsk_download_partition_cost": (C.c_int, [_P, C.POINTER(HskVoxelBox), _P]),
    "hsk_partition_at": (C.c_int, [_P, _P, C.c_size_t, C.c_int, _P]),
    "hsk_partition_floor": (C.c_int, [_P, C.POINTER(HskClearanceParams), C.c_int, C.c_int, C.c_int, C.POINTER(HskPartitionParams), _P, _P, C.c_size_t,
                                      C.POINTER(C.c_size_t), _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(HskPartitionStats)]),
    "hsk_release_partition": (C.c_int, [_P]),
    "hsk_partition_tiles_relaxed": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "hsk_merge_rooms": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_uint32, _P]),
    "hsk_invert_rigid": (C.c_int, [_F, _F]),
    "hsk_fuse_footprint": (C.c_int, [_I, _F, _I, _F, _F, C.POINTER(C.c_int32)]),
    "hsk_write_ppm": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int]),
    "hsk_write_pgm16": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int]),
    "hsk_mgpu_frame_begin": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "hsk_mgpu_prefetch": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "hsk_mgpu_frame_front": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "hsk_mgpu_icp_accumulate": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "hsk_mgpu_icp_update": (C.c_int, [_P, _P]),
    "hsk_mgpu_icp_replicated": (C.c_int, [_P]),
    "hsk_mgpu_integrate": (C.c_int, [_P]),
    "hsk_mgpu_raycast_local": (C.c_int, [_P, _P]),
    "hsk_mgpu_raycast_resolve": (C.c_int, [_P, _P, _P]),
    "hsk_mgpu_raycast_push": (C.c_int, [_P, _P, C.POINTER(_P), C.c_int]),
    "hsk_mgpu_frame_end": (C.c_int, [_P, _P, _P, _F, _I]),
    "hsk_mgpu_frame_index": (C.c_int, [_P]),
    "hsk_mgpu_frame_end_async": (C.c_int, [_P, _P, _P]),
    "hsk_mgpu_restart_pending": (C.c_int, [_P]),
    "hsk_stream": (_P, [_P]),
    "hsk_set_stream": (C.c_int, [_P, _P]),
    "hsk_synchronize": (C.c_int, [_P]),
    "hsk_set_profiling": (C.c_int, [_P, C.c_int]),
    "hsk_stage_ms": (C.c_int, [_P, _D, C.POINTER(C.c_uint64), C.c_int]),
    "hsk_icp_level_ms": (C.c_int, [_P, _D]),
    "hsk_submit_host_us": (C.c_int, [_P, _D, C.POINTER(C.c_uint64), C.c_int]),
    "hsk_integrate_queue_entries": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "hsk_integrate_light_entries": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "hsk_integrate_coarse_counts": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "hsk_bilateral_tables": (C.c_int, [_F, _F]),
    "hsk_selftest_exact_ops": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "hsk_group_create": (C.c_int, [C.POINTER(HskConfig), C.c_int, _I, C.c_int, C.POINTER(_P)]),
    "hsk_group_unique_id": (C.c_int, [_P]),
    "hsk_group_create_rank": (C.c_int, [C.POINTER(HskConfig), C.c_int, C.c_int, _P, C.c_int, C.POINTER(_P)]),
    "hsk_group_destroy": (None, [_P]),
    "hsk_group_last_error": (C.c_char_p, [_P]),
    "hsk_group_reset": (C.c_int, [_P]),
    "hsk_group_process_frame": (C.c_int, [_P, _P, C.c_int, C.c_int, _F, _I]),
    "hsk_group_submit_frame": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "hsk_group_submit_frame_dev": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int]),
    "hsk_group_wait_frame": (C.c_int, [_P, _F, _I]),
    "hsk_group_exchange_ms": (C.c_int, [_P, _D, _D, C.POINTER(C.c_ulonglong)]),
    "hsk_group_n_slabs": (C.c_int, [_P]),
    "hsk_group_ranks_seen": (C.c_int, [_P, _I]),
    "hsk_group_slab": (_P, [_P, C.c_int]),
    "hsk_group_download_tsdf": (C.c_int, [_P, _P]),
    "hsk_synth_pose": (C.c_int, [C.c_int, _F]),
    "hsk_synth_render": (C.c_int, [_F, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "hsk_synth_room_extents": (C.c_int, [C.c_int, _F]),
    "hsk_synth_room_pose": (C.c_int, [C.c_int, C.c_int, C.c_int, _F]),
    "hsk_synth_room_render": (C.c_int, [C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "hsk_synth_render_sensor": (C.c_int, [C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_float, C.c_float, C.c_int, _P, _D]),
    "hsk_synth_color_at": (C.c_int, [C.c_int, _F, _P]),
    "hsk_synth_render_rgb": (C.c_int, [C.c_int, _F, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "hsk_write_pcd_xyz": (C.c_int, [C.c_char_p, _P, C.c_size_t]),
    "hsk_write_ply_mesh": (C.c_int, [C.c_char_p, _P, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "hsk_weld_triangles": (C.c_int, [_P, C.c_size_t, _P, C.c_size_t, C.POINTER(C.c_size_t), _P]),
    "hsk_write_ply_indexed": (C.c_int, [C.c_char_p, _P, _P, _P, C.c_size_t, _P, C.c_size_t]),
    "hsk_write_ply_textured": (C.c_int, [C.c_char_p, _P, _P, C.c_size_t, _P, C.c_size_t, _P, C.c_char_p]),
    "hsk_write_png_rgb": (C.c_int, [C.c_char_p, _P, C.c_int, C.c_int]),
    "hsk_voxel_downsample": (C.c_int, [_P, C.c_size_t, C.c_float, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_voxel_downsample_attrs": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_float, _P, _P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_write_pcd_xyzrgbnormal": (C.c_int, [C.c_char_p, _P, _P, _P, C.c_size_t]),
    "hsk_detect_planes": (C.c_int, [_P, C.c_size_t, C.c_float, C.c_float, C.c_int, C.c_int, _P, _P, _I]),
    "hsk_plane_hull": (C.c_int, [_P, C.c_size_t, _P, C.c_int, _F, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "hsk_write_planes_txt": (C.c_int, [C.c_char_p, _P, C.c_int]),
    "hsk_write_xf": (C.c_int, [C.c_char_p, _F]),
    "hsk_read_xf": (C.c_int, [C.c_char_p, _F]),
    "hsk_transform_cloud": (C.c_int, [_P, C.c_size_t, _F, _P]),
    "hsk_transform_normals": (C.c_int, [_P, C.c_size_t, _F, _P]),
    "hsk_stream_create": (_P, [C.c_char_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float]),
    "hsk_stream_open": (_P, [C.c_char_p, _I, _I, _I, _F]),
    "hsk_stream_write": (C.c_int, [_P, _P]),
    "hsk_stream_read": (C.c_int, [_P, C.c_int, _P]),
    "hsk_stream_close": (C.c_int, [_P]),
    "hsk_stream_info": (C.c_int, [_P, _I, _I, _I, _F]),
    "hsk_track_stream": (C.c_int, [_P, _P, C.c_int, C.c_int, _F, _I]),
}

# every symbol include/hshouse.h declares (host-side room stitching)
_U32 = C.POINTER(C.c_uint32)
_SZ = C.POINTER(C.c_size_t)
HSH_OBJECTIVE = C.CFUNCTYPE(C.c_double, _D, C.c_int, _P)
HOUSE_SYMBOLS = {
    "hsh_create": (_P, []),
    "hsh_destroy": (None, [_P]),
    "hsh_last_error": (C.c_char_p, [_P]),
    "hsh_load_room": (C.c_int, [_P, C.c_char_p, _U32]),
    "hsh_add_room": (C.c_int, [_P, C.c_char_p, _P, C.c_size_t, _P, C.c_int, _P, _P, _U32]),
    "hsh_room_ids": (C.c_int, [_P, _P, C.c_int, _I]),
    "hsh_room_planes": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_int, _I]),
    "hsh_plane_bounds": (C.c_int, [_P, C.c_uint32, _P, C.c_int, _I]),
    "hsh_room_corners": (C.c_int, [_P, C.c_uint32, C.c_int, _P, _P, C.c_int, _I]),
    "hsh_room_cloud": (C.c_int, [_P, C.c_uint32, _P, C.c_size_t, _SZ]),
    "hsh_room_means": (C.c_int, [_P, C.c_uint32, _P, _P]),
    "hsh_set_room_corners": (C.c_int, [_P, C.c_uint32, _P, C.c_int]),
    "hsh_accept_corner_suggestion": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "hsh_translate_room": (C.c_int, [_P, C.c_uint32, _P]),
    "hsh_rotate_room": (C.c_int, [_P, C.c_uint32, _P]),
    "hsh_rotate_kinfu_room": (C.c_int, [_P, C.c_uint32]),
    "hsh_room_auto_align_axis": (C.c_int, [_P, C.c_uint32, _P]),
    "hsh_auto_align_floor": (C.c_int, [_P, C.c_uint32]),
    "hsh_remove_ceiling": (C.c_int, [_P, C.c_uint32]),
    "hsh_suggest_points": (C.c_int, [_P, C.c_uint32, C.c_float, _I, _I]),
    "hsh_fit_cuboid_to_room": (C.c_int, [_P, C.c_uint32, C.c_int, _I, _D, _D]),
    "hsh_connect_walls": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int, C.c_float, _I]),
    "hsh_disconnect_walls": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "hsh_connected_walls": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, _I]),
    "hsh_optimize_room_positions": (C.c_int, [_P, _D]),
    "hsh_room_projection": (C.c_int, [_P, C.c_uint32, _F]),
    "hsh_room_projection_string": (C.c_int, [_P, C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]),
    "hsh_export_all_room_xf_files": (C.c_int, [_P, C.c_char_p]),
    "hsh_plane_corner": (C.c_int, [_P, _P, _I]),
    "hsh_fit_plane": (C.c_int, [_P, C.c_int, _P]),
    "hsh_rotation_between": (C.c_int, [_P, _P, _P]),
    "hsh_cuboid_from_params": (C.c_int, [_P, _P]),
    "hsh_guess_dims": (C.c_int, [_P, _P]),
    "hsh_errfun": (C.c_int, [_P, _P, C.c_int, _D]),
    "hsh_fit_cuboid": (C.c_int, [_P, C.c_int, C.c_int, _P, _I, _D]),
    "hsh_nm_minimize": (C.c_int, [HSH_OBJECTIVE, _P, C.c_int, _P, _P, C.c_double, C.c_int, _P, _D, _I]),
    "hsh_lstsq_distances": (C.c_int, [_P, _P, _P, C.c_int, _P, _P, C.c_int, _I, _D]),
    "hsh_group_connected_components": (C.c_int, [_P, _P, C.c_int, _P, _I]),
    "hsh_show_float": (C.c_int, [C.c_float, C.c_char_p, C.c_size_t]),
    "hsh_read_pcd_xyz": (C.c_int, [C.c_char_p, _P, C.c_size_t, _SZ]),
    "hsh_read_planes_txt": (C.c_int, [C.c_char_p, _P, C.c_int, _I]),
    "hsh_write_ply_points": (C.c_int, [C.c_char_p, _P, C.c_size_t]),
    "hsh_read_ply_points": (C.c_int, [C.c_char_p, _P, C.c_size_t, _SZ]),
}

_lib = None


def _share_torch_hip_runtime():
    """One HIP runtime per process.  The torch wheel ships its own libamdhip64.so.7 (ROCm 7.0) beside the system's
    (ROCm 7.2, the one libhskinfu.so names in its RUNPATH); the loader keeps whichever copy comes first for BOTH, and
    torch cannot initialise on top of the system copy ("No HIP GPUs are available").  So when torch is installed but not
    imported yet, its copy is loaded first; without torch the system runtime is used."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            return  # fall back to the system runtime; a later `import torch` in this process may then fail
        # ... and one RCCL: hsk_group_* loads RCCL at run time; beside torch's HIP runtime it must be torch's copy
        rccl = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so")
        if os.path.exists(rccl):
            os.environ.setdefault("HSK_RCCL_PATH", rccl)


def load():
    """Load libhskinfu.so and bind every symbol; raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _share_torch_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C housescan_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SYMBOLS.items()) + list(HOUSE_SYMBOLS.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
