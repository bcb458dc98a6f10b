"""housescan_amd -- MI355X-native KinectFusion core behind a C ABI (include/hskinfu.h).

Importing the package loads libhskinfu.so; it fails loudly if the HIP library has not been built.
"""
from . import _lib

_lib.load()

from .kinfu import (GROUP_DIRECT, GROUP_FORCE_RCCL, GROUP_ICP_ALLREDUCE, GROUP_PROFILE, KinfuError, KinfuGroup, KinfuTracker,  # noqa: E402
                    bilateral_tables, default_config, synth_depth, synth_noisy_frames, synth_pose, synth_room_depth, synth_room_extents, synth_box_depth,
                    synth_color_at, synth_rgb, synth_room_pose, synth_sensor_depth, synth_sensor_frames, config_from_volume, volume_file_info,
                    volume_image_info, pose_lattice, rank_scores, plane_refit, default_probe, rank_views, default_prune_params, default_fill_params, FILL_SURFACE, FILL_ALL, default_diff_params, DIFF_UNSEEN, DIFF_ONLY_REF, DIFF_ONLY_CUR, DIFF_SAME, DIFF_APPEARED, DIFF_VANISHED, DIFF_MINOR, ADOPT_APPEARED, ADOPT_VANISHED, default_split_params, default_remove_params, split_planes, split_plane_kinds, SPLIT_NONE, SPLIT_FLOOR, SPLIT_CEILING, SPLIT_WALL, SPLIT_OTHER, SPLIT_OBJECT, SPLIT_MINOR, KIND_FLOOR, KIND_CEILING, KIND_WALL, KIND_OTHER, REMOVE_ERASE, REMOVE_RESTORE, default_clearance_params, clearance_d2, clearance_metres, rank_views_clear, default_reach_params, reach_metres, rank_views_reach, default_partition_params, merge_rooms, cluster_vertex,
                    SIMPLIFY_MEAN, SIMPLIFY_QUADRIC, texture_layout, TEXEL_OWNED, TEXEL_INSIDE, TEXEL_PROJECTED, TEXEL_COLORED, TEXEL_NORMAL,
                    TEXEL_KEYFRAME, KEYTEX_BEST, KEYTEX_BLEND, KEYTEX_NONE, keyframe_wanted, default_splat_params, SPLAT_DISC, SPLAT_SURFEL,
                    default_normal_params, normal_solve, NORMAL_OK, NORMAL_INVALID, NORMAL_SPARSE, NORMAL_CROWDED, NORMAL_DEGENERATE)

from .products import DepthStreamReader, DepthStreamWriter  # noqa: E402  (recorded depth streams: the HSKD container)

__all__ = ["DepthStreamReader", "DepthStreamWriter", "KinfuError", "KinfuTracker", "KinfuGroup", "GROUP_FORCE_RCCL", "GROUP_ICP_ALLREDUCE", "GROUP_DIRECT", "GROUP_PROFILE", "default_config",
           "synth_depth", "synth_noisy_frames", "synth_pose", "bilateral_tables", "synth_room_depth", "synth_room_extents", "synth_room_pose", "synth_sensor_depth", "synth_sensor_frames",
           "synth_rgb", "synth_box_depth", "synth_color_at", "config_from_volume", "volume_file_info", "volume_image_info", "pose_lattice", "rank_scores", "plane_refit", "default_probe", "rank_views", "default_prune_params", "default_fill_params", "FILL_SURFACE", "FILL_ALL", "default_diff_params", "DIFF_UNSEEN", "DIFF_ONLY_REF", "DIFF_ONLY_CUR", "DIFF_SAME", "DIFF_APPEARED", "DIFF_VANISHED", "DIFF_MINOR", "ADOPT_APPEARED", "ADOPT_VANISHED", "default_split_params", "default_remove_params", "split_planes", "split_plane_kinds", "SPLIT_NONE", "SPLIT_FLOOR", "SPLIT_CEILING", "SPLIT_WALL", "SPLIT_OTHER", "SPLIT_OBJECT", "SPLIT_MINOR", "KIND_FLOOR", "KIND_CEILING", "KIND_WALL", "KIND_OTHER", "REMOVE_ERASE", "REMOVE_RESTORE", "default_clearance_params", "clearance_d2", "clearance_metres", "rank_views_clear", "default_reach_params", "reach_metres", "rank_views_reach", "default_partition_params", "merge_rooms", "cluster_vertex", "SIMPLIFY_QUADRIC", "SIMPLIFY_MEAN", "texture_layout", "TEXEL_OWNED", "TEXEL_INSIDE", "TEXEL_PROJECTED", "TEXEL_COLORED",
           "TEXEL_NORMAL", "TEXEL_KEYFRAME", "KEYTEX_BEST", "KEYTEX_BLEND", "KEYTEX_NONE", "keyframe_wanted", "default_splat_params", "SPLAT_DISC", "SPLAT_SURFEL",
           "default_normal_params", "normal_solve", "NORMAL_OK", "NORMAL_INVALID", "NORMAL_SPARSE", "NORMAL_CROWDED", "NORMAL_DEGENERATE"]
