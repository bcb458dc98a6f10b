"""Host-side mirror of the KinFu tracker interface over the C ABI.

Names follow the upstream KinFu application that HouseScan's README points users at
(/root/reference/README.md:13-14): a tracker object fed one depth frame at a time, returning the camera
pose; `extract_cloud` yields the packed float32 xyz cloud HouseScan stores in `Cloud.cloudPoints`
(/root/reference/housescan/Main.hs:117-121).  Depth frames are numpy uint16 arrays of shape (h, w) in the
row-major layout of HoniHelper.takeDepthSnapshot (/root/reference/housescan/HoniHelper.hs:20-36).
Errors surface as `KinfuError` carrying `hsk_last_error` (the `Left String` of HoniHelper.hs:39-42).
"""
import ctypes as C

import numpy as np

from . import _lib


class KinfuError(RuntimeError):
    pass


def default_config(n=512, **over):
    lib = _lib.load()
    cfg = _lib.HskConfig()
    lib.hsk_default_config(C.byref(cfg), int(n))
    for k, v in over.items():
        if k in ("vol_size_m", "icp_iters", "init_pose"):
            arr = getattr(cfg, k)
            for i, x in enumerate(np.asarray(v).reshape(-1)):
                arr[i] = x
        else:
            setattr(cfg, k, v)
    return cfg


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _apply_view_fields(v, width, height, fx, fy, cx, cy, pose, mode, light, light_in_camera, background):
    """render_view's / render_section's keywords into the HskView `v`: those that are not None override its fields"""
    for name, val in (("width", width), ("height", height), ("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy), ("mode", mode),
                      ("light_in_camera", light_in_camera)):
        if val is not None:
            setattr(v, name, val)
    if pose is not None:
        v.pose[:] = [float(x) for x in np.asarray(pose, np.float32).reshape(16)]
        v.follow = 0
    if light is not None:
        v.light[:] = [float(x) for x in light]
    if background is not None:
        v.background[:] = [int(x) for x in background]


def _image_arrays(w, h, rgb, depth, vmap, nmap):
    """the images asked for -> (dict of empty arrays, ptr(key): an array's address or None)"""
    shapes = (("rgb", rgb, (h, w, 3), np.uint8), ("depth", depth, (h, w), np.uint16), ("vmap", vmap, (3, h, w), np.float32),
              ("nmap", nmap, (3, h, w), np.float32))
    ok = 1 <= w <= 4096 and 1 <= h <= 4096   # (otherwise the call itself refuses; nothing is allocated for it here)
    out = {key: np.empty(shape, dt) for key, want, shape, dt in shapes if want and ok}
    return out, lambda k: out[k].ctypes.data if k in out else None


def _override(p, allowed, what, over):
    """the keywords `over` into the ctypes structure `p`: a name outside `allowed` raises TypeError(f"{what} {name!r}"); a value is
    coerced by its field's C type -- float() for a float field, int() for an integer field, element by element for an array -> p"""
    types = dict(p._fields_)

    def cast(t, v):
        return float(v) if t in (C.c_float, C.c_double) else int(v)

    for name, val in over.items():
        if name not in allowed:
            raise TypeError(f"{what} {name!r}")
        t = types[name]
        setattr(p, name, t(*[cast(t._type_, v) for v in val]) if issubclass(t, C.Array) else cast(t, val))
    return p


def _params(kind, tracker, params, over, clearance=()):
    """the parameters of a call of `kind` = (structure, the C default call's name, the names a caller may set, the TypeError's
    text): a copy of the caller's `params`, or, None, the C defaults for `tracker` (None: the default configuration's) -- for the
    reach and partition calls behind `clearance` = (their clearance parameters or None,) --, then the keywords `over` -> the structure"""
    struct, default, allowed, what = kind
    if params is None:
        p = struct()
        getattr(_lib.load(), default)(tracker.h if tracker is not None else None, *(None if c is None else C.byref(c) for c in clearance), C.byref(p))
    else:
        p = struct.from_buffer_copy(params)
    return _override(p, allowed, what, over)


def _box(cfg, box):
    """box = (lo, hi), None: the whole volume -> (an `_lib.HskVoxelBox` or None, the [z, y, x] shape of its voxels)"""
    if box is None:
        return None, (cfg.vol_z, cfg.vol_y, cfg.vol_x)
    b = _lib.HskVoxelBox()
    b.lo[:] = [int(v) for v in box[0]]
    b.hi[:] = [int(v) for v in box[1]]
    return b, tuple(max(b.hi[i] - b.lo[i], 0) for i in (2, 1, 0))


def _at_points(xyz, dtypes, call):
    """the world points xyz [n, 3] through call(points, m, *outputs) in pieces of HSK_CLEAR_MAX_POINTS, what the C calls take
    (no points: one call with every pointer None) -> one [n] array per dtype"""
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    outs = [np.empty(len(pts), dt) for dt in dtypes]
    step = _lib.HSK_CLEAR_MAX_POINTS
    for at in range(0, max(len(pts), 1), step):
        m = min(step, len(pts) - at)
        call(pts[at:].ctypes.data if m else None, m, *(o[at:].ctypes.data if m else None for o in outs))
    return outs


def _records(struct, call, st=None):
    """the two calls of a record read-out: call(None, 0, n, stats) asks for the count, call(records, n, n, None) fills them (the
    fill is answered from what the size query left: its stats are the size query's) -> a structured array of `struct`"""
    n = C.c_size_t(0)
    call(None, 0, C.byref(n), None if st is None else C.byref(st))
    recs = np.zeros(n.value, np.dtype(struct))
    if n.value:
        call(recs.ctypes.data_as(C.POINTER(struct)), n.value, C.byref(n), None)
    return recs


def _stats_dict(st):
    """a ctypes stats structure as a dict in field order, `pad` left out: a scalar as an int, an array as a uint64 array"""
    return {name: np.array(getattr(st, name)).astype(np.uint64) if issubclass(t, C.Array) else int(getattr(st, name))
            for name, t in st._fields_ if name != "pad"}


def _floor_shape(cfg, axis):
    """a floor map's (nv, nu) for the up axis, u the lower-numbered remaining axis ((1, 1) for an axis the call refuses)"""
    dims = (cfg.vol_x, cfg.vol_y, cfg.vol_z)
    return (dims[1 if axis == 2 else 2], dims[1 if axis == 0 else 0]) if axis in (0, 1, 2) else (1, 1)


# the records as numpy sees them: the layout of their structures
SCORE_DTYPE = np.dtype(_lib.HskPoseScore)
PLANE_DTYPE = np.dtype(_lib.HskPlaneRecord)
VIEW_SCORE_DTYPE = np.dtype(_lib.HskViewScore)
PROBE_FIELDS = ("width", "height", "fx", "fy", "cx", "cy", "near_m", "far_m", "step_m")
_PROBE = (_lib.HskProbe, "hsk_default_probe", PROBE_FIELDS, "a probe has no field")


def default_probe(tracker=None, **fields):
    """the probe of the coverage calls (hsk_default_probe): the tracker's camera at a quarter of its resolution, near_m 0.4,
    far_m 3.5, step_m half its truncation distance (without a tracker: the default configuration's); the keywords -- width,
    height, fx, fy, cx, cy, near_m, far_m, step_m -- override its fields -> an `_lib.HskProbe`"""
    return _params(_PROBE, tracker, None, fields)


SPLAT_DISC, SPLAT_SURFEL = 0, 1
SPLAT_FIELDS = ("mode", "point_size_m", "cover", "min_half_px", "max_half_px", "near_m", "far_m")
SPLAT_STATS_DTYPE = np.dtype(_lib.HskSplatStats)
_SPLAT = (_lib.HskSplatParams, "hsk_default_splat_params", SPLAT_FIELDS, "splat parameters have no field")


def default_splat_params(tracker=None, **fields):
    """the parameters of splat_cloud and import_cloud (hsk_default_splat_params): mode SPLAT_DISC, point_size_m the tracker's
    largest cell (without a tracker 3 / 512) -- a property of the cloud: set it to the cloud's leaf size --, cover 1.5, min_half_px
    0.5, max_half_px 8, near_m 0.1, far_m 8; the keywords override its fields -> an `_lib.HskSplatParams`"""
    return _params(_SPLAT, tracker, None, fields)


NORMAL_OK, NORMAL_INVALID, NORMAL_SPARSE, NORMAL_CROWDED, NORMAL_DEGENERATE = range(5)
NORMAL_FIELDS = ("radius_m", "min_neighbours", "max_neighbours", "line_rel")
_NORMAL = (_lib.HskNormalParams, "hsk_default_normal_params", NORMAL_FIELDS, "normal parameters have no field")


def default_normal_params(tracker=None, **fields):
    """the parameters of estimate_normals (hsk_default_normal_params): radius_m 3 x the tracker's largest cell, kept to 1 / 1024 ..
    0.25 (without a tracker 9 / 512), min_neighbours 8, max_neighbours 4096, line_rel 1e-3; the keywords override its fields -> an
    `_lib.HskNormalParams`"""
    return _params(_NORMAL, tracker, None, fields)


def _viewpoints(viewpoints):
    vp = np.zeros((0, 3), np.float32) if viewpoints is None else np.ascontiguousarray(viewpoints, np.float32).reshape(-1, 3)
    return vp, (vp.ctypes.data if len(vp) else None)


def normal_solve(sums10, point, viewpoints=None, line_rel=1e-3):
    """one point's normal from its neighbours' ten integer sums (hsk_normal_solve; host only, the device solve's mirror): sums10 = m,
    S_x S_y S_z, S_xx S_xy S_xz S_yy S_yz S_zz of q_j - q_p with q = rint(coordinate * 4096); point [3] and viewpoints [v, 3] in metres
    -> (normal [3] float32, curvature float32, class: NORMAL_OK or NORMAL_DEGENERATE)"""
    s = np.ascontiguousarray(sums10, np.int64).reshape(10)
    pt = np.ascontiguousarray(point, np.float32).reshape(3)
    vp, pv = _viewpoints(viewpoints)
    nrm, curv, cls = np.zeros(3, np.float32), np.zeros(1, np.float32), C.c_int()
    if _lib.load().hsk_normal_solve(s.ctypes.data_as(C.POINTER(C.c_int64)), _fp(pt), pv, len(vp), float(line_rel), _fp(nrm), _fp(curv), C.byref(cls)) != 0:
        raise KinfuError("normal_solve: invalid arguments (m outside 1..2^20, a sum out of range, more than 256 viewpoints, a value that "
                         "is not finite or a line_rel outside (0, 1])")
    return nrm, curv[0], cls.value


COMPONENT_DTYPE = np.dtype(_lib.HskComponent)
COMPONENT_NONE = 0xFFFFFFFF
PRUNE_UNSEEN, PRUNE_FREE = 0, 1
PRUNE_FIELDS = ("min_voxels", "keep_largest", "fill")
_PRUNE = (_lib.HskPruneParams, "hsk_default_prune_params", PRUNE_FIELDS, "prune parameters have no field")


def default_prune_params(tracker=None, **fields):
    """the parameters of prune_components (hsk_default_prune_params): min_voxels = the voxels of a cube of edge four truncation
    distances of the tracker (without one: the default configuration's), keep_largest 0 (no limit), fill PRUNE_UNSEEN; the
    keywords -- min_voxels, keep_largest, fill -- override its fields -> an `_lib.HskPruneParams`"""
    return _params(_PRUNE, tracker, None, fields)


FILL_SURFACE, FILL_ALL = 0, 1
FILL_FIELDS = ("iterations", "keep", "band", "fill_weight")
_FILL = (_lib.HskFillParams, "hsk_default_fill_params", FILL_FIELDS, "fill parameters have no field")
DIFF_UNSEEN, DIFF_ONLY_REF, DIFF_ONLY_CUR, DIFF_SAME, DIFF_APPEARED, DIFF_VANISHED, DIFF_MINOR = range(7)
ADOPT_APPEARED, ADOPT_VANISHED = 1, 2
DIFF_FIELDS = ("thresh", "min_weight", "min_voxels")
_DIFF = (_lib.HskDiffParams, "hsk_default_diff_params", DIFF_FIELDS, "diff parameters have no field")
ADOPT_FIELDS = ("which", "halo")
DIFF_REGION_DTYPE = np.dtype(_lib.HskDiffRegion)


def default_diff_params(tracker=None, **fields):
    """the parameters of diff_volume (hsk_default_diff_params): thresh 16384 (half the truncation distance), min_weight 1,
    min_voxels = default_prune_params' value for the tracker (without one: the default configuration's); the keywords -- thresh,
    min_weight, min_voxels -- override its fields -> an `_lib.HskDiffParams`"""
    return _params(_DIFF, tracker, None, fields)


SPLIT_NONE, SPLIT_FLOOR, SPLIT_CEILING, SPLIT_WALL, SPLIT_OTHER, SPLIT_OBJECT, SPLIT_MINOR = range(7)
KIND_FLOOR, KIND_CEILING, KIND_WALL, KIND_OTHER = 1, 2, 3, 4
REMOVE_ERASE, REMOVE_RESTORE = 0, 1
SPLIT_FIELDS = ("dist_m", "back_m", "cos_min", "min_voxels")
REMOVE_FIELDS = ("mode", "halo", "fill_weight")
_SPLIT = (_lib.HskSplitParams, "hsk_default_split_params", SPLIT_FIELDS, "split parameters have no field")
_REMOVE = (_lib.HskRemoveParams, "hsk_default_remove_params", REMOVE_FIELDS, "remove parameters have no field")
SPLIT_PLANE_DTYPE = np.dtype(_lib.HskSplitPlane)
OBJECT_DTYPE = np.dtype(_lib.HskObject)


def default_split_params(tracker=None, **fields):
    """the parameters of split_scene (hsk_default_split_params): dist_m 0.04, back_m = the truncation distance + 0.04, cos_min
    cos 30 deg, min_voxels = default_prune_params' value for the tracker (without one: the default configuration's); the keywords
    -- dist_m, back_m, cos_min, min_voxels -- override its fields -> an `_lib.HskSplitParams`"""
    return _params(_SPLIT, tracker, None, fields)


def default_remove_params(tracker=None, **fields):
    """the parameters of remove_objects (hsk_default_remove_params): REMOVE_RESTORE, halo = clamp(ceil(tau / the smallest cell) + 1,
    1, 8), fill_weight 1; the keywords -- mode, halo, fill_weight -- override its fields -> an `_lib.HskRemoveParams`"""
    return _params(_REMOVE, tracker, None, fields)


def split_planes(abcd, kinds=KIND_OTHER):
    """n planes [n, 4] (a plane_record array's "abcd" will do) with their kinds (one, or n) -> a SPLIT_PLANE_DTYPE array"""
    a = np.asarray(abcd, np.float32).reshape(-1, 4)
    out = np.zeros(len(a), SPLIT_PLANE_DTYPE)
    out["abcd"] = a
    out["kind"] = kinds
    return out


def split_plane_kinds(planes, up, level_cos=None, wall_sin=None):
    """sets the kinds of a SPLIT_PLANE_DTYPE array (or of planes [n, 4]) from the up direction (hsk_split_plane_kinds; host only):
    KIND_FLOOR where the normal lies within level_cos (default cos 15 deg) of up, KIND_CEILING of -up, KIND_WALL within wall_sin
    (default sin 15 deg) of the horizon, else KIND_OTHER; up is minus row 1 of an upright frame's level matrix -> the array"""
    pl = np.ascontiguousarray(planes if getattr(planes, "dtype", None) == SPLIT_PLANE_DTYPE else split_planes(planes)).copy()
    u = (C.c_float * 3)(*[float(v) for v in up])
    lc = float(np.cos(np.radians(15.0))) if level_cos is None else float(level_cos)
    ws = float(np.sin(np.radians(15.0))) if wall_sin is None else float(wall_sin)
    rc = _lib.load().hsk_split_plane_kinds(pl.ctypes.data_as(C.POINTER(_lib.HskSplitPlane)) if len(pl) else None, len(pl), u, lc, ws)
    if rc != 0:
        raise KinfuError(f"hsk_split_plane_kinds failed ({rc}): {_lib.load().hsk_last_error(None).decode()}")
    return pl


def default_fill_params(tracker=None, **fields):
    """the parameters of fill_holes (hsk_default_fill_params): iterations = the voxels of 15 cm along the tracker's finest axis
    (without a tracker: the default configuration's), clamped to 1..255 -- gaps up to about 30 cm across close --, keep
    FILL_SURFACE, band 2, fill_weight 1; the keywords -- iterations, keep, band, fill_weight -- override its fields -> an
    `_lib.HskFillParams`"""
    return _params(_FILL, tracker, None, fields)


CLEAR_UNKNOWN = 1
CLEARANCE_FAR, CLEARANCE_OUTSIDE = 0xFFFFFFFF, 0xFFFFFFFE
CLEARANCE_FIELDS = ("weight", "max_d2", "flags", "unit_m")
_CLEARANCE = (_lib.HskClearanceParams, "hsk_default_clearance_params", CLEARANCE_FIELDS, "clearance parameters have no field")


def default_clearance_params(tracker=None, **fields):
    """the parameters of the clearance calls (hsk_default_clearance_params): flags CLEAR_UNKNOWN; the weights that make the
    metric the cells' -- (1, 1, 1) with unit_m = the cell for cubic cells, else rint(16 (cell / cell_min)^2) with unit_m =
    cell_min / 4 -- and max_d2 = one metre (without a tracker: the default configuration's); the keywords -- weight, max_d2,
    flags, unit_m -- override its fields -> an `_lib.HskClearanceParams`"""
    return _params(_CLEARANCE, tracker, None, fields)


def clearance_d2(params, metres):
    """the squared distance, in the field's units, of a distance in metres: ceil((metres / unit_m)^2), saturating at 0xFFFFFFFF
    (hsk_clearance_d2; host only)"""
    return int(_lib.load().hsk_clearance_d2(C.byref(params), float(metres)))


def clearance_metres(params, d2):
    """the field's values as metres: sqrt(d2) * unit_m, inf where the value is CLEARANCE_FAR, nan where CLEARANCE_OUTSIDE"""
    d = np.asarray(d2, np.uint32)
    out = np.sqrt(d.astype(np.float64)) * float(params.unit_m)
    out = np.where(d == CLEARANCE_FAR, np.inf, out)
    return np.where(d == CLEARANCE_OUTSIDE, np.nan, out)


REACH_UNREACHED, REACH_OUTSIDE, REACH_BLOCKED = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
REACH_MAX_COST = 0xF0000000
REACH_FIELDS = ("min_d2", "max_cost")
_REACH = (_lib.HskReachParams, "hsk_default_reach_params", REACH_FIELDS, "reach parameters have no field")


def default_reach_params(tracker=None, clearance=None, **fields):
    """the parameters of the reach calls (hsk_default_reach_params) for the clearance parameters `clearance` (None: the tracker's
    defaults): min_d2 = clearance_d2(clearance, 0.3) -- a person's half width -- clamped to its max_d2, max_cost = REACH_MAX_COST;
    the keywords -- min_d2, max_cost -- override its fields -> an `_lib.HskReachParams`"""
    return _params(_REACH, tracker, None, fields, (clearance,))


def reach_metres(params, g):
    """the reach field's values as metres: g * unit_m / 16 of the clearance parameters `params`, nan for the three markers
    (hsk_reach_metres, element by element)"""
    v = np.asarray(g, np.uint32)
    with np.errstate(invalid="ignore"):
        out = (v.astype(np.float64) * np.float64(np.float32(params.unit_m)) / 16.0).astype(np.float32)
    return np.where(v > REACH_MAX_COST, np.float32(np.nan), out)


def rank_views_reach(scores, eye_g, max_g=REACH_MAX_COST):
    """rank_views' order with the poses nobody can walk to behind all others: those whose eye_g -- reach_at of the camera centres --
    is REACH_UNREACHED, REACH_BLOCKED, REACH_OUTSIDE or above max_g (hsk_rank_views_reach; host only) -> indices [n] uint32"""
    s = np.ascontiguousarray(scores, VIEW_SCORE_DTYPE)
    d = np.ascontiguousarray(eye_g, np.uint32).reshape(-1)
    if len(d) != len(s):
        raise ValueError("rank_views_reach: one eye_g per score")
    order = np.empty(len(s), np.uint32)
    if len(s) and _lib.load().hsk_rank_views_reach(s.ctypes.data_as(C.POINTER(_lib.HskViewScore)), d.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   int(max_g), len(s), order.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
        raise KinfuError("rank_views_reach failed")
    return order


ROOM_UNASSIGNED, ROOM_OUTSIDE, ROOM_BLOCKED, ROOM_NONE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
PARTITION_MAX_ROOMS = 1024
PARTITION_FIELDS = ("core_d2", "min_d2", "min_core_voxels", "max_cost")
_PARTITION = (_lib.HskPartitionParams, "hsk_default_partition_params", PARTITION_FIELDS, "partition parameters have no field")
ROOM_DTYPE = np.dtype(_lib.HskRoom)
DOOR_DTYPE = np.dtype(_lib.HskDoor)


def default_partition_params(tracker=None, clearance=None, **fields):
    """the parameters of the partition calls (hsk_default_partition_params) for the clearance parameters `clearance` (None: the
    tracker's defaults): core_d2 = clearance_d2(clearance, 0.5) clamped to its max_d2, min_d2 = 1, min_core_voxels = the voxels of a
    cube of edge 0.25 m, max_cost = REACH_MAX_COST; the keywords -- core_d2, min_d2, min_core_voxels, max_cost -- override its
    fields -> an `_lib.HskPartitionParams`"""
    return _params(_PARTITION, tracker, None, fields, (clearance,))


def merge_rooms(doors, n_rooms, merge_d2):
    """the caller's remedy for a room that got two cores: per room the smallest id of its class under the union of all pairs whose
    door has max_d2 >= merge_d2 (hsk_merge_rooms; host only; doors: a DOOR_DTYPE array) -> [n_rooms] uint32"""
    d = np.ascontiguousarray(doors, DOOR_DTYPE).reshape(-1)
    out = np.empty(int(n_rooms), np.uint32)
    if _lib.load().hsk_merge_rooms(d.ctypes.data if len(d) else None, len(d), int(n_rooms), int(merge_d2), out.ctypes.data if n_rooms else None) != 0:
        raise KinfuError("merge_rooms: a door names a room that is not below n_rooms")
    return out


def rank_views_clear(scores, eye_d2, min_d2):
    """rank_views' order with the poses nobody can stand in behind all others: those whose eye_state is not 0 (free), whose eye_d2
    -- clearance_at of the camera centres -- is below min_d2 or is CLEARANCE_OUTSIDE (hsk_rank_views_clear; host only) ->
    indices [n] uint32"""
    s = np.ascontiguousarray(scores, VIEW_SCORE_DTYPE)
    d = np.ascontiguousarray(eye_d2, np.uint32).reshape(-1)
    if len(d) != len(s):
        raise ValueError("rank_views_clear: one eye_d2 per score")
    order = np.empty(len(s), np.uint32)
    if len(s) and _lib.load().hsk_rank_views_clear(s.ctypes.data_as(C.POINTER(_lib.HskViewScore)), d.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                   int(min_d2), len(s), order.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
        raise KinfuError("rank_views_clear failed")
    return order


SIMPLIFY_QUADRIC, SIMPLIFY_MEAN = 0, 1
SIMPLIFY_STATS_FIELDS = ("n_in_vertices", "n_in_faces", "n_clusters", "n_out_vertices", "n_out_faces", "n_faces_collapsed", "n_rank",
                         "n_clamped", "n_uncolored")


def simplify_stats_dict(st):
    """an `_lib.HskSimplifyStats` as a dict of ints (n_rank: a list of four)"""
    return {name: ([int(v) for v in getattr(st, name)] if name == "n_rank" else int(getattr(st, name))) for name in SIMPLIFY_STATS_FIELDS}


def cluster_vertex(sums16, cluster_voxels=4, mode=SIMPLIFY_QUADRIC, sv_floor=0.0):
    """a cluster's representative vertex from its 16 integer sums (hsk_cluster_vertex; host only, the device solve's mirror):
    n, sum p (3), sum N (3), sum N N^T (xx xy xz yy yz zz), sum N dN (3), positions in 1/256 voxel relative to the centre of the
    cluster's cell -> (xyz [3] float64 in voxels relative to that centre, rank, clamped)"""
    s = np.ascontiguousarray(sums16, np.int64).reshape(16)
    xyz, rank, clamped = np.zeros(3, np.float64), C.c_int(), C.c_int()
    if _lib.load().hsk_cluster_vertex(s.ctypes.data_as(C.POINTER(C.c_int64)), cluster_voxels, mode, sv_floor,
                                      xyz.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rank), C.byref(clamped)) != 0:
        raise KinfuError("cluster_vertex: invalid arguments (n <= 0, a cluster size outside 2, 4, 8, 16, an unknown mode or an sv_floor outside [0, 1))")
    return xyz, rank.value, bool(clamped.value)


TEXEL_OWNED, TEXEL_INSIDE, TEXEL_PROJECTED, TEXEL_COLORED, TEXEL_NORMAL = (_lib.HSK_TEXEL_OWNED, _lib.HSK_TEXEL_INSIDE, _lib.HSK_TEXEL_PROJECTED,
                                                                             _lib.HSK_TEXEL_COLORED, _lib.HSK_TEXEL_NORMAL)
TEXTURE_INFO_FIELDS = ("width", "height", "n_faces_charted", "n_faces_skipped", "n_blocks", "n_owned", "n_inside", "n_projected", "n_colored", "n_normal")
TEXTURE_CHART_DTYPE = np.dtype(_lib.HskTextureChart)


def texture_info_dict(info):
    return {name: ([int(v) for v in getattr(info, name)] if name == "n_blocks" else int(getattr(info, name))) for name in TEXTURE_INFO_FIELDS}


def _texture_mesh(vertices, faces):
    return np.ascontiguousarray(vertices, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


def texture_layout(vertices, faces, texels_per_metre, atlas_width=0):
    """the atlas layout of an indexed triangle mesh (hsk_texture_layout; host only, needs no device): two faces to a block of 8,
    16, 32 or 64 texels by their longest edge at `texels_per_metre`, blocks in Morton order inside 64 x 64 super-tiles across
    `atlas_width` (0: 1024) -> dict: uv [m, 3, 2] float32 in the faces' corner order (v = 1 at the images' top row), charts
    [m] TEXTURE_CHART_DTYPE (-1: a skipped face), and hsk_texture_info's fields (the texel counts are a bake's)"""
    v, f = _texture_mesh(vertices, faces)
    uv, charts, info = np.zeros((len(f), 3, 2), np.float32), np.zeros(len(f), TEXTURE_CHART_DTYPE), _lib.HskTextureInfo()
    lib = _lib.load()
    if lib.hsk_texture_layout(v.ctypes.data, len(v), f.ctypes.data, len(f), texels_per_metre, atlas_width, uv.ctypes.data, charts.ctypes.data,
                              C.byref(info)) != 0:
        raise KinfuError((lib.hsk_last_error(None) or b"hsk_texture_layout failed").decode())
    return dict(texture_info_dict(info), uv=uv, charts=charts)


TEXEL_KEYFRAME, KEYTEX_BEST, KEYTEX_BLEND, KEYTEX_NONE = _lib.HSK_TEXEL_KEYFRAME, _lib.HSK_KEYTEX_BEST, _lib.HSK_KEYTEX_BLEND, _lib.HSK_KEYTEX_NONE
KEYTEX_INFO_FIELDS = ("n_keyframes", "n_keyed", "n_fallback", "n_uncolored", "n_pairs_seen", "n_pairs_occluded")


def keyframe_wanted(poses, pose, min_translation_m=0.3, min_angle_rad=0.3490658503988659):   # (20 degrees)
    """the host's keyframe selection rule (hsk_keyframe_wanted; no device): True when `poses` ([n, 4, 4], the keyframes kept so far) is
    empty or every one of them differs from `pose` by more than min_translation_m in position or by more than min_angle_rad in rotation"""
    ps = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    r = _lib.load().hsk_keyframe_wanted(ps.ctypes.data if len(ps) else None, len(ps), p.ctypes.data, min_translation_m, min_angle_rad)
    if r < 0:
        raise KinfuError("keyframe_wanted: the thresholds must be finite and not negative")
    return bool(r)


def rank_views(scores):
    """the order of a score_views result: larger gain first; ties to the larger n_frontier, then to the lower index; the poses
    whose eye_state is not 0 (free) behind all others (hsk_rank_views; host only) -> indices [n] uint32"""
    s = np.ascontiguousarray(scores, VIEW_SCORE_DTYPE)
    order = np.empty(len(s), np.uint32)
    if len(s) and _lib.load().hsk_rank_views(s.ctypes.data_as(C.POINTER(_lib.HskViewScore)), len(s), order.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
        raise KinfuError("rank_views failed")
    return order


def plane_refit(sums10, prev_abcd):
    """one refit of a plane from its inliers' integer moments (hsk_plane_refit; host only): sums10 = count, sums of q (3), sums
    of q_a q_b (xx xy xz yy yz zz) with q = rint(coordinate * 4096) -> (abcd [4] float32, ok)"""
    s = np.ascontiguousarray(sums10, np.int64).reshape(10)
    prev = np.ascontiguousarray(prev_abcd, np.float32).reshape(4)
    out, ok = np.zeros(4, np.float32), C.c_int()
    if _lib.load().hsk_plane_refit(s.ctypes.data_as(C.POINTER(C.c_int64)), _fp(prev), _fp(out), C.byref(ok)) != 0:
        raise KinfuError("plane_refit: invalid arguments (a count outside 0..2^24 or a sum outside +-2^62)")
    return out, bool(ok.value)


def pose_lattice(centre, step_m, n_trans, step_rad, n_rot):
    """candidate poses around `centre` [4, 4]: centre . T(i, j, k) step_m . Ry(a step_rad) . Rx(b step_rad) for i, j, k in
    [-n_trans, n_trans] and a, b in [-n_rot, n_rot], offsets in the camera's own frame (hsk_pose_lattice; host only)
    -> [n, 4, 4] float32, i slowest, b fastest"""
    lib = _lib.load()
    c = np.ascontiguousarray(centre, np.float32).reshape(16)
    n = C.c_size_t()
    if lib.hsk_pose_lattice(_fp(c), step_m, int(n_trans), step_rad, int(n_rot), None, 0, C.byref(n)) != 0:
        raise KinfuError("pose_lattice: invalid arguments (negative counts, non-finite steps or more than 65536 poses)")
    out = np.empty((n.value, 16), np.float32)
    if lib.hsk_pose_lattice(_fp(c), step_m, int(n_trans), step_rad, int(n_rot), out.ctypes.data, n.value, C.byref(n)) != 0:
        raise KinfuError("pose_lattice failed")
    return out.reshape(-1, 4, 4)


def rank_scores(scores):
    """the order of a score_cloud result: key = n_near - n_free - n_behind, larger first; ties to the smaller sum_abs, then to
    the lower index (hsk_rank_scores; host only) -> indices [n] uint32"""
    s = np.ascontiguousarray(scores, SCORE_DTYPE)
    order = np.empty(len(s), np.uint32)
    if len(s) and _lib.load().hsk_rank_scores(s.ctypes.data_as(C.POINTER(_lib.HskPoseScore)), len(s), order.ctypes.data_as(C.POINTER(C.c_uint32))) != 0:
        raise KinfuError("rank_scores failed")
    return order


class KinfuTracker:
    """One TSDF volume + tracker on one MI355X (one `hsk_ctx`)."""

    def __init__(self, cfg=None, **over):
        self.lib = _lib.load()
        self.cfg = cfg if cfg is not None else default_config(**over)
        h = C.c_void_p()
        rc = self.lib.hsk_create(C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise KinfuError(f"hsk_create failed ({rc}): {self.lib.hsk_last_error(None).decode()}")
        self.h = h
        self.w, self.hgt = self.cfg.width, self.cfg.height
        z0, nz = C.c_int(), C.c_int()
        self.lib.hsk_stored_planes(self.h, C.byref(z0), C.byref(nz))
        self.stored_z0, self.stored_nz = z0.value, nz.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.hsk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise KinfuError(f"hskinfu error {rc}: {self.lib.hsk_last_error(self.h).decode()}")

    @staticmethod
    def _depth(depth):
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        if d.ndim != 2:
            raise KinfuError("depth must be a (h, w) uint16 array")
        return d

    # ---- whole tracker step -------------------------------------------------------------------------
    def process_frame(self, depth):
        d = self._depth(depth)
        pose = np.empty(16, np.float32)
        tracked = C.c_int()
        self._ck(self.lib.hsk_process_frame(self.h, d.ctypes.data, d.shape[1], d.shape[0], _fp(pose), C.byref(tracked)))
        return pose.reshape(4, 4), bool(tracked.value)

    def process_frame_dev(self, depth_dev_ptr):
        pose = np.empty(16, np.float32)
        tracked = C.c_int()
        self._ck(self.lib.hsk_process_frame_dev(self.h, C.c_void_p(depth_dev_ptr), self.w, self.hgt, _fp(pose),
                                                C.byref(tracked)))
        return pose.reshape(4, 4), bool(tracked.value)

    def submit_frame_dev(self, depth_dev_ptr):
        """enqueue a frame (device pointer) without waiting; collect poses in order with wait_frame()"""
        self._ck(self.lib.hsk_submit_frame_dev(self.h, C.c_void_p(depth_dev_ptr), self.w, self.hgt))

    def submit_frame(self, depth):
        """enqueue a frame held in host memory (copied before this returns); collect poses in order with wait_frame()"""
        d = self._depth(depth)
        self._ck(self.lib.hsk_submit_frame(self.h, d.ctypes.data, d.shape[1], d.shape[0]))

    def wait_frame(self):
        pose = np.empty(16, np.float32)
        tracked = C.c_int()
        self._ck(self.lib.hsk_wait_frame(self.h, _fp(pose), C.byref(tracked)))
        return pose.reshape(4, 4), bool(tracked.value)

    def track_stream(self, reader, first=0, count=None):
        """frames [first, first + count) of a recorded stream (products.DepthStreamReader) through the tracker, the
        frame feed running inside the library (hsk_track_stream) -> (poses [count, 4, 4], tracked [count] bool)"""
        if count is None:
            count = len(reader) - first
        poses = np.empty((count, 16), np.float32)
        tracked = np.zeros(count, np.int32)
        self._ck(self.lib.hsk_track_stream(self.h, reader.h, int(first), int(count), _fp(poses), tracked.ctypes.data_as(C.POINTER(C.c_int))))
        return poses.reshape(count, 4, 4), tracked.astype(bool)

    def flush_weights(self):
        """write the deferred free-space weights back into the volume (what a read-out does first); enqueued only"""
        self._ck(self.lib.hsk_flush_weights(self.h))

    def product_capacity(self):
        """the product buffer's size in bytes as it stands (hsk_product_capacity): it only grows"""
        return int(self.lib.hsk_product_capacity(self.h))

    def prepare_readout(self, product_bytes=0):
        """allocate now what a read-out would allocate on its first use (pinned staging, row tables, product buffer)"""
        self._ck(self.lib.hsk_prepare_readout(self.h, int(product_bytes)))

    def reset(self):
        self._ck(self.lib.hsk_reset(self.h))

    # ---- stages ------------------------------------------------------------------------------------
    def integrate(self, depth, pose):
        d = self._depth(depth)
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self._ck(self.lib.hsk_integrate(self.h, d.ctypes.data, d.shape[1], d.shape[0], _fp(p)))

    def count_updates(self, depth, pose):
        d = self._depth(depth)
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        n = C.c_uint64()
        self._ck(self.lib.hsk_count_updates(self.h, d.ctypes.data, d.shape[1], d.shape[0], _fp(p), C.byref(n)))
        return n.value

    def integrate_coarse_counts(self):
        """verdicts of the last integrate's coarse level over the wave-chunks: (mixed, settled as a whole, free but worked by
        pass A, chunks currently quiet)"""
        c = (C.c_uint64 * 4)()
        self._ck(self.lib.hsk_integrate_coarse_counts(self.h, c))
        return tuple(int(x) for x in c)

    def integrate_queue_entries(self):
        """lane-blocks the last integrate's classification pass handed to its per-voxel pass"""
        n = C.c_uint64()
        self._ck(self.lib.hsk_integrate_queue_entries(self.h, C.byref(n)))
        return n.value

    def submit_host_us(self, reset=False):
        """host microseconds the pipelined submissions have spent by phase (staging copy, upload + preprocessing enqueue, wait
        for the preprocessing, main chain enqueue) and their count"""
        us = (C.c_double * 4)()
        n = C.c_uint64()
        self._ck(self.lib.hsk_submit_host_us(self.h, us, C.byref(n), int(reset)))
        return list(us), n.value

    def integrate_light_entries(self):
        """lane-blocks of the last integrate's light class (free space with holes in the depth image under it)"""
        n = C.c_uint64()
        self._ck(self.lib.hsk_integrate_light_entries(self.h, C.byref(n)))
        return n.value

    def raycast(self, pose, want_keys=False):
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        v = np.empty((3, self.hgt, self.w), np.float32)
        n = np.empty((3, self.hgt, self.w), np.float32)
        keys = np.empty((self.hgt, self.w), np.int32) if want_keys else None
        self._ck(self.lib.hsk_raycast(self.h, _fp(p), v.ctypes.data, n.ctypes.data, keys.ctypes.data if want_keys else None))
        return (v, n, keys) if want_keys else (v, n)

    def preprocess(self, depth):
        d = self._depth(depth)
        self._ck(self.lib.hsk_preprocess(self.h, d.ctypes.data, d.shape[1], d.shape[0]))

    def icp_accumulate(self, level, pose_est, row0=0, row1=None):
        p = np.ascontiguousarray(pose_est, np.float32).reshape(16)
        if row1 is None:
            row1 = self.hgt >> level
        out = np.empty(27, np.float64)
        self._ck(self.lib.hsk_icp_accumulate(self.h, level, _fp(p), row0, row1, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def icp_solve(self, sums27):
        s = np.ascontiguousarray(sums27, np.float64)
        x = np.empty(6, np.float32)
        ok = C.c_int()
        self._ck(self.lib.hsk_icp_solve(s.ctypes.data_as(C.POINTER(C.c_double)), _fp(x), C.byref(ok)))
        return x, bool(ok.value)

    def download_tsdf(self, out=None):
        """the stored planes as a row-major [nz, Y, X, 2] int16 array (into `out` when given: no fresh pages to fault in)"""
        if out is None:
            out = np.empty((self.stored_nz, self.cfg.vol_y, self.cfg.vol_x, 2), np.int16)
        want = self.stored_nz * self.cfg.vol_y * self.cfg.vol_x * 2
        if not (isinstance(out, np.ndarray) and out.dtype == np.int16 and out.flags.c_contiguous and out.flags.writeable and out.size == want):
            raise ValueError(f"download_tsdf(out=...): a writeable C-contiguous int16 array of {want} elements is needed (the C side takes a bare pointer)")
        self._ck(self.lib.hsk_download_tsdf(self.h, out.ctypes.data))
        return out

    def upload_tsdf(self, vol):
        v = np.ascontiguousarray(vol, np.int16)
        if v.size != self.stored_nz * self.cfg.vol_y * self.cfg.vol_x * 2:
            raise ValueError(f"upload_tsdf: {self.stored_nz * self.cfg.vol_y * self.cfg.vol_x * 2} int16 elements are needed, got {v.size}")
        self._ck(self.lib.hsk_upload_tsdf(self.h, v.ctypes.data))

    def get_pose(self):
        p = np.empty(16, np.float32)
        self._ck(self.lib.hsk_get_pose(self.h, _fp(p)))
        return p.reshape(4, 4)

    def set_pose(self, pose):
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self._ck(self.lib.hsk_set_pose(self.h, _fp(p)))

    def download_map(self, kind, level):
        out = np.empty((3, self.hgt >> level, self.w >> level), np.float32)
        self._ck(self.lib.hsk_download_map(self.h, kind, level, out.ctypes.data))
        return out

    def upload_map(self, kind, level, arr):
        a = np.ascontiguousarray(arr, np.float32)
        self._ck(self.lib.hsk_upload_map(self.h, kind, level, a.ctypes.data))

    def download_depth_level(self, level):
        out = np.empty((self.hgt >> level, self.w >> level), np.uint16)
        self._ck(self.lib.hsk_download_depth_level(self.h, level, out.ctypes.data))
        return out

    def download_scaled_depth(self):
        out = np.empty((self.hgt, self.w), np.float32)
        self._ck(self.lib.hsk_download_scaled_depth(self.h, out.ctypes.data))
        return out

    def extract_cloud(self, cap=None):
        n = C.c_size_t()
        self._ck(self.lib.hsk_extract_cloud(self.h, None, 0, C.byref(n)))
        total = n.value
        m = total if cap is None else min(cap, total)
        out = np.empty((m, 3), np.float32)
        if m:
            self._ck(self.lib.hsk_extract_cloud(self.h, out.ctypes.data, m, C.byref(n)))
        return out, total

    def extract_mesh(self, cap=None, cubes=False):
        """TSDF zero level set as triangles [n, 3, 3], voxel order -> (triangles, total): marching tetrahedra, or
        (cubes=True) marching cubes, the form upstream's .ply export has"""
        fn = self.lib.hsk_extract_mesh_cubes if cubes else self.lib.hsk_extract_mesh
        n = C.c_size_t()
        self._ck(fn(self.h, None, 0, C.byref(n)))
        total = n.value
        m = total if cap is None else min(cap, total)
        out = np.empty((m, 3, 3), np.float32)
        if m:
            self._ck(fn(self.h, out.ctypes.data, m, C.byref(n)))
        return out, total

    # ---- colour (RGB-D; opt-in) ---------------------------------------------------------------------
    def _rgb(self, rgb):
        c = np.ascontiguousarray(rgb, dtype=np.uint8)
        if c.shape != (self.hgt, self.w, 3):
            raise KinfuError(f"rgb must be a ({self.hgt}, {self.w}, 3) uint8 array registered to the depth grid")
        return c

    def enable_color(self, max_weight=0, band_m=0.0):
        """allocate and zero the colour volume (4 B per stored voxel); max_weight 1..255 (0: 64), band_m <= 0: 2 cells"""
        self._ck(self.lib.hsk_enable_color(self.h, int(max_weight), C.c_float(band_m)))

    def process_frame_rgbd(self, depth, rgb):
        d, c = self._depth(depth), self._rgb(rgb)
        pose = np.empty(16, np.float32)
        tracked = C.c_int()
        self._ck(self.lib.hsk_process_frame_rgbd(self.h, d.ctypes.data, c.ctypes.data, d.shape[1], d.shape[0], _fp(pose), C.byref(tracked)))
        return pose.reshape(4, 4), bool(tracked.value)

    def submit_frame_rgbd(self, depth, rgb):
        """submit_frame with the frame's colour image (both copied before this returns); collect with wait_frame()"""
        d, c = self._depth(depth), self._rgb(rgb)
        self._ck(self.lib.hsk_submit_frame_rgbd(self.h, d.ctypes.data, c.ctypes.data, d.shape[1], d.shape[0]))

    def integrate_color(self, depth, rgb, pose):
        """stage level: the colour update of one frame at `pose` (the TSDF is untouched)"""
        d, c = self._depth(depth), self._rgb(rgb)
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self._ck(self.lib.hsk_integrate_color(self.h, d.ctypes.data, c.ctypes.data, d.shape[1], d.shape[0], _fp(p)))

    def download_color(self):
        """the colour volume as a row-major [nz, Y, X, 4] uint8 array of (r, g, b, w)"""
        out = np.empty((self.stored_nz, self.cfg.vol_y, self.cfg.vol_x, 4), np.uint8)
        self._ck(self.lib.hsk_download_color(self.h, out.ctypes.data))
        return out

    def upload_color(self, rgbw):
        a = np.ascontiguousarray(rgbw, np.uint8)
        if a.size != self.stored_nz * self.cfg.vol_y * self.cfg.vol_x * 4:
            raise ValueError(f"upload_color: {self.stored_nz * self.cfg.vol_y * self.cfg.vol_x * 4} uint8 elements are needed, got {a.size}")
        self._ck(self.lib.hsk_upload_color(self.h, a.ctypes.data))

    def extract_cloud_attrs(self, cap=None, normals=True, rgb=True):
        """extract_cloud with normals [n, 3] float32 (NaN near the volume's rim) and colours [n, 3] uint8 ->
        (xyz, normals or None, rgb or None, total, n_uncolored)"""
        n, nu = C.c_size_t(), C.c_size_t()
        self._ck(self.lib.hsk_extract_cloud_attrs(self.h, None, None, None, 0, C.byref(n), None))
        total = n.value
        m = total if cap is None else min(cap, total)
        xyz = np.empty((m, 3), np.float32)
        nrm = np.empty((m, 3), np.float32) if normals else None
        col = np.empty((m, 3), np.uint8) if rgb else None
        if m:
            self._ck(self.lib.hsk_extract_cloud_attrs(self.h, xyz.ctypes.data, None if nrm is None else nrm.ctypes.data,
                                                      None if col is None else col.ctypes.data, m, C.byref(n), C.byref(nu)))
        return xyz, nrm, col, total, nu.value

    def extract_mesh_indexed(self, normals=True, rgb=True):
        """extract_mesh(cubes=True)'s surface as an indexed mesh welded on the device by edge identity ->
        (vertices [n, 3] float32, faces [m, 3] int32, normals [n, 3] float32 or None, rgb [n, 3] uint8 or None, n_uncolored);
        vertices[faces] is the triangle soup bit for bit.  rgb=True needs enable_color()."""
        nu = C.c_size_t()
        return self._indexed_mesh("extract_mesh_indexed", normals, rgb, lambda first, *a: self.lib.hsk_extract_mesh_indexed(
            self.h, *a, None if first else C.byref(nu))) + (nu.value,)

    def _indexed_mesh(self, who, normals, rgb, call):
        """the size query and the fill of an indexed mesh: call(first, vertices, normals, rgb, their capacity, nv, faces, their
        capacity, nf) -> (vertices [n, 3] float32, faces [m, 3] int32, normals [n, 3] float32 or None, rgb [n, 3] uint8 or None)"""
        nv, nf = C.c_size_t(), C.c_size_t()
        self._ck(call(True, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf)))
        verts = np.empty((nv.value, 3), np.float32)
        faces = np.empty((nf.value, 3), np.int32)
        nrm = np.empty((nv.value, 3), np.float32) if normals else None
        col = np.empty((nv.value, 3), np.uint8) if rgb else None
        self._ck(call(False, verts.ctypes.data, None if nrm is None else nrm.ctypes.data, None if col is None else col.ctypes.data, len(verts),
                      C.byref(nv), faces.ctypes.data, len(faces), C.byref(nf)))
        if (nv.value, nf.value) != (len(verts), len(faces)):
            raise KinfuError(f"{who}: the counts changed between the two calls")
        return verts, faces, nrm, col

    def extract_mesh_simplified(self, cluster_voxels=4, mode=SIMPLIFY_QUADRIC, normals=True, rgb=False, sv_floor=0.0):
        """extract_mesh_indexed's surface reduced on the device by quadric vertex clustering on cells of `cluster_voxels` (2, 4, 8
        or 16) voxels (hsk_extract_mesh_simplified): one vertex per cell, placed by the quadric of the triangles that touch it
        (mode SIMPLIFY_QUADRIC) or at the mean of its vertices (SIMPLIFY_MEAN); the faces whose corners lie in three different
        cells -> (vertices [n, 3] float32, faces [m, 3] int32, normals [n, 3] float32 or None, rgb [n, 3] uint8 or None, stats:
        a dict of hsk_simplify_stats' fields).  rgb=True needs enable_color()."""
        p = _lib.HskSimplifyParams(cluster_voxels, mode, sv_floor)
        st = _lib.HskSimplifyStats()
        mesh = self._indexed_mesh("extract_mesh_simplified", normals, rgb, lambda first, *a: self.lib.hsk_extract_mesh_simplified(
            self.h, C.byref(p), *a, C.byref(st)))
        return mesh + (simplify_stats_dict(st),)

    # ---- baked textures -------------------------------------------------------------------------------
    def bake_texture(self, vertices, faces, texels_per_metre=0.0, atlas_width=0, n_iter=4, f_tol=0.01, max_offset_m=0.0, rgb=True,
                     normal_rgb=False, mask=True):
        """a colour atlas for an indexed triangle mesh in volume coordinates -- extract_mesh_simplified's, or any other -- baked
        on the device from the volume as it stands (hsk_bake_texture), legal with frames in flight: texture_layout's charts, every
        owned texel projected onto the surface and coloured from the colour volume there.  texels_per_metre 0: one texel per
        voxel; atlas_width 0: 1024; max_offset_m 0: four cells.  -> texture_layout's dict with the texel counts filled and the
        images asked for: rgb (h, w, 3) uint8 (needs enable_color()), normal_rgb (h, w, 3) uint8, mask (h, w) uint8 of TEXEL_* bits."""
        v, f = _texture_mesh(vertices, faces)
        p = _lib.HskTextureParams(texels_per_metre, atlas_width, n_iter, f_tol, max_offset_m)
        args = (self.h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(p))
        base, out = self._bake("bake_texture", len(f), {"rgb": (rgb, 3), "normal_rgb": (normal_rgb, 3), "mask": (mask, 1)},
                               lambda first, images, *a: self.lib.hsk_bake_texture(*args, *images, *a))
        return dict(base, **out)

    def _bake(self, who, n_faces, wanted, call):
        """the size query and the fill of a bake: call(first, the pointers of the images in `wanted`'s order -- name: (asked for,
        channels) --, cap_texels, uv, charts, info) -> (texture_layout's dict, the images asked for by name)"""
        info = _lib.HskTextureInfo()
        self._ck(call(True, [None] * len(wanted), 0, None, None, C.byref(info)))
        w, h = int(info.width), int(info.height)
        out = {k: np.empty((h, w, 3) if ch == 3 else (h, w), np.uint8) for k, (want, ch) in wanted.items() if want}
        uv, charts = np.zeros((n_faces, 3, 2), np.float32), np.zeros(n_faces, TEXTURE_CHART_DTYPE)
        self._ck(call(False, [out[k].ctypes.data if k in out else None for k in wanted], w * h, uv.ctypes.data, charts.ctypes.data, C.byref(info)))
        if (int(info.width), int(info.height)) != (w, h):
            raise KinfuError(f"{who}: the atlas changed size between the two calls")
        return dict(texture_info_dict(info), uv=uv, charts=charts), out

    # ---- keyframe textures ---------------------------------------------------------------------------
    def enable_keyframes(self, cap=64, w=None, h=None):
        """a device store for up to `cap` (1 .. 255) keyframes of w x h pixels (None: the sensor's size) -- hsk_enable_keyframes"""
        self._ck(self.lib.hsk_enable_keyframes(self.h, cap, self.cfg.width if w is None else w, self.cfg.height if h is None else h))

    def add_keyframe(self, depth, rgb, pose=None, intr=None):
        """keep a colour frame with its depth image (uint16 millimetres, 0 invalid: the frame's own, or render_view's depth at the same
        pose), its camera-to-world pose in the volume's frame (None: get_pose()) and fx fy cx cy (None: the sensor's); legal with
        frames in flight -> the keyframe's index"""
        d, c = np.ascontiguousarray(depth, np.uint16), np.ascontiguousarray(rgb, np.uint8)
        if d.ndim != 2 or c.shape != d.shape + (3,):
            raise ValueError("add_keyframe: depth must be (h, w) and rgb (h, w, 3)")
        p = np.ascontiguousarray(self.get_pose() if pose is None else pose, np.float32).reshape(16)
        k = None if intr is None else np.ascontiguousarray(intr, np.float32).reshape(4)
        index = C.c_int()
        self._ck(self.lib.hsk_add_keyframe(self.h, d.ctypes.data, c.ctypes.data, d.shape[1], d.shape[0], p.ctypes.data, None if k is None else k.ctypes.data,
                                           C.byref(index)))
        return index.value

    def keyframe_count(self):
        """-> dict: n, cap, w, h and the store's bytes (all 0 without a store)"""
        n, cap, w, h, b = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
        self._ck(self.lib.hsk_keyframe_count(self.h, C.byref(n), C.byref(cap), C.byref(w), C.byref(h), C.byref(b)))
        return dict(n=n.value, cap=cap.value, w=w.value, h=h.value, bytes=int(b.value))

    def get_keyframe(self, index, images=True):
        """what add_keyframe took -> (pose [4, 4] float32, intr [4] float32, depth (h, w) uint16 or None, rgb (h, w, 3) uint8 or None)"""
        kc = self.keyframe_count()
        pose, intr = np.zeros((4, 4), np.float32), np.zeros(4, np.float32)
        d = np.empty((kc["h"], kc["w"]), np.uint16) if images else None
        c = np.empty((kc["h"], kc["w"], 3), np.uint8) if images else None
        self._ck(self.lib.hsk_get_keyframe(self.h, index, pose.ctypes.data, intr.ctypes.data, None if d is None else d.ctypes.data,
                                           None if c is None else c.ctypes.data))
        return pose, intr, d, c

    def clear_keyframes(self):
        """forget the keyframes, keep the store: the caller's duty when the volume's frame is no longer theirs"""
        self._ck(self.lib.hsk_clear_keyframes(self.h))

    def release_keyframes(self):
        self._ck(self.lib.hsk_release_keyframes(self.h))

    def default_keytex_params(self):
        p = _lib.HskKeytexParams()
        self.lib.hsk_default_keytex_params(self.h, C.byref(p))
        return p

    def bake_texture_keyframes(self, vertices, faces, texels_per_metre=0.0, atlas_width=0, n_iter=4, f_tol=0.01, max_offset_m=0.0, rgb=True,
                               normal_rgb=False, mask=True, source=True, **keytex):
        """bake_texture with the colour from the keyframes (hsk_bake_texture_keyframes): every texel is projected into every keyframe,
        tested against its depth image, and coloured by the keyframe that sees it best (mode=KEYTEX_BEST) or by the weighted mean of
        those within blend_floor of the best (KEYTEX_BLEND).  Needs no enable_color(); with one, texels no keyframe passes take the
        colour volume's colour (fallback_volume).  **keytex: fields of hsk_keytex_params that replace the defaults (mode, z_min_m,
        z_max_m, cos_min, border_px, occlusion_tol_m, blend_floor, fallback_volume) -> bake_texture's dict plus source (h, w) uint8
        (the winning keyframe, KEYTEX_NONE: none) and hsk_keytex_info's fields."""
        v, f = _texture_mesh(vertices, faces)
        p = _lib.HskTextureParams(texels_per_metre, atlas_width, n_iter, f_tol, max_offset_m)
        kp = _override(self.default_keytex_params(), dict(_lib.HskKeytexParams._fields_), "bake_texture_keyframes: hsk_keytex_params has no field", keytex)
        kinfo = _lib.HskKeytexInfo()
        args = (self.h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(p), C.byref(kp))
        base, out = self._bake("bake_texture_keyframes", len(f), {"rgb": (rgb, 3), "normal_rgb": (normal_rgb, 3), "mask": (mask, 1), "source": (source, 1)},
                               lambda first, images, *a: self.lib.hsk_bake_texture_keyframes(*args, *images, *a, None if first else C.byref(kinfo)))
        return dict(base, **{k: int(getattr(kinfo, k)) for k in KEYTEX_INFO_FIELDS}, **out)

    # ---- scene views ----------------------------------------------------------------------------------
    def default_view(self):
        """the sensor's camera following the tracker, Lambert, the light at the camera (an `_lib.HskView` to edit and pass on)"""
        v = _lib.HskView()
        self.lib.hsk_default_view(self.h, C.byref(v))
        return v

    def render_view(self, view=None, *, width=None, height=None, fx=None, fy=None, cx=None, cy=None, pose=None, mode=None,
                    light=None, light_in_camera=None, background=None, rgb=True, depth=True, vmap=False, nmap=False):
        """what has been fused so far as images from a virtual camera (hsk_render_view), legal with frames in flight.  `view`: an
        HskView (default: default_view()); the keywords override its fields.  pose: a 4x4 cam->world matrix for a free camera,
        None (and view.follow) to follow the tracker.  -> dict with the arrays asked for -- rgb (h, w, 3) uint8, depth (h, w)
        uint16 millimetres, vmap / nmap (3, h, w) float32 with NaN = no hit / no normal -- and n_hit, n_uncolored."""
        if view is None:
            view = self.default_view()
        v = _lib.HskView.from_buffer_copy(view)
        _apply_view_fields(v, width, height, fx, fy, cx, cy, pose, mode, light, light_in_camera, background)
        out, ptr = _image_arrays(v.width, v.height, rgb, depth, vmap, nmap)
        nh, nu = C.c_size_t(), C.c_size_t()
        self._ck(self.lib.hsk_render_view(self.h, C.byref(v), ptr("rgb"), ptr("depth"), ptr("vmap"), ptr("nmap"), C.byref(nh), C.byref(nu)))
        out["n_hit"], out["n_uncolored"] = nh.value, nu.value
        return out

    # ---- section views ---------------------------------------------------------------------------------
    def default_section(self):
        """default_view()'s camera as a section: pinhole, a point light, no clip planes, cut colour (255, 96, 0) (an
        `_lib.HskSection` to edit and pass on)"""
        s = _lib.HskSection()
        self.lib.hsk_default_section(self.h, C.byref(s))
        return s

    def render_section(self, section=None, *, width=None, height=None, fx=None, fy=None, cx=None, cy=None, pose=None, mode=None,
                       light=None, light_in_camera=None, background=None, projection=None, light_directional=None, clip=None,
                       cut_rgb=None, rgb=True, depth=True, vmap=False, nmap=False):
        """a floor plan, elevation or dollhouse view of what has been fused so far (hsk_render_section), legal with frames in
        flight.  `section`: an HskSection (default: default_section()); the keywords override its fields, the view's as in
        render_view.  projection: _lib.HSK_PROJ_PINHOLE or HSK_PROJ_ORTHO (fx, fy are then pixels per metre); clip: up to four
        planes (a, b, c, d), keep a x + b y + c z + d >= 0 in world coordinates; light_directional: `light` is a direction
        towards the light.  -> render_view's dict plus n_cut; vmap / nmap are NaN except on shown hits."""
        if section is None:
            section = self.default_section()
        s = _lib.HskSection.from_buffer_copy(section)
        v = s.view
        _apply_view_fields(v, width, height, fx, fy, cx, cy, pose, mode, light, light_in_camera, background)
        if projection is not None:
            s.projection = int(projection)
        if light_directional is not None:
            s.light_directional = int(light_directional)
        if clip is not None:
            planes = np.asarray(clip, np.float32).reshape(-1, 4)
            s.n_clip = len(planes)       # (more than HSK_MAX_CLIP: the call refuses)
            for c, pl in enumerate(planes[:_lib.HSK_MAX_CLIP]):
                s.clip[c][:] = [float(x) for x in pl]
        if cut_rgb is not None:
            s.cut_rgb[:] = [int(x) for x in cut_rgb]
        out, ptr = _image_arrays(v.width, v.height, rgb, depth, vmap, nmap)
        nh, nc, nu = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._ck(self.lib.hsk_render_section(self.h, C.byref(s), ptr("rgb"), ptr("depth"), ptr("vmap"), ptr("nmap"), C.byref(nh),
                                             C.byref(nc), C.byref(nu)))
        out["n_hit"], out["n_cut"], out["n_uncolored"] = nh.value, nc.value, nu.value
        return out

    # ---- volume fusion --------------------------------------------------------------------------------
    def fuse_from(self, src, src_to_dst):
        """resample the volume (and, when both trackers have colour, the colour) of tracker `src` through the rigid 4x4
        matrix `src_to_dst` (p_dst = M p_src, e.g. a room's .xf) into this one and merge by weight, on the device
        (hsk_fuse_volume).  Synchronous; `src` is not changed; this tracker's pose and model maps are not touched (call
        resume_scan(pose) before scanning on).  -> dict(n_fused, n_colored, chunks_total, chunks_swept, box)"""
        m = np.ascontiguousarray(src_to_dst, np.float32).reshape(16)
        st = _lib.HskFuseStats()
        self._ck(self.lib.hsk_fuse_volume(self.h, None if src is None else src.h, _fp(m), C.byref(st)))
        return dict(_stats_dict(st), box=tuple(int(x) for x in st.box))

    # ---- volume alignment -----------------------------------------------------------------------------
    def default_align_params(self):
        """the defaults of align_cloud / align_from as values (an `_lib.HskAlignParams`)"""
        p = _lib.HskAlignParams()
        self.lib.hsk_default_align_params(self.h, C.byref(p))
        return p

    @staticmethod
    def _align_params(probes, over):
        """the keywords into an HskAlignParams (a field left out is 0: its default); probes: to either side, 0 = the point
        itself only (the C field's HSK_ALIGN_DIRECT), None = the default"""
        p = _lib.HskAlignParams()
        if probes is not None:
            p.probes = _lib.HSK_ALIGN_DIRECT if int(probes) == 0 else int(probes)
        return _override(p, [name for name, _ in p._fields_ if name != "probes"], "unknown alignment parameter", over)

    @staticmethod
    def _align_result(out, st):
        n = max(0, min(int(st.iterations), _lib.HSK_ALIGN_MAX_ITERS_CAP))
        return out.reshape(4, 4), {"status": _lib.HSK_ALIGN_STATUS[st.status], "iterations": int(st.iterations), "n_points": int(st.n_points),
                                   "stride": int(st.stride), "n_used": [int(v) for v in st.n_used[:n]],
                                   "rms_m": np.array(st.rms_m[:n], np.float32), "x_last": np.array(st.x_last[:], np.float32),
                                   "sums_last": np.array(st.sums_last[:], np.float64)}

    def align_cloud(self, xyz, normals, src_to_dst, probes=None, **params):
        """refine the rigid 4x4 matrix `src_to_dst` (p_dst = M p_src) so that the points xyz [n, 3] with unit normals [n, 3]
        towards free space (e.g. another tracker's extract_cloud_attrs) lie on this volume's surface (hsk_align_cloud).
        probes: TSDF look-ups to either side along the normal, in steps of the truncation distance (None: 3; 0: none);
        params: the other fields of hsk_align_params (max_iters, cos_gate, max_points, min_points, eps_rot, eps_trans_m,
        max_rot, max_shift_m).  Synchronous; this tracker's volume, pose and model maps are not touched.
        -> (matrix [4, 4] float32, dict(status, iterations, n_points, stride, n_used, rms_m, x_last, sums_last)); the status
        "max_iters" means: do not trust the matrix; "diverged" hands src_to_dst back."""
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(pts) != len(nrm):
            raise ValueError(f"align_cloud: {len(pts)} points but {len(nrm)} normals")
        m = np.ascontiguousarray(src_to_dst, np.float32).reshape(16)
        out, st = np.zeros(16, np.float32), _lib.HskAlignStats()
        p = self._align_params(probes, params)
        self._ck(self.lib.hsk_align_cloud(self.h, pts.ctypes.data if len(pts) else None, nrm.ctypes.data if len(pts) else None, len(pts),
                                          _fp(m), C.byref(p), _fp(out), C.byref(st)))
        return self._align_result(out, st)

    def align_from(self, src, src_to_dst, probes=None, **params):
        """align_cloud with the cloud and normals of tracker `src`'s volume (hsk_align_volume): the matrix to hand to
        fuse_from(src, .)"""
        m = np.ascontiguousarray(src_to_dst, np.float32).reshape(16)
        out, st = np.zeros(16, np.float32), _lib.HskAlignStats()
        p = self._align_params(probes, params)
        self._ck(self.lib.hsk_align_volume(self.h, None if src is None else src.h, _fp(m), C.byref(p), _fp(out), C.byref(st)))
        return self._align_result(out, st)

    # ---- loss hold and relocalisation -----------------------------------------------------------------
    def set_loss_policy(self, policy):
        """what a frame that loses tracking does to the scan: "reset" (the default: the volume is wiped) or "hold" (the frame
        is dropped, the volume and the last tracked pose stay); also the C values (hsk_set_loss_policy)"""
        self._ck(self.lib.hsk_set_loss_policy(self.h, {"reset": _lib.HSK_LOSS_RESET, "hold": _lib.HSK_LOSS_HOLD}.get(policy, policy)))

    def get_loss_policy(self):
        return ("reset", "hold")[self.lib.hsk_get_loss_policy(self.h)]

    @staticmethod
    def _poses(poses):
        p = np.ascontiguousarray(poses, np.float32)
        if p.size % 16:
            raise ValueError("poses must be [n, 4, 4] (or [n, 16]) matrices")
        return p.reshape(-1, 16)

    def score_cloud(self, xyz, poses):
        """how the points xyz [n, 3] (camera coordinates) lie in this volume under each of the poses [m, 4, 4]
        (hsk_score_cloud) -> a structured array [m] with the fields n_near, n_free, n_behind, n_unseen, n_outside,
        n_skipped (uint32) and sum_abs (uint64); rank it with rank_scores"""
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        ps = self._poses(poses)
        out = np.zeros(len(ps), SCORE_DTYPE)
        self._ck(self.lib.hsk_score_cloud(self.h, pts.ctypes.data if len(pts) else None, len(pts), ps.ctypes.data if len(ps) else None, len(ps),
                                          out.ctypes.data_as(C.POINTER(_lib.HskPoseScore)) if len(ps) else None))
        return out

    # ---- scan coverage ----------------------------------------------------------------------------------
    def _probe(self, probe, fields):
        return _params(_PROBE, self, probe, fields)

    def coverage(self, box=None):
        """the census of the volume's observation state (hsk_coverage_census) over the voxels lo <= (x, y, z) < hi of
        box = (lo, hi), None: the whole volume -> dict: n_unseen, n_free, n_solid, n_frontier (ints) and faces [6] uint64, the
        (free voxel, unseen neighbour) pairs by direction -x, +x, -y, +y, -z, +z; legal with frames in flight"""
        c = _lib.HskCoverage()
        self._ck(self.lib.hsk_coverage_census(self.h, _box(self.cfg, box)[0], C.byref(c)))
        return _stats_dict(c)

    def score_views(self, poses, probe=None, **probe_fields):
        """how much never-seen space a camera at each of the poses [m, 4, 4] would reveal (hsk_score_views).  probe: an HskProbe
        (default: default_probe(self)); the keywords override its fields -> a structured array [m] with VIEW_SCORE_DTYPE: n_hit,
        n_frontier, n_open, n_blind, n_outside, eye_state (uint32) and gain (uint64); rank it with rank_views"""
        p = self._probe(probe, probe_fields)
        ps = self._poses(poses)
        out = np.zeros(len(ps), VIEW_SCORE_DTYPE)
        self._ck(self.lib.hsk_score_views(self.h, C.byref(p), ps.ctypes.data if len(ps) else None, len(ps),
                                          out.ctypes.data_as(C.POINTER(_lib.HskViewScore)) if len(ps) else None))
        return out

    def render_coverage(self, pose, probe=None, cls=True, depth=True, gain=True, **probe_fields):
        """the probe's rays from one pose [4, 4], pixel by pixel (hsk_render_coverage) -> dict with the arrays asked for -- cls
        (h, w) uint8 (0 hit, 1 frontier, 2 open, 3 blind, 4 outside), depth (h, w) uint16: the deciding sample's millimetres, gain
        (h, w) uint16 -- and score: a VIEW_SCORE_DTYPE record, score_views' for this pose"""
        p = self._probe(probe, probe_fields)
        m = np.ascontiguousarray(pose, np.float32).reshape(16)
        ok = 1 <= p.width <= 4096 and 1 <= p.height <= 4096   # (otherwise the call itself refuses; nothing is allocated for it here)
        shapes = (("cls", cls, np.uint8), ("depth", depth, np.uint16), ("gain", gain, np.uint16))
        out = {key: np.empty((p.height, p.width), dt) for key, want, dt in shapes if want and ok}
        sc = np.zeros(1, VIEW_SCORE_DTYPE)
        self._ck(self.lib.hsk_render_coverage(self.h, C.byref(p), _fp(m), *(out[key].ctypes.data if key in out else None for key, _, _ in shapes),
                                              sc.ctypes.data_as(C.POINTER(_lib.HskViewScore))))
        out["score"] = sc[0]
        return out

    # ---- cloud import -------------------------------------------------------------------------------------
    @staticmethod
    def _cloud(xyz, normals):
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if nrm is not None and len(nrm) != len(pts):
            raise ValueError("normals must be [n, 3] like xyz")
        return pts, nrm, (pts.ctypes.data if len(pts) else None), (nrm.ctypes.data if nrm is not None and len(nrm) else None)

    def splat_cloud(self, xyz, pose, normals=None, params=None, **fields):
        """the cloud xyz [n, 3] (world coordinates; normals [n, 3] or None) as the depth image of this tracker's camera at pose [4, 4]
        (hsk_splat_cloud): a z-buffered point splat, the smallest depth a pixel; params: an HskSplatParams (default:
        default_splat_params(self)), the keywords override its fields -> (depth (h, w) uint16, stats dict).  Read-only"""
        p = _params(_SPLAT, self, params, fields)
        pts, nrm, px, pn = self._cloud(xyz, normals)
        m = np.ascontiguousarray(pose, np.float32).reshape(16)
        depth, st = np.zeros((self.cfg.height, self.cfg.width), np.uint16), _lib.HskSplatStats()
        self._ck(self.lib.hsk_splat_cloud(self.h, px, pn, len(pts), _fp(m), C.byref(p), depth.ctypes.data, C.byref(st)))
        return depth, _stats_dict(st)

    def import_cloud(self, xyz, poses, normals=None, params=None, **fields):
        """the cloud fused into the volume as a sensor at each of the poses [m, 4, 4] would have seen it, in their order
        (hsk_import_cloud): per view splat_cloud's image through integrate, on the device; leaves the pose at the last view --
        resume_scan(that pose) tracks a live sensor on -> a structured array [m] with SPLAT_STATS_DTYPE"""
        p = _params(_SPLAT, self, params, fields)
        pts, nrm, px, pn = self._cloud(xyz, normals)
        ps = self._poses(poses)
        out = np.zeros(len(ps), SPLAT_STATS_DTYPE)
        self._ck(self.lib.hsk_import_cloud(self.h, px, pn, len(pts), ps.ctypes.data if len(ps) else None, len(ps), C.byref(p),
                                           out.ctypes.data_as(C.POINTER(_lib.HskSplatStats)) if len(ps) else None))
        return out

    # ---- cloud normals ------------------------------------------------------------------------------------
    def estimate_normals(self, xyz, viewpoints=None, params=None, **fields):
        """oriented normals and curvature of the cloud xyz [n, 3], which has none (hsk_estimate_normals): a fixed-radius
        neighbourhood, integer sums, a binary64 solve, each normal turned to the nearest of viewpoints [v, 3] (None: its largest
        component positive); params: an HskNormalParams (default: default_normal_params(self)), the keywords override its fields
        -> (normals [n, 3] float32, curvature [n] float32, neighbours [n] uint32, classes [n] uint8 of NORMAL_*, stats dict).
        Read-only"""
        p = _params(_NORMAL, self, params, fields)
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        vp, pv = _viewpoints(viewpoints)
        n = len(pts)
        nrm, curv = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        cnt, cls, st = np.zeros(n, np.uint32), np.zeros(n, np.uint8), _lib.HskNormalStats()
        self._ck(self.lib.hsk_estimate_normals(self.h, pts.ctypes.data if n else None, n, pv, len(vp), C.byref(p), nrm.ctypes.data,
                                               curv.ctypes.data, cnt.ctypes.data, cls.ctypes.data, C.byref(st)))
        return nrm, curv, cnt, cls, _stats_dict(st)

    # ---- surface components ----------------------------------------------------------------------------
    def label_components(self):
        """the connected components of the volume's inside voxels (observed, TSDF < 0; 6-neighbourhood), labelled on the device
        (hsk_label_components) -> (records, stats): a structured array with COMPONENT_DTYPE -- root (x, y, z), n_voxels, the box
        lo, hi (exclusive) -- ordered by n_voxels descending, ties to the smaller root; stats: n_components, n_inside, largest,
        labels_reused (the labelling of an earlier call was still valid).  Not with frames in flight"""
        st = _lib.HskComponentStats()   # (the fill finds the labelling of the size query: labels_reused is the size query's)
        recs = _records(_lib.HskComponent, lambda *a: self._ck(self.lib.hsk_label_components(self.h, *a)), st)
        return recs, _stats_dict(st)

    def download_components(self):
        """the dense label volume [vol_z, vol_y, vol_x] uint32 (hsk_download_components): an inside voxel's label is the smallest
        (z vol_y + y) vol_x + x of its component, every other voxel's COMPONENT_NONE"""
        out = np.empty((self.cfg.vol_z, self.cfg.vol_y, self.cfg.vol_x), np.uint32)
        self._ck(self.lib.hsk_download_components(self.h, out.ctypes.data))
        return out

    def default_prune_params(self):
        return default_prune_params(self)

    def prune_components(self, params=None, **fields):
        """erases the components that are too small (hsk_prune_components): those with fewer than min_voxels voxels and, with
        keep_largest > 0, those of rank >= keep_largest; their voxels become never observed (fill = PRUNE_UNSEEN, the default)
        or observed free space (PRUNE_FREE), their colour 0; every other word stays bit for bit.  params: an HskPruneParams
        (default: default_prune_params(self)); the keywords override its fields -> dict: n_components, n_pruned,
        n_pruned_voxels, n_kept_voxels"""
        p, st = _params(_PRUNE, self, params, fields), _lib.HskPruneStats()
        self._ck(self.lib.hsk_prune_components(self.h, C.byref(p), C.byref(st)))
        return _stats_dict(st)

    # ---- hole filling ------------------------------------------------------------------------------------
    def default_fill_params(self, **fields):
        return default_fill_params(self, **fields)

    def fill_holes(self, params=None, box=None, **fields):
        """closes the volume's gaps by volumetric diffusion (hsk_fill_holes): the signed distance of the observed voxels diffuses
        for `iterations` Jacobi steps into the never-observed voxels of box = (lo, hi) (None: the whole volume); of the voxels
        reached, those within Chebyshev distance `band` of a zero crossing (keep = FILL_SURFACE, the default) or all of them
        (FILL_ALL) are written with weight fill_weight; every other word, and the colour volume, stays bit for bit.  params: an
        HskFillParams (default: default_fill_params(self)); the keywords override its fields -> dict: n_unseen, n_reached,
        n_written, n_written_negative, tile_visits, iterations_run.  download_fill_mask tells which voxels were written.  Not with
        frames in flight"""
        p, st = _params(_FILL, self, params, fields), _lib.HskFillStats()
        self._ck(self.lib.hsk_fill_holes(self.h, C.byref(p), _box(self.cfg, box)[0], C.byref(st)))
        return _stats_dict(st)

    def download_fill_mask(self, box=None):
        """which voxels the last fill_holes wrote (hsk_download_fill_mask) over the voxels lo <= (x, y, z) < hi of box = (lo, hi),
        None: the whole volume -> [z, y, x] uint8, 1 written, 0 not; refused once the volume has changed since that fill"""
        b, shape = _box(self.cfg, box)
        out = np.empty(shape, np.uint8)
        self._ck(self.lib.hsk_download_fill_mask(self.h, b, out.ctypes.data if out.size else None))
        return out

    # ---- volume differencing ----------------------------------------------------------------------------
    def default_diff_params(self, **fields):
        return default_diff_params(self, **fields)

    def diff_volume(self, cur, params=None, **fields):
        """what changed between this tracker's volume (the older scan, `ref`) and `cur`'s (the newer one) on the same grid
        (hsk_diff_volume): per voxel a class -- DIFF_UNSEEN, ONLY_REF, ONLY_CUR, SAME, APPEARED, VANISHED --, the changed voxels
        grouped into 6-connected regions, those below min_voxels turned into DIFF_MINOR.  params: an HskDiffParams (default:
        default_diff_params(self)); the keywords override its fields -> (records, stats): a structured array with
        DIFF_REGION_DTYPE -- root, n_voxels, n_appeared, n_vanished, the box lo, hi (exclusive) -- of the kept regions, ordered by
        n_voxels descending, ties to the smaller root; stats: n_class [7], n_regions, n_minor_regions, largest.  The diff is held in
        this tracker: download_diff, diff_at, adopt_diff.  A cur in another frame is resampled first (resampled_like).  The size
        query and the fill diff once: the second call is answered from the held diff"""
        p, st = _params(_DIFF, self, params, fields), _lib.HskDiffStats()
        recs = _records(_lib.HskDiffRegion, lambda *a: self._ck(self.lib.hsk_diff_volume(self.h, cur.h, C.byref(p), *a)), st)
        return recs, _stats_dict(st)

    def download_diff(self, box=None, region=True):
        """the held diff over the voxels lo <= (x, y, z) < hi of box = (lo, hi), None: the whole volume (hsk_download_diff) ->
        (cls [z, y, x] uint8, region [z, y, x] uint32 or None): a region is the root's (z vol_y + y) vol_x + x for APPEARED and
        VANISHED voxels, COMPONENT_NONE elsewhere; refused once this tracker's volume has changed since the diff"""
        b, shape = _box(self.cfg, box)
        cls = np.empty(shape, np.uint8)
        reg = np.empty(shape, np.uint32) if region else None
        self._ck(self.lib.hsk_download_diff(self.h, b, cls.ctypes.data if cls.size else None, reg.ctypes.data if region and reg.size else None))
        return cls, reg

    def diff_at(self, xyz, radius=1):
        """the held diff at the world points xyz [n, 3] (hsk_diff_at, 2^20 points a call): the nearest APPEARED or VANISHED voxel within
        Chebyshev `radius` (0..4) of the point's voxel, else the voxel's own class -> (cls [n] uint8, region [n] uint32); a point
        outside the grid gives DIFF_UNSEEN and COMPONENT_NONE"""
        return tuple(_at_points(xyz, (np.uint8, np.uint32), lambda pts, m, *out: self._ck(self.lib.hsk_diff_at(self.h, pts, m, int(radius), *out))))

    def adopt_diff(self, cur, which=ADOPT_APPEARED | ADOPT_VANISHED, halo=2):
        """takes cur's words (and colour) where a kept region of the held diff says the scene changed (hsk_adopt_diff): every voxel
        cur has observed within Chebyshev `halo` (0..8) of a kept region's voxels of the classes `which` selects; a following
        fuse_volume(cur) then merges without ghosts -> dict: n_targets, n_adopted, n_colored"""
        p = _lib.HskAdoptParams(int(which), int(halo))
        st = _lib.HskAdoptStats()
        self._ck(self.lib.hsk_adopt_diff(self.h, cur.h, C.byref(p), C.byref(st)))
        return _stats_dict(st)

    def release_diff(self):
        """frees the held diff and its scratch (hsk_release_diff)"""
        self._ck(self.lib.hsk_release_diff(self.h))

    # ---- scene split ---------------------------------------------------------------------------------------
    def default_split_params(self, **fields):
        return default_split_params(self, **fields)

    def default_remove_params(self, **fields):
        return default_remove_params(self, **fields)

    @staticmethod
    def _split_planes(planes):
        if getattr(planes, "dtype", None) == SPLIT_PLANE_DTYPE:
            return np.ascontiguousarray(planes)
        return split_planes(np.zeros((0, 4), np.float32) if planes is None else planes)

    def split_scene(self, planes, params=None, **fields):
        """which INSIDE voxels belong to the planes (the structure) and which to objects (hsk_split_scene).  planes: a
        SPLIT_PLANE_DTYPE array (split_planes, split_plane_kinds), at most 64; params: an HskSplitParams (default:
        default_split_params(self)); the keywords override its fields -> (records, stats): a structured array with OBJECT_DTYPE --
        root, n_voxels, sum, the box lo, hi (exclusive), contact, plane_mask, height_lo, height_hi -- of the kept objects, ordered
        by n_voxels descending, ties to the smaller root; stats: n_class [7], n_objects, n_minor_objects, largest, n_edge,
        n_no_normal, reused.  The split is held in this tracker: download_split, split_at, remove_objects"""
        p, st = _params(_SPLIT, self, params, fields), _lib.HskSplitStats()
        pl = self._split_planes(planes)
        ptr = pl.ctypes.data_as(C.POINTER(_lib.HskSplitPlane)) if len(pl) else None
        recs = _records(_lib.HskObject, lambda *a: self._ck(self.lib.hsk_split_scene(self.h, ptr, len(pl), C.byref(p), *a)), st)
        return recs, _stats_dict(st)

    def download_split(self, box=None, plane=True, object=True):
        """the held split over the voxels lo <= (x, y, z) < hi of box = (lo, hi), None: the whole volume (hsk_download_split) ->
        (cls [z, y, x] uint8, plane [z, y, x] uint8 or None, object [z, y, x] uint32 or None): a plane is the index of the voxel's
        plane, 0xff where it has none; an object the root's (z vol_y + y) vol_x + x for OBJECT voxels, COMPONENT_NONE elsewhere;
        refused once this tracker's volume has changed since the split"""
        b, shape = _box(self.cfg, box)
        cls = np.empty(shape, np.uint8)
        pln = np.empty(shape, np.uint8) if plane else None
        obj = np.empty(shape, np.uint32) if object else None
        self._ck(self.lib.hsk_download_split(self.h, b, cls.ctypes.data if cls.size else None, pln.ctypes.data if plane and pln.size else None,
                                             obj.ctypes.data if object and obj.size else None))
        return cls, pln, obj

    def split_at(self, xyz, radius=1):
        """the held split at the world points xyz [n, 3] (hsk_split_at, 2^20 points a call): the nearest voxel with a class within
        Chebyshev `radius` (0..4) of the point's voxel -> (cls [n] uint8, plane [n] uint8, object [n] uint32); with none, or outside
        the grid, SPLIT_NONE, 0xff and COMPONENT_NONE"""
        return tuple(_at_points(xyz, (np.uint8, np.uint8, np.uint32),
                                lambda pts, m, *out: self._ck(self.lib.hsk_split_at(self.h, pts, m, int(radius), *out))))

    def remove_objects(self, roots=None, params=None, **fields):
        """takes kept objects of the held split out of the volume (hsk_remove_objects).  roots: their labels (None: all kept);
        params: an HskRemoveParams (default: default_remove_params(self)); the keywords -- mode, halo, fill_weight -- override its
        fields.  REMOVE_RESTORE rewrites what the objects hid from the planes they touched, REMOVE_ERASE only erases -> dict:
        n_objects, n_targets, n_written, n_restored, n_colored"""
        p, st = _params(_REMOVE, self, params, fields), _lib.HskRemoveStats()
        if roots is None:
            self._ck(self.lib.hsk_remove_objects(self.h, None, 0, C.byref(p), C.byref(st)))
        else:
            r = np.ascontiguousarray(roots, np.uint32).reshape(-1)
            keep = r if len(r) else np.zeros(1, np.uint32)     # (a pointer that is not NULL: an empty selection, not "all")
            self._ck(self.lib.hsk_remove_objects(self.h, keep.ctypes.data, len(r), C.byref(p), C.byref(st)))
        return _stats_dict(st)

    def release_split(self):
        """frees the held split and its scratch (hsk_release_split)"""
        self._ck(self.lib.hsk_release_split(self.h))

    def resampled_like(self, ref, cur_to_ref=None, color=False):
        """this tracker's volume on ref's grid: a new tracker with ref's configuration, and this volume fused into it with the
        rigid matrix cur_to_ref [4, 4] (None: the identity) -- into an empty volume fusion gives exactly the sampled words; color:
        the new tracker gets a colour volume first, which the fusion fills when this tracker has colour -> the new tracker (the
        caller closes it); what ref.diff_volume takes of a scan made in another frame or at another resolution"""
        out = KinfuTracker(ref.cfg)
        try:
            if color:
                out.enable_color()
            out.fuse_from(self, np.eye(4, dtype=np.float32) if cur_to_ref is None else cur_to_ref)
        except Exception:
            out.close()
            raise
        return out

    # ---- clearance field ---------------------------------------------------------------------------------
    def default_clearance_params(self, **fields):
        return default_clearance_params(self, **fields)

    def _clearance(self, params, fields):
        return _params(_CLEARANCE, self, params, fields)

    def build_clearance(self, params=None, **fields):
        """builds the clearance field on the device (hsk_build_clearance): per voxel the exact weighted squared distance, in
        voxel index differences, to the nearest obstacle -- a solid voxel; with CLEAR_UNKNOWN (the default) also a never-observed
        one and everything outside the grid -- CLEARANCE_FAR above max_d2.  params: an HskClearanceParams (default:
        default_clearance_params(self)); the keywords override its fields -> dict: n_obstacle, n_far, scratch_bytes,
        max_d2_seen, reused (the field of an earlier call was still valid).  Not with frames in flight"""
        st = _lib.HskClearanceStats()
        self._ck(self.lib.hsk_build_clearance(self.h, C.byref(self._clearance(params, fields)), C.byref(st)))
        return _stats_dict(st)

    def download_clearance(self, params=None, box=None, **fields):
        """the field over the voxels lo <= (x, y, z) < hi of box = (lo, hi), None: the whole volume (hsk_download_clearance; builds
        first when no valid field is held) -> [z, y, x] uint32"""
        b, shape = _box(self.cfg, box)
        out = np.empty(shape, np.uint32)
        self._ck(self.lib.hsk_download_clearance(self.h, C.byref(self._clearance(params, fields)), b, out.ctypes.data))
        return out

    def clearance_at(self, xyz, params=None, **fields):
        """the field at the voxels of the world points xyz [n, 3] (hsk_clearance_at; at most 2^20) -> [n] uint32, CLEARANCE_OUTSIDE
        for a point outside the grid or with a NaN"""
        p = self._clearance(params, fields)
        return _at_points(xyz, (np.uint32,), lambda *a: self._ck(self.lib.hsk_clearance_at(self.h, C.byref(p), *a)))[0]

    def clearance_floor(self, axis, lo, hi, params=None, **fields):
        """the floor map (hsk_clearance_floor): for the up axis (0 x, 1 y, 2 z) and its planes lo <= p < hi a column is an obstacle
        when any voxel of its band is; the 2-D clearance over the two remaining axes -> (map [v, u] uint32 with u the
        lower-numbered remaining axis, stats dict)"""
        out, st = np.empty(_floor_shape(self.cfg, axis), np.uint32), _lib.HskClearanceStats()
        self._ck(self.lib.hsk_clearance_floor(self.h, C.byref(self._clearance(params, fields)), int(axis), int(lo), int(hi), out.ctypes.data, C.byref(st)))
        return out, _stats_dict(st)

    def release_clearance(self):
        """frees the field and its scratch (hsk_release_clearance); the next call that needs it builds again"""
        self._ck(self.lib.hsk_release_clearance(self.h))

    # ---- reach field -------------------------------------------------------------------------------------
    def default_reach_params(self, clearance=None, **fields):
        return default_reach_params(self, clearance, **fields)

    def _reach(self, params, reach, fields):
        """-> (HskClearanceParams, HskReachParams) of a reach call: the keywords min_d2, max_cost go to the reach parameters
        (default: default_reach_params for the clearance parameters as overridden), all others to the clearance parameters"""
        own = {k: fields.pop(k) for k in REACH_FIELDS if k in fields}
        cp = self._clearance(params, fields)
        return cp, _params(_REACH, self, reach, own, (cp,))

    @staticmethod
    def _seeds(seeds):
        return np.ascontiguousarray(seeds, np.float32).reshape(-1, 3)

    def build_reach(self, seeds, params=None, reach=None, **fields):
        """builds the reach field on the device (hsk_build_reach): per voxel the length, in sixteenths of the clearance unit, of the
        shortest chain of 26-neighbour moves from the voxels of the world points `seeds` [n, 3] (at most 4096) that keeps a
        clearance of min_d2; REACH_UNREACHED / REACH_BLOCKED elsewhere.  params: an HskClearanceParams, reach: an HskReachParams
        (defaults: the tracker's); the keywords min_d2, max_cost override the reach parameters, all others the clearance
        parameters -> dict: n_passable, n_reached, scratch_bytes, max_cost_seen, n_rounds, n_seeds_used, reused"""
        cp, rp = self._reach(params, reach, fields)
        pts = self._seeds(seeds)
        st = _lib.HskReachStats()
        self._ck(self.lib.hsk_build_reach(self.h, C.byref(cp), C.byref(rp), pts.ctypes.data if len(pts) else None, len(pts), C.byref(st)))
        return _stats_dict(st)

    def download_reach(self, box=None):
        """the reach field held over the voxels lo <= (x, y, z) < hi of box = (lo, hi), None: the whole volume
        (hsk_download_reach) -> [z, y, x] uint32"""
        b, shape = _box(self.cfg, box)
        out = np.empty(shape, np.uint32)
        self._ck(self.lib.hsk_download_reach(self.h, b, out.ctypes.data))
        return out

    def reach_at(self, xyz):
        """the reach field held at the voxels of the world points xyz [n, 3] (hsk_reach_at; at most 2^20) -> [n] uint32,
        REACH_OUTSIDE for a point outside the grid or with a NaN"""
        return _at_points(xyz, (np.uint32,), lambda *a: self._ck(self.lib.hsk_reach_at(self.h, *a)))[0]

    def reach_path(self, goal, cap=4096):
        """the path of the field held from a seed to the voxel of the world point `goal` (hsk_reach_path) -> [n, 3] int32 voxels
        (x, y, z), n = 0 when the goal holds no value; a path longer than `cap` voxels is asked for again with the room it needs"""
        g = np.ascontiguousarray(goal, np.float32).reshape(3)
        n = C.c_size_t(0)
        out = np.empty((max(int(cap), 1), 3), np.int32)
        rc = self.lib.hsk_reach_path(self.h, g.ctypes.data, out.ctypes.data, int(cap), C.byref(n))
        if rc == -1 and n.value > int(cap):
            out = np.empty((n.value, 3), np.int32)
            rc = self.lib.hsk_reach_path(self.h, g.ctypes.data, out.ctypes.data, n.value, C.byref(n))
        self._ck(rc)
        return out[:n.value].copy()

    def reach_floor(self, axis, lo, hi, seeds, params=None, reach=None, **fields):
        """the floor form (hsk_reach_floor) -- where a person can walk: the same rule on clearance_floor's map of the band, the
        seeds projected by dropping the up axis -> (map [v, u] uint32 with u the lower-numbered remaining axis, stats dict)"""
        cp, rp = self._reach(params, reach, fields)
        pts = self._seeds(seeds)
        out, st = np.empty(_floor_shape(self.cfg, axis), np.uint32), _lib.HskReachStats()
        self._ck(self.lib.hsk_reach_floor(self.h, C.byref(cp), int(axis), int(lo), int(hi), C.byref(rp), pts.ctypes.data if len(pts) else None, len(pts),
                                          out.ctypes.data, C.byref(st)))
        return out, _stats_dict(st)

    def release_reach(self):
        """frees the reach field and its scratch (hsk_release_reach)"""
        self._ck(self.lib.hsk_release_reach(self.h))

    def reach_tiles_relaxed(self):
        """of the last build_reach that built -> (the tiles relaxed over all its rounds, the tiles of the grid)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.hsk_reach_tiles_relaxed(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- room partition ----------------------------------------------------------------------------------
    def default_partition_params(self, clearance=None, **fields):
        return default_partition_params(self, clearance, **fields)

    def _partition(self, params, partition, fields):
        """-> (HskClearanceParams, HskPartitionParams) of a partition call: the keywords core_d2, min_d2, min_core_voxels, max_cost go
        to the partition parameters (default: default_partition_params for the clearance parameters as overridden), all others to
        the clearance parameters"""
        own = {k: fields.pop(k) for k in PARTITION_FIELDS if k in fields}
        cp = self._clearance(params, fields)
        return cp, _params(_PARTITION, self, partition, own, (cp,))

    def build_partition(self, params=None, partition=None, **fields):
        """splits the scanned free space into rooms on the device (hsk_build_partition): the cores -- the 6-connected pieces of the
        voxels with a clearance of core_d2 -- spread through everything with a clearance of min_d2 along the reach field's moves, a
        voxel going to the nearest core.  params: an HskClearanceParams, partition: an HskPartitionParams (defaults: the tracker's);
        the keywords core_d2, min_d2, min_core_voxels, max_cost override the partition parameters, all others the clearance
        parameters -> (rooms: a ROOM_DTYPE array in id order, stats dict: n_cores, n_passable, n_assigned, scratch_bytes, n_dropped,
        n_rooms, n_doors, n_rounds, reused)"""
        cp, pp = self._partition(params, partition, fields)
        st = _lib.HskPartitionStats()
        rooms = _records(_lib.HskRoom, lambda *a: self._ck(self.lib.hsk_build_partition(self.h, C.byref(cp), C.byref(pp), *a)), st)
        return rooms, _stats_dict(st)

    def partition_doors(self):
        """the doors of the partition held (hsk_partition_doors): one record per pair of rooms that meet -> a DOOR_DTYPE array
        ordered by (a, b)"""
        return _records(_lib.HskDoor, lambda recs, cap, n, _: self._ck(self.lib.hsk_partition_doors(self.h, recs, cap, n)))

    def _partition_box(self, call, box):
        b, shape = _box(self.cfg, box)
        out = np.empty(shape, np.uint32)
        self._ck(call(self.h, b, out.ctypes.data))
        return out

    def download_partition(self, box=None):
        """the room ids of the partition held over the voxels lo <= (x, y, z) < hi of box = (lo, hi), None: the whole volume
        (hsk_download_partition) -> [z, y, x] uint32; ROOM_UNASSIGNED / ROOM_BLOCKED where a voxel holds no room"""
        return self._partition_box(self.lib.hsk_download_partition, box)

    def download_partition_cost(self, box=None):
        """the cost G of every voxel's chain to its core (hsk_download_partition_cost): the reach field seeded at every kept core
        voxel -> [z, y, x] uint32"""
        return self._partition_box(self.lib.hsk_download_partition_cost, box)

    def partition_at(self, xyz, radius=0):
        """the room of the world points xyz [n, 3] (hsk_partition_at; at most 2^20): that of the nearest voxel holding a room
        within `radius` (0..4) voxels on every axis of the point's own -> [n] uint32; ROOM_OUTSIDE for a point outside the grid or
        with a NaN, ROOM_NONE where there is no such voxel.  With a radius above 0 a surface point gets the room whose air it borders"""
        return _at_points(xyz, (np.uint32,), lambda pts, m, out: self._ck(self.lib.hsk_partition_at(self.h, pts, m, int(radius), out)))[0]

    def partition_floor(self, axis, lo, hi, params=None, partition=None, **fields):
        """the floor form (hsk_partition_floor): the same rule on clearance_floor's map of the band -> (map [v, u] uint32 room ids
        with u the lower-numbered remaining axis, rooms, doors, stats dict)"""
        cp, pp = self._partition(params, partition, fields)
        out, st = np.empty(_floor_shape(self.cfg, axis), np.uint32), _lib.HskPartitionStats()
        rooms, doors = np.zeros(PARTITION_MAX_ROOMS, ROOM_DTYPE), np.zeros(64, DOOR_DTYPE)
        nr, nd = C.c_size_t(0), C.c_size_t(0)
        args = (self.h, C.byref(cp), int(axis), int(lo), int(hi), C.byref(pp), out.ctypes.data)
        rc = self.lib.hsk_partition_floor(*args, rooms.ctypes.data, len(rooms), C.byref(nr), doors.ctypes.data, len(doors), C.byref(nd), C.byref(st))
        if rc == -1 and nd.value > len(doors):
            doors = np.zeros(nd.value, DOOR_DTYPE)
            rc = self.lib.hsk_partition_floor(*args, rooms.ctypes.data, len(rooms), C.byref(nr), doors.ctypes.data, len(doors), C.byref(nd), C.byref(st))
        self._ck(rc)
        return out, rooms[:nr.value].copy(), doors[:nd.value].copy(), _stats_dict(st)

    def release_partition(self):
        """frees the partition and its scratch (hsk_release_partition)"""
        self._ck(self.lib.hsk_release_partition(self.h))

    def partition_tiles_relaxed(self):
        """of the last build_partition that built -> (the tiles relaxed over all its rounds, the tiles of its first worklist, the
        tiles of the grid)"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.hsk_partition_tiles_relaxed(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def default_reloc_params(self):
        p = _lib.HskRelocParams()
        self.lib.hsk_default_reloc_params(self.h, C.byref(p))
        return p

    def relocalize(self, depth, poses, level=None, n_refine=0, accept_fraction=0.0, accept_rms_m=0.0, probes=None, **align):
        """find the camera pose of one depth frame in this volume among the candidate poses [m, 4, 4] (hsk_relocalize): they are
        scored, the best n_refine refined by the volume alignment, the best accepted refinement wins.  level: 1, 2 (the
        default) or 0 for the finest; probes and the other keywords are align_cloud's.  Overwrites the image buffers, nothing
        else; hand the pose to resume_scan.  -> (pose [4, 4] float32, dict(status: "found" | "none" | "empty", n_valid,
        n_candidates, best, candidates: one dict per refined candidate, by rank))"""
        d = self._depth(depth)
        ps = self._poses(poses)
        p = _lib.HskRelocParams()
        p.level = 0 if level is None else (_lib.HSK_RELOC_FINEST if int(level) == 0 else int(level))
        p.n_refine, p.accept_fraction, p.accept_rms_m = int(n_refine), accept_fraction, accept_rms_m
        p.align = self._align_params(probes, align)
        out, st = np.zeros(16, np.float32), _lib.HskRelocStats()
        self._ck(self.lib.hsk_relocalize(self.h, d.ctypes.data, d.shape[1], d.shape[0], ps.ctypes.data if len(ps) else None, len(ps),
                                         C.byref(p), _fp(out), C.byref(st)))
        cands = [dict(index=int(st.candidate[r]), score=_stats_dict(st.score[r]), align_status=_lib.HSK_ALIGN_STATUS[st.align_status[r]],
                      iterations=int(st.iterations[r]), n_used=int(st.n_used[r]), rms_m=np.float32(st.rms_m[r]))
                 for r in range(max(0, min(int(st.n_refined), _lib.HSK_RELOC_MAX_REFINE)))]
        return out.reshape(4, 4), {"status": _lib.HSK_RELOC_STATUS[st.status], "n_valid": int(st.n_valid), "n_candidates": int(st.n_candidates),
                                   "best": int(st.best), "candidates": cands}

    # ---- oriented plane detection -------------------------------------------------------------------------
    @staticmethod
    def _plane_params(over):
        """the defaults with the keywords dist_m, cos_min, min_fraction, max_planes, n_hypotheses, refits, seed over them"""
        p = _lib.HskPlaneParams()
        _lib.load().hsk_default_plane_params(C.byref(p))
        return _override(p, dict(p._fields_), "unknown plane parameter", over)

    @staticmethod
    def _plane_records(rec, n):
        return np.frombuffer(rec, PLANE_DTYPE, count=n).copy()

    def detect_planes_cloud(self, xyz, normals, **params):
        """the planes of the points xyz [n, 3] with normals [n, 3], detected on the device (hsk_detect_planes_oriented); the
        tracker's volume is not read.  Keywords: dist_m, cos_min, min_fraction, max_planes, n_hypotheses, refits, seed.
        -> (records [k]: abcd [4] float32 with the normal into the room, n_inliers, pad, sum_abs; labels [n] int32, -1 = no
        plane; the number of invalid points)"""
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(pts) != len(nrm):
            raise ValueError(f"detect_planes_cloud: {len(pts)} points but {len(nrm)} normals")
        p = self._plane_params(params)
        rec = (_lib.HskPlaneRecord * _lib.HSK_PLANE_MAX_PLANES)()
        labels = np.full(len(pts), -1, np.int32)
        k, bad = C.c_size_t(), C.c_size_t()
        self._ck(self.lib.hsk_detect_planes_oriented(self.h, pts.ctypes.data if len(pts) else None, nrm.ctypes.data if len(pts) else None, len(pts),
                                                     C.byref(p), rec, len(rec), C.byref(k), labels.ctypes.data if len(pts) else None, C.byref(bad)))
        return self._plane_records(rec, k.value), labels, bad.value

    def detect_planes(self, **params):
        """the planes of this volume's own cloud -- extract_cloud_attrs' points and normals, which stay on the device
        (hsk_detect_planes_volume) -> (records [k], labels [n] int32 in that cloud's order)"""
        p = self._plane_params(params)
        n = C.c_size_t()
        self._ck(self.lib.hsk_detect_planes_volume(self.h, C.byref(p), None, 0, None, None, 0, C.byref(n)))
        rec = (_lib.HskPlaneRecord * _lib.HSK_PLANE_MAX_PLANES)()
        labels = np.full(n.value, -1, np.int32)
        k, again = C.c_size_t(), C.c_size_t()
        self._ck(self.lib.hsk_detect_planes_volume(self.h, C.byref(p), rec, len(rec), C.byref(k), labels.ctypes.data if n.value else None, n.value,
                                                   C.byref(again)))
        if again.value != n.value:
            raise KinfuError("detect_planes: the cloud changed between the two calls")
        return self._plane_records(rec, k.value), labels

    def score_planes(self, xyz, normals, planes_abcd, dist_m=0.02, cos_min=0.8660254037844387, labels=None):
        """the inliers of each plane [m, 4] among the points (hsk_score_planes); labels [n] (optional): a point with a label >= 0
        counts for no plane -> counts [m] uint32"""
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        pl = np.ascontiguousarray(planes_abcd, np.float32).reshape(-1, 4)
        lab = None if labels is None else np.ascontiguousarray(labels, np.int32).reshape(-1)
        if len(pts) != len(nrm) or (lab is not None and len(lab) != len(pts)):
            raise ValueError("score_planes: points, normals and labels must have one row per point")
        out = np.zeros(len(pl), np.uint32)
        self._ck(self.lib.hsk_score_planes(self.h, pts.ctypes.data if len(pts) else None, nrm.ctypes.data if len(pts) else None,
                                           lab.ctypes.data if lab is not None and len(lab) else None, len(pts), pl.ctypes.data if len(pl) else None,
                                           len(pl), dist_m, cos_min, out.ctypes.data if len(pl) else None))
        return out

    # ---- upright frame ------------------------------------------------------------------------------------
    @staticmethod
    def _upright_params(over):
        """the defaults with the keywords up_hint, max_tilt_cos, cone_cos, wall_sin, min_fraction, refits, flags over them"""
        p = _lib.HskUprightParams()
        _lib.load().hsk_default_upright_params(C.byref(p))
        return _override(p, dict(p._fields_), "unknown upright parameter", over)

    @staticmethod
    def _upright_dict(u):
        return {"level": np.array(u.level, np.float32).reshape(4, 4), "floor_m": np.float32(u.floor_m), "ceiling_m": np.float32(u.ceiling_m),
                "box_lo": np.array(u.box_lo, np.float32), "box_hi": np.array(u.box_hi, np.float32), "n_points": int(u.n_points),
                "n_invalid": int(u.n_invalid), "n_axis": [int(v) for v in u.n_axis], "n_walls": int(u.n_walls), "found": int(u.found)}

    @staticmethod
    def _upright_struct(up):
        u = _lib.HskUpright()
        u.level = (C.c_float * 16)(*np.asarray(up["level"], np.float32).reshape(16))
        u.floor_m, u.ceiling_m = float(up["floor_m"]), float(up["ceiling_m"])
        u.box_lo = (C.c_float * 3)(*np.asarray(up["box_lo"], np.float32))
        u.box_hi = (C.c_float * 3)(*np.asarray(up["box_hi"], np.float32))
        u.n_points, u.n_invalid, u.n_walls, u.found = up["n_points"], up["n_invalid"], up["n_walls"], up["found"]
        u.n_axis = (C.c_uint32 * 3)(*up["n_axis"])
        return u

    def estimate_upright(self, **params):
        """the upright frame of this volume's own cloud, which stays on the device (hsk_estimate_upright).  Keywords: up_hint,
        max_tilt_cos, cone_cos, wall_sin, min_fraction, refits, flags -> dict of hsk_upright's fields: level [4, 4] (row 1 is down),
        floor_m, ceiling_m, box_lo, box_hi, n_points, n_invalid, n_axis, n_walls, found (HSK_UPRIGHT_* bits)"""
        p, u = self._upright_params(params), _lib.HskUpright()
        self._ck(self.lib.hsk_estimate_upright(self.h, C.byref(p), C.byref(u)))
        return self._upright_dict(u)

    def estimate_upright_oriented(self, xyz, normals, cell_weights=None, **params):
        """the same on the points xyz [n, 3] with normals [n, 3] (hsk_estimate_upright_oriented); cell_weights: the three c_min / c_k
        of normals that are differences over one cell per axis, None for true normals"""
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(pts) != len(nrm):
            raise ValueError(f"estimate_upright_oriented: {len(pts)} points but {len(nrm)} normals")
        w = None if cell_weights is None else np.ascontiguousarray(cell_weights, np.float32).reshape(3)
        p, u = self._upright_params(params), _lib.HskUpright()
        self._ck(self.lib.hsk_estimate_upright_oriented(self.h, pts.ctypes.data if len(pts) else None, nrm.ctypes.data if len(pts) else None, len(pts),
                                                        None if w is None else w.ctypes.data, C.byref(p), C.byref(u)))
        return self._upright_dict(u)

    def upright_sums(self, xyz, normals, cell_weights=None, cone_cos=0.984807753012208, wall_sin=0.25881904510252074, hist=False, axes=None,
                     wall_axes=None, frame=None, heights=False):
        """the device stages of the estimate alone, for integer axes (hsk_upright_sums) -> dict with, as asked: hist [1536] uint32 and
        n_valid; axis_sums [len(axes), 4] int64; wall_sums [3] int64; box [6] int32 and -- heights -- height_counts [2, 16384] uint32,
        height_sums [2, 16384] int64"""
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        w = None if cell_weights is None else np.ascontiguousarray(cell_weights, np.float32).reshape(3)
        out = {}
        if hist:
            out["hist"], out["n_valid"] = np.zeros(_lib.HSK_UPRIGHT_HIST_BINS, np.uint32), np.zeros(1, np.uint32)
        ax = None if axes is None else np.ascontiguousarray(axes, np.int32).reshape(-1, 3)
        if ax is not None:
            out["axis_sums"] = np.zeros((len(ax), 4), np.int64)
        wa = None if wall_axes is None else np.ascontiguousarray(wall_axes, np.int32).reshape(3, 3)
        if wa is not None:
            out["wall_sums"] = np.zeros(3, np.int64)
        fr = None if frame is None else np.ascontiguousarray(frame, np.int32).reshape(3, 3)
        if fr is not None:
            out["box"] = np.zeros(6, np.int32)
            if heights:
                out["height_counts"] = np.zeros((2, _lib.HSK_UPRIGHT_HEIGHT_BINS), np.uint32)
                out["height_sums"] = np.zeros((2, _lib.HSK_UPRIGHT_HEIGHT_BINS), np.int64)

        def ptr(name):
            return out[name].ctypes.data if name in out else None

        self._ck(self.lib.hsk_upright_sums(self.h, pts.ctypes.data if len(pts) else None, nrm.ctypes.data if len(pts) else None, len(pts),
                                           None if w is None else w.ctypes.data, cone_cos, wall_sin, ptr("hist"), ptr("n_valid"),
                                           None if ax is None else ax.ctypes.data, 0 if ax is None else len(ax), ptr("axis_sums"),
                                           None if wa is None else wa.ctypes.data, ptr("wall_sums"), None if fr is None else fr.ctypes.data,
                                           ptr("box"), ptr("height_counts"), ptr("height_sums")))
        if hist:
            out["n_valid"] = int(out["n_valid"][0])
        return out

    def level_config(self, upright, margin_m=None):
        """the configuration of the levelled destination of this volume and the matrix fuse_from(self, M) takes (hsk_level_config);
        margin_m None: the effective truncation distance plus two cells -> (HskConfig, M [4, 4] float32)"""
        cfg, m = _lib.HskConfig(), np.zeros(16, np.float32)
        u = self._upright_struct(upright)
        self._ck(self.lib.hsk_level_config(self.h, C.byref(u), -1.0 if margin_m is None else margin_m, C.byref(cfg), _fp(m)))
        return cfg, m.reshape(4, 4)

    def levelled(self, margin_m=None, **params):
        """a new tracker that holds this volume levelled: estimate_upright, level_config, then the fuse of this volume into the new
        one; it stands at this tracker's pose taken into the levelled frame (call resume_scan(its pose) to scan on)
        -> (tracker, M [4, 4] float32, the upright dict)"""
        up = self.estimate_upright(**params)
        cfg, m = self.level_config(up, margin_m)
        dst = KinfuTracker(cfg)
        try:
            dst.fuse_from(self, m)
        except Exception:
            dst.close()
            raise
        return dst, m, up

    # ---- volume files -----------------------------------------------------------------------------------
    def pack_volume(self, with_info=False):
        """the volume (TSDF, and colour once enabled) as a lossless sparse image, packed on the device (hsk_pack_volume)
        -> bytes, or (bytes, info dict) with with_info"""
        n, info = C.c_size_t(), _lib.HskVolumeInfo()
        self._ck(self.lib.hsk_pack_volume(self.h, None, 0, C.byref(n), C.byref(info)))
        buf = np.empty(n.value, np.uint8)
        self._ck(self.lib.hsk_pack_volume(self.h, buf.ctypes.data, buf.size, C.byref(n), C.byref(info)))
        if n.value != buf.size:
            raise KinfuError("pack_volume: the size changed between the two calls")
        return (buf.tobytes(), _info_dict(info)) if with_info else buf.tobytes()

    def pack_volume_info(self):
        """the size query of pack_volume alone: the header and the class counts of the image the volume would make"""
        n, info = C.c_size_t(), _lib.HskVolumeInfo()
        self._ck(self.lib.hsk_pack_volume(self.h, None, 0, C.byref(n), C.byref(info)))
        return _info_dict(info)

    def unpack_volume(self, image):
        """replace the volume by a sparse image's (hsk_unpack_volume); the tracker pose and model maps are not touched"""
        a = np.frombuffer(image, np.uint8)
        self._ck(self.lib.hsk_unpack_volume(self.h, a.ctypes.data if a.size else None, a.size))

    def save_volume(self, path):
        """the image as a file (written beside itself, then renamed into place) -> info dict"""
        info = _lib.HskVolumeInfo()
        self._ck(self.lib.hsk_save_volume(self.h, str(path).encode(), C.byref(info)))
        return _info_dict(info)

    def load_volume(self, path):
        self._ck(self.lib.hsk_load_volume(self.h, str(path).encode()))

    def resume_scan(self, pose):
        """put the tracker where it stands after a tracked frame at `pose`: the model maps are raycast from the volume as it
        is, so the next frame is tracked by ICP against it (hsk_resume_scan)"""
        p = np.ascontiguousarray(pose, np.float32).reshape(16)
        self._ck(self.lib.hsk_resume_scan(self.h, _fp(p)))

    @classmethod
    def from_volume_file(cls, path, **over):
        """a tracker made for the volume file at `path` (config_from_volume; keywords override config fields) that holds
        its volume, with colour enabled when the file has colour.  The tracker stands at the file's pose; call
        resume_scan(info pose) to scan on."""
        info = volume_file_info(path)
        cfg = config_from_volume(info)
        for k, v in over.items():
            setattr(cfg, k, v)
        t = cls(cfg)
        try:
            if info["has_color"]:
                t.enable_color(info["color_max_weight"], info["color_band_m"])
            t.load_volume(path)
        except Exception:
            t.close()
            raise
        return t

    # ---- streams / profiling -----------------------------------------------------------------------
    def stream(self):
        return self.lib.hsk_stream(self.h)

    def set_stream(self, stream_ptr):
        self._ck(self.lib.hsk_set_stream(self.h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._ck(self.lib.hsk_synchronize(self.h))

    def set_profiling(self, on):
        self._ck(self.lib.hsk_set_profiling(self.h, int(on)))

    def icp_level_ms(self):
        """profiling: summed time of each ICP level's iterations (index 0 = finest), over the frames of stage_ms()"""
        ms = (C.c_double * _lib.HSK_LEVELS)()
        self._ck(self.lib.hsk_icp_level_ms(self.h, ms))
        return list(ms)

    def stage_ms(self, reset=False):
        ms = (C.c_double * _lib.HSK_NSTAGES)()
        n = C.c_uint64()
        self._ck(self.lib.hsk_stage_ms(self.h, ms, C.byref(n), int(reset)))
        return list(ms), n.value


def _info_dict(info):
    """an `_lib.HskVolumeInfo` as a dict (arrays as numpy; "raw": the structure itself, for config_from_volume)"""
    d = {}
    for name, _ in _lib.HskVolumeInfo._fields_:
        v = getattr(info, name)
        d[name] = np.array(v[:]) if hasattr(v, "__len__") else v
    d["pose"] = np.array(info.pose[:], np.float32).reshape(4, 4)
    d["size_m"] = np.array(info.size_m[:], np.float32)
    d["has_color"] = bool(info.flags & 1)
    d["raw"] = _lib.HskVolumeInfo.from_buffer_copy(info)
    return d


def volume_image_info(image):
    """host only: validate a sparse volume image (bytes) and return its header as a dict; KinfuError when it is refused"""
    lib = _lib.load()
    a = np.frombuffer(image, np.uint8)
    info = _lib.HskVolumeInfo()
    rc = lib.hsk_volume_image_info(a.ctypes.data if a.size else None, a.size, C.byref(info))
    if rc != 0:
        raise KinfuError(f"hsk_volume_image_info failed ({rc}): {lib.hsk_last_error(None).decode()}")
    return _info_dict(info)


def volume_file_info(path):
    """host only: the same for a volume file (reads the header and the class tables only)"""
    lib = _lib.load()
    info = _lib.HskVolumeInfo()
    rc = lib.hsk_volume_file_info(str(path).encode(), C.byref(info))
    if rc != 0:
        raise KinfuError(f"hsk_volume_file_info failed ({rc}): {lib.hsk_last_error(None).decode()}")
    return _info_dict(info)


def config_from_volume(info):
    """host only: the configuration of a context that accepts the image whose header `info` is (a dict of
    volume_*_info, or an `_lib.HskVolumeInfo`); the image's pose becomes init_pose"""
    lib = _lib.load()
    raw = info["raw"] if isinstance(info, dict) else info
    cfg = _lib.HskConfig()
    rc = lib.hsk_config_from_volume(C.byref(raw), C.byref(cfg))
    if rc != 0:
        raise KinfuError(f"hsk_config_from_volume failed ({rc}): {lib.hsk_last_error(None).decode()}")
    return cfg


GROUP_FORCE_RCCL = 1
GROUP_ICP_ALLREDUCE = 2
GROUP_DIRECT = 4      # composites as a one-hop exchange over peer-mapped memory (no RCCL)
GROUP_PROFILE = 8     # events round the exchange (exchange_ms)


class KinfuGroup:
    """One TSDF volume sharded as z-slabs over several GPUs, behind one frame call (`hsk_group_*`): the slab frame loop
    and its RCCL collectives live inside the library.  `device_ids` names the device of every slab (single process), or
    pass rank / world / comm_id for one process per GPU."""

    def __init__(self, cfg=None, device_ids=(0,), flags=0, rank=None, world=None, comm_id=None, **over):
        self.lib = _lib.load()
        self.cfg = cfg if cfg is not None else default_config(**over)
        h = C.c_void_p()
        if rank is None:
            ids = (C.c_int * len(device_ids))(*device_ids)
            rc = self.lib.hsk_group_create(C.byref(self.cfg), len(device_ids), ids, int(flags), C.byref(h))
        else:
            buf = C.create_string_buffer(bytes(comm_id), 128) if comm_id is not None else None
            rc = self.lib.hsk_group_create_rank(C.byref(self.cfg), int(rank), int(world), buf, int(flags), C.byref(h))
        if rc != 0:
            raise KinfuError(f"hsk_group_create failed ({rc}): {self.lib.hsk_group_last_error(None).decode()}")
        self.h = h
        self.w, self.hgt = self.cfg.width, self.cfg.height

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = _lib.load().hsk_group_unique_id(buf)
        if rc != 0:
            raise KinfuError(f"hsk_group_unique_id failed ({rc}): {_lib.load().hsk_group_last_error(None).decode()}")
        return buf.raw

    def _ck(self, rc):
        if rc != 0:
            raise KinfuError(f"hskinfu group error {rc}: {self.lib.hsk_group_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.hsk_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process_frame(self, depth):
        d = KinfuTracker._depth(depth)
        pose = np.empty(16, np.float32)
        tracked = C.c_int()
        self._ck(self.lib.hsk_group_process_frame(self.h, d.ctypes.data, d.shape[1], d.shape[0], _fp(pose), C.byref(tracked)))
        return pose.reshape(4, 4), bool(tracked.value)

    def submit_frame(self, depth):
        d = KinfuTracker._depth(depth)
        self._ck(self.lib.hsk_group_submit_frame(self.h, d.ctypes.data, d.shape[1], d.shape[0]))

    def submit_frame_dev(self, device_ptrs):
        arr = (C.c_void_p * len(device_ptrs))(*device_ptrs)
        self._ck(self.lib.hsk_group_submit_frame_dev(self.h, arr, self.w, self.hgt))

    def wait_frame(self):
        pose = np.empty(16, np.float32)
        tracked = C.c_int()
        self._ck(self.lib.hsk_group_wait_frame(self.h, _fp(pose), C.byref(tracked)))
        return pose.reshape(4, 4), bool(tracked.value)

    def reset(self):
        self._ck(self.lib.hsk_group_reset(self.h))

    def n_slabs(self):
        return self.lib.hsk_group_n_slabs(self.h)

    def ranks_seen(self):
        """ranks / devices the group's exchange spans, as the communicator (or the shared flag page) itself counts them"""
        n = C.c_int()
        self._ck(self.lib.hsk_group_ranks_seen(self.h, C.byref(n)))
        return n.value

    def exchange_ms(self):
        """GROUP_PROFILE: (summed ms of the per-frame exchange, summed ms of the slab work before it, frames counted) on
        the first local device"""
        ms, front, n = C.c_double(), C.c_double(), C.c_ulonglong()
        self._ck(self.lib.hsk_group_exchange_ms(self.h, C.byref(ms), C.byref(front), C.byref(n)))
        return ms.value, front.value, n.value

    def slab(self, i):
        """a borrowed KinfuTracker view of slab i (owned by the group: never close it)"""
        t = KinfuTracker.__new__(KinfuTracker)
        t.lib, t.cfg, t.h = self.lib, self.cfg, C.c_void_p(self.lib.hsk_group_slab(self.h, i))
        t.w, t.hgt = self.w, self.hgt
        z0, nz = C.c_int(), C.c_int()
        self.lib.hsk_stored_planes(t.h, C.byref(z0), C.byref(nz))
        t.stored_z0, t.stored_nz = z0.value, nz.value
        t.close = lambda: None
        return t

    def download_tsdf(self, out=None):
        """the planes this process owns, at their place in a full [Z, Y, X, 2] array"""
        if out is None:
            out = np.zeros((self.cfg.vol_z, self.cfg.vol_y, self.cfg.vol_x, 2), np.int16)
        self._ck(self.lib.hsk_group_download_tsdf(self.h, out.ctypes.data))
        return out


def synth_pose(frame):
    lib = _lib.load()
    p = np.empty(16, np.float32)
    lib.hsk_synth_pose(int(frame), _fp(p))
    return p.reshape(4, 4)


def synth_depth(pose, w=640, h=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    lib = _lib.load()
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    d = np.empty((h, w), np.uint16)
    rc = lib.hsk_synth_render(_fp(p), w, h, fx, fy, cx, cy, d.ctypes.data)
    if rc != 0:
        raise KinfuError(f"hsk_synth_render failed ({rc})")
    return d


def synth_noisy_frames(count, first=0, sigma_mm=1.2, dropout=0.02, seeds=(1234, 5678)):
    """SURVEY.md 8(d)'s noise run: the scripted stream with sensor noise -- sigma = 1.2 mm x (z / 1 m)^2 on every pixel
    (generator seed 1234) and 2 % of the pixels dropped to 0 (seed 5678), what a real takeDepthSnapshot frame looks like
    (/root/reference/housescan/HoniHelper.hs:20-36) where the render is exact.  Frames `first .. first + count - 1`; the
    generators are drawn from frame 0 on, so frame k is the same whatever `first` is.  -> (ground-truth poses, uint16 frames)"""
    rn, rd = np.random.default_rng(seeds[0]), np.random.default_rng(seeds[1])
    poses, frames = [], []
    for k in range(first + count):
        gt = synth_pose(k)
        d = synth_depth(gt).astype(np.float64)
        z = d / 1000.0
        d = d + rn.normal(size=d.shape) * sigma_mm * z * z
        d[rd.random(d.shape) < dropout] = 0
        if k >= first:
            poses.append(gt)
            frames.append(np.clip(np.rint(d), 0, 65535).astype(np.uint16))
    return poses, frames


def synth_sensor_depth(pose, scene=-1, seed=1234, sigma_mm=1.2, range_cut_m=3.5, absorbing=False, w=640, h=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    """one frame with holes as a structured-light sensor makes them (hsk_synth_render_sensor: grazing rays, shadow bands behind
    depth discontinuities, the 3.5 m range cut, sigma_mm x z^2 noise); scene -1 = the open scene of synth_depth, 0..3 = the
    closed rooms -> (uint16 depth, share of pixels without depth)"""
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    d = np.empty((h, w), np.uint16)
    frac = C.c_double()
    rc = _lib.load().hsk_synth_render_sensor(int(scene), _fp(p), w, h, fx, fy, cx, cy, int(seed), float(sigma_mm), float(range_cut_m), int(bool(absorbing)),
                                             d.ctypes.data, C.byref(frac))
    if rc != 0:
        raise KinfuError(f"hsk_synth_render_sensor failed ({rc})")
    return d, frac.value


def synth_sensor_frames(count, first=0, seed=1234, sigma_mm=1.2, range_cut_m=3.5, absorbing=False, room=None, scan=720):
    """the scripted stream of SURVEY.md 8(d) -- or, room = 0..3, the three-turn scan inside a closed room -- seen by a sensor
    (synth_sensor_depth; frame k's noise is keyed by seed + k) -> (ground-truth poses, uint16 frames)"""
    if room is None:
        poses = [synth_pose(k) for k in range(first, first + count)]
    else:
        poses = [synth_room_pose(room, k, scan) for k in range(first, first + count)]
    return poses, [synth_sensor_depth(p, -1 if room is None else room, seed + first + i, sigma_mm, range_cut_m, absorbing)[0] for i, p in enumerate(poses)]


def synth_box_depth(depth, pose, lo, hi, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    """a depth frame with an axis-aligned box lo .. hi (metres, in the frame of `pose`) composited in: per pixel min(depth, the
    box's depth along the pixel's ray), a pixel without depth (0) taking the box's -> uint16 millimetres.  What a second scan of
    a room with a new object in it looks like (tools/diff_demo.py)"""
    d = np.asarray(depth)
    h, w = d.shape
    m = np.asarray(pose, np.float64).reshape(4, 4)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ m[:3, :3].T      # world direction per unit of depth
    t0, t1 = np.zeros((h, w)), np.full((h, w), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for ax in range(3):
            a, b = (lo[ax] - m[ax, 3]) / ray[..., ax], (hi[ax] - m[ax, 3]) / ray[..., ax]
            t0, t1 = np.maximum(t0, np.minimum(a, b)), np.minimum(t1, np.maximum(a, b))
    mm = np.rint(t0 * 1000.0)
    hit = (t0 <= t1) & (t0 > 1e-9) & (mm >= 1) & (mm <= 65535)
    out = d.copy()
    take = hit & ((d == 0) | (mm < d))
    out[take] = mm[take].astype(np.uint16)
    return out


def synth_room_extents(variant):
    """(x0, x1, y0, y1, z0, z1) of closed synthetic room `variant` in its own scan frame"""
    e = np.empty(6, np.float32)
    _lib.load().hsk_synth_room_extents(int(variant), _fp(e))
    return e


def synth_room_pose(variant, frame, n_frames):
    p = np.empty(16, np.float32)
    rc = _lib.load().hsk_synth_room_pose(int(variant), int(frame), int(n_frames), _fp(p))
    if rc != 0:
        raise KinfuError(f"hsk_synth_room_pose failed ({rc})")
    return p.reshape(4, 4)


def synth_room_depth(variant, pose, w=640, h=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    d = np.empty((h, w), np.uint16)
    rc = _lib.load().hsk_synth_room_render(int(variant), _fp(p), w, h, fx, fy, cx, cy, d.ctypes.data)
    if rc != 0:
        raise KinfuError(f"hsk_synth_room_render failed ({rc})")
    return d


def synth_rgb(pose, scene=-1, w=640, h=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
    """the colour image registered to synth_depth (scene -1) / synth_room_depth (scene 0..3): (h, w, 3) uint8, (0, 0, 0) exactly
    where the clean depth render has no depth"""
    p = np.ascontiguousarray(pose, np.float32).reshape(16)
    out = np.empty((h, w, 3), np.uint8)
    rc = _lib.load().hsk_synth_render_rgb(int(scene), _fp(p), w, h, fx, fy, cx, cy, out.ctypes.data)
    if rc != 0:
        raise KinfuError(f"hsk_synth_render_rgb failed ({rc})")
    return out


def synth_color_at(p, scene=-1):
    """the synthetic colour (uint8 r, g, b) of world point p"""
    q = np.ascontiguousarray(p, np.float32).reshape(3)
    out = np.empty(3, np.uint8)
    rc = _lib.load().hsk_synth_color_at(int(scene), _fp(q), out.ctypes.data)
    if rc != 0:
        raise KinfuError(f"hsk_synth_color_at failed ({rc})")
    return out


def bilateral_tables():
    lib = _lib.load()
    ws = np.empty(169, np.float32)
    wc = np.empty(512, np.float32)
    lib.hsk_bilateral_tables(_fp(ws), _fp(wc))
    return ws, wc
