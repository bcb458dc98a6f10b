"""The binding's shared paths (housescan_amd/kinfu.py) without a GPU and without a tracker: the record dtypes against their
structures and against the literals they replaced; the ten default_* functions through the one parameter path; the box, point,
record and stats helpers, the C calls played by Python callables."""
import ctypes as C

import numpy as np
import pytest

# the layouts as they were typed out in kinfu.py before they were derived from the structures: a later edit of _lib.py that moves
# a layout fails here
LITERALS = {
    "SCORE_DTYPE": ("HskPoseScore", 32, [("n_near", "<u4"), ("n_free", "<u4"), ("n_behind", "<u4"), ("n_unseen", "<u4"), ("n_outside", "<u4"),
                                         ("n_skipped", "<u4"), ("sum_abs", "<u8")]),
    "PLANE_DTYPE": ("HskPlaneRecord", 32, [("abcd", "<f4", (4,)), ("n_inliers", "<u4"), ("pad", "<u4"), ("sum_abs", "<u8")]),
    "VIEW_SCORE_DTYPE": ("HskViewScore", 32, [("n_hit", "<u4"), ("n_frontier", "<u4"), ("n_open", "<u4"), ("n_blind", "<u4"), ("n_outside", "<u4"),
                                              ("eye_state", "<u4"), ("gain", "<u8")]),
    "COMPONENT_DTYPE": ("HskComponent", 48, [("root", "<i4", (3,)), ("pad", "<i4"), ("n_voxels", "<u8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,))]),
    "DIFF_REGION_DTYPE": ("HskDiffRegion", 64, [("root", "<i4", (3,)), ("pad", "<i4"), ("n_voxels", "<u8"), ("n_appeared", "<u8"), ("n_vanished", "<u8"),
                                                ("lo", "<i4", (3,)), ("hi", "<i4", (3,))]),
    "SPLIT_PLANE_DTYPE": ("HskSplitPlane", 24, [("abcd", "<f4", (4,)), ("kind", "<i4"), ("pad", "<i4")]),
    "OBJECT_DTYPE": ("HskObject", 104, [("root", "<i4", (3,)), ("pad", "<i4"), ("n_voxels", "<u8"), ("sum", "<u8", (3,)), ("lo", "<i4", (3,)),
                                        ("hi", "<i4", (3,)), ("contact", "<u4", (4,)), ("plane_mask", "<u8"), ("height_lo", "<i4"), ("height_hi", "<i4")]),
    "ROOM_DTYPE": ("HskRoom", 88, [("n_voxels", "<u8"), ("n_core_voxels", "<u8"), ("sum", "<u8", 3), ("root", "<u4", 3), ("lo", "<u4", 3), ("hi", "<u4", 3),
                                   ("max_d2", "<u4"), ("max_g", "<u4"), ("pad", "<u4")]),
    "DOOR_DTYPE": ("HskDoor", 72, [("sum2", "<u8", 3), ("a", "<u4"), ("b", "<u4"), ("n_faces", "<u4", 3), ("lo", "<u4", 3), ("hi", "<u4", 3),
                                   ("max_d2", "<u4")]),
    "TEXTURE_CHART_DTYPE": ("HskTextureChart", 16, [("x0", np.int32), ("y0", np.int32), ("s", np.int32), ("half_rot", np.int32)]),
}

# default function -> (its structure, its *_FIELDS, an integer field, a float field or None, the names it must refuse)
DEFAULTS = {
    "default_probe": ("HskProbe", "PROBE_FIELDS", "width", "fx", ()),
    "default_prune_params": ("HskPruneParams", "PRUNE_FIELDS", "min_voxels", None, ()),
    "default_fill_params": ("HskFillParams", "FILL_FIELDS", "iterations", None, ()),
    "default_diff_params": ("HskDiffParams", "DIFF_FIELDS", "min_voxels", None, ()),
    "default_split_params": ("HskSplitParams", "SPLIT_FIELDS", "min_voxels", "dist_m", ("pad",)),
    "default_remove_params": ("HskRemoveParams", "REMOVE_FIELDS", "halo", None, ()),
    "default_clearance_params": ("HskClearanceParams", "CLEARANCE_FIELDS", "max_d2", "unit_m", ()),
    "default_reach_params": ("HskReachParams", "REACH_FIELDS", "min_d2", None, ("flags", "pad")),
    "default_partition_params": ("HskPartitionParams", "PARTITION_FIELDS", "core_d2", None, ("flags", "pad")),
}


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_a_record_dtype_is_its_structure_and_the_literal_it_replaced(hsk, name):
    struct, size, literal = LITERALS[name]
    dt = getattr(hsk.kinfu, name)
    assert dt == np.dtype(getattr(hsk._lib, struct)) and dt == np.dtype(literal)
    assert dt.itemsize == size == C.sizeof(getattr(hsk._lib, struct))


def test_reach_and_partition_defaults_follow_the_clearance_parameters_they_are_given(hsk):
    """both clamp to the clearance parameters' max_d2: the C default call got them, in front of its own structure"""
    k = hsk.kinfu
    cp = k.default_clearance_params(max_d2=4)
    assert k.default_reach_params().min_d2 > 4 and k.default_reach_params(None, cp).min_d2 == 4
    assert k.default_partition_params().core_d2 > 4 and k.default_partition_params(None, cp, min_d2=2).core_d2 == 4
    assert k.default_partition_params(None, cp, min_d2=2).min_d2 == 2 and k.default_reach_params(clearance=cp, max_cost=5).max_cost == 5


@pytest.mark.parametrize("name", sorted(DEFAULTS))
def test_a_default_function_sets_reads_back_coerces_and_refuses(hsk, name):
    struct, fields_name, int_field, float_field, refused = DEFAULTS[name]
    fn, fields = getattr(hsk.kinfu, name), getattr(hsk.kinfu, fields_name)
    assert type(fn()) is getattr(hsk._lib, struct)
    types = dict(getattr(hsk._lib, struct)._fields_)
    for i, f in enumerate(fields):                      # every name a caller may set can be set and reads back
        if issubclass(types[f], C.Array):
            want = [3 + i + j for j in range(types[f]._length_)]
            assert list(getattr(fn(**{f: want}), f)) == want
            assert list(getattr(fn(**{f: np.array(want, np.int64)}), f)) == want
        else:
            want = 3 + i                                # (small integers: exact in every field type)
            assert getattr(fn(**{f: want}), f) == want
    with pytest.raises(TypeError, match="no field"):
        fn(no_such_field=1)
    for f in refused:
        assert f in types
        with pytest.raises(TypeError, match="no field"):
            fn(**{f: 0})
    assert getattr(fn(**{int_field: np.int64(7)}), int_field) == 7 and getattr(fn(**{int_field: np.uint32(9)}), int_field) == 9
    if float_field is not None:
        assert getattr(fn(**{float_field: np.float32(0.25)}), float_field) == 0.25
        assert getattr(fn(**{float_field: np.float64(0.5)}), float_field) == 0.5


def test_the_box_helper(hsk):
    cfg = hsk.default_config(32, vol_x=48, vol_y=40, vol_z=32)
    b, shape = hsk.kinfu._box(cfg, None)
    assert b is None and shape == (32, 40, 48)
    b, shape = hsk.kinfu._box(cfg, ((1, 2, 3), (5, 4, 4)))
    assert type(b) is hsk._lib.HskVoxelBox and (list(b.lo), list(b.hi)) == ([1, 2, 3], [5, 4, 4]) and shape == (1, 2, 4)
    b, shape = hsk.kinfu._box(cfg, ((5, 2, 3), (1, 4, 4)))      # inverted along x: no voxels, not a negative extent
    assert shape == (1, 2, 0) and (list(b.lo), list(b.hi)) == ([5, 2, 3], [1, 4, 4])
    b, shape = hsk.kinfu._box(cfg, (np.array([0, 0, 0], np.int64), np.array([48.0, 40.0, 32.0])))
    assert shape == (32, 40, 48) and list(b.hi) == [48, 40, 32]


def fake_point_call(log):
    """a C point call played in Python: logs (m, which pointers were None) and writes the piece's index into the outputs"""
    def call(pts, m, cls, word):
        log.append((m, (pts is None, cls is None, word is None)))
        if m:
            xyz = np.ctypeslib.as_array((C.c_float * (3 * m)).from_address(pts))
            assert xyz[0] == call.seen                       # the piece starts where the last one ended
            call.seen += m
            (C.c_uint8 * m).from_address(cls)[:] = [len(log) - 1] * m
            (C.c_uint32 * m).from_address(word)[:] = [1000 + len(log) - 1] * m
    call.seen = 0
    return call


def points(n):
    return np.repeat(np.arange(n, dtype=np.float32), 3).reshape(n, 3)     # point i is (i, i, i)


def test_the_point_helper(hsk, monkeypatch):
    log = []
    cls, word = hsk.kinfu._at_points(np.zeros((0, 3), np.float32), (np.uint8, np.uint32), fake_point_call(log))
    assert log == [(0, (True, True, True))] and cls.shape == (0,) and word.shape == (0,) and (cls.dtype, word.dtype) == (np.uint8, np.uint32)
    log = []
    cls, word = hsk.kinfu._at_points(points(5).astype(np.float64).tolist(), (np.uint8, np.uint32), fake_point_call(log))
    assert log == [(5, (False, False, False))] and cls.tolist() == [0] * 5 and word.tolist() == [1000] * 5
    monkeypatch.setattr(hsk._lib, "HSK_CLEAR_MAX_POINTS", 4)
    log = []
    cls, word = hsk.kinfu._at_points(points(9), (np.uint8, np.uint32), fake_point_call(log))
    assert [m for m, _ in log] == [4, 4, 1] and all(nones == (False, False, False) for _, nones in log)
    assert cls.tolist() == [0] * 4 + [1] * 4 + [2] and word.tolist() == [1000] * 4 + [1001] * 4 + [1002]
    log = []
    hsk.kinfu._at_points(points(8), (np.uint8, np.uint32), fake_point_call(log))
    assert [m for m, _ in log] == [4, 4]                     # (a whole number of pieces: no empty call behind them)


def test_the_record_helper(hsk):
    def fake(total, log):
        def call(recs, cap, n_ref, stats):
            log.append((recs is None, cap, stats is None))
            n_ref._obj.value = total
            if stats is not None:
                stats._obj.n_components = total
            if recs is not None:
                for i in range(cap):
                    recs[i].n_voxels = 10 + i
        return call

    log, st = [], hsk._lib.HskComponentStats()
    recs = hsk.kinfu._records(hsk._lib.HskComponent, fake(0, log), st)
    assert log == [(True, 0, False)] and recs.shape == (0,) and recs.dtype == hsk.kinfu.COMPONENT_DTYPE
    log = []
    recs = hsk.kinfu._records(hsk._lib.HskComponent, fake(3, log), st)
    assert log == [(True, 0, False), (False, 3, True)] and recs["n_voxels"].tolist() == [10, 11, 12] and st.n_components == 3
    log = []
    assert len(hsk.kinfu._records(hsk._lib.HskDoor, fake(2, log))) == 2 and log == [(True, 0, True), (False, 2, True)]     # (a call without stats)


def test_the_stats_dict(hsk):
    st = hsk._lib.HskSplitStats()
    st.n_class[:] = [1, 2, 3, 4, 5, 6, 1 << 40]
    st.n_objects, st.n_minor_objects, st.largest, st.n_edge, st.n_no_normal, st.reused, st.pad = 7, 8, 9, 10, 11, 1, 99
    d = hsk.kinfu._stats_dict(st)
    assert list(d) == ["n_class", "n_objects", "n_minor_objects", "largest", "n_edge", "n_no_normal", "reused"]
    assert d["n_class"].dtype == np.uint64 and d["n_class"].tolist() == [1, 2, 3, 4, 5, 6, 1 << 40]
    assert all(type(v) is int for k, v in d.items() if k != "n_class") and [d[k] for k in list(d)[1:]] == [7, 8, 9, 10, 11, 1]
    fs = hsk._lib.HskFillStats(1, 2, 3, 4, 5, 6, 99)
    d = hsk.kinfu._stats_dict(fs)
    assert d == {"n_unseen": 1, "n_reached": 2, "n_written": 3, "n_written_negative": 4, "tile_visits": 5, "iterations_run": 6}
    assert all(type(v) is int for v in d.values())
