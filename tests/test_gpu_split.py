"""The scene split on the device (hsk_split_scene, hsk_download_split, hsk_split_at, hsk_remove_objects) against
the numpy twin (tests/split_twin.py): class bytes, plane bytes, object labels, records in order, every stats field, the point query
and every word and colour word after a removal are EQUAL to the twin's."""
import ctypes as C

import numpy as np
import pytest

import diff_twin as DT
import split_cases as SC
import split_twin as ST
from kit import same_bits, volume_ctx
from split_cases import records_as_dicts

pytestmark = pytest.mark.gpu


def loaded(hsk, key):
    """a context holding the case's volume (and colour volume)"""
    c, col = SC.case_of(key), SC.color_of(key)
    trk = volume_ctx(hsk, c["dims"], c["size"], color=col is not None)
    trk.upload_tsdf(c["vol"])
    if col is not None:
        trk.upload_color(col)
    return trk


def planes_of(hsk, c):
    return hsk.split_planes(c["abcd"], c["kinds"])


def split(hsk, trk, c, **over):
    return trk.split_scene(planes_of(hsk, c), **dict({k: (int(v) if k == "min_voxels" else float(v)) for k, v in c["params"].items()}, **over))


def check_split(hsk, trk, key):
    """splits; everything the three read calls give equals the twin's"""
    c = SC.case_of(key)
    t_cls, t_plane, t_label, t_recs, t_st = SC.twin_of(key)
    recs, st = split(hsk, trk, c)
    print(f"{key}: {st['n_class'].tolist()} objects {st['n_objects']} minor {st['n_minor_objects']} largest {st['largest']} edge {st['n_edge']} flat {st['n_no_normal']}")
    assert records_as_dicts(recs) == t_recs, key
    assert st.pop("reused") == 0 and {k: (v.tolist() if k == "n_class" else v) for k, v in st.items()} == t_st, key
    cls, plane, label = trk.download_split()
    assert cls.dtype == np.uint8 and int((cls != t_cls).sum()) == 0, f"{key}: {int((cls != t_cls).sum())} class bytes differ"
    assert plane.dtype == np.uint8 and int((plane != t_plane).sum()) == 0, f"{key}: {int((plane != t_plane).sum())} plane bytes differ"
    assert label.dtype == np.uint32 and int((label != t_label).sum()) == 0, f"{key}: {int((label != t_label).sum())} labels differ"
    X, Y, Z = c["dims"]
    for lo, hi in ([c["box"]] if c["box"] else []) + [((13, 5, 3), (19, 18, 8)), ((0, 0, Z - 1), (X, Y, Z)), ((3, 3, 3), (3, 9, 9))]:
        at = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        pc, pp, pl = trk.download_split(box=(lo, hi))
        assert pc.shape == (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]), (key, lo, hi)
        assert np.array_equal(pc, t_cls[at]) and np.array_equal(pp, t_plane[at]) and np.array_equal(pl, t_label[at]), (key, lo, hi)
    assert trk.download_split(plane=False, object=False)[1:] == (None, None)
    pts = SC.query_points(c["dims"], c["size"])
    for radius in (0, 2, 4):
        for got, want in zip(trk.split_at(pts, radius), ST.split_at(t_cls, t_plane, t_label, c["size"], pts, radius)):
            assert np.array_equal(got, want), f"{key}: split_at radius {radius}"
    return st


def check_remove(hsk, trk, key, which, mode, halo, fw):
    c, col = SC.case_of(key), SC.color_of(key)
    t_out, t_col, t_st = SC.remove_twin(key, which, mode, halo, fw)
    st = trk.remove_objects(SC.roots_of(key, which), mode=mode, halo=halo, fill_weight=fw)
    print(f"{key} remove {which} mode {mode} halo {halo} weight {fw}: {st}")
    assert st == t_st, key
    out = trk.download_tsdf()
    assert int((out != t_out).sum()) == 0, f"{key}: {int((out != t_out).any(axis=-1).sum())} words differ"
    if col is not None:
        assert trk.download_color().tobytes() == t_col.tobytes(), f"{key}: colour"
    return st


# ---- 1. every shared case: random volumes with 0, 1, 7 and 64 planes, anisotropic cells, the rooms, the hand-built shapes ------------
@pytest.mark.parametrize("key", SC.all_keys(), ids=lambda k: " ".join(str(v) for v in k))
def test_the_split_and_its_removals_match_the_twin(hsk, key):
    """46 and 41 planes: the last plane group holds padding planes, which are no voxels; 72 x 56: X and Y are 8 mod 16, the last
    tiles of the labelling are half empty; size (2.7, 2.8, 1.6): w = (4096, 3072, 3840)"""
    c, col = SC.case_of(key), SC.color_of(key)
    trk = loaded(hsk, key)
    try:
        t = ST.default_params(c["size"], c["dims"])
        p = trk.default_split_params()
        assert (p.dist_m, p.back_m, p.cos_min, p.min_voxels) == (float(t["dist_m"]), float(t["back_m"]), float(t["cos_min"]), t["min_voxels"])
        assert trk.default_remove_params().halo == ST.default_halo(c["size"], c["dims"])
        check_split(hsk, trk, key)
        for i, (which, mode, halo, fw) in enumerate(c["removes"]):
            if i > 0:                                          # (the removal before changed the volume: the same split again from the same upload)
                trk.upload_tsdf(c["vol"])
                if col is not None:
                    trk.upload_color(col)
                assert records_as_dicts(split(hsk, trk, c)[0]) == SC.twin_of(key)[3]
            check_remove(hsk, trk, key, which, mode, halo, fw)
    finally:
        trk.close()


# ---- 2. properties on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a box on the floor", "a box against the wall", "a box lifted off the floor"])
def test_a_removal_gives_the_empty_room(hsk, name):
    """DESIGN.md 8r, on the analytic room: after remove_objects(RESTORE, halo 3) the volume equals the empty room within 1 raw unit
    wherever both are observed, and the crossing counts are the empty room's: 2400 z, 0 y, 1632 x"""
    key = ("room", name)
    trk = loaded(hsk, key)
    try:
        recs, st = split(hsk, trk, SC.case_of(key))
        assert len(recs) == 1 and int(recs[0]["plane_mask"]) == {"a box on the floor": 1, "a box against the wall": 3, "a box lifted off the floor": 0}[name]
        rst = trk.remove_objects(halo=3)
        out, empty = trk.download_tsdf(), DT.room(None)
        both = (out[..., 1] != 0) & (empty[..., 1] != 0)
        worst = int(np.abs(out[..., 0].astype(np.int64) - empty[..., 0])[both].max())
        counts = [int(x.sum()) for x in DT.crossings(out)]
        print(f"{name}: {rst}, worst difference {worst}, crossings {counts}")
        assert worst <= 1 and counts == [2400, 0, 1632]
        recs, st = split(hsk, trk, SC.case_of(key))
        assert len(recs) == 0 and st["n_class"][ST.OBJECT] == st["n_class"][ST.MINOR] == 0
    finally:
        trk.close()


def test_the_split_is_held_and_dropped_with_the_volume(hsk):
    key = ("room", "two boxes")
    c = SC.case_of(key)
    trk = loaded(hsk, key)
    try:
        for call in (lambda: trk.download_split(), lambda: trk.split_at(np.zeros((1, 3), np.float32)), lambda: trk.remove_objects()):
            with pytest.raises(hsk.KinfuError, match="no split is held"):
                call()
        trk.label_components()
        r1, s1 = split(hsk, trk, c)
        d1 = trk.download_split()
        assert s1["reused"] == 0 and trk.label_components()[1]["labels_reused"] == 1          # the split's labelling is its own
        r2, s2 = split(hsk, trk, c)
        assert s2["reused"] == 1 and r1.tobytes() == r2.tobytes() and {k: np.asarray(v).tolist() for k, v in s1.items() if k != "reused"} == {
            k: np.asarray(v).tolist() for k, v in s2.items() if k != "reused"}
        assert all(np.array_equal(x, y) for x, y in zip(d1, trk.download_split()))
        # other parameters and other planes are not answered from the held split: both boxes fall below 5000 voxels
        r3, s3 = split(hsk, trk, c, min_voxels=5000)
        assert s3["reused"] == 0 and len(r3) == 0 and s3["n_minor_objects"] == 2 and s3["n_class"][ST.MINOR] == s1["n_class"][ST.OBJECT]
        r4, s4 = trk.split_scene(hsk.split_planes(c["abcd"][:1], c["kinds"][:1]), **{k: float(v) for k, v in c["params"].items() if k != "min_voxels"}, min_voxels=64)
        assert s4["reused"] == 0 and s4["n_class"][ST.WALL] == 0
        r5, s5 = split(hsk, trk, c)
        assert s5["reused"] == 0 and r5.tobytes() == r1.tobytes() and all(np.array_equal(x, y) for x, y in zip(d1, trk.download_split()))
        # an empty selection writes nothing and keeps cached passes and the split
        assert trk.remove_objects([]) == {"n_objects": 0, "n_targets": 0, "n_written": 0, "n_restored": 0, "n_colored": 0}
        assert trk.label_components()[1]["labels_reused"] == 1 and np.array_equal(trk.download_tsdf(), c["vol"])
        assert all(np.array_equal(x, y) for x, y in zip(d1, trk.download_split())) and split(hsk, trk, c)[1]["reused"] == 1
        trk.release_split()
        with pytest.raises(hsk.KinfuError, match="no split is held"):
            trk.download_split()
        assert split(hsk, trk, c)[1]["reused"] == 0 and all(np.array_equal(x, y) for x, y in zip(d1, trk.download_split()))
        # dropped after any volume change: a removal, an upload, an integrate
        assert trk.remove_objects(halo=2)["n_written"] > 0
        lib = trk.lib
        cls = np.full(c["vol"].shape[:3], 9, np.uint8)
        assert lib.hsk_download_split(trk.h, None, cls.ctypes.data, None, None) == -3 and (cls == 9).all()
        split(hsk, trk, c)
        trk.upload_tsdf(c["vol"])
        one = np.zeros(3, np.float32)
        assert lib.hsk_split_at(trk.h, one.ctypes.data, 1, 0, cls.ctypes.data, None, None) == -3 and (cls == 9).all()
        split(hsk, trk, c)
        pose = hsk.synth_pose(0)
        trk.integrate(hsk.synth_depth(pose), pose)
        st = hsk._lib.HskRemoveStats(n_written=77)
        assert lib.hsk_remove_objects(trk.h, None, 0, None, C.byref(st)) == -3 and st.n_written == 77
    finally:
        trk.close()


def test_every_subset_of_the_optional_arrays_gives_the_full_calls_bytes(hsk):
    """hsk_split_at, hsk_download_split and hsk_download_diff called directly with their optional arrays null, both or each alone, on
    the small room's 32 x 24 x 20 grid and a box that is neither empty nor the whole volume: cls, and whichever array is present,
    equal the full call's (an absent array takes no room in the product buffer: the others move up)"""
    key = ("shape", "objects in the small room")
    c = SC.case_of(key)
    trk, cur = loaded(hsk, key), volume_ctx(hsk, c["dims"], c["size"])
    try:
        lib = trk.lib
        recs, _ = split(hsk, trk, c)
        assert len(recs) > 0
        pts = SC.query_points(c["dims"], c["size"])
        full = trk.split_at(pts, 2)
        assert len(set(full[1].tolist())) > 1 and len(set(full[2].tolist())) > 1          # (planes and objects are both met)
        for want_plane, want_object in ((False, False), (True, False), (False, True)):
            cls, pln, obj = np.full(len(pts), 9, np.uint8), np.full(len(pts), 9, np.uint8), np.full(len(pts), 9, np.uint32)
            assert lib.hsk_split_at(trk.h, pts.ctypes.data, len(pts), 2, cls.ctypes.data, pln.ctypes.data if want_plane else None,
                                    obj.ctypes.data if want_object else None) == 0
            assert np.array_equal(cls, full[0]) and np.array_equal(pln, full[1] if want_plane else np.full(len(pts), 9, np.uint8))
            assert np.array_equal(obj, full[2] if want_object else np.full(len(pts), 9, np.uint32)), (want_plane, want_object)
        lo, hi = (3, 2, 1), (29, 20, 17)
        box = hsk._lib.HskVoxelBox((C.c_int * 3)(*lo), (C.c_int * 3)(*hi))
        shape = (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])
        full = trk.download_split(box=(lo, hi))
        assert full[0].shape == shape and len(np.unique(full[1])) > 1 and len(np.unique(full[2])) > 1
        for want_plane, want_object in ((False, False), (True, False), (False, True)):
            cls, pln, obj = np.full(shape, 9, np.uint8), np.full(shape, 9, np.uint8), np.full(shape, 9, np.uint32)
            assert lib.hsk_download_split(trk.h, C.byref(box), cls.ctypes.data, pln.ctypes.data if want_plane else None,
                                          obj.ctypes.data if want_object else None) == 0
            assert np.array_equal(cls, full[0]) and np.array_equal(pln, full[1] if want_plane else np.full(shape, 9, np.uint8))
            assert np.array_equal(obj, full[2] if want_object else np.full(shape, 9, np.uint32)), (want_plane, want_object)
        # the diff against the small room without its objects
        cur.upload_tsdf(SC.small_room())
        regions, _ = trk.diff_volume(cur, min_voxels=1)
        assert len(regions) > 0
        full = trk.download_diff(box=(lo, hi))
        assert full[0].shape == shape and len(np.unique(full[0])) > 1 and len(np.unique(full[1])) > 1
        for want_region in (False, True):
            cls, reg = np.full(shape, 9, np.uint8), np.full(shape, 9, np.uint32)
            assert lib.hsk_download_diff(trk.h, C.byref(box), cls.ctypes.data, reg.ctypes.data if want_region else None) == 0
            assert np.array_equal(cls, full[0]) and np.array_equal(reg, full[1] if want_region else np.full(shape, 9, np.uint32)), want_region
    finally:
        trk.close()
        cur.close()


def test_the_context_after_a_removal_equals_a_fresh_one_with_the_same_words(hsk):
    key = ("room", "two boxes")
    c, col = SC.case_of(key), SC.color_of(key)
    trk, fresh = loaded(hsk, key), volume_ctx(hsk, c["dims"], c["size"], color=True)
    try:
        split(hsk, trk, c)
        trk.label_components()
        trk.coverage()
        assert trk.remove_objects(halo=3)["n_restored"] > 0
        out, out_col = trk.download_tsdf(), trk.download_color()
        fresh.upload_tsdf(out)
        fresh.upload_color(out_col)
        for x, y in zip(trk.extract_cloud_attrs(), fresh.extract_cloud_attrs()):
            assert x is None or same_bits(np.asarray(x), np.asarray(y)), "cloud"
        (ra, sa), (rb, sb) = trk.label_components(), fresh.label_components()
        assert ra.tobytes() == rb.tobytes() and sa["labels_reused"] == 0 and sa["n_inside"] == sb["n_inside"]
        assert np.array_equal(trk.download_components(), fresh.download_components())
        ca, cb = trk.coverage(), fresh.coverage()
        assert {k: np.asarray(v).tolist() for k, v in ca.items()} == {k: np.asarray(v).tolist() for k, v in cb.items()}
    finally:
        trk.close()
        fresh.close()


def test_errors_leave_everything_untouched(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    key = ("room", "two boxes")
    c = SC.case_of(key)
    trk = loaded(hsk, key)
    try:
        trk.label_components()
        recs, _ = split(hsk, trk, c)
        held = trk.download_split()
        good = planes_of(hsk, c)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(L.HskSplitPlane))
        n = C.c_size_t(77)
        for bad in (dict(dist_m=0.0), dict(dist_m=1.5), dict(back_m=0.0), dict(back_m=2.5), dict(cos_min=-0.1), dict(cos_min=1.1), dict(cos_min=float("nan")),
                    dict(min_voxels=0)):
            p = hsk.default_split_params(trk, **bad)
            assert lib.hsk_split_scene(trk.h, ptr(good), len(good), C.byref(p), None, 0, C.byref(n), None) == -1 and n.value == 77 and lib.hsk_last_error(trk.h), bad
        for i, (field, value) in enumerate((("abcd", [np.nan, 0, 1, 0]), ("abcd", [0, 0, 1, np.inf]), ("abcd", [0, 0, 0.4, 0]), ("abcd", [0, 0, 2.1, 0]), ("abcd", [0, 0, 1, 64.5]),
                                            ("kind", 0), ("kind", 5))):
            pl = good.copy()
            pl[field][1] = value
            assert lib.hsk_split_scene(trk.h, ptr(pl), len(pl), None, None, 0, C.byref(n), None) == -1 and n.value == 77, (field, value)
        many = hsk.split_planes(np.tile(c["abcd"][:1], (65, 1)), 1)
        assert lib.hsk_split_scene(trk.h, ptr(many), 65, None, None, 0, C.byref(n), None) == -1 and b"64 planes" in lib.hsk_last_error(trk.h)
        assert lib.hsk_split_scene(trk.h, None, 2, None, None, 0, C.byref(n), None) == -1 and lib.hsk_split_scene(trk.h, ptr(good), 2, None, None, 0, None, None) == -1
        for mode, halo, fw in ((2, 2, 1), (-1, 2, 1), (1, -1, 1), (1, 9, 1), (1, 2, 0), (1, 2, 129)):
            p, st = L.HskRemoveParams(mode, halo, fw), L.HskRemoveStats(n_written=77)
            assert lib.hsk_remove_objects(trk.h, None, 0, C.byref(p), C.byref(st)) == -1 and st.n_written == 77, (mode, halo, fw)
        with pytest.raises(hsk.KinfuError, match="no kept object"):
            trk.remove_objects([5])
        with pytest.raises(hsk.KinfuError, match="256 roots"):
            trk.remove_objects(np.zeros(257, np.uint32))
        X, Y, Z = c["dims"]
        for lo, hi in (((-1, 0, 0), (X, Y, Z)), ((0, 0, 0), (X, Y + 1, Z)), ((0, 0, 5), (X, Y, 4))):
            with pytest.raises(hsk.KinfuError, match="the box must satisfy"):
                trk.download_split(box=(lo, hi))
        for radius in (5, -1):
            with pytest.raises(hsk.KinfuError, match="radius"):
                trk.split_at(np.zeros((1, 3), np.float32), radius)
        with pytest.raises(TypeError, match="no field"):
            trk.split_scene(good, halo=3)
        # cap below the count: the counts are set, no record is written, the split is held
        out = np.zeros(2, hsk.kinfu.OBJECT_DTYPE)
        st = L.HskSplitStats()
        p = hsk.default_split_params(trk, **{k: (int(v) if k == "min_voxels" else float(v)) for k, v in c["params"].items()})
        assert lib.hsk_split_scene(trk.h, ptr(good), len(good), C.byref(p), out.ctypes.data_as(C.POINTER(L.HskObject)), 1, C.byref(n), C.byref(st)) == -1
        assert n.value == 2 and st.n_objects == 2 and st.reused == 1 and not out.tobytes().strip(b"\0")
        assert trk.label_components()[1]["labels_reused"] == 1 and np.array_equal(trk.download_tsdf(), c["vol"])
        assert all(np.array_equal(x, y) for x, y in zip(held, trk.download_split()))
    finally:
        trk.close()
    # between submit and wait; a context that stores part of its volume; the slabs of a group
    busy = hsk.KinfuTracker(n=64)
    try:
        busy.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        busy.split_scene(None)
        busy.submit_frame(hsk.synth_depth(hsk.synth_pose(1)))
        n, cls = C.c_size_t(77), np.full(64 ** 3, 9, np.uint8)
        assert lib.hsk_split_scene(busy.h, None, 0, None, None, 0, C.byref(n), None) == -3 and n.value == 77 and b"in flight" in lib.hsk_last_error(busy.h)
        assert lib.hsk_download_split(busy.h, None, cls.ctypes.data, None, None) == -3 and (cls == 9).all() and lib.hsk_remove_objects(busy.h, None, 0, None, None) == -3
        _, ok = busy.wait_frame()
        assert ok and busy.split_scene(None)[1]["n_class"].sum() == 64 ** 3
    finally:
        busy.close()
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        for call in (lambda: part.split_scene(None), lambda: part.download_split(), lambda: part.remove_objects(), lambda: part.split_at(np.zeros((1, 3), np.float32))):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call()
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        for i in range(g.n_slabs()):
            for call in (lambda t: t.split_scene(None), lambda t: t.download_split()):
                with pytest.raises(hsk.KinfuError, match="slab"):
                    call(g.slab(i))
    finally:
        g.close()


# ---- 3. end to end through the tracker ------------------------------------------------------------------------------------------------
def test_a_box_in_a_scanned_room_is_an_object_and_can_be_taken_out(hsk):
    """room 0 scanned at 128^3 with every twelfth frame of the script, a box composited into the depth (tests/test_gpu_diff.py's:
    hovering 1.4 voxels above the floor); the planes from detect_planes, their kinds from estimate_upright: the box is a kept
    object whose voxel box contains the true box's; after its removal hsk_label_components finds no component inside the true box"""
    cell = 3.0 / 128
    vlo, vhi = (38, 89, 34), (56, 115, 52)
    lo, hi = tuple((v + 0.4) * cell for v in vlo), tuple((v - 0.4) * cell for v in vhi)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 720, 12)]
    trk = hsk.KinfuTracker(n=128, init_pose=poses[0])
    try:
        for p in poses:
            trk.integrate(hsk.synth_box_depth(hsk.synth_room_depth(0, p), p, lo, hi), p)
        planes, _ = trk.detect_planes()
        up = -np.asarray(trk.estimate_upright()["level"], np.float64).reshape(4, 4)[1, :3]
        pl = hsk.split_plane_kinds(planes["abcd"], up)
        recs, st = trk.split_scene(pl)
        print(f"box in a scanned room: planes {pl['kind'].tolist()}, {st['n_class'].tolist()}, objects {st['n_objects']}, minor {st['n_minor_objects']}")
        print([(c["n_voxels"], c["lo"].tolist(), c["hi"].tolist(), c["contact"].tolist(), hex(int(c["plane_mask"]))) for c in recs[:8]])
        # (the walls' false objects are larger than the room's furniture: the box is the one object that contains the true box and
        # ends within 3 voxels of it)
        box = [c for c in recs if all(vlo[i] - 3 <= c["lo"][i] <= vlo[i] and vhi[i] <= c["hi"][i] <= vhi[i] + 3 for i in range(3))]
        assert len(box) == 1
        root = (int(box[0]["root"][2]) * 128 + int(box[0]["root"][1])) * 128 + int(box[0]["root"][0])
        rst = trk.remove_objects([root])
        print(f"removed: {rst}")
        assert rst["n_targets"] == int(box[0]["n_voxels"])
        labels = trk.download_components()[vlo[2]:vhi[2], vlo[1]:vhi[1], vlo[0]:vhi[0]]
        assert int((labels != hsk._lib.HSK_COMPONENT_NONE).sum()) == 0
    finally:
        trk.close()
