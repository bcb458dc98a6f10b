"""Volume differencing on the device (hsk_diff_volume, hsk_download_diff, hsk_diff_at, hsk_adopt_diff) against
the numpy twin (tests/diff_twin.py): class bytes, region labels, records in order, every stats field, the point query and the
adopted volume and colour are EQUAL to the twin's."""
import ctypes as C

import numpy as np
import pytest

import diff_cases as DC
import diff_twin as DT
import fuse_twin as FT
from diff_cases import records_as_dicts
from kit import dims_of, same_bits, volume_ctx

pytestmark = pytest.mark.gpu
CELL = 0.05      # the hand-built grids' cell; the truncation distance is then 2.1 cells


def size_of(dims):
    return tuple(CELL * d for d in dims)


def ctx(hsk, dims, size=None, color=False, **over):
    return volume_ctx(hsk, dims, size or size_of(dims), color, **over)


def pair(hsk, ref, cur, ref_color=None, cur_color=None):
    """two contexts on one grid holding the two volumes (and colour volumes)"""
    dims = dims_of(ref)
    a, b = ctx(hsk, dims, color=ref_color is not None), ctx(hsk, dims, color=cur_color is not None)
    a.upload_tsdf(ref)
    b.upload_tsdf(cur)
    if ref_color is not None:
        a.upload_color(ref_color)
    if cur_color is not None:
        b.upload_color(cur_color)
    return a, b


def check_diff(a, b, name, twin, params, box=None):
    """diffs b against a; everything the three read calls give equals the twin's"""
    t_cls, t_region, t_recs, t_st = twin
    recs, st = a.diff_volume(b, **params)
    print(f"{name}: {st['n_class'].tolist()} regions {st['n_regions']} minor {st['n_minor_regions']} largest {st['largest']}")
    assert records_as_dicts(recs) == t_recs, name
    assert {k: (v.tolist() if k == "n_class" else v) for k, v in st.items()} == t_st, name
    cls, region = a.download_diff()
    assert cls.dtype == np.uint8 and int((cls != t_cls).sum()) == 0, f"{name}: {int((cls != t_cls).sum())} class bytes differ"
    assert region.dtype == np.uint32 and int((region != t_region).sum()) == 0, f"{name}: {int((region != t_region).sum())} labels differ"
    X, Y, Z = dims_of(t_cls[..., None])
    for lo, hi in ([box] if box else []) + [((13, 5, 3), (19, 18, 8)), ((0, 0, Z - 1), (X, Y, Z)), ((3, 3, 3), (3, 9, 9))]:
        pc, pr = a.download_diff(box=(lo, hi))
        assert pc.shape == (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]) and np.array_equal(pc, t_cls[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]), (name, lo, hi)
        assert np.array_equal(pr, t_region[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]), (name, lo, hi)
    assert a.download_diff(region=False)[1] is None
    size = size_of((X, Y, Z))
    pts = DC.query_points((X, Y, Z), size)
    for radius in (0, 2, 4):
        got_c, got_r = a.diff_at(pts, radius)
        ref_c, ref_r = DT.diff_at(t_cls, t_region, size, pts, radius)
        assert np.array_equal(got_c, ref_c) and np.array_equal(got_r, ref_r), f"{name}: diff_at radius {radius}"
    return st


def check_adopt(a, b, name, key, ref, cur, t_cls, which, halo, ca, cb):
    t_out, t_col, t_st = DC.adopt_twin(key, ref, cur, t_cls, which, halo, ca, cb)
    st = a.adopt_diff(b, which, halo)
    print(f"{name} which {which} halo {halo}: {st}")
    assert st == t_st, name
    out = a.download_tsdf()
    assert int((out != t_out).sum()) == 0, f"{name}: {int((out != t_out).any(axis=-1).sum())} words differ"
    if ca is not None:
        assert a.download_color().tobytes() == t_col.tobytes(), f"{name}: colour"
    assert np.array_equal(b.download_tsdf(), cur) and (cb is None or b.download_color().tobytes() == cb.tobytes()), f"{name}: cur was touched"
    return st


# ---- 1. random pairs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", DC.RANDOM_DIMS)
def test_random_pairs_match_the_twin(hsk, dims):
    """46 and 41 planes: the last plane group holds padding planes, which are no voxels; 72 x 56: X and Y are 8 mod 16, the last
    tiles of the labelling are half empty"""
    ref, cur = DC.random_pair(dims)
    ca, cb = DC.random_colors(dims)
    twin = DC.random_twin(dims)
    a, b = pair(hsk, ref, cur, ca, cb)
    try:
        st = check_diff(a, b, f"random {dims}", twin, dict(min_voxels=DC.RANDOM_MIN_VOXELS))
        assert st["n_regions"] >= 3 and st["n_minor_regions"] >= 1
        check_adopt(a, b, f"random {dims}", ("random", dims), ref, cur, twin[0], DC.BOTH, 2, ca, cb)
    finally:
        a.close()
        b.close()


# ---- 2. hand-built shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DC.shapes()))
def test_hand_built_shapes_match_the_twin(hsk, name):
    c = DC.shapes()[name]
    ca, cb = DC.colors_of(name)
    twin = DC.shape_twin(name)
    a, b = pair(hsk, c["ref"], c["cur"], ca, cb)
    try:
        check_diff(a, b, name, twin, c["params"], c["box"])
        for i, (which, halo) in enumerate(c["adopts"]):
            if i > 0:                                          # (the adopt before changed ref: the same diff again from the same upload)
                a.upload_tsdf(c["ref"])
                if ca is not None:
                    a.upload_color(ca)
                recs, _ = a.diff_volume(b, **c["params"])
                assert records_as_dicts(recs) == twin[2]
            check_adopt(a, b, name, ("shape", name), c["ref"], c["cur"], twin[0], which, halo, ca, cb)
    finally:
        a.close()
        b.close()


# ---- 3. properties on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [1, 2])
def test_after_an_adopt_the_diff_is_empty_and_the_surfaces_are_curs(hsk, halo):
    """DESIGN.md 8q, on the analytic room: with halo >= 1 differencing again finds no CHANGED voxel, ref's zero crossings are
    cur's, and ref equals cur on every voxel both observe"""
    c = DC.shapes()["the box appears"]
    a, b = pair(hsk, c["ref"], c["cur"])
    try:
        a.diff_volume(b, **c["params"])
        assert a.adopt_diff(b, halo=halo)["n_targets"] == 2758
        recs, st = a.diff_volume(b, min_voxels=1)
        assert len(recs) == 0 and st["n_class"][DT.APPEARED] + st["n_class"][DT.VANISHED] + st["n_class"][DT.MINOR] == 0
        out = a.download_tsdf()
        assert all(np.array_equal(x, y) for x, y in zip(DT.crossings(out), DT.crossings(c["cur"])))
        both = (out[..., 1] != 0) & (c["cur"][..., 1] != 0)
        assert np.array_equal(out[both], c["cur"][both])
    finally:
        a.close()
        b.close()


def test_an_empty_adopt_writes_nothing_and_a_second_diff_gives_the_same_bytes(hsk):
    c = DC.shapes()["the wall shifted by 0.5"]
    a, b = pair(hsk, c["ref"], c["cur"])
    try:
        a.label_components()
        recs, st = a.diff_volume(b, **c["params"])
        first = a.download_diff()
        assert a.label_components()[1]["labels_reused"] == 1          # the diff's labelling is its own
        assert a.adopt_diff(b) == {"n_targets": 0, "n_adopted": 0, "n_colored": 0}
        assert a.label_components()[1]["labels_reused"] == 1 and np.array_equal(a.download_tsdf(), c["ref"])
        assert all(np.array_equal(x, y) for x, y in zip(first, a.download_diff()))          # the diff is still held
        recs2, st2 = a.diff_volume(b, **c["params"])
        assert len(recs2) == len(recs) == 0 and st2["n_class"].tolist() == st["n_class"].tolist()
        assert all(np.array_equal(x, y) for x, y in zip(first, a.download_diff()))
        a.release_diff()
        with pytest.raises(hsk.KinfuError, match="no diff is held"):
            a.download_diff()
        a.diff_volume(b, **c["params"])
        assert all(np.array_equal(x, y) for x, y in zip(first, a.download_diff()))
    finally:
        a.close()
        b.close()
    c = DC.shapes()["the box moves"]
    a, b = pair(hsk, c["ref"], c["cur"])
    try:
        r1, s1 = a.diff_volume(b, **c["params"])
        d1 = a.download_diff()
        r2, s2 = a.diff_volume(b, **c["params"])
        assert r1.tobytes() == r2.tobytes() and s1["n_class"].tolist() == s2["n_class"].tolist()
        assert all(np.array_equal(x, y) for x, y in zip(d1, a.download_diff()))
        # other parameters are not answered from the held diff: both regions (1221 voxels each) fall below 2000
        r3, s3 = a.diff_volume(b, min_voxels=2000)
        t3 = DT.diff(c["ref"], c["cur"], min_voxels=2000)
        assert len(r3) == 0 and s3["n_class"].tolist() == t3[3]["n_class"] and s3["n_minor_regions"] == 2 and np.array_equal(a.download_diff()[0], t3[0])
        r4, s4 = a.diff_volume(b, **c["params"])
        assert r4.tobytes() == r1.tobytes() and all(np.array_equal(x, y) for x, y in zip(d1, a.download_diff()))
        # ... nor is another cur with the same volume, nor the same cur after its volume changed
        b.upload_tsdf(c["ref"])
        assert len(a.diff_volume(b, **c["params"])[0]) == 0
    finally:
        a.close()
        b.close()


# ---- 4. two real scans: deferred weights, and ref is a whole context after the adopt -----------------------------------------------
ROOM_CELL = 3.0 / 64


def scanned_pair(hsk, n, frames, lo, hi):
    """(ref, cur) at n^3: the same frames of room 0 at the script's own poses, cur's with the box lo .. hi composited into the depth"""
    poses = [hsk.synth_room_pose(0, k, 720) for k in frames]
    ref, cur = hsk.KinfuTracker(n=n, init_pose=poses[0]), hsk.KinfuTracker(n=n, init_pose=poses[0])
    for p in poses:
        d = hsk.synth_room_depth(0, p)
        ref.integrate(d, p)
        cur.integrate(hsk.synth_box_depth(d, p, lo, hi), p)
    return ref, cur


def test_the_adopted_context_equals_a_fresh_one_with_the_same_volume(hsk):
    """ref and cur are grown by integrate and hold deferred free-space weights: the diff, run BEFORE any download, equals the
    twin fed by the downloads of two identically grown contexts; after the adopt a cloud, a raycast and one more integrate agree
    byte for byte with a fresh context that was handed the same volume by upload"""
    lo, hi = (0.9, 2.1, 0.8), (1.3, 2.65, 1.2)
    frames = list(range(600, 720, 12))
    a, b = scanned_pair(hsk, 64, frames, lo, hi)
    a2, b2 = scanned_pair(hsk, 64, frames, lo, hi)
    fresh = hsk.KinfuTracker(n=64)
    try:
        mv = 100                                   # (at 64^3 the box's shell has 339 voxels, below the default of 593)
        recs, st = a.diff_volume(b, min_voxels=mv)
        ref, cur = a2.download_tsdf(), b2.download_tsdf()
        assert (ref[..., 1] > 1).any() and a.default_diff_params().min_voxels == DT.default_min_voxels((3.0,) * 3, (64,) * 3, 2.1 * 3.0 / 64)
        t_cls, t_region, t_recs, t_st = DT.diff(ref, cur, min_voxels=mv)
        print(f"scanned pair: {st['n_class'].tolist()}, {len(recs)} regions, min_voxels {mv}")
        assert records_as_dicts(recs) == t_recs and st["n_class"].tolist() == t_st["n_class"] and len(recs) >= 1
        cls, region = a.download_diff()
        assert np.array_equal(cls, t_cls) and np.array_equal(region, t_region)
        ast = a.adopt_diff(b)
        t_out, _, t_ast = DT.adopt(ref, cur, t_cls)
        tsdf = a.download_tsdf()
        assert ast == t_ast and ast["n_adopted"] > 0 and np.array_equal(tsdf, t_out) and np.array_equal(b.download_tsdf(), cur)
        fresh.upload_tsdf(tsdf)
        for x, y in zip(a.extract_cloud_attrs(rgb=False), fresh.extract_cloud_attrs(rgb=False)):
            assert x is None or same_bits(np.asarray(x), np.asarray(y)), "cloud"
        assert a.extract_cloud(cap=0)[1] > 1000
        pose = hsk.synth_room_pose(0, 640, 720)
        for x, y in zip(a.raycast(pose, want_keys=True), fresh.raycast(pose, want_keys=True)):
            assert same_bits(x, y), "raycast"
        depth = hsk.synth_room_depth(0, pose)
        a.integrate(depth, pose)
        fresh.integrate(depth, pose)
        assert a.integrate_coarse_counts() == fresh.integrate_coarse_counts()
        ta, tb = a.download_tsdf(), fresh.download_tsdf()
        assert np.array_equal(ta, tb) and not np.array_equal(ta, tsdf)
    finally:
        for t in (a, b, a2, b2, fresh):
            t.close()


# ---- 5. through the resampling chain --------------------------------------------------------------------------------------------------
def test_a_cur_in_another_frame_is_resampled_then_diffed(hsk):
    """cur lives in a frame rotated by a few degrees about the room's centre and shifted: resampled_like puts it on ref's grid --
    equal, bit for bit, to the twin's fusion into an empty volume -- and the diff of that equals the twin's"""
    c = DC.shapes()["the box appears"]
    ref, cur = c["ref"], c["cur"]
    dims = dims_of(ref)
    size = size_of(dims)
    m = FT.rot_about("z", 3.0, tuple(0.5 * s for s in size), (0.04, -0.03, 0.02))
    empty = np.zeros_like(ref)
    res, _, fst = FT.fuse(empty, size, cur, size, m)
    twin = DT.diff(ref, res, min_voxels=64)
    assert fst["n_fused"] > 50000 and twin[3]["n_regions"] >= 1
    a, b = pair(hsk, ref, cur)
    r = b.resampled_like(a, m)
    try:
        assert np.array_equal(r.download_tsdf(), res)
        check_diff(a, r, "resampled", twin, dict(min_voxels=64))
        with pytest.raises(hsk.KinfuError, match="same grid"):
            other = ctx(hsk, (dims[0], dims[1], dims[2] + 4))
            try:
                a.diff_volume(other)
            finally:
                other.close()
    finally:
        for t in (a, b, r):
            t.close()


def test_a_box_carried_into_a_scanned_room_is_one_region(hsk):
    """room 0 scanned twice at 128^3 with every twelfth frame of the script, the second time with a box composited into the depth
    (its faces 0.4 voxel inside their boundary voxels' centres, hovering 1.4 voxels above the floor, so that every boundary voxel
    of its voxel box lies within the truncation band behind a face the camera sees): exactly one kept region, and its box
    contains the box's voxel box"""
    cell = 3.0 / 128
    vlo, vhi = (38, 89, 34), (56, 115, 52)
    lo, hi = tuple((v + 0.4) * cell for v in vlo), tuple((v - 0.4) * cell for v in vhi)
    a, b = scanned_pair(hsk, 128, list(range(0, 720, 12)), lo, hi)
    try:
        recs, st = a.diff_volume(b)
        print(f"box in a scanned room: {records_as_dicts(recs)}, {st['n_class'].tolist()}, minor regions {st['n_minor_regions']}")
        assert len(recs) == 1
        assert all(recs[0]["lo"][i] <= vlo[i] and vhi[i] <= recs[0]["hi"][i] for i in range(3))
        assert recs[0]["n_appeared"] > 500
    finally:
        a.close()
        b.close()


# ---- 6. validity and errors -----------------------------------------------------------------------------------------------------------
def test_the_diff_is_held_while_both_volumes_stand(hsk):
    c = DC.shapes()["the box moves"]
    a, b = pair(hsk, c["ref"], c["cur"])
    third = ctx(hsk, dims_of(c["ref"]))
    lib = a.lib
    try:
        third.upload_tsdf(c["cur"])
        for call in (lambda: a.download_diff(), lambda: a.diff_at(np.zeros((1, 3), np.float32)), lambda: a.adopt_diff(b)):
            with pytest.raises(hsk.KinfuError, match="no diff is held"):
                call()
        a.diff_volume(b, **c["params"])
        held = a.download_diff()
        # a third context, and cur changed: the adopt is refused, ref and the held diff stay
        with pytest.raises(hsk.KinfuError, match="no diff is held for the volumes"):
            a.adopt_diff(third)
        b.upload_tsdf(c["cur"])
        with pytest.raises(hsk.KinfuError, match="no diff is held for the volumes"):
            a.adopt_diff(b)
        assert np.array_equal(a.download_tsdf(), c["ref"]) and all(np.array_equal(x, y) for x, y in zip(held, a.download_diff()))
        a.diff_volume(b, **c["params"])
        assert a.adopt_diff(b)["n_adopted"] > 0
        with pytest.raises(hsk.KinfuError, match="no diff is held"):       # after a write the held diff is no longer valid
            a.download_diff()
        # ref changed by an integrate
        a.diff_volume(b, **c["params"])
        pose = hsk.synth_pose(0)
        a.integrate(hsk.synth_depth(pose), pose)
        cls = np.full(c["ref"].shape[:3], 9, np.uint8)
        assert lib.hsk_download_diff(a.h, None, cls.ctypes.data, None) == -3 and (cls == 9).all()
        one = np.zeros(3, np.float32)
        assert lib.hsk_diff_at(a.h, one.ctypes.data, 1, 0, cls.ctypes.data, None) == -3 and (cls == 9).all()
        st = hsk._lib.HskAdoptStats(n_adopted=77)
        assert lib.hsk_adopt_diff(a.h, b.h, None, C.byref(st)) == -3 and st.n_adopted == 77
    finally:
        for t in (a, b, third):
            t.close()


def test_errors_leave_everything_untouched(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    c = DC.shapes()["the box moves"]
    dims = dims_of(c["ref"])
    a, b = pair(hsk, c["ref"], c["cur"])
    try:
        a.label_components()
        a.diff_volume(b, **c["params"])
        held = a.download_diff()
        n = C.c_size_t(77)
        for bad in (dict(thresh=0), dict(thresh=65535), dict(min_weight=0), dict(min_weight=129), dict(min_voxels=0)):
            p = hsk.default_diff_params(a, **bad)
            assert lib.hsk_diff_volume(a.h, b.h, C.byref(p), None, 0, C.byref(n), None) == -1 and n.value == 77 and lib.hsk_last_error(a.h), bad
        assert lib.hsk_diff_volume(a.h, a.h, None, None, 0, C.byref(n), None) == -1 and b"same context" in lib.hsk_last_error(a.h)
        assert lib.hsk_diff_volume(a.h, None, None, None, 0, C.byref(n), None) == -1 and lib.hsk_diff_volume(a.h, b.h, None, None, 0, None, None) == -1
        for other in (ctx(hsk, (dims[0] + 8, dims[1], dims[2])), ctx(hsk, dims, size=(3.3, 2.4, 2.0)), ctx(hsk, dims, trunc_dist_m=0.2)):
            try:
                assert lib.hsk_diff_volume(a.h, other.h, None, None, 0, C.byref(n), None) == -1 and b"hsk_fuse_volume into an empty context" in lib.hsk_last_error(a.h)
            finally:
                other.close()
        assert n.value == 77
        for which, halo in ((0, 2), (4, 2), (3, -1), (3, 9)):
            p, st = L.HskAdoptParams(which, halo), L.HskAdoptStats(n_adopted=77)
            assert lib.hsk_adopt_diff(a.h, b.h, C.byref(p), C.byref(st)) == -1 and st.n_adopted == 77, (which, halo)
        assert lib.hsk_adopt_diff(a.h, a.h, None, None) == -1 and lib.hsk_adopt_diff(a.h, None, None, None) == -1
        X, Y, Z = dims
        for lo, hi in (((-1, 0, 0), (X, Y, Z)), ((0, 0, 0), (X, Y + 1, Z)), ((0, 0, 5), (X, Y, 4))):
            with pytest.raises(hsk.KinfuError, match="the box must satisfy"):
                a.download_diff(box=(lo, hi))
        with pytest.raises(hsk.KinfuError, match="radius"):
            a.diff_at(np.zeros((1, 3), np.float32), 5)
        with pytest.raises(hsk.KinfuError, match="radius"):
            a.diff_at(np.zeros((1, 3), np.float32), -1)
        with pytest.raises(TypeError, match="no field"):
            a.diff_volume(b, halo=3)
        # cap below the count: the counts are set, no record is written, the diff is held
        recs = np.zeros(2, hsk.kinfu.DIFF_REGION_DTYPE)
        st = L.HskDiffStats()
        p = hsk.default_diff_params(a, **c["params"])
        assert lib.hsk_diff_volume(a.h, b.h, C.byref(p), recs.ctypes.data_as(C.POINTER(L.HskDiffRegion)), 1, C.byref(n), C.byref(st)) == -1
        assert n.value == 2 and st.n_regions == 2 and not recs.tobytes().strip(b"\0")
        assert a.label_components()[1]["labels_reused"] == 1 and np.array_equal(a.download_tsdf(), c["ref"])
        assert all(np.array_equal(x, y) for x, y in zip(held, a.download_diff()))
    finally:
        a.close()
        b.close()
    # between submit and wait, in either context
    trk, idle = hsk.KinfuTracker(n=64), hsk.KinfuTracker(n=64)
    try:
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        idle.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        idle.diff_volume(trk)
        trk.submit_frame(hsk.synth_depth(hsk.synth_pose(1)))
        n, cls = C.c_size_t(77), np.full(64 ** 3, 9, np.uint8)
        for ref, cur in ((trk, idle), (idle, trk)):
            assert lib.hsk_diff_volume(ref.h, cur.h, None, None, 0, C.byref(n), None) == -3 and n.value == 77 and b"in flight" in lib.hsk_last_error(ref.h)
            assert lib.hsk_adopt_diff(ref.h, cur.h, None, None) == -3
        assert lib.hsk_download_diff(trk.h, None, cls.ctypes.data, None) == -3 and (cls == 9).all()
        _, ok = trk.wait_frame()
        assert ok and idle.diff_volume(trk)[1]["n_class"].sum() == 64 ** 3
    finally:
        trk.close()
        idle.close()
    # a context that stores part of its volume, and the slabs of a group
    part, whole = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32), hsk.KinfuTracker(n=64)
    try:
        for call in (lambda: part.diff_volume(whole), lambda: whole.diff_volume(part), lambda: part.download_diff(), lambda: part.adopt_diff(whole),
                     lambda: part.diff_at(np.zeros((1, 3), np.float32))):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call()
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        for i in range(g.n_slabs()):
            for call in (lambda t: t.diff_volume(whole), lambda t: whole.diff_volume(t), lambda t: t.download_diff()):
                with pytest.raises(hsk.KinfuError, match="slab"):
                    call(g.slab(i))
        _, ok = g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))
        assert ok
    finally:
        g.close()
        whole.close()
