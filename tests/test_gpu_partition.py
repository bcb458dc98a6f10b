"""The room partition on the GPU: hsk_build_partition, hsk_partition_doors, hsk_download_partition, hsk_download_partition_cost,
hsk_partition_at and hsk_partition_floor against the numpy restatement of the rule (tests/partition_twin.py), every id, key, record,
door and stat EQUAL: two rooms with a door at the threshold where one core becomes two; ragged speckled volumes with hundreds of
cores, dropped ones, and the cap of 1024; ties at the corner eight tiles share and on a mirror plane of voxels; a long spread
through a serpentine; one-voxel corridors where the labelling alone decides; the carved room at the default parameters; the cache;
a volume with deferred weights while a scan goes on; the point lookup; the floor form; the errors.  Unless said otherwise the
volumes are hand-built from FREE and SOLID words with clearance flags 0: the twin alone decides the expectations."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import clearance_twin as CL
import partition_twin as PT
import reach_twin as RE
from clearance_cases import SCENE_DEFAULTS, twin_field
from components_cases import injected_volume
from cover_cases import carved_volume
from kit import volume_ctx
from partition_cases import (DOOR_THRESHOLD, MIRROR_DIMS, MIRROR_PAD, RAGGED, clear_params, d2_of, mirror_rooms, ragged_case, serpentine_core_d2, twin_partition)
from reach_cases import CORNER_DIMS, SERPENTINE_DIMS, SOLID_WORD, TILE, WEIGHTS, centre, corridors, scene_size, serpentine, tile_corner, two_rooms

pytestmark = pytest.mark.gpu
f32 = np.float32
STAT_KEYS = ("n_cores", "n_rooms", "n_dropped", "n_passable", "n_assigned", "n_doors")


def ctx(hsk, dims, size=None, **over):
    return volume_ctx(hsk, dims, size or scene_size(dims), **over)


def scratch_bound(dims, n_rooms):
    """12 bytes per voxel, four words per tile, the tables of 1024 rooms, 64 bytes per pair of rooms -- of the most rooms the context
    has had: the door table only grows --, and the 256-byte rounding"""
    tiles = int(np.prod([-(-n // t) for n, t in zip(dims, TILE)]))
    return 12 * dims[0] * dims[1] * dims[2] + 16 * tiles + 3 * 4096 + 1024 * 128 + 64 * n_rooms * n_rooms + 12 * 256


def same_records(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), (name, got[name][:4], want[name][:4])


def check(trk, name, vol, weight, scale, **par):
    """build, the three downloads and the doors of a hand-built volume equal the twin's; -> (the build's stats, the twin's dict)"""
    Z, Y, X = vol.shape[:3]
    rooms, st = trk.build_partition(**clear_params(weight, scale), **par)
    p = twin_partition(name, d2_of(name, vol, weight, scale), weight, **par)
    print(f"{name} {weight} {par}: {st}, tiles {trk.partition_tiles_relaxed()}")
    ids, cost = trk.download_partition(), trk.download_partition_cost()
    assert ids.dtype == np.uint32 and ids.shape == p["ids"].shape and int((ids != p["ids"]).sum()) == 0, f"{int((ids != p['ids']).sum())} ids differ"
    assert int((cost != p["cost"]).sum()) == 0, f"{int((cost != p['cost']).sum())} costs differ"
    assert {k: st[k] for k in STAT_KEYS} == p["stats"] and st["reused"] == 0
    same_records(rooms, p["rooms"])
    same_records(trk.partition_doors(), p["doors"])
    trk.most_rooms = max(getattr(trk, "most_rooms", 0), st["n_rooms"])
    assert st["scratch_bytes"] <= scratch_bound((X, Y, Z), trk.most_rooms)
    return st, p


# ---- 1. two rooms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sealed", [False, True])
def test_two_rooms_open_and_sealed(hsk, sealed):
    vol = two_rooms(sealed)
    name = "two sealed rooms" if sealed else "two rooms"
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        for weight in WEIGHTS:
            thr = DOOR_THRESHOLD[weight]
            lower, _ = check(trk, name, vol, weight, 4096, core_d2=thr, min_d2=min(weight), min_core_voxels=1, max_cost=RE.MAX_COST)
            upper, p = check(trk, name, vol, weight, 4096, core_d2=thr + 1, min_d2=min(weight), min_core_voxels=1, max_cost=RE.MAX_COST)
            assert (lower["n_rooms"], upper["n_rooms"]) == ((2, 2) if sealed else (1, 2)) and upper["n_doors"] == (0 if sealed else 1)
            assert upper["n_assigned"] == upper["n_passable"] and upper["n_rounds"] >= 1
            if not sealed:
                assert p["rooms"]["n_voxels"].tolist() == [123360, 119808] and p["doors"]["n_faces"].tolist() == [[480, 0, 0]]
    finally:
        trk.close()


# ---- 2. ragged shapes, dropping, the cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", RAGGED)
def test_ragged_speckled_volumes_match_the_twin(hsk, dims):
    """41 and 46 planes: a last plane of tiles that is part empty; 72: a last tile a quarter full; hundreds of cores, most dropped"""
    trk = ctx(hsk, dims)
    try:
        for weight in WEIGHTS:
            for min_core in (1, 8):
                vol, d2, par = ragged_case(dims, weight, min_core)
                if weight == WEIGHTS[0] and min_core == 1:
                    trk.upload_tsdf(vol)
                st, p = check(trk, f"speckled {dims}", vol, weight, 16, **par)
                assert st["n_cores"] >= 500 and st["n_rooms"] >= 16 and (min_core == 1) == (st["n_dropped"] == 0) and st["n_passable"] > st["n_assigned"]
        if dims == RAGGED[1]:
            lib, L = hsk._lib.load(), hsk._lib
            cp = trk.default_clearance_params(**clear_params((16, 25, 44)))
            pp = trk.default_partition_params(cp, core_d2=9 * 16, min_d2=16, min_core_voxels=1)
            st, n = L.HskPartitionStats(n_cores=77), C.c_size_t(5)
            assert lib.hsk_build_partition(trk.h, C.byref(cp), C.byref(pp), None, 0, C.byref(n), C.byref(st)) == -1 and b"HSK_PARTITION_MAX_ROOMS" in lib.hsk_last_error(trk.h)
            assert (st.n_cores, st.n_rooms, st.n_dropped, st.n_doors, st.n_rounds, st.n_assigned, n.value) == (1121, 1121, 0, 0, 0, 0, 5)
            with pytest.raises(hsk.KinfuError, match="no partition"):
                trk.download_partition()
            vol, d2, par = ragged_case(dims, (16, 25, 44), 8)
            check(trk, f"speckled {dims}", vol, (16, 25, 44), 16, **par)
    finally:
        trk.close()


# ---- 3. ties --------------------------------------------------------------------------------------------------------------------------------
def test_ties_at_the_tile_corner_and_on_a_mirror_plane(hsk):
    trk = ctx(hsk, CORNER_DIMS)
    try:
        vol = tile_corner()
        trk.upload_tsdf(vol)
        st, p = check(trk, "tile corner", vol, (1, 1, 1), 16, core_d2=4, min_d2=1, min_core_voxels=1, max_cost=RE.MAX_COST)
        assert p["rooms"]["n_voxels"].tolist() == [1473, 1473] and p["doors"]["n_faces"].tolist() == [[2, 2, 2]]
    finally:
        trk.close()
    trk = ctx(hsk, (MIRROR_DIMS[0] + MIRROR_PAD,) + MIRROR_DIMS[1:])          # (a volume's X is a multiple of 8: the odd scene, padded with solid planes)
    try:
        vol = mirror_rooms(MIRROR_PAD)
        trk.upload_tsdf(vol)
        for weight in WEIGHTS:
            st, p = check(trk, "mirror rooms, padded", vol, weight, 16, core_d2=9 * min(weight), min_d2=min(weight), min_core_voxels=1, max_cost=RE.MAX_COST)
            plane = p["ids"][:, :, MIRROR_DIMS[0] // 2]
            assert st["n_rooms"] == 2 and (plane[plane < PT.NONE] == 0).all() and (plane < PT.NONE).sum() == 16
            odd = twin_partition("mirror rooms", d2_of("mirror rooms", mirror_rooms(), weight), weight, 9 * min(weight), min(weight), 1)
            assert np.array_equal(p["ids"][:, :, :MIRROR_DIMS[0]], odd["ids"]) and (p["ids"][:, :, MIRROR_DIMS[0]:] == PT.BLOCKED).all()
    finally:
        trk.close()


# ---- 4. a long spread -------------------------------------------------------------------------------------------------------------------------
def test_a_long_spread_through_the_serpentine(hsk):
    vol, walls = serpentine()
    trk = ctx(hsk, SERPENTINE_DIMS)
    try:
        trk.upload_tsdf(vol)
        for weight in WEIGHTS:
            st, p = check(trk, "serpentine", vol, weight, 256, core_d2=serpentine_core_d2(weight), min_d2=min(weight), min_core_voxels=1, max_cost=RE.MAX_COST)
            relaxed, first, tiles = trk.partition_tiles_relaxed()
            assert st["n_rooms"] == st["n_cores"] == 2 and st["n_rounds"] >= 5 and relaxed > tiles >= first >= 1, "tiles are re-entered"
            assert walls[1] < p["doors"]["lo"][0][0] and p["doors"]["hi"][0][0] <= walls[-2] + 1, "the rooms meet mid-way"
            seeds = [(int(x), int(y), int(z)) for z, y, x in np.argwhere(p["cost"] == 0)]
            ref, _ = RE.field(d2_of("serpentine", vol, weight, 256), weight, min(weight), RE.MAX_COST, seeds)
            assert np.array_equal(trk.download_partition_cost(), ref) and (ref == RE.UNREACHED).sum() == 0
        # max_cost: what lies beyond it stays unassigned
        weight = WEIGHTS[1]
        cap = int(np.sort(p["cost"][p["cost"] <= RE.MAX_COST])[p["cost"].size // 2])
        st, q = check(trk, "serpentine", vol, weight, 256, core_d2=serpentine_core_d2(weight), min_d2=min(weight), min_core_voxels=1, max_cost=cap)
        assert st["n_passable"] - st["n_assigned"] >= 1000 and q["rooms"]["max_g"].max() == cap and st["n_doors"] == 0
    finally:
        trk.close()


# ---- 5. corridors: the labelling alone ---------------------------------------------------------------------------------------------------------
def test_one_voxel_corridors_across_tile_faces(hsk):
    """core_d2 = min_d2: every free voxel is a core voxel.  The corridors cross the face x = TILE_X in the rows (0, 0) -- local 0 of
    its tile on y and z -- and step round the corner eight tiles share from local TILE - 1 to local 0 on every axis"""
    vol, _ = corridors()
    trk = ctx(hsk, CORNER_DIMS)
    try:
        trk.upload_tsdf(vol)
        for weight in WEIGHTS:
            st, p = check(trk, "corridors", vol, weight, 16, core_d2=min(weight), min_d2=min(weight), min_core_voxels=1, max_cost=RE.MAX_COST)
            assert (st["n_rooms"], st["n_rounds"], st["n_doors"]) == (2, 0, 0) and p["rooms"]["n_voxels"].tolist() == [2 * TILE[0], 2 * TILE[0] - 2]
            assert np.array_equal(p["rooms"]["n_core_voxels"], p["rooms"]["n_voxels"])
        st, p = check(trk, "corridors", vol, (1, 1, 1), 16, core_d2=1, min_d2=1, min_core_voxels=2 * TILE[0], max_cost=RE.MAX_COST)
        assert (st["n_rooms"], st["n_dropped"], st["n_assigned"], st["n_passable"]) == (1, 1, 2 * TILE[0], 4 * TILE[0] - 2)
    finally:
        trk.close()


# ---- 6. the carved room at default parameters -----------------------------------------------------------------------------------------------
def test_the_carved_room_at_default_parameters(hsk):
    vol = carved_volume()
    d = SCENE_DEFAULTS
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        want = PT.default_params(d, AT.DST_SIZE, AT.DST_DIMS)
        pp = trk.default_partition_params()
        assert (pp.core_d2, pp.min_d2, pp.min_core_voxels, pp.max_cost, pp.flags) == (want["core_d2"], 1, want["min_core_voxels"], RE.MAX_COST, 0)
        p = twin_partition("carved", twin_field("carved", vol, d["weight"], d["max_d2"], CL.UNKNOWN), d["weight"], **want)
        rooms, st = trk.build_partition()
        print(f"the carved room: {st}")
        assert {k: st[k] for k in STAT_KEYS} == p["stats"] and st["reused"] == 0 and st["n_rooms"] >= 1 and st["n_assigned"] >= 10000
        assert np.array_equal(trk.download_partition(), p["ids"]) and np.array_equal(trk.download_partition_cost(), p["cost"])
        same_records(rooms, p["rooms"])
        same_records(trk.partition_doors(), p["doors"])
        again_rooms, again = trk.build_partition()
        assert (again["reused"], again["n_rounds"]) == (1, 0) and {k: again[k] for k in STAT_KEYS} == p["stats"]
        same_records(again_rooms, p["rooms"])
        assert trk.build_clearance()["reused"] == 1 and np.array_equal(trk.download_tsdf(), vol)
    finally:
        trk.close()


# ---- 7. the cache; deferred weights ------------------------------------------------------------------------------------------------------------
def test_the_cache(hsk):
    vol = injected_volume()[0]
    d = SCENE_DEFAULTS
    want = PT.default_params(d, AT.DST_SIZE, AT.DST_DIMS)

    def twin(v):
        return PT.partition(CL.field(v, d["weight"], d["max_d2"], CL.UNKNOWN), d["weight"], **want)

    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        rooms, first = trk.build_partition()
        assert first["reused"] == 0 and first["n_rooms"] >= 1
        assert trk.build_partition()[1]["reused"] == 1 and trk.build_partition(unit_m=0.5, **want)[1]["reused"] == 1, "unit_m is not the device's"
        assert np.array_equal(trk.download_partition(), twin(vol)["ids"])
        for change in (dict(core_d2=want["core_d2"] - 1), dict(min_d2=2), dict(min_core_voxels=want["min_core_voxels"] + 1), dict(max_cost=50000),
                       dict(max_d2=d["max_d2"] - 1), dict(flags=0), dict(weight=(16, 25, 45))):
            kw = dict(want, **change)
            a, b = trk.build_partition(**kw)[1], trk.build_partition(**kw)[1]
            assert (a["reused"], b["reused"], b["n_rounds"]) == (0, 1, 0), change
        assert trk.build_partition()[1]["reused"] == 0 and trk.build_partition()[1]["reused"] == 1          # back to the defaults: built again
        trk.upload_tsdf(vol)
        assert trk.build_partition()[1]["reused"] == 0, "a volume change invalidates the partition"
        assert trk.prune_components()["n_pruned"] > 0
        with pytest.raises(hsk.KinfuError, match="no partition"):
            trk.partition_doors()
        rooms, st = trk.build_partition()
        pruned = twin(trk.download_tsdf())
        assert st["reused"] == 0 and np.array_equal(trk.download_partition(), pruned["ids"])
        same_records(rooms, pruned["rooms"])
        trk.release_partition()
        with pytest.raises(hsk.KinfuError, match="no partition"):
            trk.download_partition()
        trk.release_partition()
        st = trk.build_partition()[1]
        assert st["reused"] == 0 and st["scratch_bytes"] == first["scratch_bytes"] and trk.build_clearance()["reused"] == 1
        box = ((3, 5, 7), (77, 33, 48))
        whole, cost = trk.download_partition(), trk.download_partition_cost()
        assert np.array_equal(trk.download_partition(box=box), whole[7:48, 5:33, 3:77]) and np.array_equal(trk.download_partition_cost(box=box), cost[7:48, 5:33, 3:77])
        assert trk.download_partition(box=((4, 4, 4), (4, 9, 9))).size == 0
    finally:
        trk.close()


def test_a_volume_with_deferred_weights_while_a_scan_goes_on(hsk):
    """24 frames of room 0 integrated at 64^3 leave free-space weights in the summaries; the partition is built BEFORE any download
    and equals the twin fed by the download of a second, identically grown context; one more frame: it is built again"""
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 300, 12)]
    depths = [hsk.synth_room_depth(0, p) for p in poses]

    def grown(n):
        trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
        for d, p in zip(depths[:n], poses[:n]):
            trk.integrate(d, p)
        return trk

    par = dict(core_d2=100, min_d2=1, min_core_voxels=8, max_cost=RE.MAX_COST)
    a, b = grown(24), grown(24)
    try:
        rooms, st = b.build_partition(flags=0, **par)
        ids = b.download_partition()
        vol = a.download_tsdf()
        assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
        p = PT.partition(CL.field(vol, (1, 1, 1), 456, 0), (1, 1, 1), **par)
        print(f"deferred weights: {st}")
        assert st["reused"] == 0 and int((ids != p["ids"]).sum()) == 0 and {k: st[k] for k in STAT_KEYS} == p["stats"] and st["n_assigned"] >= 1000
        same_records(rooms, p["rooms"])
        assert b.build_partition(flags=0, **par)[1]["reused"] == 1 and np.array_equal(b.download_tsdf(), vol)
        for t in (a, b):
            t.integrate(depths[24], poses[24])
        with pytest.raises(hsk.KinfuError, match="no partition"):
            b.partition_at([(1.5, 1.5, 1.5)])
        st3 = b.build_partition(flags=0, **par)[1]
        vol3 = a.download_tsdf()
        assert st3["reused"] == 0 and not np.array_equal(vol3, vol)
        assert np.array_equal(b.download_partition(), PT.partition(CL.field(vol3, (1, 1, 1), 456, 0), (1, 1, 1), **par)["ids"])
    finally:
        a.close()
        b.close()


# ---- 8. the point lookup ----------------------------------------------------------------------------------------------------------------------
def test_partition_at(hsk):
    """two sealed rooms with a wall two voxels thick: a point in the wall's left voxel gets the left room, one in its right voxel
    the right room, for every radius above 0; radius 0 asks the voxel itself"""
    vol = two_rooms(True)
    vol[:, :, 41] = SOLID_WORD
    weight = (16, 25, 44)
    par = dict(core_d2=DOOR_THRESHOLD[weight] + 1, min_d2=min(weight), min_core_voxels=1, max_cost=RE.MAX_COST)
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        with pytest.raises(hsk.KinfuError, match="no partition"):
            trk.partition_at(np.ones((3, 3), f32))
        st, p = check(trk, "two rooms, a thick wall", vol, weight, 4096, **par)
        assert st["n_rooms"] == 2
        rng = np.random.default_rng(8)
        many = rng.uniform(-0.2, 3.2, (600, 3)).astype(f32)
        many[:3] = ((np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, 1.0))
        left = np.array([centre((40, y, z), AT.DST_DIMS) for y, z in rng.integers(0, 48, (50, 2))], f32)
        right = np.array([centre((41, y, z), AT.DST_DIMS) for y, z in rng.integers(0, 48, (50, 2))], f32)
        for radius in (0, 2, 4):
            want = PT.lookup(p["ids"], weight, AT.DST_SIZE, many, radius)
            got = trk.partition_at(many, radius)
            assert got.dtype == np.uint32 and np.array_equal(got, want), radius
            assert (got[:2] == PT.OUTSIDE).all() and got[2] == 0 and min((want == PT.OUTSIDE).sum(), (want < PT.NONE).sum()) >= 100
            in_wall = (trk.partition_at(left, radius).tolist(), trk.partition_at(right, radius).tolist())
            assert in_wall == (([0] * 50, [1] * 50) if radius else ([PT.NONE] * 50, [PT.NONE] * 50)), radius
            assert np.array_equal(trk.partition_at(left, radius), PT.lookup(p["ids"], weight, AT.DST_SIZE, left, radius))
        assert len(trk.partition_at(np.zeros((0, 3), f32), 2)) == 0
    finally:
        trk.close()


# ---- 9. the floor form ------------------------------------------------------------------------------------------------------------------------
def test_floor_maps(hsk):
    vol = two_rooms(False)
    vol[:, :10, 20] = SOLID_WORD                                  # a stub wall in the left room
    weight = (16, 25, 44)
    cp = clear_params(weight, 4096)
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        n_rooms = 0
        for axis, lo, hi in ((1, 10, 40), (1, 0, 64), (2, 0, 30), (2, 30, 48), (2, 7, 7), (0, 39, 42)):
            au = 1 if axis == 0 else 0
            for core in (DOOR_THRESHOLD[weight] + 1, 400):
                par = dict(core_d2=core, min_d2=weight[au], min_core_voxels=4, max_cost=RE.MAX_COST)
                fmap, rooms, doors, st = trk.partition_floor(axis, lo, hi, **cp, **par)
                want = PT.floor(vol, weight, cp["max_d2"], 0, axis, lo, hi, **par)
                assert fmap.shape == want["ids"][0].shape and int((fmap != want["ids"][0]).sum()) == 0, (axis, lo, hi, core)
                assert {k: st[k] for k in STAT_KEYS} == want["stats"] and st["reused"] == 0, (axis, lo, hi, core, st, want["stats"])
                same_records(rooms, want["rooms"])
                same_records(doors, want["doors"])
                n_rooms += st["n_rooms"]
        assert n_rooms >= 12
        fmap, rooms, doors, st = trk.partition_floor(2, 0, 30, **cp, core_d2=DOOR_THRESHOLD[weight] + 1, min_d2=16, min_core_voxels=1)
        assert st["n_rooms"] == 2 and doors["n_faces"].tolist() == [[16, 0, 0]] and doors["lo"].tolist() == [[40, 24, 0]] and (rooms["root"][:, 2] == 0).all()
    finally:
        trk.close()


# ---- 10. errors -------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    vol = two_rooms(False)
    weight = (16, 25, 44)
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        out = np.full(80 * 64 * 48, 9, np.uint32)
        recs, doors = np.full(8, 9, PT.ROOM_DTYPE), np.full(8, 9, PT.DOOR_DTYPE)
        pts = np.array([(1.0, 1.5, 1.4), (2.0, 0.8, 2.2)], f32)
        n, m = C.c_size_t(5), C.c_size_t(6)
        st = L.HskPartitionStats(n_cores=77)

        def untouched():
            return (out == 9).all() and (recs["n_voxels"] == 9).all() and (doors["a"] == 9).all() and st.n_cores == 77

        # reads with no partition held
        assert lib.hsk_download_partition(trk.h, None, out.ctypes.data) == -3 and b"no partition" in lib.hsk_last_error(trk.h)
        assert lib.hsk_download_partition_cost(trk.h, None, out.ctypes.data) == -3 and lib.hsk_partition_at(trk.h, pts.ctypes.data, 2, 0, out.ctypes.data) == -3
        assert lib.hsk_partition_doors(trk.h, doors.ctypes.data, 8, C.byref(n)) == -3 and n.value == 5 and untouched()
        par = dict(core_d2=DOOR_THRESHOLD[weight] + 1, min_d2=16, min_core_voxels=1)
        cp = trk.default_clearance_params(**clear_params(weight, 4096))
        pp = trk.default_partition_params(cp, **par)
        first_rooms, first = trk.build_partition(cp, pp)
        first_doors = trk.partition_doors()
        ids = trk.download_partition()
        assert (first["n_rooms"], first["n_doors"]) == (2, 1)

        def refused(cpar, ppar, code=-1):
            assert lib.hsk_build_partition(trk.h, C.byref(cpar), C.byref(ppar), recs.ctypes.data, 8, C.byref(n), C.byref(st)) == code and lib.hsk_last_error(trk.h)
            assert lib.hsk_partition_floor(trk.h, C.byref(cpar), 1, 0, 4, C.byref(ppar), out.ctypes.data, recs.ctypes.data, 8, C.byref(n), doors.ctypes.data, 8,
                                           C.byref(m), C.byref(st)) == code
            assert untouched() and (n.value, m.value) == (5, 6)

        for bad in (dict(min_d2=0), dict(min_d2=par["core_d2"] + 1), dict(core_d2=cp.max_d2 + 1), dict(core_d2=15), dict(max_cost=RE.MAX_COST + 1)):
            refused(cp, trk.default_partition_params(cp, **dict(par, **bad)))
        flagged = trk.default_partition_params(cp, **par)
        flagged.flags = 1
        refused(cp, flagged)
        for bad in (dict(weight=(0, 1, 1)), dict(flags=2), dict(max_d2=16 * 256 * 256)):
            refused(trk.default_clearance_params(**bad), pp)
        # a cap too small: the count, and nothing else
        assert lib.hsk_build_partition(trk.h, C.byref(cp), C.byref(pp), recs.ctypes.data, first["n_rooms"] - 1, C.byref(n), C.byref(st)) == -1
        assert n.value == first["n_rooms"] and untouched() and b"cap" in lib.hsk_last_error(trk.h)
        assert lib.hsk_build_partition(trk.h, C.byref(cp), C.byref(pp), recs.ctypes.data, 8, None, C.byref(st)) == -1 and untouched()
        n.value = 5
        assert lib.hsk_partition_doors(trk.h, doors.ctypes.data, first["n_doors"] - 1, C.byref(n)) == -1 and n.value == first["n_doors"] and untouched()
        assert lib.hsk_partition_doors(trk.h, doors.ctypes.data, 8, None) == -1 and untouched()
        assert lib.hsk_partition_doors(trk.h, None, 0, C.byref(n)) == 0 and n.value == first["n_doors"]
        n.value, m.value = 5, 6
        assert lib.hsk_partition_floor(trk.h, C.byref(cp), 1, 10, 40, C.byref(pp), out.ctypes.data, recs.ctypes.data, 0, C.byref(n), doors.ctypes.data, 0, C.byref(m),
                                       C.byref(st)) == -1 and untouched() and n.value >= 1 and b"cap" in lib.hsk_last_error(trk.h)
        n.value, m.value = 5, 6
        for axis, lo, hi in ((-1, 0, 1), (3, 0, 1), (0, -1, 4), (0, 0, 81), (1, 0, 65), (2, 0, 49), (2, 9, 8)):
            assert lib.hsk_partition_floor(trk.h, C.byref(cp), axis, lo, hi, C.byref(pp), out.ctypes.data, None, 0, None, None, 0, None, C.byref(st)) == -1 and untouched()
        assert lib.hsk_partition_floor(trk.h, C.byref(cp), 1, 0, 4, C.byref(pp), None, None, 0, None, None, 0, None, None) == -1
        for lo, hi in (((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (81, 4, 4)), ((0, 5, 0), (4, 4, 4)), ((0, 0, 0), (4, 4, 49))):
            b = L.HskVoxelBox()
            b.lo[:], b.hi[:] = lo, hi
            assert lib.hsk_download_partition(trk.h, C.byref(b), out.ctypes.data) == -1 and b"box" in lib.hsk_last_error(trk.h)
            assert lib.hsk_download_partition_cost(trk.h, C.byref(b), out.ctypes.data) == -1
        assert lib.hsk_download_partition(trk.h, None, None) == -1 and lib.hsk_download_partition_cost(trk.h, None, None) == -1
        assert lib.hsk_partition_at(trk.h, pts.ctypes.data, (1 << 20) + 1, 0, out.ctypes.data) == -1 and b"2^20" in lib.hsk_last_error(trk.h)
        assert lib.hsk_partition_at(trk.h, None, 2, 0, out.ctypes.data) == -1 and lib.hsk_partition_at(trk.h, pts.ctypes.data, 2, 0, None) == -1
        for radius in (-1, 5):
            assert lib.hsk_partition_at(trk.h, pts.ctypes.data, 2, radius, out.ctypes.data) == -1 and b"radius" in lib.hsk_last_error(trk.h)
        assert untouched()
        with pytest.raises(hsk.KinfuError, match="min_d2"):
            trk.build_partition(min_d2=0)
        again_rooms, again = trk.build_partition(cp, pp)
        assert again["reused"] == 1 and {k: again[k] for k in STAT_KEYS} == {k: first[k] for k in STAT_KEYS}
        same_records(again_rooms, first_rooms)
        same_records(trk.partition_doors(), first_doors)
        assert np.array_equal(trk.download_partition(), ids) and np.array_equal(trk.download_tsdf(), vol)
        assert lib.hsk_build_partition(trk.h, None, None, None, 0, None, None) == 0                      # NULL parameters: the defaults; counts only, no stats
    finally:
        trk.close()
    # between submit and wait
    trk = hsk.KinfuTracker(n=64)
    try:
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        trk.build_partition(flags=0, core_d2=100, min_core_voxels=8)
        trk.submit_frame(hsk.synth_depth(hsk.synth_pose(1)))
        out, st, pts, n = np.full(64 ** 3, 9, np.uint32), L.HskPartitionStats(n_cores=77), np.full((2, 3), 1.5, f32), C.c_size_t(5)
        assert lib.hsk_build_partition(trk.h, None, None, None, 0, C.byref(n), C.byref(st)) == -3 and st.n_cores == 77 and b"in flight" in lib.hsk_last_error(trk.h)
        assert lib.hsk_download_partition(trk.h, None, out.ctypes.data) == -3 and lib.hsk_partition_at(trk.h, pts.ctypes.data, 2, 1, out.ctypes.data) == -3
        assert lib.hsk_partition_doors(trk.h, None, 0, C.byref(n)) == -3 and n.value == 5
        assert lib.hsk_partition_floor(trk.h, None, 1, 0, 4, None, out.ctypes.data, None, 0, None, None, 0, None, C.byref(st)) == -3 and st.n_cores == 77
        assert (out == 9).all()
        _, ok = trk.wait_frame()
        assert ok and trk.build_partition(flags=0, core_d2=100, min_core_voxels=8)[1]["reused"] == 0
    finally:
        trk.close()
    # a context that stores part of its volume
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        one = np.full((1, 3), 1.5, f32)
        for call in (lambda t: t.build_partition(), lambda t: t.download_partition(), lambda t: t.download_partition_cost(), lambda t: t.partition_doors(),
                     lambda t: t.partition_at(one), lambda t: t.partition_floor(1, 0, 4)):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call(part)
    finally:
        part.close()
