"""The reach field on the GPU: hsk_build_reach, hsk_download_reach, hsk_reach_at, hsk_reach_path and hsk_reach_floor against the numpy
restatement of the rule (tests/reach_twin.py), every value, count and flag EQUAL: the carved room at the default parameters; ragged
speckled volumes; a serpentine whose shortest path re-enters tiles; the box rule; a path across the corner eight tiles share; the
seeds; max_cost; the cache; a volume with deferred weights while a scan goes on; the lookup and the path; the floor form; what it is
for (viewpoints nobody can walk to leave the head of the ranking); the errors.  Unless said otherwise the volumes are hand-built
from FREE and SOLID words with clearance flags 0 and min_d2 = min(weight): the twin alone decides the expectations."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import clearance_twin as CL
import reach_twin as RE
import reloc_twin as RT
from clearance_cases import SCENE_DEFAULTS, twin_field
from components_cases import injected_volume, speckled
from cover_cases import EYE, carved_volume
from kit import same_bits, state_of, volume_ctx
from reach_cases import (CORNER_DIMS, FREE_WORD, SERPENTINE_DIMS, SOLID_WORD, STAIR_DIMS, TILE, WEIGHTS, centre, check_path, corridors, free_volume, hand_d2, hand_params, scene_size, serpentine, staircase, tile_corner, twin_reach, two_rooms)

pytestmark = pytest.mark.gpu
f32 = np.float32
STAT_KEYS = ("n_passable", "n_reached", "max_cost_seen")


def ctx(hsk, dims, size=None, **over):
    return volume_ctx(hsk, dims, size or scene_size(dims), **over)


def scratch_bound(dims):
    """one word per voxel, four per tile, and the 256-byte rounding of the six arrays"""
    tiles = int(np.prod([-(-n // t) for n, t in zip(dims, TILE)]))
    return 4 * dims[0] * dims[1] * dims[2] + 16 * tiles + 6 * 256


def check_hand(trk, name, vol, weight, pts, max_cost=RE.MAX_COST, min_reached=1000):
    """build + download for a hand-built volume equal the twin's field; -> (the build's stats, the twin's field)"""
    Z, Y, X = vol.shape[:3]
    cp, min_d2 = hand_params(weight)
    st = trk.build_reach(pts, min_d2=min_d2, max_cost=max_cost, **cp)
    g = trk.download_reach()
    ref, used = twin_reach(name, hand_d2(vol, weight), weight, min_d2, max_cost, tuple(RE.seed_voxels(scene_size((X, Y, Z)), (X, Y, Z), pts)))
    print(f"{name} {weight} max_cost {max_cost}: {st}")
    assert g.dtype == np.uint32 and g.shape == ref.shape and int((g != ref).sum()) == 0, f"{int((g != ref).sum())} values differ"
    assert {k: st[k] for k in STAT_KEYS} == RE.stats(ref) and st["n_seeds_used"] == used and st["reused"] == 0
    assert st["scratch_bytes"] <= scratch_bound((X, Y, Z)) and st["n_reached"] >= min_reached
    return st, ref


# ---- 1. the carved room at default parameters ------------------------------------------------------------------------------------------
def carved_reference():
    d = SCENE_DEFAULTS
    d2 = twin_field("carved", carved_volume(), d["weight"], d["max_d2"], CL.UNKNOWN)
    return twin_reach("carved", d2, d["weight"], RE.default_params(d)["min_d2"], RE.MAX_COST, tuple(RE.seed_voxels(AT.DST_SIZE, AT.DST_DIMS, [EYE])))


def test_the_carved_room_matches_the_twin(hsk):
    vol = carved_volume()
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        p = trk.default_reach_params()
        assert (p.min_d2, p.max_cost, p.flags) == (RE.default_params(SCENE_DEFAULTS)["min_d2"], RE.MAX_COST, 0)
        ref, used = carved_reference()
        st = trk.build_reach([EYE])
        g = trk.download_reach()
        print(f"the carved room: {st}")
        assert g.dtype == np.uint32 and int((g != ref).sum()) == 0
        assert {k: st[k] for k in STAT_KEYS} == RE.stats(ref) and (st["n_seeds_used"], st["reused"]) == (used, 0) and st["n_rounds"] >= 1
        assert st["n_reached"] >= 1000 and (ref == RE.BLOCKED).sum() == 80 * 64 * 48 - st["n_passable"] >= 100000
        assert st["scratch_bytes"] <= scratch_bound(AT.DST_DIMS)
        again = trk.build_reach([EYE])
        assert {k: again[k] for k in STAT_KEYS} == RE.stats(ref) and (again["reused"], again["n_rounds"], again["n_seeds_used"]) == (1, 0, used)
        assert trk.build_clearance()["reused"] == 1 and np.array_equal(trk.download_tsdf(), vol)
    finally:
        trk.close()


# ---- 2. ragged shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(72, 56, 41), (80, 64, 46)])
def test_ragged_speckled_volumes_match_the_twin(hsk, dims):
    """41 and 46 planes: padding planes in the volume, a last plane of tiles that is part empty; 72: X is no multiple of 64 and its
    last tile a quarter full; 56, 64: whole tiles in y"""
    X, Y, Z = dims
    vol = np.ascontiguousarray(speckled(carved_volume(), Z)[:Z, :Y, :X])
    trk = ctx(hsk, dims)
    try:
        trk.upload_tsdf(vol)
        pts = [centre(v, dims) for v in ((30, 30, 20), (X - 1, Y - 1, Z - 1), (0, 0, 0))]
        for weight in WEIGHTS:
            st, ref = check_hand(trk, f"speckled {dims}", vol, weight, pts)
            assert (ref == RE.BLOCKED).sum() >= 5000 and (ref == RE.UNREACHED).sum() >= 10
    finally:
        trk.close()


# ---- 3. a serpentine ----------------------------------------------------------------------------------------------------------------------
def test_a_serpentine_re_enters_tiles(hsk):
    vol, walls = serpentine()
    X, Y, Z = SERPENTINE_DIMS
    trk = ctx(hsk, SERPENTINE_DIMS)
    try:
        trk.upload_tsdf(vol)
        assert len(walls) >= 4 and X >= 3 * TILE[0] and Y >= 3 * TILE[1]
        for weight in WEIGHTS:
            st, ref = check_hand(trk, "serpentine", vol, weight, [centre((2, 2, 2), SERPENTINE_DIMS)])
            behind = trk.reach_at([centre((X - 2, 2, 2), SERPENTINE_DIMS)])[0]
            assert st["n_rounds"] >= 5 and behind == ref[2, 2, X - 2] <= RE.MAX_COST and (ref == RE.BLOCKED).sum() == (Y - 3) * Z * len(walls)
    finally:
        trk.close()


# ---- 4. the box rule ----------------------------------------------------------------------------------------------------------------------
def test_no_path_slips_between_solids_that_touch_by_an_edge(hsk):
    vol = staircase()
    trk = ctx(hsk, STAIR_DIMS)
    try:
        trk.upload_tsdf(vol)
        st, ref = check_hand(trk, "staircase", vol, (1, 1, 1), [centre((2, 12, 6), STAIR_DIMS)])
        g = trk.download_reach()
        zz, yy, xx = np.indices(g.shape)
        assert (g[xx - yy > 8] == RE.UNREACHED).all() and (xx - yy > 8).sum() == st["n_passable"] - st["n_reached"] >= 1000
    finally:
        trk.close()


# ---- 5. the tile corner -------------------------------------------------------------------------------------------------------------------
def test_a_path_across_the_corner_eight_tiles_share(hsk):
    vol = tile_corner()
    trk = ctx(hsk, CORNER_DIMS)
    try:
        trk.upload_tsdf(vol)
        for weight in WEIGHTS:
            st, ref = check_hand(trk, "tile corner", vol, weight, [centre((4, 3, 3), CORNER_DIMS)])
            far = ref[TILE[2]:, TILE[1]:, TILE[0]:]
            assert (far <= RE.MAX_COST).sum() >= 500 and (ref == RE.UNREACHED).sum() == 0 and (ref == RE.BLOCKED).sum() >= 1000
            assert ref[TILE[2], TILE[1], TILE[0]] == ref[TILE[2] - 1, TILE[1] - 1, TILE[0] - 1] + RE.costs(weight)[26]
    finally:
        trk.close()


def test_seeds_on_tile_faces_of_one_voxel_corridors(hsk):
    """corridors one voxel wide that cross a tile face and go round the corner eight tiles share, the seed at local 0 and at local
    TILE - 1 of its tile, right at the crossing: no in-tile neighbour of the seed lies on the face the next tile sees it through, so
    that tile is relaxed only because placing the seed marked it"""
    vol, seeds = corridors()
    trk = ctx(hsk, CORNER_DIMS)
    try:
        trk.upload_tsdf(vol)
        for weight in WEIGHTS:
            for name, seed in seeds.items():
                st, ref = check_hand(trk, "corridors", vol, weight, [centre(seed, CORNER_DIMS)], min_reached=2 * TILE[0] - 2)
                assert st["n_reached"] == (2 * TILE[0] if name.startswith("face") else 2 * TILE[0] - 2) and st["n_seeds_used"] == 1, (name, weight)
                assert (ref == RE.BLOCKED).sum() >= 1000 and (ref == RE.UNREACHED).sum() >= 60
        both = [centre(seeds["face, local 0"], CORNER_DIMS), centre(seeds["corner, local TILE - 1"], CORNER_DIMS)]
        st, ref = check_hand(trk, "corridors", vol, (1, 1, 1), both, min_reached=4 * TILE[0] - 2)
        assert (ref == RE.UNREACHED).sum() == 0 and st["n_seeds_used"] == 2
    finally:
        trk.close()


# ---- 6. the seeds -------------------------------------------------------------------------------------------------------------------------
def test_seeds(hsk):
    vol = staircase()
    X, Y, Z = STAIR_DIMS
    size = scene_size(STAIR_DIMS)
    rng = np.random.default_rng(21)
    trk = ctx(hsk, STAIR_DIMS)
    try:
        trk.upload_tsdf(vol)
        one = [centre((2, 12, 6), STAIR_DIMS)]
        two = one + [centre((38, 2, 3), STAIR_DIMS)]
        many = rng.uniform(-0.1, 1.1, (4096, 3)).astype(f32) * np.array(size, f32)
        many[:50] = many[50:100]                                     # duplicates
        many[100] = (np.nan, 0.5, 0.2)
        many[101] = centre((9, 1, 3), STAIR_DIMS)                     # on the wall
        last = [centre((X - 1, Y - 1, Z - 1), STAIR_DIMS)]
        odd = [(np.nan, 0.5, 0.2), (-0.01, 0.5, 0.2), (0.5, 0.5, 40.0), centre((9, 1, 3), STAIR_DIMS), (np.inf, 0.1, 0.1)]
        used = {}
        for name, pts in (("one", one), ("two", two), ("duplicates", one + one + two), ("many", many), ("last", last), ("mixed", one + odd)):
            st, ref = check_hand(trk, "staircase", vol, (1, 1, 1), pts)
            used[name] = st["n_seeds_used"]
            if name == "last":
                assert ref[Z - 1, Y - 1, X - 1] == 0 and trk.reach_at(last)[0] == 0
        assert (used["one"], used["two"], used["duplicates"], used["last"], used["mixed"]) == (1, 2, 4, 1, 1) and 1000 < used["many"] < 4094
        for pts in (odd, np.zeros((0, 3), f32)):
            st = trk.build_reach(pts, min_d2=1, **hand_params((1, 1, 1))[0])
            g = trk.download_reach()
            assert (st["n_rounds"], st["n_reached"], st["n_seeds_used"], st["max_cost_seen"], st["reused"]) == (0, 0, 0, 0, 0) and st["n_passable"] == X * Y * Z - Y * Z
            assert ((g == RE.UNREACHED) | (g == RE.BLOCKED)).all() and (g == RE.BLOCKED).sum() == Y * Z
    finally:
        trk.close()


# ---- 7. max_cost --------------------------------------------------------------------------------------------------------------------------
def test_max_cost(hsk):
    vol, _ = serpentine()
    trk = ctx(hsk, SERPENTINE_DIMS)
    try:
        trk.upload_tsdf(vol)
        seed = [centre((2, 2, 2), SERPENTINE_DIMS)]
        weight = (16, 25, 44)
        _, full = check_hand(trk, "serpentine", vol, weight, seed)
        cap = int(np.sort(full[full <= RE.MAX_COST])[full.size // 8])
        st, ref = check_hand(trk, "serpentine", vol, weight, seed, max_cost=cap)
        g = trk.download_reach()
        assert st["max_cost_seen"] == cap and (g == cap).sum() >= 1 and np.array_equal(g, np.where((full <= RE.MAX_COST) & (full > cap), RE.UNREACHED, full))
        assert (g == RE.UNREACHED).sum() >= 1000 and st["n_rounds"] >= 1
        st0, ref0 = check_hand(trk, "serpentine", vol, weight, seed, max_cost=0, min_reached=1)
        assert (st0["n_reached"], st0["max_cost_seen"], st0["n_seeds_used"]) == (1, 0, 1) and trk.download_reach()[2, 2, 2] == 0
    finally:
        trk.close()


# ---- 8. the cache -------------------------------------------------------------------------------------------------------------------------
def test_the_cache(hsk):
    vol = injected_volume()[0]
    d = SCENE_DEFAULTS
    min_d2 = RE.default_params(d)["min_d2"]
    seeds = tuple(RE.seed_voxels(AT.DST_SIZE, AT.DST_DIMS, [EYE]))
    cell = [f32(AT.DST_SIZE[i]) / f32(AT.DST_DIMS[i]) for i in range(3)]

    def twin(v):
        return RE.field(CL.field(v, d["weight"], d["max_d2"], CL.UNKNOWN), d["weight"], min_d2, RE.MAX_COST, seeds)[0]

    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        first = trk.build_reach([EYE])
        assert first["reused"] == 0 and first["n_reached"] >= 1000 and first["scratch_bytes"] <= scratch_bound(AT.DST_DIMS)
        assert trk.build_reach([EYE])["reused"] == 1 and trk.build_reach([EYE], unit_m=0.5, min_d2=min_d2)["reused"] == 1, "unit_m is not the device's"
        assert np.array_equal(trk.download_reach(), twin(vol)) and trk.build_reach([EYE])["reused"] == 1
        for change in (dict(min_d2=min_d2 - 1), dict(max_cost=50000), dict(max_d2=d["max_d2"] - 1), dict(flags=0), dict(weight=(16, 25, 45)), dict(weight=(17, 25, 44))):
            kw = dict(dict(min_d2=min_d2), **change)
            a, b = trk.build_reach([EYE], **kw), trk.build_reach([EYE], **kw)
            assert (a["reused"], b["reused"], b["n_rounds"]) == (0, 1, 0), change
        assert trk.build_reach([EYE])["reused"] == 0 and trk.build_reach([EYE])["reused"] == 1          # back to the defaults: built again
        inside = tuple(float(c) + 0.3 * float(cell[i]) for i, c in enumerate(EYE))
        assert tuple(RE.seed_voxels(AT.DST_SIZE, AT.DST_DIMS, [inside])) == seeds and trk.build_reach([inside])["reused"] == 1, "a seed moved inside its voxel"
        other = (EYE[0] + 2.0 * float(cell[0]), EYE[1], EYE[2])
        assert trk.build_reach([other])["reused"] == 0 and trk.build_reach([other])["reused"] == 1 and trk.build_reach([EYE])["reused"] == 0
        assert trk.build_reach([EYE, (np.nan, 1.0, 1.0), (-1.0, 1.0, 1.0)])["reused"] == 1, "seeds outside the grid do not count"
        trk.upload_tsdf(vol)
        assert trk.build_reach([EYE])["reused"] == 0
        assert trk.prune_components(min_voxels=0)["n_pruned"] == 0 and trk.build_reach([EYE])["reused"] == 1          # nothing pruned: nothing moved
        assert trk.prune_components()["n_pruned"] > 0
        st = trk.build_reach([EYE])
        pruned = trk.download_tsdf()
        assert st["reused"] == 0 and np.array_equal(trk.download_reach(), twin(pruned)) and trk.build_reach([EYE])["reused"] == 1
        trk.release_reach()
        with pytest.raises(hsk.KinfuError, match="no reach field"):
            trk.download_reach()
        trk.release_reach()
        st = trk.build_reach([EYE])
        assert st["reused"] == 0 and st["scratch_bytes"] == first["scratch_bytes"] and trk.build_clearance()["reused"] == 1
        box = ((3, 5, 7), (77, 33, 48))
        whole = trk.download_reach()
        assert np.array_equal(trk.download_reach(box=box), whole[7:48, 5:33, 3:77]) and trk.download_reach(box=((4, 4, 4), (4, 9, 9))).size == 0
    finally:
        trk.close()


# ---- 9. deferred weights; nothing else moves and a scan goes on ----------------------------------------------------------------------------
def test_a_volume_with_deferred_weights(hsk):
    """24 frames of room 0 integrated at 64^3 leave free-space weights in the summaries; the field is built BEFORE any download and
    equals the twin fed by the download of a second, identically grown context; one more frame: the field is built again"""
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 300, 12)]
    depths = [hsk.synth_room_depth(0, p) for p in poses]

    def grown(n):
        trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
        for d, p in zip(depths[:n], poses[:n]):
            trk.integrate(d, p)
        return trk

    a, b = grown(24), grown(24)
    try:
        pts = [tuple(float(v) for v in poses[23][:3, 3]), (1.5, 1.5, 1.5)]
        seeds = tuple(RE.seed_voxels((3.0, 3.0, 3.0), (64, 64, 64), pts))
        p = b.default_reach_params()
        assert p.min_d2 == 41
        st = b.build_reach(pts, flags=0)
        g = b.download_reach()
        vol = a.download_tsdf()
        assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
        ref, used = RE.field(CL.field(vol, (1, 1, 1), 456, 0), (1, 1, 1), 41, RE.MAX_COST, seeds)
        print(f"deferred weights: {st}")
        assert st["reused"] == 0 and int((g != ref).sum()) == 0 and {k: st[k] for k in STAT_KEYS} == RE.stats(ref) and st["n_seeds_used"] == used
        assert st["n_reached"] >= 1000 and (ref == RE.BLOCKED).sum() >= 1000
        assert b.build_reach(pts, flags=0)["reused"] == 1 and np.array_equal(b.download_tsdf(), vol)
        for t in (a, b):
            t.integrate(depths[24], poses[24])
        with pytest.raises(hsk.KinfuError, match="no reach field"):
            b.reach_at(pts)
        st3 = b.build_reach(pts, flags=0)
        vol3 = a.download_tsdf()
        assert st3["reused"] == 0 and not np.array_equal(vol3, vol)
        assert np.array_equal(b.download_reach(), RE.field(CL.field(vol3, (1, 1, 1), 456, 0), (1, 1, 1), 41, RE.MAX_COST, seeds)[0])
    finally:
        a.close()
        b.close()


def test_nothing_else_moves_and_a_scan_goes_on(hsk, synth_frames):
    a, b = hsk.KinfuTracker(n=64), hsk.KinfuTracker(n=64)
    try:
        poses_a, poses_b = [], []
        pts = [(1.5, 1.5, 1.5), (1.5, 1.5, 1.0)]
        for k in range(8):
            depth = synth_frames(k)[1]
            pa, oka = a.process_frame(depth)
            pb, okb = b.process_frame(depth)
            assert oka == okb and (oka or k == 0), f"frame {k}: tracked {oka} with the field, {okb} without"
            poses_a.append(pa), poses_b.append(pb)
            if k == 3:
                before, vol = state_of(a, False), a.download_tsdf()
                st = a.build_reach(pts, flags=0)
                g = a.download_reach()
                a.reach_at(np.array(pts, f32))
                a.reach_path(pts[1])
                a.reach_floor(1, 10, 40, pts, flags=0)
                for u, v in zip(before, state_of(a, False)):
                    assert same_bits(u, v)
                ref, used = RE.field(CL.field(vol, (1, 1, 1), 456, 0), (1, 1, 1), 41, RE.MAX_COST, tuple(RE.seed_voxels((3.0,) * 3, (64,) * 3, pts)))
                assert np.array_equal(a.download_tsdf(), vol) and np.array_equal(g, ref) and st["n_seeds_used"] == used and st["n_reached"] >= 1000
                b.download_tsdf()                     # (the same flush of the deferred weights on both sides)
            else:
                a.build_reach(pts, flags=k & 1)
        for pa, pb in zip(poses_a, poses_b):
            assert same_bits(pa, pb)
        assert np.array_equal(a.download_tsdf(), b.download_tsdf())
    finally:
        a.close()
        b.close()


# ---- 10. the point lookup and the path -------------------------------------------------------------------------------------------------------
def test_reach_at_and_reach_path(hsk):
    vol = carved_volume()
    d = SCENE_DEFAULTS
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        ref, _ = carved_reference()
        with pytest.raises(hsk.KinfuError, match="no reach field"):
            trk.reach_at(np.ones((3, 3), f32))
        trk.build_reach([EYE])
        many = np.random.default_rng(4).uniform(-0.2, 3.2, (5000, 3)).astype(f32)
        many[:3] = ((np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), EYE)
        want = RE.lookup(ref, AT.DST_SIZE, many)
        got = trk.reach_at(many)
        assert got.dtype == np.uint32 and np.array_equal(got, want) and got[2] == 0 and len(trk.reach_at(np.zeros((0, 3), f32))) == 0
        assert min((want == RE.OUTSIDE).sum(), (want == RE.BLOCKED).sum(), (want <= RE.MAX_COST).sum()) >= 100
        reached = np.argwhere(ref <= RE.MAX_COST)
        ok = RE.allowed(ref != RE.BLOCKED)
        rng = np.random.default_rng(6)
        goals = [tuple(int(v) for v in reached[i][::-1]) for i in rng.integers(0, len(reached), 9)] + [tuple(int(v) for v in reached[np.argmax(ref[tuple(reached.T)])][::-1])]
        cell = np.array([f32(AT.DST_SIZE[i]) / f32(AT.DST_DIMS[i]) for i in range(3)], np.float64)
        for goal in goals:
            p = trk.reach_path((np.array(goal) + 0.5) * cell)
            assert p.dtype == np.int32 and np.array_equal(p, RE.path(ref, d["weight"], goal))
            check_path(ref, ok, d["weight"], p, goal)
        longest = RE.path(ref, d["weight"], goals[-1])
        assert len(longest) >= 20
        # an unreached goal, one outside the grid; a cap one too small, a cap that fits
        blocked = tuple(int(v) for v in np.argwhere(ref == RE.BLOCKED)[0][::-1])
        assert len(trk.reach_path((np.array(blocked) + 0.5) * cell)) == 0 and len(trk.reach_path((-1.0, 1.0, 1.0))) == 0 and len(trk.reach_path((np.nan, 1.0, 1.0))) == 0
        lib = hsk._lib.load()
        goal_pt = np.ascontiguousarray((np.array(goals[-1]) + 0.5) * cell, f32)
        out = np.full((len(longest), 3), -7, np.int32)
        n = C.c_size_t(0)
        assert lib.hsk_reach_path(trk.h, goal_pt.ctypes.data, out.ctypes.data, len(longest) - 1, C.byref(n)) == -1 and n.value == len(longest) and (out == -7).all()
        assert lib.hsk_reach_path(trk.h, goal_pt.ctypes.data, None, 0, C.byref(n)) == -1 and n.value == len(longest)
        assert lib.hsk_reach_path(trk.h, goal_pt.ctypes.data, out.ctypes.data, len(longest), C.byref(n)) == 0 and n.value == len(longest) and np.array_equal(out, longest)
        assert np.array_equal(trk.reach_path(goal_pt, cap=3), longest)
    finally:
        trk.close()


# ---- 11. the floor form ---------------------------------------------------------------------------------------------------------------------
def test_floor_maps(hsk):
    vol = carved_volume()
    d = SCENE_DEFAULTS
    min_d2 = RE.default_params(d)["min_d2"]
    pts = [EYE, (2.0, 0.8, 2.2), (np.nan, 1.0, 1.0), (-0.5, 1.0, 1.0)]
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        n_reached = 0
        for axis, n in enumerate(AT.DST_DIMS):
            for lo, hi in ((n // 4, n // 2), (0, n), (n // 3, n // 3), (n - 1, n)):
                for flags in (CL.UNKNOWN, 0):
                    fmap, st = trk.reach_floor(axis, lo, hi, pts, flags=flags)
                    want, used = RE.floor(vol, d["weight"], d["max_d2"], flags, axis, lo, hi, min_d2, RE.MAX_COST, AT.DST_SIZE, pts)
                    assert fmap.shape == want.shape and int((fmap != want).sum()) == 0, (axis, lo, hi, flags)
                    assert {k: st[k] for k in STAT_KEYS} == RE.stats(want) and (st["n_seeds_used"], st["reused"]) == (used, 0), (axis, lo, hi, flags)
                    n_reached += st["n_reached"]
        assert n_reached >= 1000
        # a wall in the plane x = 40 with a gap over z in [20, 34): the middle of the doorway is 7 voxels from either jamb
        wall = free_volume(AT.DST_DIMS)
        wall[:20, :, 40] = SOLID_WORD
        wall[34:, :, 40] = SOLID_WORD
        trk.upload_tsdf(wall)
        seed = [centre((10, 30, 27), AT.DST_DIMS)]
        for min_gap, through in ((49, True), (50, False)):
            fmap, st = trk.reach_floor(1, 0, AT.DST_DIMS[1], seed, weight=(1, 1, 1), max_d2=10000, flags=0, min_d2=min_gap)
            want, used = RE.floor(wall, (1, 1, 1), 10000, 0, 1, 0, AT.DST_DIMS[1], min_gap, RE.MAX_COST, AT.DST_SIZE, seed)
            assert fmap.shape == (48, 80) and np.array_equal(fmap, want) and used == 1 and st["n_reached"] >= 1000
            assert ((fmap[:, 48:] <= RE.MAX_COST).sum() >= 1000) == through and (through or (fmap[:, 41:] <= RE.MAX_COST).sum() == 0)
            assert (fmap[26, 40] <= RE.MAX_COST) == through and fmap[20, 40] == RE.BLOCKED
    finally:
        trk.close()


# ---- 12. what it is for -------------------------------------------------------------------------------------------------------------------
def test_viewpoints_nobody_can_walk_to_leave_the_head_of_the_ranking(hsk):
    vol = two_rooms(sealed=True)
    vol[16:28, 25:42, 0:3] = (0, 0)                        # a never-observed patch in either room's outer wall
    vol[16:28, 25:42, 77:80] = (0, 0)
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        cp, min_d2 = hand_params(SCENE_DEFAULTS["weight"])
        here = [(8 + 3 * i, 20 + 3 * i, 20) for i in range(8)]            # the seeded room: x < 40
        there = [(48 + 3 * i, 20 + 3 * i, 20) for i in range(8)]
        voxels = [v for pair in zip(here, there) for v in pair]           # alternating: even indices can be walked to
        eyes = np.array([centre(v, AT.DST_DIMS) for v in voxels], f32)
        targets = [(0.056, 1.57, 1.375) if v[0] < 40 else (2.944, 1.57, 1.375) for v in voxels]
        poses = np.array([RT.look_at(tuple(float(c) for c in e), t) for e, t in zip(eyes, targets)], f32)
        scores = trk.score_views(poses)
        st = trk.build_reach([centre((20, 32, 24), AT.DST_DIMS)], min_d2=min_d2, **cp)
        eye_g = trk.reach_at(eyes)
        eye_d2 = trk.clearance_at(eyes, **cp)
        ref, _ = twin_reach("two sealed rooms", hand_d2(vol, cp["weight"]), cp["weight"], min_d2, RE.MAX_COST, ((20, 32, 24),))
        assert np.array_equal(trk.download_reach(), ref) and np.array_equal(eye_g, RE.lookup(ref, AT.DST_SIZE, eyes)) and st["n_reached"] >= 1000
        assert (scores["eye_state"] == 0).all() and (eye_d2 >= min_d2).all()
        assert (eye_g[0::2] <= RE.MAX_COST).all() and (eye_g[1::2] == RE.UNREACHED).all() and (ref == RE.UNREACHED).sum() >= 100000
        plain = hsk.rank_views(scores).tolist()
        clear = hsk.rank_views_clear(scores, eye_d2, min_d2).tolist()
        ranked = hsk.rank_views_reach(scores, eye_g).tolist()
        print(f"gains {scores['gain'].tolist()}, eye_g {eye_g.tolist()}, rank_views {plain}, rank_views_clear {clear}, rank_views_reach {ranked}")
        assert clear == plain and min(clear.index(i) for i in range(1, 16, 2)) < max(clear.index(i) for i in range(0, 16, 2)), "rank_views_clear mixes them"
        assert ranked[:8] == [i for i in plain if i % 2 == 0] and ranked[8:] == [i for i in plain if i % 2 == 1]
        assert np.array_equal(ranked, RE.rank_views_reach(scores, eye_g, RE.MAX_COST))
        for max_g in (int(np.sort(eye_g[0::2])[3]), 0):
            assert np.array_equal(hsk.rank_views_reach(scores, eye_g, max_g), RE.rank_views_reach(scores, eye_g, max_g))
    finally:
        trk.close()


# ---- 13. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    vol = carved_volume()
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        out = np.full(80 * 64 * 48, 9, np.uint32)
        vox = np.full((64, 3), -7, np.int32)
        pts = np.array([EYE, (2.0, 0.8, 2.2)], f32)
        big = np.ones((4097, 3), f32)
        n = C.c_size_t(5)
        st = L.HskReachStats(n_reached=77)
        # reads with no field held
        assert lib.hsk_download_reach(trk.h, None, out.ctypes.data) == -3 and b"no reach field" in lib.hsk_last_error(trk.h)
        assert lib.hsk_reach_at(trk.h, pts.ctypes.data, 2, out.ctypes.data) == -3
        assert lib.hsk_reach_path(trk.h, pts.ctypes.data, vox.ctypes.data, 64, C.byref(n)) == -3 and n.value == 5
        assert (out == 9).all() and (vox == -7).all()
        first = trk.build_reach(pts)
        g = trk.download_reach()
        cp = trk.default_clearance_params()
        rp = trk.default_reach_params()

        def refused(cpar, rpar, seeds, n_seeds, code=-1):
            assert lib.hsk_build_reach(trk.h, C.byref(cpar), C.byref(rpar), seeds, n_seeds, C.byref(st)) == code and st.n_reached == 77 and lib.hsk_last_error(trk.h)
            assert lib.hsk_reach_floor(trk.h, C.byref(cpar), 1, 0, 4, C.byref(rpar), seeds, n_seeds, out.ctypes.data, C.byref(st)) == code and st.n_reached == 77
            assert (out == 9).all()

        for bad in (dict(min_d2=0), dict(min_d2=cp.max_d2 + 1), dict(max_cost=RE.MAX_COST + 1), dict(max_cost=0xFFFFFFFF)):
            refused(cp, trk.default_reach_params(**bad), pts.ctypes.data, 2)
        flagged = trk.default_reach_params()
        flagged.flags = 1
        refused(cp, flagged, pts.ctypes.data, 2)
        for bad in (dict(weight=(0, 1, 1)), dict(flags=2), dict(max_d2=16 * 256 * 256)):
            refused(trk.default_clearance_params(**bad), rp, pts.ctypes.data, 2)
        refused(cp, rp, big.ctypes.data, 4097)
        assert b"4096" in lib.hsk_last_error(trk.h)
        refused(cp, rp, None, 2)
        for axis, lo, hi in ((-1, 0, 1), (3, 0, 1), (0, -1, 4), (0, 0, 81), (1, 0, 65), (2, 0, 49), (2, 9, 8)):
            assert lib.hsk_reach_floor(trk.h, C.byref(cp), axis, lo, hi, C.byref(rp), pts.ctypes.data, 2, out.ctypes.data, C.byref(st)) == -1 and st.n_reached == 77
        assert lib.hsk_reach_floor(trk.h, C.byref(cp), 1, 0, 4, C.byref(rp), pts.ctypes.data, 2, None, None) == -1
        for lo, hi in (((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (81, 4, 4)), ((0, 5, 0), (4, 4, 4)), ((0, 0, 0), (4, 4, 49))):
            b = L.HskVoxelBox()
            b.lo[:], b.hi[:] = lo, hi
            assert lib.hsk_download_reach(trk.h, C.byref(b), out.ctypes.data) == -1 and b"box" in lib.hsk_last_error(trk.h)
        assert lib.hsk_download_reach(trk.h, None, None) == -1
        assert lib.hsk_reach_at(trk.h, pts.ctypes.data, (1 << 20) + 1, out.ctypes.data) == -1 and b"2^20" in lib.hsk_last_error(trk.h)
        assert lib.hsk_reach_at(trk.h, None, 2, out.ctypes.data) == -1 and lib.hsk_reach_at(trk.h, pts.ctypes.data, 2, None) == -1
        assert lib.hsk_reach_path(trk.h, None, vox.ctypes.data, 64, C.byref(n)) == -1 and lib.hsk_reach_path(trk.h, pts.ctypes.data, vox.ctypes.data, 64, None) == -1
        assert lib.hsk_reach_path(trk.h, pts.ctypes.data, None, 64, C.byref(n)) == -1 and n.value == 5
        assert (out == 9).all() and (vox == -7).all()
        with pytest.raises(hsk.KinfuError, match="min_d2"):
            trk.build_reach(pts, min_d2=0)
        again = trk.build_reach(pts)
        assert again["reused"] == 1 and {k: again[k] for k in STAT_KEYS} == {k: first[k] for k in STAT_KEYS}
        assert np.array_equal(trk.download_reach(), g) and np.array_equal(trk.download_tsdf(), vol)
        assert lib.hsk_build_reach(trk.h, None, None, pts.ctypes.data, 2, None) == 0                      # NULL parameters: the defaults; no stats
        assert lib.hsk_build_reach(trk.h, None, None, None, 0, C.byref(st)) == 0 and (st.n_reached, st.n_rounds, st.reused) == (0, 0, 0)
    finally:
        trk.close()
    # between submit and wait
    trk = hsk.KinfuTracker(n=64)
    try:
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        trk.build_reach([(1.5, 1.5, 1.5)], flags=0)
        trk.submit_frame(hsk.synth_depth(hsk.synth_pose(1)))
        out, st, pts, n = np.full(64 ** 3, 9, np.uint32), L.HskReachStats(n_reached=77), np.full((2, 3), 1.5, f32), C.c_size_t(5)
        vox = np.full((64, 3), -7, np.int32)
        assert lib.hsk_build_reach(trk.h, None, None, pts.ctypes.data, 2, C.byref(st)) == -3 and st.n_reached == 77 and b"in flight" in lib.hsk_last_error(trk.h)
        assert lib.hsk_download_reach(trk.h, None, out.ctypes.data) == -3 and lib.hsk_reach_at(trk.h, pts.ctypes.data, 2, out.ctypes.data) == -3
        assert lib.hsk_reach_path(trk.h, pts.ctypes.data, vox.ctypes.data, 64, C.byref(n)) == -3 and n.value == 5
        assert lib.hsk_reach_floor(trk.h, None, 1, 0, 4, None, pts.ctypes.data, 2, out.ctypes.data, C.byref(st)) == -3 and st.n_reached == 77
        assert (out == 9).all() and (vox == -7).all()
        _, ok = trk.wait_frame()
        assert ok and trk.build_reach(pts, flags=0)["reused"] == 0
    finally:
        trk.close()
    # a context that stores part of its volume
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        one = np.full((1, 3), 1.5, f32)
        for call in (lambda t: t.build_reach(one), lambda t: t.download_reach(), lambda t: t.reach_at(one), lambda t: t.reach_path(one[0]),
                     lambda t: t.reach_floor(1, 0, 4, one)):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call(part)
        st = L.HskReachStats(n_reached=77)
        assert lib.hsk_build_reach(part.h, None, None, one.ctypes.data, 1, C.byref(st)) == -3 and st.n_reached == 77
    finally:
        part.close()
