"""The clearance field on the GPU: hsk_build_clearance, hsk_download_clearance, hsk_clearance_at and hsk_clearance_floor against the
numpy restatement of the rule (tests/clearance_twin.py), every value, count and flag EQUAL: the carved room and random volumes at
the sizes that have padding planes, an X that is no multiple of 64 and half-empty last tiles; hand-built shapes, analytic as well;
the caps; a volume with deferred weights; the cache; the point lookup; the floor map; nothing else of the context moves and a scan
goes on; what it is for (viewpoints next to a wall leave the head of the ranking); the errors."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import clearance_twin as CL
import reloc_twin as RT
from clearance_cases import AXIS_SEG, MASK_BITS, SCENE_DEFAULTS, lookup_points, twin_field
from components_cases import injected_volume, speckled
from cover_cases import PATCH_CENTRE, carved_volume
from kit import same_bits, state_of, volume_ctx

pytestmark = pytest.mark.gpu
f32 = np.float32
FREE_WORD = (32767, 1)
SOLID_WORD = (-100, 1)


def ctx(hsk, dims, size=None, **over):
    return volume_ctx(hsk, dims, size or (3.0 * dims[0] / 80, 3.0 * dims[1] / 64, 3.0 * dims[2] / 48), **over)       # the scene's cells at every shape


def check(trk, vol, ref, flags, **par):
    """build + download with the parameters given equal the twin's field `ref` of `vol`; -> the build's stats"""
    st = trk.build_clearance(flags=flags, **par)
    fld = trk.download_clearance(flags=flags, **par)
    want = CL.stats(vol, ref, flags)
    print(f"{par} flags {flags}: {st}")
    assert fld.dtype == np.uint32 and fld.shape == ref.shape and int((fld != ref).sum()) == 0, f"{int((fld != ref).sum())} values differ"
    assert {k: st[k] for k in want} == want
    assert st["scratch_bytes"] <= 2.5 * vol.shape[0] * vol.shape[1] * vol.shape[2] * 4 + 4 * 256
    return st


def free_volume(dims):
    X, Y, Z = dims
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[...] = FREE_WORD
    return vol


# ---- 1. the carved room at default parameters ------------------------------------------------------------------------------------------
def test_the_carved_room_matches_the_twin(hsk):
    vol = carved_volume()
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        p = trk.default_clearance_params()
        assert {"weight": tuple(p.weight), "max_d2": p.max_d2, "flags": p.flags, "unit_m": f32(p.unit_m)} == SCENE_DEFAULTS
        for flags in (CL.UNKNOWN, 0):
            ref = twin_field("carved", vol, SCENE_DEFAULTS["weight"], SCENE_DEFAULTS["max_d2"], flags)
            st = check(trk, vol, ref, flags)
            assert st["reused"] == 0 and trk.build_clearance(flags=flags)["reused"] == 1
            again = trk.build_clearance(flags=flags)
            assert {k: again[k] for k in ("n_obstacle", "n_far", "max_d2_seen")} == CL.stats(vol, ref, flags)
        assert np.array_equal(trk.download_tsdf(), vol)
    finally:
        trk.close()


# ---- 2. speckled volumes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(80, 64, 48), (80, 64, 46), (80, 64, 41), (72, 56, 40)])
def test_speckled_volumes_match_the_twin(hsk, dims):
    """a fifth of the voxels in random states; 46 and 41 planes: the last plane group holds padding planes, which are no voxels and
    no obstacles; 72: X is no multiple of 64, the second mask word is an eighth full; 56, 40, 41: the last segments are ragged"""
    X, Y, Z = dims
    vol = np.ascontiguousarray(speckled(carved_volume(), Z)[:Z, :Y, :X])
    trk = ctx(hsk, dims)
    try:
        trk.upload_tsdf(vol)
        d = trk.default_clearance_params()
        assert tuple(d.weight) == (16, 25, 44)
        for weight, max_d2, flags in ((tuple(d.weight), d.max_d2, CL.UNKNOWN), (tuple(d.weight), d.max_d2, 0), ((1, 1, 1), 400, CL.UNKNOWN), ((1, 1, 1), 400, 0)):
            ref = twin_field(f"speckled {dims}", vol, weight, max_d2, flags)
            check(trk, vol, ref, flags, weight=weight, max_d2=max_d2)
    finally:
        trk.close()


# ---- 3. hand-built shapes, analytic as well as against the twin ---------------------------------------------------------------------------
SHAPE_DIMS = (136, 40, 36)        # three mask words, the last an eighth full; three segments in y and z, the last ragged


def solids(points):
    vol = free_volume(SHAPE_DIMS)
    for x, y, z in points:
        vol[z, y, x] = SOLID_WORD
    return vol


def test_hand_built_shapes(hsk):
    X, Y, Z = SHAPE_DIMS
    zz, yy, xx = np.indices((Z, Y, X)).astype(np.int64)
    trk = ctx(hsk, SHAPE_DIMS)
    try:
        def run(vol, weight, max_d2, flags):
            trk.upload_tsdf(vol)
            ref = CL.field(vol, weight, max_d2, flags)
            check(trk, vol, ref, flags, weight=weight, max_d2=max_d2)
            return ref

        w, cap = (2, 3, 5), 2 * 255 * 255
        # all UNSEEN, all FREE
        unseen = np.zeros((Z, Y, X, 2), np.int16)
        assert (run(unseen, w, cap, CL.UNKNOWN) == 0).all() and (run(unseen, w, cap, 0) == CL.FAR).all()
        border = np.minimum(np.minimum(w[0] * np.minimum(xx + 1, X - xx) ** 2, w[1] * np.minimum(yy + 1, Y - yy) ** 2), w[2] * np.minimum(zz + 1, Z - zz) ** 2)
        assert np.array_equal(run(free_volume(SHAPE_DIMS), w, cap, CL.UNKNOWN), border) and (run(free_volume(SHAPE_DIMS), w, cap, 0) == CL.FAR).all()
        small = run(free_volume(SHAPE_DIMS), w, 50, CL.UNKNOWN)
        assert np.array_equal(small, np.where(border <= 50, border, CL.FAR)) and (small == CL.FAR).any()
        # a SOLID voxel at each of the eight corners and at the centre, without the flag
        nine = [(x, y, z) for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)] + [(X // 2, Y // 2, Z // 2)]
        for cap9 in (cap, 3000):
            want = np.min([w[0] * (xx - x) ** 2 + w[1] * (yy - y) ** 2 + w[2] * (zz - z) ** 2 for x, y, z in nine], axis=0)
            got = run(solids(nine), w, cap9, 0)
            assert np.array_equal(got, np.where(want <= cap9, want, CL.FAR))
        assert (got == CL.FAR).any() and (got == 0).sum() == 9
        # the reach edge: max_d2 = w_x R^2
        R = 50
        edge = run(solids([(10, 20, 18)]), (4, 1, 1), 4 * R * R, 0)
        assert edge[18, 20, 10 + R] == 4 * R * R and edge[18, 20, 10 + R + 1] == CL.FAR and edge[18, 20, 10 + R - 1] == 4 * (R - 1) ** 2
        assert edge[18, 20, 0] == 400 and edge[18, 21, 10 + R] == CL.FAR and edge[19, 20, 10] == 1
        # two obstacles equally far away
        two = run(solids([(20, 9, 7), (30, 9, 7)]), (3, 1, 1), 1000, 0)
        assert two[7, 9, 25] == 75 and two[7, 9, 24] == 48 and two[7, 9, 26] == 48
        # obstacles exactly on the seams: the last bit of a mask word and the first of the next; the last output of an axis
        # segment and the first of the next
        seams = [(MASK_BITS - 1, AXIS_SEG - 1, AXIS_SEG - 1), (MASK_BITS, AXIS_SEG, AXIS_SEG), (2 * MASK_BITS - 1, 2 * AXIS_SEG - 1, 2 * AXIS_SEG - 1),
                 (2 * MASK_BITS, 2 * AXIS_SEG, 2 * AXIS_SEG)]
        assert 2 * MASK_BITS < X and 2 * AXIS_SEG < min(Y, Z)
        for pts in ([seams[0]], [seams[1]], [seams[2], seams[3]], seams):
            for flags in (0, CL.UNKNOWN):
                vol = solids(pts)
                got = run(vol, (1, 2, 3), 255 * 255, flags)
                assert np.array_equal(got, CL.literal(CL.obstacles(vol, flags), (1, 2, 3), 255 * 255, flags))
    finally:
        trk.close()


# ---- 4. caps --------------------------------------------------------------------------------------------------------------------------
def test_caps(hsk):
    vol = carved_volume()
    w = SCENE_DEFAULTS["weight"]
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        for weight, max_d2 in ((w, 0), (w, 1), (w, 255 * 255 * min(w)), ((1024, 1, 1), 65535), ((1, 1, 1024), 65535)):
            assert max(CL.reach(max_d2, k) for k in weight) <= 255
            for flags in (CL.UNKNOWN, 0):
                ref = twin_field("carved", vol, weight, max_d2, flags)
                check(trk, vol, ref, flags, weight=weight, max_d2=max_d2)
                if max_d2 == 0:
                    assert ((ref == 0) == CL.obstacles(vol, flags)).all() and ((ref == CL.FAR) == ~CL.obstacles(vol, flags)).all()
        assert all(CL.reach(255 * 255 * min(w), k) >= n for k, n in zip(w, AT.DST_DIMS)), "the reach lies beyond the grid on every axis"
        assert (twin_field("carved", vol, w, 255 * 255 * min(w), 0) != CL.FAR).all()
    finally:
        trk.close()


# ---- 5. deferred weights; a frame voids the cache -------------------------------------------------------------------------------------------
def test_a_volume_with_deferred_weights(hsk):
    """24 frames of room 0 integrated at 64^3 leave free-space weights in the summaries; the field is built BEFORE any download and
    equals the twin fed by the download of a second, identically grown context -- and the first context's download afterwards equals
    the second's: the build enqueued no flush that changed anything.  One more frame: the field is built again"""
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 300, 12)]
    depths = [hsk.synth_room_depth(0, p) for p in poses]

    def grown(n):
        trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
        for d, p in zip(depths[:n], poses[:n]):
            trk.integrate(d, p)
        return trk

    a, b = grown(24), grown(24)
    try:
        p = b.default_clearance_params()
        assert (tuple(p.weight), p.max_d2) == ((1, 1, 1), 456)
        for flags in (CL.UNKNOWN, 0):
            st = b.build_clearance(flags=flags)
            fld = b.download_clearance(flags=flags)
            if flags:
                vol = a.download_tsdf()
                assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
            ref = CL.field(vol, (1, 1, 1), 456, flags)
            assert st["reused"] == 0 and int((fld != ref).sum()) == 0 and {k: st[k] for k in ("n_obstacle", "n_far", "max_d2_seen")} == CL.stats(vol, ref, flags)
        assert b.build_clearance(flags=0)["reused"] == 1
        assert np.array_equal(b.download_tsdf(), vol)
        for t in (a, b):
            t.integrate(depths[24], poses[24])
        st3 = b.build_clearance(flags=0)
        vol3 = a.download_tsdf()
        assert st3["reused"] == 0 and not np.array_equal(vol3, vol)
        assert np.array_equal(b.download_clearance(flags=0), CL.field(vol3, (1, 1, 1), 456, 0))
    finally:
        a.close()
        b.close()


# ---- 6. the cache ----------------------------------------------------------------------------------------------------------------------
def test_the_cache(hsk):
    vol = injected_volume()[0]
    d = SCENE_DEFAULTS
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        ref = CL.field(vol, d["weight"], d["max_d2"], CL.UNKNOWN)
        first = trk.build_clearance()
        assert first["reused"] == 0 and trk.build_clearance()["reused"] == 1
        assert trk.build_clearance(unit_m=0.5)["reused"] == 1, "unit_m is not the device's"
        fld = trk.download_clearance()
        assert np.array_equal(fld, ref) and trk.build_clearance()["reused"] == 1
        for change in (dict(max_d2=d["max_d2"] - 1), dict(flags=0), dict(weight=(16, 25, 45)), dict(weight=(17, 25, 44)), dict(weight=(16, 24, 44))):
            assert trk.build_clearance(**change)["reused"] == 0 and trk.build_clearance(**change)["reused"] == 1, change
        assert trk.build_clearance()["reused"] == 0 and trk.build_clearance()["reused"] == 1          # back to the defaults: built again
        trk.upload_tsdf(vol)
        assert trk.build_clearance()["reused"] == 0
        assert trk.prune_components(min_voxels=0)["n_pruned"] == 0 and trk.build_clearance()["reused"] == 1     # nothing pruned: nothing moved
        assert trk.prune_components()["n_pruned"] > 0
        st = trk.build_clearance()
        pruned = trk.download_tsdf()
        assert st["reused"] == 0 and np.array_equal(trk.download_clearance(), CL.field(pruned, d["weight"], d["max_d2"], CL.UNKNOWN))
        trk.release_clearance()
        again = trk.download_clearance()                                                                 # builds again
        assert np.array_equal(again, CL.field(pruned, d["weight"], d["max_d2"], CL.UNKNOWN))
        assert trk.build_clearance()["reused"] == 1
        trk.release_clearance()
        trk.release_clearance()
        st = trk.build_clearance()
        assert st["reused"] == 0 and st["scratch_bytes"] == first["scratch_bytes"]
        box = ((3, 5, 7), (77, 33, 48))
        assert np.array_equal(trk.download_clearance(box=box), again[7:48, 5:33, 3:77]) and trk.download_clearance(box=((4, 4, 4), (4, 9, 9))).size == 0
    finally:
        trk.close()


# ---- 7. the point lookup -----------------------------------------------------------------------------------------------------------------
def test_clearance_at(hsk):
    vol = carved_volume()
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        pts = lookup_points(AT.DST_SIZE, AT.DST_DIMS)
        ref = twin_field("carved", vol, SCENE_DEFAULTS["weight"], SCENE_DEFAULTS["max_d2"], CL.UNKNOWN)
        want = CL.lookup(ref, AT.DST_SIZE, pts)
        got = trk.clearance_at(pts)                       # (no field yet: builds first)
        assert got.dtype == np.uint32 and np.array_equal(got, want) and trk.build_clearance()["reused"] == 1
        assert (want == CL.OUTSIDE).sum() >= 9 and (want != CL.OUTSIDE).sum() >= 83
        assert len(trk.clearance_at(np.zeros((0, 3), f32))) == 0
        many = np.random.default_rng(4).uniform(-0.2, 3.2, (5000, 3)).astype(f32)
        assert np.array_equal(trk.clearance_at(many), CL.lookup(ref, AT.DST_SIZE, many))
    finally:
        trk.close()


# ---- 8. the floor map ----------------------------------------------------------------------------------------------------------------------
def test_floor_maps(hsk):
    vol = carved_volume()
    d = SCENE_DEFAULTS
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        for axis, n in enumerate(AT.DST_DIMS):
            for lo, hi in ((n // 4, n // 2), (0, n), (n // 3, n // 3), (n - 1, n)):
                for flags in (CL.UNKNOWN, 0):
                    fmap, st = trk.clearance_floor(axis, lo, hi, flags=flags)
                    want = CL.floor_map(vol, d["weight"], d["max_d2"], flags, axis, lo, hi)
                    assert fmap.shape == want.shape and int((fmap != want).sum()) == 0, (axis, lo, hi, flags)
                    assert {k: st[k] for k in ("n_obstacle", "n_far", "max_d2_seen")} == CL.floor_stats(want) and st["reused"] == 0
                    if lo == hi:
                        assert st["n_obstacle"] == 0 and (flags or (fmap == CL.FAR).all())
        # a wall in the plane x = 40 with a gap over z in [20, 34): the middle of the doorway is 7 voxels from either jamb
        wall = free_volume(AT.DST_DIMS)
        wall[:20, :, 40] = SOLID_WORD
        wall[34:, :, 40] = SOLID_WORD
        trk.upload_tsdf(wall)
        for flags in (0, CL.UNKNOWN):
            fmap, st = trk.clearance_floor(1, 0, AT.DST_DIMS[1], weight=(1, 1, 1), max_d2=10000, flags=flags)
            assert fmap.shape == (48, 80) and fmap[26, 40] == 49 and fmap[27, 40] == 49 and fmap[20, 40] == 1 and fmap[19, 40] == 0
            assert np.array_equal(fmap, CL.floor_map(wall, (1, 1, 1), 10000, flags, 1, 0, AT.DST_DIMS[1])) and st["n_obstacle"] == 34
    finally:
        trk.close()


# ---- 9. nothing else moves ----------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves_and_a_scan_goes_on(hsk, synth_frames):
    a, b = hsk.KinfuTracker(n=64), hsk.KinfuTracker(n=64)
    try:
        poses_a, poses_b = [], []
        for k in range(8):
            depth = synth_frames(k)[1]
            pa, oka = a.process_frame(depth)
            pb, okb = b.process_frame(depth)
            assert oka == okb and (oka or k == 0), f"frame {k}: tracked {oka} with the field, {okb} without"
            poses_a.append(pa), poses_b.append(pb)
            if k == 3:
                before, vol = state_of(a, False), a.download_tsdf()
                a.build_clearance()
                fld = a.download_clearance()
                a.clearance_at(np.array([[1.5, 1.5, 1.0]], f32))
                a.clearance_floor(1, 10, 40)
                for u, v in zip(before, state_of(a, False)):
                    assert same_bits(u, v)
                assert np.array_equal(a.download_tsdf(), vol) and np.array_equal(fld, CL.field(vol, (1, 1, 1), 456, CL.UNKNOWN))
                b.download_tsdf()                     # (the same flush of the deferred weights on both sides)
            else:
                a.build_clearance(flags=k & 1)
        for pa, pb in zip(poses_a, poses_b):
            assert same_bits(pa, pb)
        assert np.array_equal(a.download_tsdf(), b.download_tsdf())
    finally:
        a.close()
        b.close()


# ---- 10. what it is for ------------------------------------------------------------------------------------------------------------------
def test_viewpoints_next_to_a_wall_leave_the_head_of_the_ranking(hsk):
    vol = carved_volume()
    d = SCENE_DEFAULTS
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        p = trk.default_clearance_params()
        min_d2 = hsk.clearance_d2(p, 0.3)
        assert min_d2 in (1024, 1025)
        ref = twin_field("carved", vol, d["weight"], d["max_d2"], CL.UNKNOWN)
        to_solid = twin_field("carved", vol, d["weight"], d["max_d2"], 0)
        free = (vol[..., 1] != 0) & (vol[..., 0] > 0)
        near = np.argwhere(free & (to_solid <= max(d["weight"])))          # one voxel from a wall
        clear = np.argwhere(free & (ref >= min_d2) & (ref != CL.FAR))
        assert len(near) > 50 and len(clear) > 50
        near, clear = near[:: len(near) // 8][:8], clear[:: len(clear) // 8][:8]
        cell = np.array([f32(AT.DST_SIZE[i]) / f32(AT.DST_DIMS[i]) for i in range(3)], np.float64)
        eyes = np.array([(v[::-1] + 0.5) * cell for v in np.concatenate([near, clear])], f32)
        targets = [PATCH_CENTRE] * 8 + [PATCH_CENTRE if i % 2 == 0 else (0.3, 1.5, 1.4) for i in range(8)]
        poses = np.array([RT.look_at(tuple(float(c) for c in e), t) for e, t in zip(eyes, targets)], f32)
        scores = trk.score_views(poses)
        eye_d2 = trk.clearance_at(eyes)
        assert np.array_equal(eye_d2, CL.lookup(ref, AT.DST_SIZE, eyes)) and (scores["eye_state"] == 0).all()
        assert (eye_d2[:8] < min_d2).all() and (eye_d2[8:] >= min_d2).all()
        plain = hsk.rank_views(scores).tolist()
        ranked = hsk.rank_views_clear(scores, eye_d2, min_d2).tolist()
        print(f"gains {scores['gain'].tolist()}, eye_d2 {eye_d2.tolist()}, rank_views {plain}, rank_views_clear {ranked}")
        assert min(plain.index(i) for i in range(8)) < max(plain.index(i) for i in range(8, 16)), "rank_views lets a viewpoint at a wall ahead of a clear one"
        assert sorted(ranked[:8]) == list(range(8, 16)) and sorted(ranked[8:]) == list(range(8))
        assert ranked[:8] == [i for i in plain if i >= 8] and ranked[8:] == [i for i in plain if i < 8]
        assert np.array_equal(ranked, CL.rank_views_clear(scores, eye_d2, min_d2))
    finally:
        trk.close()


# ---- 11. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    vol = carved_volume()
    trk = ctx(hsk, AT.DST_DIMS, AT.DST_SIZE)
    try:
        trk.upload_tsdf(vol)
        fld = trk.download_clearance()
        out = np.full(80 * 64 * 48, 9, np.uint32)
        pts = np.ones((4, 3), f32)
        for bad in (dict(weight=(0, 1, 1)), dict(weight=(1, 1025, 1)), dict(weight=(1, 1, 0xFFFFFFFF)), dict(flags=2), dict(flags=3), dict(max_d2=16 * 256 * 256),
                    dict(weight=(1, 1, 1), max_d2=65536), dict(max_d2=0xFFFFFFFF)):
            p = trk.default_clearance_params(**bad)
            st = L.HskClearanceStats(n_far=77)
            assert lib.hsk_build_clearance(trk.h, C.byref(p), C.byref(st)) == -1 and st.n_far == 77 and lib.hsk_last_error(trk.h), bad
            assert lib.hsk_download_clearance(trk.h, C.byref(p), None, out.ctypes.data) == -1
            assert lib.hsk_clearance_at(trk.h, C.byref(p), pts.ctypes.data, 4, out.ctypes.data) == -1
            assert lib.hsk_clearance_floor(trk.h, C.byref(p), 1, 0, 4, out.ctypes.data, C.byref(st)) == -1 and st.n_far == 77
            assert (out == 9).all()
        p = trk.default_clearance_params()
        for lo, hi in (((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (81, 4, 4)), ((0, 5, 0), (4, 4, 4)), ((0, 0, 0), (4, 4, 49))):
            b = L.HskVoxelBox()
            b.lo[:], b.hi[:] = lo, hi
            assert lib.hsk_download_clearance(trk.h, C.byref(p), C.byref(b), out.ctypes.data) == -1 and b"box" in lib.hsk_last_error(trk.h)
        st = L.HskClearanceStats(n_far=77)
        for axis, lo, hi in ((-1, 0, 1), (3, 0, 1), (0, -1, 4), (0, 0, 81), (1, 0, 65), (2, 0, 49), (2, 9, 8)):
            assert lib.hsk_clearance_floor(trk.h, C.byref(p), axis, lo, hi, out.ctypes.data, C.byref(st)) == -1 and st.n_far == 77, (axis, lo, hi)
        assert lib.hsk_clearance_floor(trk.h, C.byref(p), 1, 0, 4, None, None) == -1
        assert lib.hsk_download_clearance(trk.h, C.byref(p), None, None) == -1
        assert lib.hsk_clearance_at(trk.h, C.byref(p), pts.ctypes.data, (1 << 20) + 1, out.ctypes.data) == -1 and b"2^20" in lib.hsk_last_error(trk.h)
        assert lib.hsk_clearance_at(trk.h, C.byref(p), None, 4, out.ctypes.data) == -1 and lib.hsk_clearance_at(trk.h, C.byref(p), pts.ctypes.data, 4, None) == -1
        assert (out == 9).all()
        with pytest.raises(hsk.KinfuError, match="weight"):
            trk.build_clearance(weight=(1, 2000, 1))
        assert trk.build_clearance()["reused"] == 1 and np.array_equal(trk.download_clearance(), fld) and np.array_equal(trk.download_tsdf(), vol)
        assert lib.hsk_build_clearance(trk.h, None, None) == 0                                     # NULL parameters: the defaults; no stats
    finally:
        trk.close()
    # between submit and wait
    trk = hsk.KinfuTracker(n=64)
    try:
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        trk.submit_frame(hsk.synth_depth(hsk.synth_pose(1)))
        out, st, pts = np.full(64 ** 3, 9, np.uint32), L.HskClearanceStats(n_far=77), np.ones((4, 3), f32)
        assert lib.hsk_build_clearance(trk.h, None, C.byref(st)) == -3 and st.n_far == 77 and b"in flight" in lib.hsk_last_error(trk.h)
        assert lib.hsk_download_clearance(trk.h, None, None, out.ctypes.data) == -3
        assert lib.hsk_clearance_at(trk.h, None, pts.ctypes.data, 4, out.ctypes.data) == -3
        assert lib.hsk_clearance_floor(trk.h, None, 1, 0, 4, out.ctypes.data, C.byref(st)) == -3 and st.n_far == 77 and (out == 9).all()
        _, ok = trk.wait_frame()
        assert ok and trk.build_clearance()["reused"] == 0
    finally:
        trk.close()
    # a context that stores part of its volume
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        for call in (lambda t: t.build_clearance(), lambda t: t.download_clearance(), lambda t: t.clearance_at(np.ones((1, 3), f32)), lambda t: t.clearance_floor(1, 0, 4)):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call(part)
        st = L.HskClearanceStats(n_far=77)
        assert lib.hsk_build_clearance(part.h, None, C.byref(st)) == -3 and st.n_far == 77
    finally:
        part.close()
