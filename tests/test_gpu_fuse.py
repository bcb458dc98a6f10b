"""hsk_fuse_volume on the GPU against the numpy restatement of the rule (tests/fuse_twin.py), BIT FOR BIT: the TSDF pairs, the
colour volume, n_fused, n_colored and the footprint box.  Two rooms scanned with colour at 128^3 are fused into a
128^3 volume and into a 256 x 128 x 128 volume over 6 x 3 x 3 m, each case only after the twin's own result has been shown to
be non-trivial.  Then: the destination is a whole, consistent context afterwards (every product, a raycast and an integrate
agree byte for byte with a fresh context that was handed the same volume by hsk_upload_tsdf / hsk_upload_color); the source is
untouched; the skip test bites where it must; the rule's own properties on the device; the errors."""
import ctypes as C

import numpy as np
import pytest

import fuse_twin as FT
import section_twin as ST
import view_twin as VT
from fuse_cases import (HOUSE_DIMS, HOUSE_SIZE, N, PLANE_N, PLANE_TAU, SIZE, _close_scans, assert_fused, assert_nontrivial,  # noqa: F401  (the fixture closes the scans)
                        empty_like_ctx, general, make_ctx, plane_case, room_scan)
from kit import same_bits_nan
from section_cases import SCAN_FRAMES, ortho_cam, room_frames

pytestmark = pytest.mark.gpu
f32 = np.float32
CELL = 3.0 / N


TRANSFORMS = {
    "identity": lambda: np.eye(4, dtype=f32),
    "offset": lambda: FT.translation(((10 + 0.5) * CELL, -(6 + 0.5) * CELL, (4 + 0.5) * CELL)),
    "rotation": lambda: general(n=N),
    "corner": lambda: FT.rot_about("y", 30.0, (1.5, 1.5, 1.5), (1.25, -0.4, 1.3)),   # only a corner of the source stays inside
}


# ---- 1. into an empty destination, four transforms --------------------------------------------------------
@pytest.mark.parametrize("name", list(TRANSFORMS))
def test_fuse_into_an_empty_volume_matches_the_twin(hsk, name):
    src, s_tsdf, s_col = room_scan(hsk, 0)
    m = TRANSFORMS[name]()
    d_tsdf, d_col = empty_like_ctx((N, N, N))
    ref_t, ref_c, ref_s = FT.fuse(d_tsdf, SIZE, s_tsdf, SIZE, m, d_col, s_col, max_w=64)
    assert_nontrivial(ref_t, ref_s, s_tsdf, name)
    assert ref_s["n_colored"] > 0
    dst = make_ctx(hsk)
    try:
        st = dst.fuse_from(src, m)
        print(f"{name}: {st}")
        assert_fused(dst, st, ref_t, ref_c, ref_s, FT.footprint((N,) * 3, SIZE, (N,) * 3, SIZE, m), name)
        assert st["chunks_swept"] > 0
        if name == "corner":
            assert st["chunks_swept"] < st["chunks_total"], f"the skip test does not bite: {st}"
    finally:
        dst.close()


# ---- 2. two rooms into a house volume, overlapping --------------------------------------------------------
def house_case(hsk):
    """room 0 turned by 20 degrees 0.7 m into the house, room 1 turned the other way and placed 2.6 m along x: their boxes
    (and their observed interiors) intersect, and each footprint holds chunks its room never reaches"""
    m0 = FT.rot_about("y", 20.0, (1.5, 1.5, 1.5), (0.7 + 0.4 * CELL, 0.3 * CELL, -0.2 * CELL))
    m1 = FT.rot_about("y", -10.0, (1.5, 1.5, 1.5), (2.6, 0.1 * CELL, 0.2 * CELL))
    (_, t0, c0), (_, t1, c1) = room_scan(hsk, 0), room_scan(hsk, 1)
    d_tsdf, d_col = empty_like_ctx(HOUSE_DIMS)
    r0 = FT.fuse(d_tsdf, HOUSE_SIZE, t0, SIZE, m0, d_col, c0)
    r1 = FT.fuse(r0[0], HOUSE_SIZE, t1, SIZE, m1, r0[1], c1)
    return (m0, m1), r0, r1


def test_two_rooms_into_a_house_volume(hsk):
    (m0, m1), r0, r1 = house_case(hsk)
    src0, t0, _ = room_scan(hsk, 0)
    src1, t1, _ = room_scan(hsk, 1)
    assert_nontrivial(r0[0], r0[2], t0, "room 0 into the house")
    assert_nontrivial(r1[0], r1[2], t1, "room 1 into the house")
    both = int((r0[2]["fused"] & r1[2]["fused"]).sum())
    assert both >= 1000, f"only {both} house voxels took a sample from both rooms"
    b0 = FT.footprint((N,) * 3, SIZE, HOUSE_DIMS, HOUSE_SIZE, m0)
    b1 = FT.footprint((N,) * 3, SIZE, HOUSE_DIMS, HOUSE_SIZE, m1)
    assert all(max(b0[2 * i], b1[2 * i]) < min(b0[2 * i + 1], b1[2 * i + 1]) for i in range(3)), "the rooms' boxes do not intersect"
    house = make_ctx(hsk, HOUSE_DIMS, HOUSE_SIZE)
    try:
        s0 = house.fuse_from(src0, m0)
        print(f"room 0: {s0}")
        assert_fused(house, s0, r0[0], r0[1], r0[2], b0, "room 0 into the house")
        assert 0 < s0["chunks_swept"] < s0["chunks_total"], f"the skip test does not bite in the 6 m volume: {s0}"
        n_before = house.extract_cloud(cap=0)[1]
        s1 = house.fuse_from(src1, m1)
        print(f"room 1: {s1}")
        assert_fused(house, s1, r1[0], r1[1], r1[2], b1, "room 1 into the house with room 0 in it")
        assert 0 < s1["chunks_swept"] < s1["chunks_total"]
        # a count taken before the fuse is not served from the count cache after it
        fresh = make_ctx(hsk, HOUSE_DIMS, HOUSE_SIZE)
        try:
            fresh.upload_tsdf(r1[0])
            n_after, n_fresh = house.extract_cloud(cap=0)[1], fresh.extract_cloud(cap=0)[1]
            assert n_after == n_fresh and n_after != n_before, (n_before, n_after, n_fresh)
        finally:
            fresh.close()
    finally:
        house.close()


# ---- 3. a destination whose weights are partly deferred ------------------------------------------------------
def test_fuse_into_a_volume_with_deferred_weights(hsk):
    """30 frames of room 1's scan through the tracker leave free-space weights in the summaries; the fuse must write them
    back first"""
    src, s_tsdf, s_col = room_scan(hsk, 0)
    frames = room_frames(hsk, 1, 0, 30)
    m = FT.rot_about("y", -5.0, (1.5, 1.5, 1.5), (0.2 * CELL, 0.0, 0.4 * CELL))

    def scanned():
        trk = hsk.KinfuTracker(n=N, init_pose=hsk.synth_room_pose(1, 0, SCAN_FRAMES))
        trk.enable_color()
        verdicts = [trk.process_frame_rgbd(d, c)[1] for d, c in frames]
        assert all(verdicts[1:])
        return trk

    a, b = scanned(), scanned()
    try:
        base_t, base_c = a.download_tsdf(), a.download_color()   # (a's weights are written back by the download; b's stay deferred)
        assert (base_t[..., 1] > 1).any()
        ref_t, ref_c, ref_s = FT.fuse(base_t, SIZE, s_tsdf, SIZE, m, base_c, s_col)
        assert_nontrivial(ref_t, ref_s, s_tsdf, "deferred")
        mixed = int((ref_s["fused"] & (base_t[..., 1] > 0)).sum())
        assert mixed >= 1000, f"only {mixed} voxels merged a sample with an observation"
        st = b.fuse_from(src, m)
        assert_fused(b, st, ref_t, ref_c, ref_s, FT.footprint((N,) * 3, SIZE, (N,) * 3, SIZE, m), "deferred")
    finally:
        a.close()
        b.close()


# ---- 4. the destination is a whole, consistent context afterwards ---------------------------------------------
def test_the_fused_context_equals_a_fresh_one_with_the_same_volume(hsk):
    src0, _, _ = room_scan(hsk, 0)
    src1, _, _ = room_scan(hsk, 1)
    m0 = general(n=N)
    m1 = FT.rot_about("y", 7.0, (1.5, 1.5, 1.5), (0.9, 0.1, -0.2))
    fused, fresh = make_ctx(hsk), make_ctx(hsk)
    try:
        assert fused.fuse_from(src0, m0)["n_fused"] > 0
        assert fused.fuse_from(src1, m1)["n_fused"] > 0
        tsdf, col = fused.download_tsdf(), fused.download_color()
        fresh.upload_tsdf(tsdf)
        fresh.upload_color(col)
        for a, b in zip(fused.extract_cloud_attrs(), fresh.extract_cloud_attrs()):
            assert same_bits_nan(np.asarray(a), np.asarray(b)), "cloud"
        assert fused.extract_cloud(cap=0)[1] > 1000
        for a, b in zip(fused.extract_mesh_indexed(), fresh.extract_mesh_indexed()):
            assert same_bits_nan(np.asarray(a), np.asarray(b)), "indexed mesh"
        pose = hsk.synth_room_pose(0, 40, SCAN_FRAMES)
        va = fused.render_view(pose=pose, mode=VT.COLOR_LIT, vmap=True, nmap=True)
        vb = fresh.render_view(pose=pose, mode=VT.COLOR_LIT, vmap=True, nmap=True)
        assert va["n_hit"] > 1000
        for key in va:
            assert same_bits_nan(np.asarray(va[key]), np.asarray(vb[key])), f"view: {key}"
        down = ST.look((1.5, -0.5, 1.5), (1.5, 0.5, 1.5), (0, 0, 1))
        sec = dict(ortho_cam(down), clip=[(0, 1, 0, -1.4)], mode=VT.LAMBERT, light=(0.3, -1.0, 0.2), light_in_camera=False,
                   light_directional=True, vmap=True, nmap=True)
        sa, sb = fused.render_section(**sec), fresh.render_section(**sec)
        assert sa["n_hit"] + sa["n_cut"] > 1000
        for key in sa:
            assert same_bits_nan(np.asarray(sa[key]), np.asarray(sb[key])), f"section: {key}"
        # scanning on: the raycast sets the pose and the model maps; then the same frame integrates into both
        for a, b in zip(fused.raycast(pose, want_keys=True), fresh.raycast(pose, want_keys=True)):
            assert same_bits_nan(a, b), "raycast"
        depth = hsk.synth_room_depth(0, pose)
        fused.integrate(depth, pose)
        fresh.integrate(depth, pose)
        assert fused.integrate_coarse_counts() == fresh.integrate_coarse_counts()
        ta, tb = fused.download_tsdf(), fresh.download_tsdf()
        assert np.array_equal(ta, tb) and not np.array_equal(ta, tsdf)
    finally:
        fused.close()
        fresh.close()


# ---- 5. the source is untouched ---------------------------------------------------------------------------------
def test_the_source_is_untouched(hsk):
    src, s_tsdf, s_col = room_scan(hsk, 1)
    cloud = src.extract_cloud_attrs()
    dst = make_ctx(hsk)
    try:
        assert dst.fuse_from(src, general(n=N))["n_fused"] > 0
    finally:
        dst.close()
    assert np.array_equal(src.download_tsdf(), s_tsdf) and np.array_equal(src.download_color(), s_col)
    for a, b in zip(cloud, src.extract_cloud_attrs()):
        assert same_bits_nan(np.asarray(a), np.asarray(b))


# ---- 6. the rule's own properties, on the device -----------------------------------------------------------------
def test_identity_and_fuse_twice_on_the_device(hsk):
    n = 64
    rng = np.random.default_rng(4)
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    vol = np.empty((n, n, n, 2), np.int16)
    vol[..., 0] = rng.integers(-32767, 32768, (n, n, n))
    vol[..., 1] = 1
    src, dst = hsk.KinfuTracker(n=n), hsk.KinfuTracker(n=n)
    try:
        src.upload_tsdf(vol)
        st = dst.fuse_from(src, np.eye(4, dtype=f32))
        assert st["n_fused"] == (n - 2) ** 3 == 238328 and st["n_colored"] == 0
        once = dst.download_tsdf()
        inner = (slice(1, n - 1),) * 3
        assert np.array_equal(once[inner][..., 0], vol[inner][..., 0]) and (once[inner][..., 1] == 1).all()
        shell = np.ones((n, n, n), bool)
        shell[inner] = False
        assert (once[shell] == 0).all()
        assert dst.fuse_from(src, np.eye(4, dtype=f32))["n_fused"] == (n - 2) ** 3
        twice = dst.download_tsdf()
        assert np.array_equal(twice[..., 0], once[..., 0]) and (twice[inner][..., 1] == 2).all() and (twice[shell] == 0).all()
    finally:
        src.close()
        dst.close()


def test_a_rotated_plane_stays_within_two_raw_units_on_the_device(hsk):
    """test_fuse_host's plane through hsk_extract_cloud on the destination: every point of the cloud within 2 tau / 32767 =
    18 um of the moved plane"""
    vol, m, nrm, d = plane_case()
    src = hsk.KinfuTracker(n=PLANE_N, trunc_dist_m=PLANE_TAU)
    dst = hsk.KinfuTracker(n=PLANE_N, trunc_dist_m=PLANE_TAU)
    try:
        src.upload_tsdf(vol)
        st = dst.fuse_from(src, m)
        assert st["n_fused"] > 100000
        ref_t, _, ref_s = FT.fuse(np.zeros_like(vol), SIZE, vol, SIZE, m)
        assert st["n_fused"] == ref_s["n_fused"] and np.array_equal(dst.download_tsdf(), ref_t)
        pts, total = dst.extract_cloud()
        assert total == len(pts) > 1000
        err = np.abs(pts.astype(np.float64) @ nrm - d)
        print(f"fused {st['n_fused']}, {len(pts)} cloud points, worst {err.max() * 1e6:.2f} um")
        assert err.max() <= 2 * PLANE_TAU / 32767
    finally:
        src.close()
        dst.close()


def test_a_source_whose_brick_table_does_not_fit_the_lds(hsk):
    """1024 x 1024 x 512 voxels have 1 Mi bricks, a table of 128 KiB: the sweep reads it from memory instead of staging it
    (fuse.hip: k_fuse_sweep<false, ..>); a 64^3 destination of 0.4 m is placed across the edge of the one observed block"""
    sdims, ssize = (1024, 1024, 512), (3.0, 3.0, 1.5)
    rng = np.random.default_rng(12)
    vol = np.zeros((sdims[2], sdims[1], sdims[0], 2), np.int16)
    blk = (slice(120, 260), slice(300, 520), slice(400, 640))          # (z, y, x)
    shape = tuple(s.stop - s.start for s in blk)
    vol[blk + (0,)] = rng.integers(-32767, 32768, shape)
    vol[blk + (1,)] = rng.integers(1, 6, shape)
    cell = 3.0 / 1024
    m = np.linalg.inv(FT.rot_about("z", 17.0, (0.2, 0.2, 0.2), (520 * cell, 440 * cell, 90 * cell)).astype(np.float64)).astype(f32)
    ref_t, _, ref_s = FT.fuse(np.zeros((64, 64, 64, 2), np.int16), (0.4,) * 3, vol, ssize, m)
    assert 20000 < ref_s["n_fused"] < 64 ** 3 - 20000
    src = hsk.KinfuTracker(hsk.default_config(sdims[2], vol_x=sdims[0], vol_y=sdims[1], vol_z=sdims[2], vol_size_m=ssize))
    dst = hsk.KinfuTracker(hsk.default_config(64, vol_size_m=(0.4,) * 3))
    try:
        src.upload_tsdf(vol)
        st = dst.fuse_from(src, m)
        print(f"large source: {st}")
        assert_fused(dst, st, ref_t, None, ref_s, FT.footprint(sdims, ssize, (64,) * 3, (0.4,) * 3, m), "large source")
    finally:
        src.close()
        dst.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------
def test_errors(hsk):
    lib = hsk._lib.load()
    fp = C.POINTER(C.c_float)
    eye = np.eye(4, dtype=f32)
    src, dst = make_ctx(hsk, (64, 64, 64)), make_ctx(hsk, (64, 64, 64))
    depth = hsk.synth_depth(hsk.synth_pose(0))
    try:
        src.integrate(depth, hsk.synth_pose(0))
        code = lambda d, s, m=eye: lib.hsk_fuse_volume(d, s, None if m is None else np.ascontiguousarray(m, f32).reshape(16).ctypes.data_as(fp), None)  # noqa: E731
        assert code(dst.h, src.h) == 0
        assert code(None, src.h) == -1 and code(dst.h, None) == -1 and code(dst.h, src.h, None) == -1
        with pytest.raises(hsk.KinfuError, match="same context"):
            dst.fuse_from(dst, eye)
        scaled = eye.copy()
        scaled[:3, :3] *= f32(1.05)
        with pytest.raises(hsk.KinfuError, match="rigid"):
            dst.fuse_from(src, scaled)
        row = eye.copy()
        row[3, 3] = 0.5
        with pytest.raises(hsk.KinfuError, match="rigid"):
            dst.fuse_from(src, row)
        other_tau = make_ctx(hsk, (64, 64, 64), trunc_dist_m=0.25)
        try:
            with pytest.raises(hsk.KinfuError, match="truncation"):
                dst.fuse_from(other_tau, eye)
            with pytest.raises(hsk.KinfuError, match="truncation"):
                other_tau.fuse_from(src, eye)
        finally:
            other_tau.close()
        # a frame in flight, in either context
        for busy, args in ((src, (dst, src)), (dst, (dst, src))):
            busy.submit_frame(depth)
            with pytest.raises(hsk.KinfuError, match="in flight"):
                args[0].fuse_from(args[1], eye)
            busy.wait_frame()
        # an empty footprint: nothing happens
        before = dst.download_tsdf()
        st = dst.fuse_from(src, FT.translation((9.0, 0.0, 0.0)))
        assert st == {"n_fused": 0, "n_colored": 0, "chunks_total": 0, "chunks_swept": 0, "box": (0,) * 6}
        assert np.array_equal(dst.download_tsdf(), before)
        # colour in one context only is not an error: the TSDF is fused, the colour untouched
        plain = make_ctx(hsk, (64, 64, 64), color=False)
        try:
            plain.integrate(depth, hsk.synth_pose(0))
            col = dst.download_color()
            st = dst.fuse_from(plain, eye)
            assert st["n_fused"] > 0 and st["n_colored"] == 0 and np.array_equal(dst.download_color(), col)
            assert plain.fuse_from(src, eye)["n_colored"] == 0
        finally:
            plain.close()
    finally:
        src.close()
        dst.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    whole = hsk.KinfuTracker(n=64)
    try:
        g.process_frame(depth)
        for i in range(g.n_slabs()):
            with pytest.raises(hsk.KinfuError, match="slab"):
                whole.fuse_from(g.slab(i), eye)
            with pytest.raises(hsk.KinfuError, match="hskinfu error -3"):
                g.slab(i).fuse_from(whole, eye)
        assert g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))[1]
    finally:
        whole.close()
        g.close()
