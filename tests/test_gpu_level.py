"""The upright-frame estimate on the GPU, BIT FOR BIT against the numpy restatement of the rule (tests/level_twin.py): the device
stages alone (hsk_upright_sums) at the sizes where a wave, a block or the grid is partly filled; hsk_estimate_upright on the
uploaded tilted scene, every field, and what it leaves untouched; the levelled volume end to end -- hsk_level_config, hsk_create,
hsk_fuse_volume, then the estimate, the planes and the floor map on the result; the errors."""
import ctypes as C
import math

import numpy as np
import pytest

import align_twin as AT
import level_twin as LT
from kit import same_bits, state_of, volume_ctx
from level_cases import ANGLE_BAR_DEG, assert_same_upright, jittered, tilted, twin_of

pytestmark = pytest.mark.gpu
f32 = np.float32


def ctx(hsk, scene, **over):
    return volume_ctx(hsk, *LT.SCENES[scene], **over)


@pytest.fixture(scope="module")
def trk(hsk):
    """a context for the cloud forms, which read no volume"""
    t = ctx(hsk, "64")
    yield t
    t.close()


@pytest.fixture(scope="module")
def tilted_src(hsk):
    """the 80 x 64 x 48 scene under tilt a, uploaded"""
    t = ctx(hsk, "80x64x48")
    t.upload_tsdf(tilted("80x64x48", "a")[0])
    yield t
    t.close()


# ---- 1. the device stages against the twin ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 70001, 262209])
def test_upright_sums_match_the_twin(hsk, trk, n):
    """a partial wave, a whole one, one lane more, more than a block, 274 blocks with a partial last one, and the grid's cap of 1024
    blocks with a second trip of one block's partial wave (1024 x 256 + 65); the clouds are the tilted scene's repeated with
    jitter behind the edge cases; the axes are integers, so no float decides an inlier: zero differences"""
    ps, ns = jittered(n)
    assert len(ps) == n
    w = LT.cell_weights(*LT.SCENES["80x64x48"])
    ref = twin_of("80x64x48", "a")
    rows = [LT.quantise_axis([float(v) for v in ref["level"][k, :3]]) for k in range(3)]
    up = [-v for v in rows[1]]
    wall_axes = [up, rows[0], rows[2]]
    odd = [[4096, 0, 0], [2365, -2365, 2365], [0, 0, -1]]
    ok, N, P = LT.quantise(ps, ns, w)
    for axes, cone_cos, wall_sin in ((rows, LT.DEFAULTS["cone_cos"], LT.DEFAULTS["wall_sin"]), (odd, 0.5, 1.0), (rows[1:2], 1.0, 0.0)):
        got = trk.upright_sums(ps, ns, w, cone_cos, wall_sin, hist=True, axes=axes, wall_axes=wall_axes, frame=rows, heights=True)
        assert got["n_valid"] == int(ok.sum()) and np.array_equal(got["hist"], LT.histogram(ok, N)), n
        want = np.array([LT.axis_sums(ok, N, a, cone_cos) for a in axes], np.int64)
        assert np.array_equal(got["axis_sums"], want), (n, got["axis_sums"], want)
        want = np.array(LT.wall_sums(ok, N, *wall_axes, wall_sin), np.int64)
        assert np.array_equal(got["wall_sums"], want), (n, got["wall_sums"], want)
        box, cnt, sm = LT.extents(ok, N, P, rows, cone_cos)
        assert list(got["box"]) == box, (n, got["box"], box)
        assert np.array_equal(got["height_counts"], cnt) and np.array_equal(got["height_sums"], sm), n
    # the stages one at a time, and without the weights
    ok1, N1, P1 = LT.quantise(ps, ns)
    only = trk.upright_sums(ps, ns, hist=True)
    assert set(only) == {"hist", "n_valid"} and np.array_equal(only["hist"], LT.histogram(ok1, N1))
    only = trk.upright_sums(ps, ns, frame=rows)
    assert set(only) == {"box"} and list(only["box"]) == LT.extents(ok1, N1, P1, rows, 0.9, classes=False)[0]
    only = trk.upright_sums(ps, ns, wall_axes=wall_axes)
    assert set(only) == {"wall_sums"} and list(only["wall_sums"]) == LT.wall_sums(ok1, N1, *wall_axes, LT.DEFAULTS["wall_sin"])


def test_upright_sums_of_nothing_and_of_invalid_points(hsk, trk):
    rows = [[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]]
    for ps, ns in ((np.zeros((0, 3), f32), np.zeros((0, 3), f32)), (np.ones((300, 3), f32), np.full((300, 3), np.nan, f32))):
        got = trk.upright_sums(ps, ns, hist=True, axes=rows, wall_axes=rows, frame=rows, heights=True)
        assert got["n_valid"] == 0 and not got["hist"].any() and not got["axis_sums"].any() and not got["wall_sums"].any()
        assert not got["box"].any() and not got["height_counts"].any() and not got["height_sums"].any()


# ---- 2. the estimate against the twin -------------------------------------------------------------------------------------------
def test_estimate_upright_oriented_matches_the_twin(hsk, trk):
    """the whole estimate on caller clouds: the tilted scenes, the parameters' corners, the edge cases, nothing"""
    for scene, tilt, params in (("80x64x48", "a", {}), ("64", "b", {}), ("80x64x48", "a", dict(flags=LT.NO_YAW)), ("64", "b", dict(refits=0)),
                                ("80x64x48", "b", dict(refits=8, min_fraction=0.1, cone_cos=0.9, wall_sin=0.5))):
        _, ps, ns, w, _ = tilted(scene, tilt)
        assert_same_upright(trk.estimate_upright_oriented(ps, ns, w, **params), twin_of(scene, tilt, **params), (scene, tilt, params))
    eps, ens = LT.edge_cloud()
    assert_same_upright(trk.estimate_upright_oriented(eps, ens), LT.estimate(eps, ens), "the edge cases")
    ps, ns = jittered(3000)
    assert_same_upright(trk.estimate_upright_oriented(ps, ns, up_hint=(0.1, 1.0, 0.0)), LT.estimate(ps, ns, up_hint=(0.1, 1.0, 0.0)), "jitter, up along +y")
    none = trk.estimate_upright_oriented(np.zeros((0, 3), f32), np.zeros((0, 3), f32))
    assert none["found"] == 0 and same_bits(none["level"], np.eye(4, dtype=f32)) and none["n_points"] == 0
    bad = trk.estimate_upright_oriented(ps[:500], np.full((500, 3), np.nan, f32))
    assert_same_upright(bad, LT.estimate(ps[:500], np.full((500, 3), np.nan, f32)), "only NaN normals")
    assert bad["found"] == 0 and bad["n_invalid"] == 500


@pytest.mark.parametrize("scene", list(LT.SCENES))
def test_estimate_upright_on_the_uploaded_tilted_scene(hsk, scene):
    """every field of hsk_upright equals the twin's on (extract_cloud, normal_at), bit for bit; pose, TSDF and model maps stay; the
    cached count pass is still valid: extract_cloud_attrs afterwards returns the same cloud; a second context gives the same bits"""
    vol, ps, ns, w, R = tilted(scene, "a")
    ref = twin_of(scene, "a")
    t, other = ctx(hsk, scene), ctx(hsk, scene)
    try:
        t.upload_tsdf(vol)
        xyz, nrm, _, total, _ = t.extract_cloud_attrs(rgb=False)
        assert total == len(ps) and same_bits(xyz, ps)
        before = state_of(t, True)
        got = t.estimate_upright()
        for a, b in zip(before, state_of(t, True)):
            assert same_bits(a, b), "hsk_estimate_upright moved something"
        assert_same_upright(got, ref, scene)
        xyz2, nrm2, _, total2, _ = t.extract_cloud_attrs(rgb=False)
        assert total2 == total and same_bits(xyz2, xyz) and np.array_equal(nrm2.view(np.uint32), nrm.view(np.uint32))
        assert_same_upright(t.estimate_upright(), ref, "a second call, behind another product")
        assert_same_upright(t.estimate_upright_oriented(xyz, nrm, w), ref, "the cloud form on the same cloud")
        other.upload_tsdf(vol)
        assert_same_upright(other.estimate_upright(), got, "a second context")
        assert_same_upright(t.estimate_upright(refits=1, flags=LT.NO_YAW), twin_of(scene, "a", refits=1, flags=LT.NO_YAW), "other parameters")
        t.reset()
        empty = t.estimate_upright()
        assert empty["found"] == 0 and empty["n_points"] == 0 and same_bits(empty["level"], np.eye(4, dtype=f32))
    finally:
        t.close()
        other.close()


# ---- 3. end to end: the levelled volume ---------------------------------------------------------------------------------------------
def free_outline(fmap):
    """the bounding box of the free columns of a floor map [v, u]: (u0, u1, v0, v1), half-open"""
    v, u = np.nonzero(fmap)
    return int(u.min()), int(u.max()) + 1, int(v.min()), int(v.max()) + 1


def outline_defect_m2(fmap, rect, cu, cv):
    """how far the free columns are from filling the rectangle (u0, u1, v0, v1), to within two cells: the area of the columns that
    are not free inside the rectangle drawn in by two cells, plus that of the free columns outside the rectangle let out by two"""
    u0, u1, v0, v1 = rect
    free = fmap != 0
    u, v = np.meshgrid(np.arange(free.shape[1]) + 0.5, np.arange(free.shape[0]) + 0.5)
    inner = (u >= u0 + 2) & (u <= u1 - 2) & (v >= v0 + 2) & (v <= v1 - 2)
    outer = (u >= u0 - 2) & (u <= u1 + 2) & (v >= v0 - 2) & (v <= v1 + 2)
    return (int((inner & ~free).sum()) + int((free & ~outer).sum())) * cu * cv


def test_the_levelled_volume_end_to_end(hsk, tilted_src):
    src = tilted_src
    dims, size = LT.SCENES["80x64x48"]
    R = tilted("80x64x48", "a")[4]
    up = src.estimate_upright()
    assert up["found"] == 15
    cfg, M = src.level_config(up)
    t_dims, t_size, t_trunc, t_M = LT.level_config(dims, size, 0.03, twin_of("80x64x48", "a"))
    assert (cfg.vol_x, cfg.vol_y, cfg.vol_z) == t_dims and same_bits(np.array(cfg.vol_size_m, f32), t_size) and same_bits(f32(cfg.trunc_dist_m), t_trunc)
    assert same_bits(M, t_M) and (cfg.own_z0, cfg.own_z1, cfg.halo) == (0, cfg.vol_z, 0)
    assert np.allclose(np.array(cfg.init_pose, np.float64).reshape(4, 4), M.astype(np.float64) @ src.get_pose().astype(np.float64), atol=1e-5)
    dst = hsk.KinfuTracker(cfg)
    try:
        st = dst.fuse_from(src, M)
        assert st["n_fused"] > 10000
        cell = float(cfg.vol_size_m[0]) / cfg.vol_x
        assert cell <= 0.0625 and cell > 0.06249
        # the estimate on the levelled volume: level within the bar of the identity, the floor where level_config put it
        lev = dst.estimate_upright()
        L = lev["level"][:3, :3].astype(np.float64)
        off = [math.degrees(math.acos(min(1.0, float(L[k, k])))) for k in range(3)]
        want_floor = float(up["floor_m"]) + float(M[1, 3])
        print(f"levelled: rows {off} degrees off the axes, floor {lev['floor_m']:.4f} (put at {want_floor:.4f}), dims {t_dims}, fused {st['n_fused']}")
        assert lev["found"] == 15 and max(off) <= ANGLE_BAR_DEG
        assert abs(float(lev["floor_m"]) - want_floor) <= cell
        # the planes of the levelled volume: the room's six faces, each within half a degree of a volume axis (one resampling lies between)
        rec, _ = dst.detect_planes()
        big = rec[:6]
        seen = set()
        for r in big:
            n = r["abcd"][:3].astype(np.float64)
            k = int(np.argmax(np.abs(n)))
            ang = math.degrees(math.acos(min(1.0, abs(float(n[k])) / float(np.linalg.norm(n)))))
            print(f"   plane {r['abcd']} with {r['n_inliers']} points: {ang:.4f} degrees off axis {k}")
            assert ang <= 2 * ANGLE_BAR_DEG
            seen.add((k, bool(n[k] > 0)))
        assert len(rec) >= 6 and len(seen) == 6
        # the floor map of the band 0.1 .. 1.8 m above the floor (y points down): its free columns' outline is the room's rectangle
        lo, hi = math.ceil((float(lev["floor_m"]) - 1.8) / cell), math.floor((float(lev["floor_m"]) - 0.1) / cell)
        fmap, _ = dst.clearance_floor(1, lo, hi)
        c = np.array(AT.CENTRE)
        corners = np.array([[x, y, z] for x in (AT.ROOM[0][0], AT.ROOM[1][0]) for y in (AT.ROOM[0][1], AT.ROOM[1][1]) for z in (AT.ROOM[0][2], AT.ROOM[1][2])])
        in_dst = ((corners - c) @ R + c) @ M[:3, :3].astype(np.float64).T + M[:3, 3].astype(np.float64)       # (scene -> tilted volume: R^T (s - c) + c)
        want = (in_dst[:, 0].min() / cell, in_dst[:, 0].max() / cell, in_dst[:, 2].min() / cell, in_dst[:, 2].max() / cell)
        got = free_outline(fmap)
        print(f"   band planes {lo} .. {hi}: free outline {got}, the room's rectangle {tuple(round(v, 2) for v in want)} (cells)")
        assert all(abs(g - w_) <= 2.0 for g, w_ in zip(got, want))
        # ... and they fill it, but for the furniture, which reaches into the band: 0.5 x 0.5 m and a cell of solid voxels around it
        furniture = (AT.FURNITURE[1][0] - AT.FURNITURE[0][0] + 2 * cell) * (AT.FURNITURE[1][2] - AT.FURNITURE[0][2] + 2 * cell)
        defect = outline_defect_m2(fmap, want, cell, cell)
        print(f"   not free inside it, or free outside: {defect:.3f} m2 (the furniture: at most {furniture:.3f} m2)")
        assert defect <= furniture
        # On the tilted source the same band, about the floor's centre, has no such outline: measured against the rectangle most in
        # its favour, the free columns' own bounding box, it misses the bar the levelled volume meets.  (The yaw alone cuts four
        # corners of 1.7 m2 together off that box; the tilt lifts the floor into the band along one wall.)
        floor_centre = (np.array([c[0], AT.ROOM[1][1], c[2]]) - c) @ R + c
        cy = 3.0 / 64
        smap, _ = src.clearance_floor(1, math.ceil((floor_centre[1] - 1.8) / cy), math.floor((floor_centre[1] - 0.1) / cy))
        s_defect = outline_defect_m2(smap, free_outline(smap), 3.0 / 80, 3.0 / 48)
        print(f"   tilted source: {s_defect:.3f} m2 against its own bounding box {free_outline(smap)}")
        assert s_defect > furniture
    finally:
        dst.close()
    # the convenience: a new tracker that holds the levelled volume
    lv, M2, up2 = src.levelled()
    try:
        assert same_bits(M2, M) and up2["found"] == 15 and (lv.cfg.vol_x, lv.cfg.vol_y, lv.cfg.vol_z) == t_dims
        assert lv.extract_cloud()[1] > 5000
    finally:
        lv.close()


# ---- 4. the errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors(hsk, trk, tilted_src):
    lib = hsk._lib.load()
    _, ps, ns, w, _ = tilted("64", "a")
    ps, ns = np.ascontiguousarray(ps[:256]), np.ascontiguousarray(ns[:256])
    u = hsk._lib.HskUpright()
    rows = np.array([[4096, 0, 0], [0, 4096, 0], [0, 0, 4096]], np.int32)
    s12, box = np.zeros(12, np.int64), np.zeros(6, np.int32)

    def est(h=trk.h, p=ps.ctypes.data, q=ns.ctypes.data, m=256, wt=None, params=None, out=C.byref(u)):
        return lib.hsk_estimate_upright_oriented(h, p, q, m, wt, params, out)

    def sums(h=trk.h, p=ps.ctypes.data, q=ns.ctypes.data, m=256, cone=0.9, wall=0.2, axes=rows.ctypes.data, na=3, out=s12.ctypes.data, frame=None, b=None):
        return lib.hsk_upright_sums(h, p, q, m, None, cone, wall, None, None, axes, na, out, None, None, frame, b, None, None)

    assert est() == 0 and sums() == 0 and s12[0] > 0
    assert est(p=None) == -1 and est(q=None) == -1 and est(out=None) == -1
    assert est(m=(1 << 24) + 1) == -1 and "2^24" in lib.hsk_last_error(trk.h).decode()
    for bad in ((0.0, 1.0, 1.0), (1.0, 1.5, 1.0), (1.0, 1.0, float("nan")), (-1.0, 1.0, 1.0)):
        assert est(wt=np.array(bad, f32).ctypes.data) == -1 and "weight" in lib.hsk_last_error(trk.h).decode()
    for name, bad in (("up_hint", (0, 0, 0)), ("up_hint", (0, float("nan"), 1)), ("up_hint", (float("inf"), 0, 0)), ("max_tilt_cos", 1.5), ("max_tilt_cos", -1.5),
                      ("max_tilt_cos", float("nan")), ("cone_cos", 0.0), ("cone_cos", 1.5), ("cone_cos", float("nan")), ("wall_sin", -0.1), ("wall_sin", 1.5),
                      ("wall_sin", float("nan")), ("min_fraction", float("nan")), ("min_fraction", -0.1), ("min_fraction", float("inf")), ("refits", -1),
                      ("refits", 9), ("flags", 2)):
        p = hsk.KinfuTracker._upright_params({name: bad})
        assert est(params=C.byref(p)) == -1 and "range" in lib.hsk_last_error(trk.h).decode(), (name, bad)
        assert lib.hsk_estimate_upright(tilted_src.h, C.byref(p), C.byref(u)) == -1, (name, bad)
    p = hsk.KinfuTracker._upright_params(dict(max_tilt_cos=-1.0, cone_cos=1.0, wall_sin=1.0, min_fraction=2.0, refits=8, flags=1))
    assert est(params=C.byref(p)) == 0 and u.found == 0               # the least count is above the cloud's size
    assert lib.hsk_estimate_upright(tilted_src.h, None, None) == -1
    assert sums(p=None) == -1 and sums(na=4) == -1 and sums(na=-1) == -1 and sums(axes=None) == -1 and sums(cone=0.0) == -1 and sums(wall=1.5) == -1
    assert sums(m=(1 << 24) + 1) == -1 and sums(b=box.ctypes.data) == -1                 # (a box without its frame)
    for bad in ([0, 0, 0], [4101, 0, 0], [2400, 2400, 2400]):
        long_axes = rows.copy()
        long_axes[1] = bad
        assert sums(axes=long_axes.ctypes.data) == -1 and "axis" in lib.hsk_last_error(trk.h).decode(), bad
        assert sums(na=0, out=None, frame=long_axes.ctypes.data, b=box.ctypes.data) == -1
    assert sums(m=0, p=None, q=None) == 0 and not s12.any() and est(m=0, p=None, q=None) == 0 and u.found == 0 and u.level[0] == 1.0
    with pytest.raises(ValueError, match="normals"):
        trk.estimate_upright_oriented(ps, ns[:-1])
    # hsk_level_config: UP not found, a margin that is not finite
    cfg, m = hsk._lib.HskConfig(), np.zeros(16, f32)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    none = hsk._lib.HskUpright()
    assert lib.hsk_level_config(tilted_src.h, C.byref(none), -1.0, C.byref(cfg), fp) == -1 and "not found" in lib.hsk_last_error(tilted_src.h).decode()
    good = hsk.KinfuTracker._upright_struct(tilted_src.estimate_upright())
    assert lib.hsk_level_config(tilted_src.h, C.byref(good), float("nan"), C.byref(cfg), fp) == -1
    assert lib.hsk_level_config(tilted_src.h, None, -1.0, C.byref(cfg), fp) == -1 and lib.hsk_level_config(tilted_src.h, C.byref(good), -1.0, None, fp) == -1
    assert lib.hsk_level_config(tilted_src.h, C.byref(good), -1.0, C.byref(cfg), None) == -1 and not m.any()
    assert lib.hsk_level_config(tilted_src.h, C.byref(good), 0.25, C.byref(cfg), fp) == 0 and cfg.vol_x % 8 == 0 and m[15] == 1.0
    # HSK_ERR_STATE: a frame in flight
    busy = hsk.KinfuTracker(n=64)
    try:
        busy.submit_frame(hsk.synth_depth(hsk.synth_pose(0)))
        assert est(h=busy.h) == -3 and "in flight" in lib.hsk_last_error(busy.h).decode()
        assert sums(h=busy.h) == -3 and lib.hsk_estimate_upright(busy.h, None, C.byref(u)) == -3
        busy.wait_frame()
        assert est(h=busy.h) == 0 and sums(h=busy.h) == 0
        assert lib.hsk_estimate_upright(busy.h, None, C.byref(u)) == 0 and u.n_points > 1000
    finally:
        busy.close()
    # ... the volume form on a context that stores part of its volume, and on the slabs of a group; the cloud forms read no volume
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        assert lib.hsk_estimate_upright(part.h, None, C.byref(u)) == -3 and "slab" in lib.hsk_last_error(part.h).decode()
        assert est(h=part.h) == 0 and sums(h=part.h) == 0
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        for i in range(g.n_slabs()):
            assert lib.hsk_estimate_upright(g.slab(i).h, None, C.byref(u)) == -3
        assert g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))[1]
    finally:
        g.close()
