"""hsk_render_section on the GPU.  The degenerate section (pinhole, no planes, a point light) against hsk_render_view, byte for
byte; floor plans, elevations and dollhouse views of a room the tracker scanned from inside against the numpy restatement of
the rule (tests/section_twin.py), every output and every count, each named camera only after the twin's own image has been
shown to hold hits, cut outlines and background; a tracker that does not notice sections rendered between its pipelined
frames; the errors; two rooms placed by .xf matrices composited into one floor plan; and what the floor plan of room 0 must
look like physically."""
import ctypes as C

import numpy as np
import pytest

import section_twin as ST
import view_twin as VT
from kit import same_bits_nan
from section_cases import SCAN_FRAMES, SIDE, SPAN, ortho_cam, room_frames
from view_cases import RAGGED, SENSOR, assert_trackers_equal, frames_of, moved, scan
from view_shape_cases import assert_section

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZE, TRUNC = (3.0, 3.0, 3.0), 0.03
KEYS = ("rgb", "depth", "vmap", "nmap")


# ---- scans --------------------------------------------------------------------------------------------


def scan_room(hsk, variant, n):
    """the tracker after the whole RGB-D scan of a room, pipelined; every frame must stay tracked"""
    trk = hsk.KinfuTracker(n=n, init_pose=hsk.synth_room_pose(variant, 0, SCAN_FRAMES))
    trk.enable_color()
    sent, verdicts = 0, []
    for lo in range(0, SCAN_FRAMES, 48):
        for d, c in room_frames(hsk, variant, lo, min(lo + 48, SCAN_FRAMES)):
            trk.submit_frame_rgbd(d, c)
            sent += 1
            if sent >= 2:
                verdicts.append(trk.wait_frame()[1])
    verdicts.append(trk.wait_frame()[1])
    assert all(verdicts[1:]), f"room {variant} at {n}^3: the scan lost tracking at frames {[i for i, ok in enumerate(verdicts) if not ok][:8]}"
    return trk


_SCANS = {}


def room_scan(hsk, variant, n):
    """(tracker, tsdf, colour volume) of a room's scan, made once per module"""
    key = (variant, n)
    if key not in _SCANS:
        trk = scan_room(hsk, variant, n)
        _SCANS[key] = (trk, trk.download_tsdf(), trk.download_color())
    return _SCANS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_scans():
    yield
    for trk, _, _ in _SCANS.values():
        trk.close()
    _SCANS.clear()


# ---- cameras ------------------------------------------------------------------------------------------


def room_cameras(ext):
    """name -> (section fields, required shares of (hit, cut, background) in the twin's image, or None)"""
    x0, x1, y0, y1, z0, z1 = (float(v) for v in ext)
    cx, cy, cz = 0.5 * (x0 + x1), 0.5 * (y0 + y1), 0.5 * (z0 + z1)
    at = lambda f: y0 + f * (y1 - y0)  # noqa: E731   (y points down: y1 is the floor)
    down = ST.look((cx, -0.5, cz), (cx, 0.5, cz), (0, 0, 1))       # exactly axis aligned: two direction components are 0
    up = ST.look((cx, 3.5, cz), (cx, 2.5, cz), (0, 0, 1))
    front = ST.look((cx, cy, -0.5), (cx, cy, 1.0), (0, -1, 0))
    doll = ST.look((cx - 2.6, y0 - 2.0, cz - 2.6), (cx, cy, cz), (0, -1, 0))
    diag = ST.look((cx - 2.0, cy, cz - 2.0), (cx, cy, cz), (0, -1, 0))   # along (1, 0, 1) / sqrt 2: d0 == d2 in binary32
    inside = ST.look((cx, cy, cz), (cx, cy + 1.0, cz), (0, 0, 1))
    ORTH, DOLL = (0.05, 0.01, 0.05), (0.0, 0.0025, 0.0)
    sun = dict(light=(0.3, -1.0, 0.2), light_in_camera=False, light_directional=True)
    cams = {
        "top-down 1/4": (dict(ortho_cam(down), clip=[(0, 1, 0, -at(0.25))], mode=VT.LAMBERT, **sun), ORTH),
        "top-down 1/2": (dict(ortho_cam(down), clip=[(0, 1, 0, -at(0.5))], mode=VT.COLOR_LIT, **sun, background=(20, 30, 40)), ORTH),
        "top-down 3/4": (dict(ortho_cam(down), clip=[(0, 1, 0, -at(0.75))], mode=VT.NORMALS, cut_rgb=(1, 2, 3)), ORTH),
        "bottom-up": (dict(ortho_cam(up), clip=[(0, -1, 0, at(0.5))], mode=VT.COLOR, background=(255, 255, 255)), ORTH),
        "elevation": (dict(ortho_cam(front), clip=[(0, 0, 1, -cz)], mode=VT.LAMBERT, light=(0, 0, -1), light_in_camera=True,
                           light_directional=True), ORTH),
        "dollhouse": (dict(width=SIDE, height=SIDE, fx=180.0, fy=180.0, cx=99.5, cy=99.5, pose=doll, projection=ST.PINHOLE,
                           clip=[(0, 1, 0, -at(0.4))], mode=VT.COLOR_LIT, light=(0.0, 0.0, 0.0), light_in_camera=True), DOLL),
        "two planes": (dict(ortho_cam(down), clip=[(0, 1, 0, -at(0.5)), (1, 0, 0, -cx)], mode=VT.LAMBERT, **sun), None),
        "box of four": (dict(ortho_cam(down), clip=[(0, 1, 0, -at(0.5)), (1, 0, 0, -(x0 + 0.5)), (-1, 0, 0, x1 - 0.5), (0, 0, 1, -cz)],
                             mode=VT.COLOR_LIT, light=(cx, cy, cz), light_in_camera=False), None),
        # a plane that contains the rays' direction (sd == 0 exactly): the rays on its far side are dead, the others are not
        # touched by it; a second plane cuts the near half of the room away
        "parallel plane": (dict(ortho_cam(diag), clip=[(1, 0, -1, cz - cx), (1, 0, 1, -(cx + cz))], mode=VT.LAMBERT, **sun), None),
        "parallel plane, other side": (dict(ortho_cam(diag), clip=[(-1, 0, 1, cx - cz), (1, 0, 1, -(cx + cz))], mode=VT.NORMALS), None),
        # the camera's plane inside the volume: the rays start on it (t_box = 0), nothing is cut; with a plane behind it, the same
        "camera inside": (dict(ortho_cam(inside), mode=VT.LAMBERT, **sun), None),
        "camera inside, plane behind": (dict(ortho_cam(inside), clip=[(0, 1, 0, -at(0.25))], mode=VT.LAMBERT, **sun), None),
        "no clip": (dict(ortho_cam(down), mode=VT.LAMBERT, **sun), None),
    }
    return cams, down, at(0.5)


def twin_and_gpu(trk, tsdf, color, fields):
    sec = ST.section(**fields)
    ref = ST.render(tsdf, SIZE, TRUNC, sec, color=color)
    from housescan_amd import _lib
    got = trk.render_section(ST.to_struct(sec, _lib), vmap=True, nmap=True)
    return sec, ref, got


def shares(ref):
    return tuple(float((ref["cls"] == c).mean()) for c in (ST.HIT, ST.CUT, ST.BACKGROUND))


# ---- 1. the degenerate section is hsk_render_view ---------------------------------------------------------
@pytest.mark.parametrize("n,color", [(256, True), (512, True), (1024, False)])
def test_degenerate_section_is_render_view(hsk, n, color):
    """pinhole, no planes, a point light: rgb, depth_mm, vmap, nmap, n_hit and n_uncolored are hsk_render_view's, n_cut is 0 --
    all four modes, a `follow` view, 640 x 480 and a ragged size (1024^3: geometry only, the 16 x 4 tile form)"""
    trk, last = scan(hsk, (n, n, n), "synth", 12 if n < 1024 else 3, color=color)
    modes = (VT.LAMBERT, VT.NORMALS, VT.COLOR, VT.COLOR_LIT) if color else (VT.LAMBERT, VT.NORMALS)
    free = moved(hsk.synth_pose(2), 8.0, 0.1)
    checked = 0
    for cam, pose in ((SENSOR, None), (SENSOR, free), (RAGGED, free), (RAGGED, last)):
        for mode in modes:
            kw = dict(mode=mode, light=(0.2, -0.1, 0.05), light_in_camera=int(mode != VT.COLOR_LIT), background=(9, 8, 7), vmap=True,
                      nmap=True, **cam)
            if pose is not None:
                kw["pose"] = pose
            a = trk.render_view(**kw)
            b = trk.render_section(**kw)
            what = f"{n}^3 {cam['width']}x{cam['height']} mode {mode} {'follow' if pose is None else 'free'}"
            assert a["n_hit"] > 0.2 * cam["width"] * cam["height"], what
            assert (b["n_hit"], b["n_uncolored"], b["n_cut"]) == (a["n_hit"], a["n_uncolored"], 0), what
            for key in KEYS:
                assert same_bits_nan(a[key], b[key]), f"{what}: {key}"
            checked += 1
    assert checked == 4 * len(modes)
    trk.close()


# ---- 2. + 3. sections of a scanned room against the twin -----------------------------------------------------
def test_room_sections_against_twin_256(hsk):
    trk, tsdf, color = room_scan(hsk, 0, 256)
    cams, down, y_mid = room_cameras(hsk.synth_room_extents(0))
    seen = {}
    for name, (fields, need) in cams.items():
        sec, ref, got = twin_and_gpu(trk, tsdf, color, fields)
        sh = shares(ref)
        seen[name] = ref
        print(f"256^3 {name}: twin hit {sh[0]:.4f} cut {sh[1]:.4f} background {sh[2]:.4f}")
        if need is not None:   # the condition on the twin's own image, before anything is compared
            assert all(s >= m for s, m in zip(sh, need)), f"{name}: shares {sh} below {need}"
        else:
            assert ref["n_hit"] > 0, name
        assert_section(got, ref, name)
    # what the planes are for: the same camera without one sees less
    assert seen["no clip"]["n_hit"] < seen["top-down 1/2"]["n_hit"]
    assert seen["no clip"]["n_cut"] == 0
    # the parallel plane kills rays on one side and leaves the others: both kinds are in the image, the two sides are complementary
    for name in ("parallel plane", "parallel plane, other side"):
        sec = ST.section(**cams[name][0])
        o, d = ST.rays(sec)
        tb, te = ST.box(o, d, SIZE)
        _, _, alive = ST.clip_rays(o, d, tb, te, sec["clip"])
        a, b, c, e = sec["clip"][0]
        assert (((a * d[0] + b * d[1]) + c * d[2]) == 0).all(), "the plane must contain the rays' direction exactly"
        assert 0.2 < alive.mean() < 0.8, (name, alive.mean())
        assert seen[name]["n_cut"] > 0 and (seen[name]["cls"][~alive] == ST.BACKGROUND).all()
    assert seen["camera inside"]["n_cut"] == 0 and seen["camera inside, plane behind"]["n_cut"] == 0
    assert np.array_equal(seen["camera inside"]["rgb"], seen["camera inside, plane behind"]["rgb"])
    # the axis-aligned pose takes step 1's 1e-15 path on two axes
    _, d = ST.rays(ST.section(**cams["top-down 1/2"][0]))
    assert (d[0] == f32(1e-15)).all() and (d[2] == f32(1e-15)).all() and (d[1] == 1).all()
    # sizes: ragged, one pixel, a strip of ragged tiles
    base = cams["top-down 1/2"][0]
    for w, h in ((333, 217), (1, 1), (4096, 3)):
        fields = dict(base, **{k: v for k, v in ortho_cam(down, width=w, height=h).items() if k != "pose"})
        if (w, h) == (4096, 3):
            fields.update(fx=4096 / SPAN, cx=2047.5)   # the strip spans the room in x at 1280 px/m
        sec, ref, got = twin_and_gpu(trk, tsdf, color, fields)
        if w > 1:
            assert ref["n_hit"] > 0 and ref["n_cut"] > 0, (w, h, shares(ref))
        assert_section(got, ref, f"top-down 1/2 at {w}x{h}")
    # NULL outputs: the counts alone
    from housescan_amd import _lib
    s = ST.to_struct(ST.section(**base), _lib)
    only = trk.render_section(s, rgb=False, depth=False)
    assert (only["n_hit"], only["n_cut"], only["n_uncolored"]) == tuple(seen["top-down 1/2"][k] for k in ("n_hit", "n_cut", "n_uncolored"))


def test_room_sections_against_twin_512(hsk):
    trk = scan_room(hsk, 0, 512)
    tsdf, color = trk.download_tsdf(), trk.download_color()
    cams, _, _ = room_cameras(hsk.synth_room_extents(0))
    for name in ("top-down 1/2", "dollhouse"):
        fields, need = cams[name]
        sec, ref, got = twin_and_gpu(trk, tsdf, color, fields)
        sh = shares(ref)
        print(f"512^3 {name}: twin hit {sh[0]:.4f} cut {sh[1]:.4f} background {sh[2]:.4f}")
        assert all(s >= m for s, m in zip(sh, need)), f"{name}: shares {sh} below {need}"
        assert_section(got, ref, f"512^3 {name}")
    trk.close()


def layered_volume(n=64):
    """written in numpy: along z a positive space, a wall of negative voxels (20..22), and behind it -- for x in the lower half
    only -- four layers of exact zeros, then positive space again and a second surface at voxel 40.  A ray that starts on a
    plane inside the first wall is CUT; where the zeros lie, its march leaves the wall without a back-face abort (no sample
    pair is negative then positive) and goes on to HIT the second surface: cut must win"""
    cell = 3.0 / n
    tau = max(TRUNC, 2.1 * cell)
    zc = (np.arange(n) + 0.5) * cell
    prof = np.clip((40.3 * cell - zc) / tau, -1.0, 1.0)
    prof[20:23] = -0.8
    vol = np.empty((n, n, n, 2), np.int16)
    vol[..., 0] = np.rint(prof * 32767).astype(np.int16)[:, None, None]
    vol[23:27, :, : n // 2, 0] = 0
    vol[..., 1] = 1
    return vol


def test_empty_plane_and_layered_volumes(hsk):
    n = 64
    cell = 3.0 / n
    trk = hsk.KinfuTracker(n=n)
    trk.enable_color()
    color = trk.download_color()
    pose = np.eye(4, dtype=f32)
    pose[:3, 3] = (1.5, 1.5, -0.5)
    cam = ortho_cam(pose, side=128, span=4.0)
    # an empty volume: background everywhere, whatever the planes
    sec, ref, got = twin_and_gpu(trk, trk.download_tsdf(), color, dict(cam, clip=[(0, 0, 1, -1.0)], background=(7, 8, 9)))
    assert_section(got, ref, "empty")
    assert got["n_hit"] == got["n_cut"] == 0 and (got["rgb"] == (7, 8, 9)).all() and not got["depth"].any()
    # the wall of view_twin.plane_volume: faced, cut inside its negative band, and seen by a pinhole camera
    vol = VT.plane_volume(n, 3.3)
    trk.upload_tsdf(vol)
    color[...] = (200, 100, 50, 3)
    color[::3, :, :, 3] = 0
    trk.upload_color(color)
    wall_z = 3.0 - 3.3 * cell
    for what, extra in (("wall", dict(mode=VT.COLOR_LIT, light=(0, 0, -1), light_in_camera=False, light_directional=True)),
                        ("wall cut", dict(clip=[(0, 0, 1, -(wall_z + cell))], cut_rgb=(9, 8, 7))),
                        ("wall beyond a far plane", dict(clip=[(0, 0, -1, wall_z - 2 * cell)])),
                        ("wall, pinhole", dict(SENSOR, pose=hsk.synth_pose(0), projection=ST.PINHOLE, mode=VT.COLOR,
                                               clip=[(0, 0, 1, -0.5), (0, 1, 0, -1.0)]))):
        sec, ref, got = twin_and_gpu(trk, vol, color, dict(cam, **extra))
        print(f"{what}: twin shares {shares(ref)}")
        assert_section(got, ref, what)
    sec, ref, got = twin_and_gpu(trk, vol, color, dict(cam, clip=[(0, 0, 1, -(wall_z + cell))]))
    assert ref["n_cut"] > 0.3 * 128 * 128 and ref["n_hit"] == 0
    # cut pixels that are march hits too
    vol = layered_volume(n)
    trk.upload_tsdf(vol)
    sec, ref, got = twin_and_gpu(trk, vol, color, dict(cam, clip=[(0, 0, 1, -21.5 * cell)], mode=VT.LAMBERT))
    both = ref["raw_hit"] & (ref["cls"] == ST.CUT)
    assert both.sum() > 1000, f"the twin must hold cut pixels whose march hit: {both.sum()}"
    assert ((ref["cls"] == ST.CUT) & ~ref["raw_hit"]).sum() > 1000
    assert_section(got, ref, "layered volume")
    assert (got["rgb"][both] == (255, 96, 0)).all() and np.isnan(got["vmap"][0][both]).all()
    trk.close()


# ---- 4. the tracker does not notice ------------------------------------------------------------------------
def run_stream(hsk, n, frames, with_sections, use_graph):
    trk = hsk.KinfuTracker(n=n, use_graph=use_graph)
    pose = ST.look((1.5, -0.5, 1.5), (1.5, 0.5, 1.5), (0, 0, 1))
    out = []
    for i, d in enumerate(frames):
        trk.submit_frame(d)
        if with_sections:   # between submit and wait of EVERY frame: alternately a floor plan and a clipped `follow` pinhole view
            if i % 2:
                r = trk.render_section(clip=[(0, 0, -1, 2.0)], mode=VT.NORMALS, vmap=True, nmap=True)
            else:
                r = trk.render_section(pose=pose, projection=ST.ORTHO, width=512, height=512, fx=160.0, fy=160.0, cx=255.5, cy=255.5,
                                       clip=[(0, 1, 0, -1.0)], mode=VT.LAMBERT, light=(0, -1, 0), light_in_camera=0, light_directional=1,
                                       vmap=True, nmap=True)
            assert r["rgb"].shape[2] == 3
            if i >= 3:
                assert r["n_hit"] + r["n_cut"] > 0
        if i >= 1:
            out.append(trk.wait_frame())
    out.append(trk.wait_frame())
    return trk, out


@pytest.mark.parametrize("use_graph", [0, 2])
def test_tracker_does_not_notice_sections(hsk, use_graph):
    """two contexts run the same 30 pipelined frames at 512^3; one renders a section between submit and wait of every frame.
    Poses, verdicts, TSDF and all levels of the model maps are bit-equal"""
    frames = [d for d, _ in frames_of(hsk, "synth", 30)[0]]
    a, ra = run_stream(hsk, 512, frames, True, use_graph)
    b, rb = run_stream(hsk, 512, frames, False, use_graph)
    assert all(ok for _, ok in ra[1:])
    assert_trackers_equal(a, ra, b, rb, False)
    a.close()
    b.close()


# ---- 5. errors ---------------------------------------------------------------------------------------------
def test_section_errors_leave_the_context_usable(hsk):
    from housescan_amd import _lib
    lib = _lib.load()
    n = 64
    trk, last = scan(hsk, (n, n, n), "synth", 4, color=False)
    tsdf = trk.download_tsdf()
    fields = dict(ortho_cam(ST.look((1.5, -0.5, 1.5), (1.5, 0.5, 1.5), (0, 0, 1)), side=96, span=3.2), clip=[(0, 1, 0, -1.4)])

    def good():
        sec, ref, got = twin_and_gpu(trk, tsdf, None, fields)
        assert ref["n_hit"] > 0
        assert_section(got, ref, "after an error")

    def code(view=None, **kw):
        s = trk.default_section()
        for key, val in (view or {}).items():
            setattr(s.view, key, val)
        for key, val in kw.items():
            if key == "planes":
                for c, pl in enumerate(val):
                    s.clip[c][:] = pl
            else:
                setattr(s, key, val)
        rc = lib.hsk_render_section(trk.h, C.byref(s), None, None, None, None, None, None, None)
        if rc != 0:
            assert lib.hsk_last_error(trk.h), "hsk_last_error must be set"
        return rc
    good()
    assert code() == 0
    for bad in (dict(mode=VT.COLOR), dict(mode=VT.COLOR_LIT)):
        assert code(view=bad) == -3
        assert b"colour" in lib.hsk_last_error(trk.h)
        good()
    for bad in (dict(width=0), dict(height=0), dict(width=4097), dict(height=4097), dict(mode=4), dict(mode=-1), dict(fx=0.0),
                dict(fy=-1.0), dict(fx=float("nan")), dict(fy=float("inf"))):
        assert code(view=bad) == -1, bad
        good()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(projection=2), dict(projection=-1), dict(n_clip=-1), dict(n_clip=5),
                dict(n_clip=1, planes=[(0, 0, 0, 1)]), dict(n_clip=1, planes=[(nan, 0, 1, 0)]), dict(n_clip=1, planes=[(0, 1, 0, inf)]),
                dict(n_clip=2, planes=[(0, 1, 0, -1), (0, -inf, 0, 0)]), dict(n_clip=4, planes=[(0, 1, 0, -1)] * 3 + [(0, 0, 0, 0)])):
        assert code(**bad) == -1, bad
        good()
    # planes beyond n_clip are not looked at
    assert code(n_clip=1, planes=[(0, 1, 0, -1), (nan, nan, nan, nan)]) == 0
    assert lib.hsk_render_section(trk.h, None, None, None, None, None, None, None, None) == -1
    with pytest.raises(hsk.KinfuError):
        trk.render_section(clip=[(0, 1, 0, 0)] * 5)
    good()
    trk.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
    for i in range(g.n_slabs()):
        with pytest.raises(hsk.KinfuError, match="slab"):
            g.slab(i).render_section()
    pose, ok = g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))
    assert ok
    g.close()


# ---- 6. the house ------------------------------------------------------------------------------------------
def quarter_turn_beside(ext0, ext1):
    """room 1 -> house: a quarter turn about y, then the translation that puts room 1's box against room 0's x1 wall, floors
    level, centred on room 0 in z (room 0 -> house is the identity plus a small translation)"""
    R = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)
    x0, x1, y0, y1, z0, z1 = (float(v) for v in ext1)
    corners = np.array([[x, y, z] for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)]) @ R.T
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    e0 = [float(v) for v in ext0]
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = (e0[1] - lo[0], e0[3] - hi[1], 0.5 * (e0[4] + e0[5]) - 0.5 * (lo[2] + hi[2]))
    return M.astype(f32)


def test_house_floor_plan_of_two_rooms(hsk):
    from housescan_amd import _lib, products
    rooms = [room_scan(hsk, 0, 256), room_scan(hsk, 1, 256)]
    ext0, ext1 = hsk.synth_room_extents(0), hsk.synth_room_extents(1)
    M0 = np.eye(4, dtype=f32)
    M0[:3, 3] = (0.25, 0.0, -0.5)
    M1 = (M0.astype(np.float64) @ quarter_turn_beside(ext0, ext1).astype(np.float64)).astype(f32)
    M1[:3, :3] = np.rint(M1[:3, :3])   # (an exact quarter turn)
    xfs = [M0, M1]
    # the house section: top-down over both rooms, cut at room 0's mid height (house y = room 0's y).  The image is fitted to the house:
    # the two boxes reach 2.5 m to either side of the shared wall and 1.3 m to either side of zc, so 5.6 m x 3.2 m at 50 px/m holds
    # them with 0.3 m to spare all round
    x_wall = float(ext0[1]) + 0.25
    zc = 0.5 * float(ext0[4] + ext0[5]) - 0.5
    y_mid = 0.5 * float(ext0[2] + ext0[3])
    pose = ST.look((x_wall, -0.5, zc), (x_wall, 0.5, zc), (0, 0, 1))
    W_, H_ = 280, 160
    house = ST.section(W_, H_, 50.0, 50.0, (W_ - 1) / 2.0, (H_ - 1) / 2.0, pose, ST.ORTHO, [(0, 1, 0, -y_mid)], VT.COLOR_LIT,
                       (0.2, -1.0, 0.3), False, True, (0, 0, 0), (255, 96, 0))
    hs = ST.to_struct(house, _lib)
    gpu, twin = [], []
    for (trk, tsdf, color), M in zip(rooms, xfs):
        rs = products.section_in_room(hs, M)
        rt = ST.in_room(house, M)
        assert same_bits_nan(ST.from_struct(rs)["pose"], rt["pose"]) and same_bits_nan(np.array(ST.from_struct(rs)["clip"], f32), np.array(rt["clip"], f32))
        got = trk.render_section(rs, vmap=True, nmap=True)
        ref = ST.render(tsdf, SIZE, TRUNC, rt, color=color)
        sh = shares(ref)
        print(f"house: room in its frame: twin hit {sh[0]:.4f} cut {sh[1]:.4f} background {sh[2]:.4f}")
        # (the smaller room's box is 2.5 m x 2.2 m of the 5.6 m x 3.2 m image, 31 % of it, and the floor plan of one room shows
        # under half of its box as hits -- 27.9 % of a 3.2 m square over a 2.5 m x 2.6 m room is 44 %: 13 % expected, a quarter
        # of that required; an outline of 100 pixels is 2 m of wall at 50 px/m)
        assert sh[0] >= 0.03 and ref["n_cut"] > 100, (sh, ref["n_cut"])
        assert_section(got, ref, "a room of the house")
        gpu.append(got)
        twin.append(ref)
    rgb, dep, idx = products.composite_views([g["rgb"] for g in gpu], [g["depth"] for g in gpu], (0, 0, 0))
    t_rgb, t_dep, t_idx = ST.composite([t["rgb"] for t in twin], [t["depth"] for t in twin], (0, 0, 0))
    assert np.array_equal(rgb, t_rgb) and np.array_equal(dep, t_dep) and np.array_equal(idx, t_idx)
    # house x of a pixel column: the camera's x axis is -x (look(): up x z)
    u = np.arange(W_)
    house_x = x_wall - (u - (W_ - 1) / 2.0) / 50.0
    margin = 0.03 + 1.5 * 3.0 / 256 + 1 / 50.0      # tau + 1.5 cells + a pixel round the shared wall
    left, right = house_x < x_wall - margin, house_x > x_wall + margin
    # each side of the wall is 2.7 m x 3.2 m of image; the smaller room's box covers 63 % of its side, and 44 % + the outline of
    # a box are shown (above): 0.3 expected on the emptier side, two thirds of it required
    assert (idx[:, left] >= 0).mean() > 0.2 and (idx[:, right] >= 0).mean() > 0.2, ((idx[:, left] >= 0).mean(), (idx[:, right] >= 0).mean())
    assert (idx[:, left][idx[:, left] >= 0] == 0).all(), "room 0's side must show room 0 only"
    assert (idx[:, right][idx[:, right] >= 0] == 1).all(), "room 1's side must show room 1 only"
    # a cut pixel of any room stays a cut pixel of the house: no floor overwrites a wall outline
    any_cut = (twin[0]["cls"] == ST.CUT) | (twin[1]["cls"] == ST.CUT)
    assert any_cut.sum() > 200
    assert (rgb[any_cut] == (255, 96, 0)).all()
    win_cls = np.where(idx == 1, twin[1]["cls"], twin[0]["cls"])
    assert (win_cls[any_cut] == ST.CUT).all()
    band = np.abs(house_x - x_wall) <= margin
    assert any_cut[:, band].sum() > 20, "the shared wall must be outlined"


# ---- 7. physical -------------------------------------------------------------------------------------------
def test_room_floor_plan_physical(hsk):
    """room 0 from above, cut at mid height, 256^3: the hits' median height is the floor's within 1.5 cells (DESIGN.md 4 item
    4's tolerance), and each of the four wall strips -- the pixels within tau + 1.5 cells + 1 pixel of the wall's plane -- holds
    cut pixels.  The outlined share of each wall's length is printed, not asserted: it depends on what the scripted scan saw"""
    trk, _, _ = room_scan(hsk, 0, 256)
    ext = hsk.synth_room_extents(0)
    x0, x1, y0, y1, z0, z1 = (float(v) for v in ext)
    cams, down, y_mid = room_cameras(ext)
    from housescan_amd import _lib
    r = trk.render_section(ST.to_struct(ST.section(**cams["top-down 1/2"][0]), _lib), vmap=True)
    cell = 3.0 / 256
    hit = ~np.isnan(r["vmap"][0])
    assert r["n_hit"] == hit.sum() > 0.05 * SIDE * SIDE
    cut = (r["rgb"] == (255, 96, 0)).all(axis=2) & ~hit & (r["depth"] > 0)
    assert cut.sum() == r["n_cut"] > 0.01 * SIDE * SIDE
    height = r["vmap"][1][hit].astype(np.float64)
    print(f"floor plan of room 0: hits {hit.sum()}, cut {cut.sum()}, median height {np.median(height):.5f} m (floor {y1} m)")
    assert abs(np.median(height) - y1) <= 1.5 * cell
    # the height map agrees: depth is the distance from the camera's plane at y = -0.5
    assert abs(np.median(r["depth"][hit]) / 1000.0 - 0.5 - y1) <= 1.5 * cell + 0.001
    # the plane's own depth on every cut pixel
    assert np.abs(r["depth"][cut].astype(np.float64) - (y_mid + 0.5) * 1000).max() <= 1.0
    ppm = SIDE / SPAN
    c = (SIDE - 1) / 2.0
    cxw, czw = 0.5 * (x0 + x1), 0.5 * (z0 + z1)
    wx = cxw - (np.arange(SIDE)[None, :] - c) / ppm + np.zeros((SIDE, 1))      # the camera's x axis is -x, its y axis +z
    wz = czw + (np.arange(SIDE)[:, None] - c) / ppm + np.zeros((1, SIDE))
    strip = 0.03 + 1.5 * cell + 1.0 / ppm
    for name, coord, plane, along, lo, hi in (("x0", wx, x0, wz, z0, z1), ("x1", wx, x1, wz, z0, z1), ("z0", wz, z0, wx, x0, x1),
                                              ("z1", wz, z1, wx, x0, x1)):
        m = (np.abs(coord - plane) <= strip) & (along >= lo) & (along <= hi)
        n_cut = (cut & m).sum()
        axis = 0 if name[0] == "z" else 1
        outlined = (cut & m).any(axis=axis)[m.any(axis=axis)].mean()
        print(f"wall {name}: {n_cut} cut pixels in its strip, {outlined:.2f} of its length outlined")
        assert n_cut > 0, f"wall {name} has no outline"
