"""hsk_render_view on the GPU: every image bit-exact against the CPU oracle's raycast for the view's camera plus the numpy
restatement of the shading rule (tests/view_twin.py), on volumes the tracker itself made; the same geometry as the stage
call; a tracker that does not notice views rendered between its pipelined frames; `follow`; the errors; and what a
scanned room's colour view looks like."""
import ctypes as C

import numpy as np
import pytest

import view_twin as VT
from kit import same_bits_nan
from view_cases import RAGGED, SENSOR, assert_trackers_equal, frames_of, moved, rot_y, scan
from view_shape_cases import MODES, assert_view, check_camera

pytestmark = pytest.mark.gpu
f32 = np.float32
WIDE = dict(width=800, height=600, fx=400.0, fy=400.0, cx=399.5, cy=299.5)
FULLHD = dict(width=1920, height=1080, fx=1000.0, fy=1000.0, cx=959.5, cy=539.5)
FREE = dict(width=1280, height=960, fx=1050.0, fy=1050.0, cx=639.5, cy=479.5)
ONE = dict(width=1, height=1, fx=525.0, fy=525.0, cx=0.0, cy=0.0)


def reference(oracle, dims, tsdf, color, cam, pose, mode, light, light_in_camera, background):
    cfg = VT.view_config(oracle, dims, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    vm, nm = VT.geometry(oracle, cfg, tsdf, pose)
    return vm, nm, VT.shade(vm, nm, pose, mode, light, light_in_camera, background, color=color)


def turned_away(pose):
    """outside the volume, looking away from it"""
    p = np.asarray(pose, f32).copy()
    p[:3, :3] = (p[:3, :3].astype(np.float64) @ rot_y(180.0)[:3, :3].astype(np.float64)).astype(f32)
    p[:3, 3] = (1.5, 1.5, -0.5)
    return p


CASES = {
    "synth64": ((64, 64, 64), "synth", 12), "synth128": ((128, 128, 128), "synth", 12), "synth256": ((256, 256, 256), "synth", 12),
    "synth512": ((512, 512, 512), "synth", 12), "room256": ((256, 256, 256), "room", 40), "ragged": ((64, 160, 96), "synth", 12),
}


@pytest.mark.parametrize("case", list(CASES))
def test_bitexact_scanned(hsk, oracle, case):
    """volumes the tracker made, downloaded; cameras: the sensor's, a wider one at another size, a ragged size, 1 x 1, full HD
    (256^3), from the last pose and from a pose the stream never visited, and one that looks away from the volume"""
    dims, src, count = CASES[case]
    trk, last = scan(hsk, dims, src, count)
    tsdf, color = trk.download_tsdf(), trk.download_color()
    if src == "synth":
        away = moved(hsk.synth_pose(6))
    else:
        away = (np.asarray(last, np.float64) @ rot_y(15.0).astype(np.float64)).astype(f32)
    args = (trk, oracle, dims, tsdf, color)
    # (the scripted stream's last pose sees almost nothing but surface at fine cells -- 0.2 % background at 512^3 -- so the
    # sensor's camera is also placed 0.1 m beside it, where the condition on the reference holds: 89-94 % hits at 64^3-512^3)
    check_camera(*args, SENSOR, last, f"{case} sensor, last pose", degenerate=src == "synth")
    if src == "synth":
        check_camera(*args, SENSOR, moved(last, 0.0, 0.1), f"{case} sensor, beside the last pose")
    check_camera(*args, WIDE, last, f"{case} 800x600, last pose")
    check_camera(*args, RAGGED, away, f"{case} 333x217, moved pose")
    check_camera(*args, SENSOR, away, f"{case} sensor, moved pose", modes=(VT.LAMBERT, VT.COLOR_LIT))
    check_camera(*args, ONE, last, f"{case} 1x1", degenerate=True)
    if case in ("synth256", "room256"):
        check_camera(*args, FULLHD, last if case == "synth256" else away, f"{case} 1920x1080", modes=(VT.COLOR_LIT, VT.NORMALS))
    hit = check_camera(*args, SENSOR, turned_away(last), f"{case} looking away", degenerate=True, modes=(VT.LAMBERT,))
    assert not hit.any()
    # the tracker's own state is where the scan left it
    assert np.array_equal(trk.get_pose().view(np.uint32), np.asarray(last).view(np.uint32))
    assert np.array_equal(trk.download_tsdf(), tsdf)
    trk.close()


def test_bitexact_empty_and_plane(hsk, oracle):
    """an empty volume (background everywhere, also in `follow`), and a volume written in numpy whose hits partly have no
    normal (view_twin.plane_volume: LAMBERT gives those the ambient 50, NORMALS the background)"""
    n = 64
    trk = hsk.KinfuTracker(n=n)
    trk.enable_color()
    pose = hsk.synth_pose(0)
    dims = (n, n, n)
    tsdf, color = trk.download_tsdf(), trk.download_color()
    hit = check_camera(trk, oracle, dims, tsdf, color, SENSOR, pose, "empty", degenerate=True)
    assert not hit.any()
    got = trk.render_view(background=(7, 8, 9))
    assert got["n_hit"] == 0 and (got["rgb"] == (7, 8, 9)).all() and not got["depth"].any()
    vol = VT.plane_volume(n, 3.5)
    trk.upload_tsdf(vol)
    color[...] = (200, 100, 50, 3)
    color[::3, :, :, 3] = 0
    trk.upload_color(color)
    cfg = VT.view_config(oracle, dims, 640, 480, 525.0, 525.0, 319.5, 239.5)
    vm, nm = VT.geometry(oracle, cfg, vol, pose)
    bare = ~np.isnan(vm[0]) & np.isnan(nm[0])
    assert bare.sum() > 1000, "the reference must have hits without a normal"
    hit = check_camera(trk, oracle, dims, vol, color, SENSOR, pose, "plane volume", degenerate=True)
    assert hit.mean() > 0.2
    check_camera(trk, oracle, dims, vol, color, RAGGED, pose, "plane volume 333x217", degenerate=True)
    lam = trk.render_view(pose=pose, mode=VT.LAMBERT)
    assert (lam["rgb"][bare] == 50).all()
    trk.close()


@pytest.mark.parametrize("n,frames", [(256, 8), (512, 8), (1024, 3)])
def test_same_geometry_as_stage_raycast(hsk, n, frames):
    """the sensor's camera and an explicit pose: vmap / nmap equal hsk_raycast's bit for bit (1024^3: the 16 x 4 tile form)"""
    trk, last = scan(hsk, (n, n, n), "synth", frames, color=False)
    for pose in (last, moved(hsk.synth_pose(2), 8.0, 0.1)):
        got = trk.render_view(pose=pose, vmap=True, nmap=True)
        assert got["n_hit"] > 0.2 * 640 * 480
        v, nm = trk.raycast(pose)   # (overwrites the tracker's pose and model maps: the stage call)
        assert same_bits_nan(got["vmap"], v) and same_bits_nan(got["nmap"], nm)
        assert got["n_hit"] == (~np.isnan(v[0])).sum()
    trk.close()


def run_pair(hsk, n, frames, with_views, use_graph=0, color=False, resubmit_after_loss=False):
    """the frames through a pipelined tracker; with_views: a view after every third submission, frames in flight, alternately
    `follow` and a free 1280 x 960 camera, every output asked for"""
    trk = hsk.KinfuTracker(n=n, use_graph=use_graph)
    if color:
        trk.enable_color()
    free_pose = moved(hsk.synth_pose(3), 10.0, 0.2)
    out, views = [], 0
    for i, (d, c) in enumerate(frames):
        trk.submit_frame_rgbd(d, c) if color else trk.submit_frame(d)
        if with_views and i % 3 == 2:
            mode = (VT.COLOR_LIT if color else VT.LAMBERT) if views % 2 else VT.NORMALS
            if views % 2:
                r = trk.render_view(pose=free_pose, mode=mode, vmap=True, nmap=True, **FREE)
            else:
                r = trk.render_view(mode=mode, vmap=True, nmap=True)
            assert r["rgb"].shape[2] == 3
            views += 1
        if i >= 2:
            out.append(trk.wait_frame())
    while len(out) < len(frames):
        out.append(trk.wait_frame())
    return trk, out


@pytest.mark.parametrize("use_graph,color", [(0, False), (2, False), (0, True)])
def test_tracker_does_not_notice(hsk, use_graph, color):
    """two contexts run the same 30 pipelined frames at 512^3; one renders views in between.  Poses, verdicts, TSDF, colour
    volume and all levels of the model maps are bit-equal"""
    frames, _ = frames_of(hsk, "synth", 30)
    a, ra = run_pair(hsk, 512, frames, True, use_graph, color)
    b, rb = run_pair(hsk, 512, frames, False, use_graph, color)
    assert all(ok for _, ok in ra[1:])
    assert_trackers_equal(a, ra, b, rb, color)
    a.close()
    b.close()


def test_tracker_does_not_notice_fuzz(hsk, synth_frames):
    """the same on a stream with garbage and empty frames (test_tracker_fuzz_vs_oracle's, seed 1: lost frames, resets)"""
    from parity_cases import _random_depth
    rng = np.random.default_rng(2001)
    frames, k = [], 0
    for i in range(14):
        r = rng.random()
        if i >= 2 and r < 0.2:
            frames.append(_random_depth(rng))
        elif i >= 2 and r < 0.3:
            frames.append(np.zeros((480, 640), np.uint16))
        elif i >= 2 and r < 0.4:
            k += int(rng.integers(5, 30))
            frames.append(synth_frames(k)[1])
        else:
            frames.append(synth_frames(k)[1])
            k += 1

    def run(with_views):
        trk = hsk.KinfuTracker(n=96)
        out = []
        for i, d in enumerate(frames):
            trk.submit_frame(d)
            if with_views:
                trk.render_view(mode=VT.LAMBERT if i % 2 else VT.NORMALS, vmap=True, nmap=True, **(FREE if i % 3 == 0 else SENSOR))
            out.append(trk.wait_frame())
        return trk, out
    a, ra = run(True)
    b, rb = run(False)
    assert sum(not ok for _, ok in ra[1:]) >= 2, "the stream must lose frames"
    assert_trackers_equal(a, ra, b, rb, False)
    a.close()
    b.close()


def test_follow_is_the_pose_the_host_would_get(hsk):
    trk, last = scan(hsk, (256, 256, 256), "synth", 10)
    trk.synchronize()
    pose = trk.get_pose()
    assert np.array_equal(pose.view(np.uint32), np.asarray(last).view(np.uint32))
    for mode in MODES:
        a = trk.render_view(mode=mode, vmap=True, nmap=True, light=(0.2, 0.1, 0.0))
        b = trk.render_view(pose=pose, mode=mode, vmap=True, nmap=True, light=(0.2, 0.1, 0.0))
        assert a["n_hit"] == b["n_hit"] > 0.5 * 640 * 480 and a["n_uncolored"] == b["n_uncolored"]
        for key in ("rgb", "depth", "vmap", "nmap"):
            assert same_bits_nan(a[key], b[key]), (mode, key)
    # after a tracking loss: the pose hsk_get_pose returns, over the reset volume
    _, ok = trk.process_frame(np.zeros((480, 640), np.uint16))
    assert not ok
    r = trk.render_view(background=(1, 2, 3))
    assert r["n_hit"] == 0 and (r["rgb"] == (1, 2, 3)).all()
    trk.close()


def test_mid_stream_order(hsk, oracle):
    """a `follow` view requested right behind submit_frame of frame k, not yet waited for, is the twin's view of the oracle
    tracker's volume and pose after frame k"""
    n = 128
    ot = oracle.Tracker(oracle.default_config(n), omp=True)
    trk = hsk.KinfuTracker(n=n)
    cfg = VT.view_config(oracle, (n, n, n), 640, 480, 525.0, 525.0, 319.5, 239.5)
    checked = 0
    for k in range(9):
        d = hsk.synth_depth(hsk.synth_pose(k))
        po, _ = ot.process(d)
        trk.submit_frame(d)
        if k in (0, 1, 4, 8):
            got = trk.render_view(mode=VT.LAMBERT, vmap=True, nmap=True, background=(0, 0, 64))
            vm, nm = VT.geometry(oracle, cfg, ot.volume().copy(), po)
            ref = VT.shade(vm, nm, po, VT.LAMBERT, (0, 0, 0), True, (0, 0, 64))
            assert ref["n_hit"] > 0.5 * 640 * 480
            assert_view(got, vm, nm, ref, f"behind frame {k}")
            checked += 1
        ph, _ = trk.wait_frame()
        assert np.array_equal(ph.view(np.uint32), po.view(np.uint32))
    assert checked == 4
    trk.close()


def test_errors_leave_the_context_usable(hsk, oracle):
    from housescan_amd import _lib
    lib = _lib.load()
    n = 64
    trk, last = scan(hsk, (n, n, n), "synth", 4, color=False)
    tsdf = trk.download_tsdf()

    def good():
        vm, nm, ref = reference(oracle, (n, n, n), tsdf, None, SENSOR, last, VT.LAMBERT, (0, 0, 0), True, (0, 0, 0))
        assert_view(trk.render_view(pose=last, vmap=True, nmap=True), vm, nm, ref, "after an error")

    def code(**kw):
        v = trk.default_view()
        for key, val in kw.items():
            setattr(v, key, val)
        rc = lib.hsk_render_view(trk.h, C.byref(v), None, None, None, None, None, None)
        if rc != 0:
            assert lib.hsk_last_error(trk.h), "hsk_last_error must be set"
        return rc
    assert code() == 0
    for bad in (dict(mode=VT.COLOR), dict(mode=VT.COLOR_LIT)):
        assert code(**bad) == -3
        assert b"colour" in lib.hsk_last_error(trk.h)
        good()
    for bad in (dict(width=0), dict(height=0), dict(width=4097), dict(height=4097), dict(mode=4), dict(mode=-1), dict(fx=0.0),
                dict(fy=-1.0), dict(fx=float("nan")), dict(fy=float("inf"))):
        assert code(**bad) == -1, bad
        good()
    assert lib.hsk_render_view(trk.h, None, None, None, None, None, None, None) == -1
    with pytest.raises(hsk.KinfuError):
        trk.render_view(width=4097)
    good()
    trk.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
    for i in range(g.n_slabs()):
        with pytest.raises(hsk.KinfuError, match="slab"):
            g.slab(i).render_view()
    pose, ok = g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))
    assert ok
    g.close()


def test_sizes_up_to_4096(hsk, oracle):
    """4096 x 4096 is one launch; a tall 3 x 4096 strip has ragged tiles in x on every row"""
    n = 128
    trk, last = scan(hsk, (n, n, n), "synth", 6, color=False)
    big = trk.render_view(pose=last, width=4096, height=4096, fx=3400.0, fy=3400.0, cx=2047.5, cy=2047.5)
    assert big["rgb"].shape == (4096, 4096, 3) and big["n_hit"] == (big["depth"] > 0).sum() > 0.2 * 4096 * 4096
    tsdf = trk.download_tsdf()
    cam = dict(width=3, height=4096, fx=3400.0, fy=3400.0, cx=1.0, cy=2047.5)
    check_camera(trk, oracle, (n, n, n), tsdf, None, cam, last, "3x4096", degenerate=True, modes=(VT.LAMBERT,))
    trk.close()


def test_room_scan_colour_view_physical(hsk):
    """room 0 as a sensor sees it, RGB-D, 256^3, 150 frames (the scan of test_gpu_color.test_room_scan_physical): the COLOR
    view from the last pose -- per hit pixel with colour, the largest channel distance in levels between the rendered colour
    and the scene's colour at the vertex.  The bounds are the figures of the first run on the GPU plus 2 levels
    (profiles/r10/view_notes.md)."""
    n, scan_len, count = 256, 720, 150
    poses, frames = hsk.synth_sensor_frames(count, room=0, scan=scan_len)
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    trk.enable_color()
    trk.submit_frame_rgbd(frames[0], hsk.synth_rgb(poses[0], 0))
    tracked = []
    for k in range(1, count):
        trk.submit_frame_rgbd(frames[k], hsk.synth_rgb(poses[k], 0))
        tracked.append(trk.wait_frame()[1])
    tracked.append(trk.wait_frame()[1])
    assert all(tracked[1:]), "the room scan must stay tracked"
    r = trk.render_view(mode=VT.COLOR, vmap=True)
    P = 640 * 480
    assert r["n_hit"] > 0.5 * P and r["n_uncolored"] < 0.1 * r["n_hit"], (r["n_hit"], r["n_uncolored"])
    hit = ~np.isnan(r["vmap"][0])
    col = hit & (r["rgb"] != 0).any(axis=2)
    v = r["vmap"][:, col].T.astype(np.float64)
    want = np.rint(128.0 + 100.0 * np.sin(2.0 * np.pi * v / 1.2))
    err = np.abs(r["rgb"][col].astype(np.float64) - want).max(axis=1)
    med, p99, worst = np.median(err), np.percentile(err, 99), err.max()
    print(f"colour view, room 0, 256^3, 150 frames: hits {r['n_hit']} ({r['n_hit'] / P:.3f}), uncoloured {r['n_uncolored']}, "
          f"error median {med} p99 {p99} worst {worst}")
    assert med <= MEDIAN_BOUND and p99 <= P99_BOUND, (med, p99, worst)
    trk.close()


# measured on the first run (profiles/r10/view_notes.md) + 2 levels
MEDIAN_BOUND = 4    # first run: median 2, 99th percentile 7, worst 14 levels (285 269 hits, 1460 of them uncoloured)
P99_BOUND = 9
