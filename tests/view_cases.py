"""The view tests' sensor, scans and tracker comparison, shared with the section, fusion and pack tests."""
import numpy as np

from kit import same_bits_nan

f32 = np.float32
SENSOR = dict(width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5)
RAGGED = dict(width=333, height=217, fx=270.0, fy=270.0, cx=166.0, cy=108.0)


def rot_y(deg):
    a = np.radians(deg)
    m = np.eye(4, dtype=f32)
    m[0, 0] = m[2, 2] = np.cos(a)
    m[0, 2] = np.sin(a)
    m[2, 0] = -np.sin(a)
    return m


def moved(pose, deg=15.0, dx=0.3):
    """`pose` turned about the camera's own y axis, then shifted sideways in the world: a place the stream never visited"""
    p = (np.asarray(pose, np.float64) @ rot_y(deg).astype(np.float64)).astype(f32)
    p[0, 3] = f32(p[0, 3] + f32(dx))
    return p


def frames_of(hsk, src, count):
    """[(depth, rgb)] of the scripted stream ("synth") or of room 0's scan ("room"), and the first pose"""
    if src == "synth":
        poses = [hsk.synth_pose(k) for k in range(count)]
        return [(hsk.synth_depth(p), hsk.synth_rgb(p)) for p in poses], poses[0]
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(count)]
    return [(hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0)) for p in poses], poses[0]


def scan(hsk, dims, src, count, color=True, **over):
    """a tracker that has taken `count` RGB-D frames, pipelined; its last pose"""
    frames, first = frames_of(hsk, src, count)
    if src == "room":
        over["init_pose"] = first
    trk = hsk.KinfuTracker(n=dims[0], vol_x=dims[0], vol_y=dims[1], vol_z=dims[2], own_z1=dims[2], **over)
    if color:
        trk.enable_color()
    pose = None
    for i, (d, c) in enumerate(frames):
        trk.submit_frame_rgbd(d, c) if color else trk.submit_frame(d)
        if i >= 1:
            pose, ok = trk.wait_frame()
            assert ok or i == 1
    pose, ok = trk.wait_frame()
    assert ok
    return trk, pose


def assert_trackers_equal(a, ra, b, rb, color):
    for k, ((pa, oka), (pb, okb)) in enumerate(zip(ra, rb)):
        assert oka == okb, f"verdict of frame {k}"
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), f"pose of frame {k}"
    a.synchronize()
    b.synchronize()
    for level in range(3):
        for kind in (2, 3):
            assert same_bits_nan(a.download_map(kind, level), b.download_map(kind, level)), f"model map {kind} level {level}"
    assert np.array_equal(a.get_pose().view(np.uint32), b.get_pose().view(np.uint32))
    assert np.array_equal(a.download_tsdf(), b.download_tsdf()), "TSDF"
    if color:
        assert np.array_equal(a.download_color(), b.download_color()), "colour volume"
