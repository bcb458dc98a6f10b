"""The fusion tests' plane and general cases on the host, and the room scans the device tests share."""
import numpy as np
import pytest

import fuse_twin as FT
from section_cases import SCAN_FRAMES
from view_twin import plane_volume

f32 = np.float32


def general(n_cells_shift=0.37, size=3.0, n=32):
    """a general rotation about the volume's centre (no axis of it is a grid axis) with a sub-cell shift"""
    c = size / 2
    m = FT.rot_about("y", 25.0, (c, c, c)) @ FT.rot_about("x", -13.0, (c, c, c)) @ FT.rot_about("z", 8.0, (c, c, c))
    m = m.astype(np.float64)
    m[:3, 3] += n_cells_shift * size / n * np.array([1.0, -0.6, 0.3])
    return m.astype(f32)


PLANE_N, PLANE_TAU = 64, 0.3


def plane_case():
    """(source volume, source -> destination matrix, the moved plane as (unit normal, offset): n . p = d)"""
    src = plane_volume(PLANE_N, cells_in_front=3.5, size=3.0, trunc=PLANE_TAU)
    cell = 3.0 / PLANE_N
    m = FT.rot_about("y", 30.0, (1.5, 1.5, 1.5), (0.31 * cell, -0.23 * cell, 0.17 * cell))
    M = m.astype(np.float64)
    nrm = M[:3, :3] @ np.array([0.0, 0.0, 1.0])
    d = (3.0 - 3.5 * cell) + nrm @ M[:3, 3]
    return src, m, nrm, d


N = 128
SIZE = (3.0, 3.0, 3.0)
HOUSE_DIMS, HOUSE_SIZE = (256, 128, 128), (6.0, 3.0, 3.0)

SCAN_STEP = 3    # every third frame of the scripted three-turn scan: 240 frames per room

_SCANS = {}


def scan_room(hsk, variant, lo=0, hi=SCAN_FRAMES, step=SCAN_STEP):
    """a room's RGB-D scan at 128^3: depth and colour of the scripted trajectory's frames, fused at the script's own poses
    through the stage-level calls (at 47 mm of truncation the TRACKER loses this trajectory near frame 190; what is under test
    here is what happens to a scanned volume, not how its poses were found)"""
    trk = hsk.KinfuTracker(n=N, init_pose=hsk.synth_room_pose(variant, 0, SCAN_FRAMES))
    trk.enable_color()
    for at in range(lo, hi, 48 * step):
        ks = list(range(at, min(at + 48 * step, hi), step))
        for k, (d, c) in zip(ks, room_frames_at(hsk, variant, ks)):
            pose = hsk.synth_room_pose(variant, k, SCAN_FRAMES)
            trk.integrate(d, pose)
            trk.integrate_color(d, c, pose)
    return trk


def room_frames_at(hsk, variant, ks):
    from concurrent.futures import ThreadPoolExecutor
    poses = [hsk.synth_room_pose(variant, k, SCAN_FRAMES) for k in ks]
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda p: (hsk.synth_room_depth(variant, p), hsk.synth_rgb(p, variant)), poses))


def room_scan(hsk, variant):
    """(tracker, tsdf, colour volume) of a room's RGB-D scan at 128^3, made once per module"""
    if variant not in _SCANS:
        trk = scan_room(hsk, variant)
        _SCANS[variant] = (trk, trk.download_tsdf(), trk.download_color())
    return _SCANS[variant]


@pytest.fixture(scope="module", autouse=True)
def _close_scans():
    yield
    for trk, _, _ in _SCANS.values():
        trk.close()
    _SCANS.clear()


def make_ctx(hsk, dims=(N, N, N), size=SIZE, color=True, **over):
    cfg = hsk.default_config(dims[2], vol_x=dims[0], vol_y=dims[1], vol_z=dims[2], vol_size_m=size, **over)
    trk = hsk.KinfuTracker(cfg)
    if color:
        trk.enable_color()
    return trk
