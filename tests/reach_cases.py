"""The reach tests' corridors, serpentine, rooms and staircase, their constants, twin fields, path checker and host harness call."""
import os
import re

import numpy as np

import align_twin as AT
import clearance_twin as CL
import kit
import reach_twin as RE
from kit import ROOT

f32 = np.float32
FREE_WORD = (32767, 1)
SOLID_WORD = (-100, 1)
WEIGHTS = ((1, 1, 1), (16, 25, 44))
_CACHE = {}


def header_constant(name):
    src = open(os.path.join(ROOT, "housescan_amd", "csrc", "hsk_reach_point.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, src).group(1))


TILE = tuple(header_constant("REACH_TILE_" + a) for a in "XYZ")


def scene_size(dims):
    """the project's test scene's cells at every shape"""
    return (3.0 * dims[0] / 80, 3.0 * dims[1] / 64, 3.0 * dims[2] / 48)


def free_volume(dims):
    X, Y, Z = dims
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[...] = FREE_WORD
    return vol


def hand_params(weight):
    """the hand-built volumes' parameters: clearance flags 0, a cap that lets the field tell min_d2 = min(w) apart"""
    return dict(weight=tuple(weight), max_d2=4 * max(weight), flags=0), min(weight)


def hand_d2(vol, weight):
    cp, _ = hand_params(weight)
    return CL.field(vol, cp["weight"], cp["max_d2"], 0)


def centre(v, dims):
    """the world point at the centre of voxel v = (x, y, z)"""
    return tuple(float((v[i] + 0.5) * (f32(scene_size(dims)[i]) / f32(dims[i]))) for i in range(3))


def twin_reach(name, d2, weight, min_d2, max_cost, seeds):
    """the twin's field of a named clearance field, made once per (name, parameters) -> (G, n_seeds_used)"""
    key = (name, tuple(weight), int(min_d2), int(max_cost), tuple(seeds))
    if key not in _CACHE:
        _CACHE[key] = RE.field(d2, weight, min_d2, max_cost, seeds)
    return _CACHE[key]


SERPENTINE_DIMS = (3 * TILE[0], 3 * TILE[1], 20)          # three tiles on every axis, the last plane of tiles half empty


def serpentine():
    """walls one voxel thick across x, all z, with gaps alternating between the two ends of y: the shortest path to the far end
    crosses every tile row of y again and again"""
    X, Y, Z = SERPENTINE_DIMS
    vol = free_volume(SERPENTINE_DIMS)
    walls = list(range(10, X - 6, 14))
    for i, x in enumerate(walls):
        if i % 2 == 0:
            vol[:, : Y - 3, x] = SOLID_WORD
        else:
            vol[:, 3:, x] = SOLID_WORD
    return vol, walls


STAIR_DIMS = (40, 24, 12)


def staircase():
    """a wall x - y == 8, all z, one voxel thick: its solids touch only by edges, and only the box rule keeps a path from slipping
    between them"""
    vol = free_volume(STAIR_DIMS)
    for y in range(STAIR_DIMS[1]):
        vol[:, y, y + 8] = SOLID_WORD
    return vol


CORNER_DIMS = (2 * TILE[0], 2 * TILE[1], 2 * TILE[2])


def tile_corner():
    """two chambers in the diagonally opposite tiles (0, 0, 0) and (1, 1, 1) of a solid block, joined only by the free 2 x 2 x 2
    cube centred on the corner all eight tiles share"""
    X, Y, Z = CORNER_DIMS
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[...] = SOLID_WORD
    tx, ty, tz = TILE
    vol[1:tz, 1:ty, 2:tx] = FREE_WORD                                  # (up to the cube's voxel in its own tile)
    vol[tz:Z - 1, ty:Y - 1, tx:X - 2] = FREE_WORD
    vol[tz - 1:tz + 1, ty - 1:ty + 1, tx - 1:tx + 1] = FREE_WORD
    return vol


def corridors():
    """a solid block of 2 x 2 x 2 tiles with corridors ONE voxel wide: `face` runs along x in the row y = 0, z = 0 and crosses the
    tile face x = TILE_X; `corner` runs along x in the row (TILE_Y - 1, TILE_Z - 1), steps +x, +y, +z by face moves round the corner
    all eight tiles share, and runs on in the row (TILE_Y, TILE_Z).  -> (volume, {name: seed voxel}): seeds at local 0 and at local
    TILE - 1 of their tiles, next to the face and the corner: no in-tile neighbour of such a seed lies on the face it is seen through"""
    X, Y, Z = CORNER_DIMS
    tx, ty, tz = TILE
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[...] = SOLID_WORD
    vol[0, 0, :] = FREE_WORD
    vol[tz - 1, ty - 1, 2:tx + 1] = FREE_WORD
    vol[tz - 1, ty, tx] = FREE_WORD
    vol[tz, ty, tx:X - 2] = FREE_WORD
    seeds = {"face, local 0": (tx, 0, 0), "face, local TILE - 1": (tx - 1, 0, 0), "corner, local 0": (tx, ty, tz),
             "corner, local TILE - 1": (tx - 1, ty - 1, tz - 1), "corner, on the edge": (tx, ty - 1, tz - 1)}
    return vol, seeds


def two_rooms(sealed):
    """80 x 64 x 48: a wall in the plane x = 40, sealed or with a door over y in [24, 40), z in [0, 30)"""
    vol = free_volume(AT.DST_DIMS)
    vol[:, :, 40] = SOLID_WORD
    if not sealed:
        vol[:30, 24:40, 40] = FREE_WORD
    return vol


def run_harness(exe, tmp_path, d2, weight, min_d2, max_cost, order, seeds, goals=()):
    Z, Y, X = d2.shape
    lin = lambda v: v[0] + X * (v[1] + Y * v[2])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for part in (np.array([X, Y, Z], np.int32), np.array(list(weight) + [min_d2, max_cost, order, len(seeds)], np.uint32),
                     np.array([lin(s) for s in seeds], np.uint32), np.uint32(len(goals)), np.array([lin(v) for v in goals], np.uint32),
                     np.ascontiguousarray(d2, np.uint32)):
            f.write(np.ascontiguousarray(part).tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    n = X * Y * Z
    g = np.frombuffer(raw, np.uint32, n).reshape(Z, Y, X)
    st = np.frombuffer(raw, np.uint64, 6, n * 4)
    at, paths = n * 4 + 48, []
    for _ in goals:
        k = int(np.frombuffer(raw, np.uint32, 1, at)[0])
        paths.append(np.frombuffer(raw, np.int32, 3 * k, at + 4).reshape(k, 3))
        at += 4 + 12 * k
    assert at == len(raw)
    return g, {"n_passable": int(st[0]), "n_reached": int(st[1]), "max_cost_seen": int(st[2])}, int(st[3]), int(st[4]), int(st[5]), paths


def check_path(g, ok, weight, p, goal):
    """every step of the path is an allowed move (ok = RE.allowed of the field's passable voxels), the costs sum to G(goal), it
    starts at a seed and ends at the goal"""
    c = RE.costs(weight)
    assert tuple(p[-1]) == tuple(goal) and g[p[0][2], p[0][1], p[0][0]] == 0
    total = 0
    for a, b in zip(p[:-1], p[1:]):
        d = b - a
        m = int((d[2] + 1) * 9 + (d[1] + 1) * 3 + d[0] + 1)
        assert np.abs(d).max() == 1 and ok[m, a[2], a[1], a[0]]
        total += c[m]
    assert total == int(g[goal[2], goal[1], goal[0]])
