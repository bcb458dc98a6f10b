#!/usr/bin/env python3
"""Level a scan that started tilted: find the volume's upright frame on the device and resample the scan into it.

Room 0 is scanned from an init_pose tilted by Rx(15) Rz(5) Ry(20) degrees about the volume's centre -- the frames are rendered from the
untilted poses, so the room lands in the volume tilted, as a hand-held scan that starts looking down does.  hsk_estimate_upright finds
the up direction, the walls' direction, floor and ceiling; hsk_level_config and hsk_fuse_volume make the levelled volume.  Written: the
floor map of the band 0.1 .. 1.8 m above the ESTIMATED floor before levelling (floor_tilted.pgm: the band is a slanted cut) and after
(floor_levelled.pgm: the room's rectangle), and the levelled frame as level.xf (hsk_write_xf; hsk_transform_cloud takes the same
matrix).  Printed: the recovered angles against the tilt.

usage: python tools/level_demo.py [--n 256] [--frames 720] [--stride 4] [--out level_demo]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pgm(path, grey):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (grey.shape[1], grey.shape[0]))
        f.write(np.ascontiguousarray(grey, np.uint8).tobytes())


def estimated_floor(trk, fallback):
    """the levelled y of the floor as hsk_estimate_upright finds it (for a scan that starts level that is the volume's y)"""
    up = trk.estimate_upright()
    if not up["found"] & 4:
        print(f"estimate_upright found no floor (found = {up['found']}): keeping the extents' {fallback:.3f} m")
        return fallback
    tilt = float(np.degrees(np.arccos(min(1.0, float(up["level"][1, 1])))))
    print(f"estimate_upright: floor at y = {float(up['floor_m']):.3f} m (the extents say {fallback:.3f} m), up {tilt:.2f} degrees off the volume's y")
    return float(up["floor_m"])


def rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def floor_map(hsk, trk, floor_y, cell_y, dim_y, path):
    lo, hi = max(0, int(np.ceil((floor_y - 1.8) / cell_y))), min(dim_y, int(np.floor((floor_y - 0.1) / cell_y)))
    par = trk.default_clearance_params()
    fmap, st = trk.clearance_floor(1, lo, max(lo, hi), par)
    metres = hsk.clearance_metres(par, fmap)
    write_pgm(path, np.where(np.isinf(metres), 255, np.clip(metres, 0.0, 1.0) * 254.0).astype(np.uint8))
    print(f"    floor map of the planes y = {lo} .. {hi - 1}: {fmap.size - st['n_obstacle']} free columns of {fmap.size} -> {path}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=720, help="frames of the 720-frame scan to fuse")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--out", default="level_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd import products as P

    os.makedirs(args.out, exist_ok=True)
    R = rot(0, 15.0) @ rot(2, 5.0) @ rot(1, 20.0)
    tilt = np.eye(4)
    tilt[:3, :3] = R
    tilt[:3, 3] = 1.5 - R @ np.full(3, 1.5)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=(tilt @ poses[0].astype(np.float64)).astype(np.float32))
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), (tilt @ p.astype(np.float64)).astype(np.float32))
    up = trk.estimate_upright()
    L = up["level"][:3, :3].astype(np.float64)
    deg = lambda a, b: float(np.degrees(np.arccos(min(1.0, abs(float(a @ b))))))
    true_down = R @ [0.0, 1.0, 0.0]
    walls = [R @ [1.0, 0.0, 0.0], R @ [0.0, 0.0, 1.0]]
    print(f"scan of {len(poses)} frames at {args.n}^3, tilted by Rx(15) Rz(5) Ry(20): {up['n_points']} points, found = {up['found']}")
    print(f"    up: {deg(-L[1], [0.0, -1.0, 0.0]):.3f} degrees off the volume's y (the tilt: {deg(true_down, [0.0, 1.0, 0.0]):.3f}), "
          f"{deg(L[1], true_down):.3f} degrees off the truth")
    print(f"    walls: row 0 is {min(deg(L[0], w) for w in walls):.3f} degrees off the nearest wall direction; {up['n_walls']} wall points, "
          f"supporters of the rows {up['n_axis']}")
    print(f"    floor at levelled y = {float(up['floor_m']):.3f} m, ceiling at {float(up['ceiling_m']):.3f} m: {float(up['floor_m'] - up['ceiling_m']):.3f} m high; "
          f"box {np.round(up['box_lo'], 3)} .. {np.round(up['box_hi'], 3)}")
    if not up["found"] & 1:
        print("the up direction was not found: nothing to level")
        return 1
    cell = 3.0 / args.n
    # before: the band about the floor's height where the up axis through the box's centre meets it, in the tilted volume
    centre = L.T @ np.array([(up["box_lo"][0] + up["box_hi"][0]) / 2, float(up["floor_m"]), (up["box_lo"][2] + up["box_hi"][2]) / 2])
    floor_map(hsk, trk, float(centre[1]), cell, args.n, os.path.join(args.out, "floor_tilted.pgm"))
    lev, M, _ = trk.levelled()
    print(f"levelled volume: {lev.cfg.vol_x} x {lev.cfg.vol_y} x {lev.cfg.vol_z} voxels over {np.round(np.array(lev.cfg.vol_size_m), 3)} m "
          f"({lev.cfg.vol_x * lev.cfg.vol_y * lev.cfg.vol_z / args.n ** 3:.2f} of the source's)")
    again = lev.estimate_upright()
    A = again["level"][:3, :3].astype(np.float64)
    print(f"    its own estimate: rows {[round(deg(A[k], np.eye(3)[k]), 3) for k in range(3)]} degrees off its axes, floor at y = {float(again['floor_m']):.3f} m "
          f"(put at {float(up['floor_m']) + float(M[1, 3]):.3f} m)")
    floor_map(hsk, lev, float(again["floor_m"]), float(lev.cfg.vol_size_m[1]) / lev.cfg.vol_y, lev.cfg.vol_y, os.path.join(args.out, "floor_levelled.pgm"))
    P.write_xf(os.path.join(args.out, "level.xf"), M)
    print(f"    the levelling matrix -> {os.path.join(args.out, 'level.xf')}")
    lev.close()
    trk.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
