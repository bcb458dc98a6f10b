#!/usr/bin/env python3
"""The reach field on a scanned house: which viewpoints can a person walk to, and how far is the walk.

Rooms 0 and 1 are scanned, each in its own 3 m volume, and fused side by side into one house volume of 6 x 3 x 3 m
(hsk_fuse_volume; room 1 moved 3 m along x).  The seed is the camera's last position in room 0; the reach field takes solids only
as obstacles (clearance flags 0): the camera's own position lies inside the sensor's near range, in space a scan from one spot
never observes, and HSK_CLEAR_UNKNOWN would count it as an obstacle.  The floor reach map of the band
0.1 .. 1.8 m above the floor (hsk_reach_floor; y grows downward in the scan frame, so the floor is the room's high-y wall) is
written as floor_reach.pgm -- black: a column nobody can stand in, grey: one no walk arrives at, brighter: a longer walk.  A lattice
of candidate poses around the last pose of either room is scored (hsk_score_views) and ranked three times: by hsk_rank_views, by
hsk_rank_views_clear (0.3 m of room at the camera centre) and by hsk_rank_views_reach (the camera centre can be walked to from the
seed).  Printed: the three heads, the walk to each of them in metres, and the path to hsk_rank_views_reach's best pose.

usage: python tools/reach_demo.py [--n 128] [--frames 720] [--stride 8] [--min-clear 0.3] [--out reach_demo] [--estimate-floor]"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--frames", type=int, default=720, help="frames of either room's 720-frame scan to fuse")
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--min-clear", type=float, default=0.3, help="metres a person keeps from anything solid or unknown")
    ap.add_argument("--out", default="reach_demo")
    ap.add_argument("--estimate-floor", action="store_true", help="take the floor's height from hsk_estimate_upright instead of the synthetic room's extents")
    args = ap.parse_args()
    import housescan_amd as hsk
    from level_demo import estimated_floor        # (beside this file)

    os.makedirs(args.out, exist_ok=True)
    n = args.n
    house = hsk.KinfuTracker(hsk.default_config(n, vol_x=2 * n, vol_size_m=(6.0, 3.0, 3.0)))
    last = []
    for room in (0, 1):
        poses = [hsk.synth_room_pose(room, k, 720) for k in range(0, args.frames, args.stride)]
        trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
        for p in poses:
            trk.integrate(hsk.synth_room_depth(room, p), p)
        move = np.eye(4, dtype=np.float32)
        move[0, 3] = 3.0 * room
        st = house.fuse_from(trk, move)
        last.append(move @ poses[-1])
        print(f"room {room}: {len(poses)} frames, {st['n_fused']} voxels fused at x + {3.0 * room:.0f} m")
        trk.close()
    par = house.default_clearance_params()
    walk = house.default_clearance_params(flags=0)          # what a person cannot walk through: solids
    rp = house.default_reach_params(par, min_d2=hsk.clearance_d2(par, args.min_clear))
    seed = [tuple(float(v) for v in last[0][:3, 3])]
    st = house.build_reach(seed, walk, rp)
    relaxed, tiles = house.reach_tiles_relaxed()
    print(f"reach field: min_d2 {rp.min_d2} ({args.min_clear} m), {st['n_passable']} passable voxels, {st['n_reached']} reached from {seed[0]}, "
          f"farthest {float(hsk.reach_metres(par, st['max_cost_seen'])):.2f} m; {st['n_rounds']} rounds, {relaxed} tile relaxations "
          f"({100.0 * relaxed / (tiles * max(st['n_rounds'], 1)):.1f} % of tiles x rounds), scratch {st['scratch_bytes'] / 2 ** 20:.0f} MiB")
    e = hsk.synth_room_extents(0).astype(np.float64)
    cell = 3.0 / n
    floor_y = estimated_floor(house, e[3]) if args.estimate_floor else e[3]
    lo, hi = max(0, int(np.floor((floor_y - 1.8) / cell))), min(n, int(np.ceil((floor_y - 0.1) / cell)))
    fmap, fst = house.reach_floor(1, lo, hi, seed, walk, rp)
    m = hsk.reach_metres(par, fmap)
    top = max(float(np.nanmax(m)) if np.isfinite(m).any() else 1.0, 1e-6)
    grey = np.where(fmap == hsk.kinfu.REACH_BLOCKED, 0, np.where(fmap == hsk.kinfu.REACH_UNREACHED, 64, 96 + np.nan_to_num(m) / top * 159.0)).astype(np.uint8)
    path = os.path.join(args.out, "floor_reach.pgm")
    write_pgm(path, grey)
    print(f"floor reach map of the planes y = {lo} .. {hi - 1}: {fst['n_passable']} columns a person can stand in, {fst['n_reached']} of them "
          f"({fst['n_reached'] * cell * cell:.2f} m^2) within a walk, the longest {top:.2f} m -> {path}")
    lattice = np.concatenate([hsk.pose_lattice(p, 0.4, 2, float(np.radians(35.0)), 1) for p in last])
    scores = house.score_views(lattice)
    eyes = lattice[:, :3, 3]
    eye_d2 = house.clearance_at(eyes, par)
    eye_g = house.reach_at(eyes)
    plain, clear, reach = hsk.rank_views(scores), hsk.rank_views_clear(scores, eye_d2, rp.min_d2), hsk.rank_views_reach(scores, eye_g)
    print(f"{len(lattice)} candidate poses, half of them around the last pose of each room; {int((eye_g <= hsk.kinfu.REACH_MAX_COST).sum())} can be walked to")
    for name, order in (("hsk_rank_views", plain), ("hsk_rank_views_clear", clear), ("hsk_rank_views_reach", reach)):
        head = [int(i) for i in order[:8]]
        print(f"    {name}: top 8 {head}, the walk to them (m) {[round(float(v), 2) for v in hsk.reach_metres(par, eye_g[head])]}")
    best = int(reach[0])
    steps = house.reach_path(eyes[best], cap=1 << 16)
    print(f"path to pose {best} at {tuple(round(float(v), 2) for v in eyes[best])}: {len(steps)} voxels, {float(hsk.reach_metres(par, eye_g[best])):.2f} m")
    if len(steps):
        shown = steps[:: max(1, len(steps) // 12)]
        print("    " + " -> ".join(str(tuple(int(c) for c in v)) for v in shown) + (" -> " + str(tuple(int(c) for c in steps[-1])) if tuple(shown[-1]) != tuple(steps[-1]) else ""))
    house.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
