#!/usr/bin/env python3
"""The clearance field on a scanned room: how much room is there, and which viewpoints can a person actually hold a sensor at.

Room 0 is scanned; the floor map of the band 0.1 .. 1.8 m above the floor (hsk_clearance_floor; y grows downward in the scan frame,
so the floor is the room's high-y wall) is written as a .pgm -- black: an obstacle column, brighter: more room, white: a metre or
more (floor_map.pgm: solid or never observed; floor_map_solid.pgm: solids only); a lattice of candidate poses around the last pose is scored (hsk_score_views) and ranked twice, by hsk_rank_views and by
hsk_rank_views_clear with min_d2 = hsk_clearance_d2(0.3 m) on the clearance at the camera centres (hsk_clearance_at); printed:
how many of hsk_rank_views' top 10 the clearance moved back.

usage: python tools/clearance_demo.py [--n 256] [--frames 720] [--stride 4] [--min-clear 0.3] [--out clearance_demo] [--estimate-floor]"""
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
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=720, help="frames of the 720-frame scan to fuse")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--min-clear", type=float, default=0.3, help="metres a viewpoint must keep from anything solid or unknown")
    ap.add_argument("--out", default="clearance_demo")
    ap.add_argument("--estimate-floor", action="store_true", help="take the floor's height from hsk_estimate_upright instead of the synthetic room's extents")
    args = ap.parse_args()
    import housescan_amd as hsk
    from level_demo import estimated_floor        # (beside this file)

    os.makedirs(args.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    par = trk.default_clearance_params()
    st = trk.build_clearance(par)
    print(f"field: weights {tuple(par.weight)}, unit {par.unit_m * 1e3:.2f} mm, max_d2 {par.max_d2}; {st['n_obstacle']} obstacle voxels, "
          f"{st['n_far']} farther than a metre, scratch {st['scratch_bytes'] / 2 ** 20:.0f} MiB")
    e = hsk.synth_room_extents(0).astype(np.float64)
    cell = 3.0 / args.n
    floor_y = estimated_floor(trk, e[3]) if args.estimate_floor else e[3]
    lo, hi = max(0, int(np.floor((floor_y - 1.8) / cell))), min(args.n, int(np.ceil((floor_y - 0.1) / cell)))
    fmap, fst = trk.clearance_floor(1, lo, hi, par)
    metres = hsk.clearance_metres(par, fmap)
    grey = np.where(np.isinf(metres), 255, np.clip(metres, 0.0, 1.0) * 254.0).astype(np.uint8)
    path = os.path.join(args.out, "floor_map.pgm")
    write_pgm(path, grey)
    solid, _ = trk.clearance_floor(1, lo, hi, par, flags=0)         # the same band with only solids as obstacles: the room's own shape
    m0 = hsk.clearance_metres(par, solid)
    write_pgm(os.path.join(args.out, "floor_map_solid.pgm"), np.where(np.isinf(m0), 255, np.clip(m0, 0.0, 1.0) * 254.0).astype(np.uint8))
    standable = int((fmap >= hsk.clearance_d2(par, args.min_clear)).sum())
    print(f"floor map of the planes y = {lo} .. {hi - 1} (0.1 .. 1.8 m above the floor): {fst['n_obstacle']} obstacle columns of {fmap.size}, "
          f"{standable} columns with {args.min_clear} m of room ({standable * cell * cell:.2f} m^2) -> {path}")
    lattice = hsk.pose_lattice(poses[-1], 0.4, 2, float(np.radians(35.0)), 1)
    scores = trk.score_views(lattice)
    eye_d2 = trk.clearance_at(lattice[:, :3, 3], par)
    min_d2 = hsk.clearance_d2(par, args.min_clear)
    plain = hsk.rank_views(scores)
    clear = hsk.rank_views_clear(scores, eye_d2, min_d2)
    top = [int(i) for i in plain[:10]]
    moved = [i for i in top if i not in set(int(j) for j in clear[:10])]
    print(f"{len(lattice)} candidate poses, min_d2 {min_d2}: hsk_rank_views' top 10 {top}")
    print(f"    their clearance (m): {[round(float(m), 3) for m in hsk.clearance_metres(par, eye_d2[top])]}")
    print(f"    hsk_rank_views_clear's top 10 {[int(i) for i in clear[:10]]}: the clearance moved {len(moved)} of the top 10 back")
    trk.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
