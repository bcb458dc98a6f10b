#!/usr/bin/env python3
"""The room partition on a scanned house: where one room ends and the next begins, and the room directories that follow from it.

Rooms 0 and 1 are scanned, each in its own 3 m volume, and fused side by side into one house volume of 6 x 3 x 3 m
(hsk_fuse_volume; room 1 moved 3 m along x), as tools/reach_demo.py does.  The scripted scan turns on one spot in a closed box: it never
sees the space around the camera nor most of the ceiling and the floor, and there is no door.  So the demo finishes the scan by
hand: the never-observed voxels inside either room's box (5 cm off its walls) are set to observed free space, as a scan that
walked the room leaves them, and a doorway 0.8 m wide and 2 m high is cut through the two walls that face each other.  The house volume is partitioned (hsk_build_partition) at the default parameters: solids
and never-observed space are obstacles (a scan from one spot leaves the space behind the walls and most of the ceiling unseen;
counted as air it would join everything to everything).  Printed: the rooms -- voxels, volume,
centroid and box in metres -- and the doors -- the two rooms, the faces, the centre and the upper estimate of the width in metres.
The floor form (hsk_partition_floor) of the band 0.1 .. 1.8 m above the floor is written as floor_rooms.ppm: black a column nobody
can stand in, grey one that belongs to no room, a colour per room.  The house cloud is extracted and every point labelled with the
room whose air it borders (hsk_partition_at, radius 2); the points of every room are written as a room directory
(products.write_room_dir) and the directories loaded back (hsh_load_room).

usage: python tools/partition_demo.py [--n 128] [--frames 720] [--stride 8] [--core 0.5] [--out partition_demo] [--estimate-floor]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLOURS = np.array([(230, 80, 60), (60, 140, 230), (90, 200, 90), (230, 200, 60), (170, 90, 200), (60, 200, 200), (240, 140, 40), (150, 150, 150)], np.uint8)


def write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--frames", type=int, default=720, help="frames of either room's 720-frame scan to fuse")
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--core", type=float, default=0.5, help="metres of clearance that make a voxel part of a room's core")
    ap.add_argument("--out", default="partition_demo")
    ap.add_argument("--estimate-floor", action="store_true", help="take the floor's height from hsk_estimate_upright instead of the synthetic room's extents")
    args = ap.parse_args()
    import housescan_amd as hsk
    from level_demo import estimated_floor        # (beside this file)
    from housescan_amd import house as H
    from housescan_amd import products as P

    os.makedirs(args.out, exist_ok=True)
    n = args.n
    house = hsk.KinfuTracker(hsk.default_config(n, vol_x=2 * n, vol_size_m=(6.0, 3.0, 3.0)))
    for room in (0, 1):
        poses = [hsk.synth_room_pose(room, k, 720) for k in range(0, args.frames, args.stride)]
        trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
        for p in poses:
            trk.integrate(hsk.synth_room_depth(room, p), p)
        move = np.eye(4, dtype=np.float32)
        move[0, 3] = 3.0 * room
        st = house.fuse_from(trk, move)
        print(f"room {room}: {len(poses)} frames, {st['n_fused']} voxels fused at x + {3.0 * room:.0f} m")
        trk.close()
    cell = 3.0 / n
    # the doorway: x through room 0's wall at 2.75 m and room 1's at 3.40 m, z 0.35 .. 1.15 m, from 2 m above the floor down to it
    e = hsk.synth_room_extents(0).astype(np.float64)
    vol = house.download_tsdf()
    for room in (0, 1):
        r = hsk.synth_room_extents(room).astype(np.float64)
        a = [int(np.ceil((r[2 * i] + 0.05 + (3.0 * room if i == 0 else 0.0)) / cell)) for i in range(3)]
        b = [int(np.floor((r[2 * i + 1] - 0.05 + (3.0 * room if i == 0 else 0.0)) / cell)) for i in range(3)]
        inside = vol[a[2]:b[2], a[1]:b[1], a[0]:b[0]]
        unseen = inside[..., 1] == 0
        inside[unseen] = (32767, 1)
        print(f"room {room}: {int(unseen.sum())} never-observed voxels inside its box set to free")
    box = [(int(round(a / cell)), int(round(b / cell))) for a, b in ((2.55, 3.60), (e[3] - 2.0, e[3]), (0.35, 1.15))]
    vol[box[2][0]:box[2][1], box[1][0]:box[1][1], box[0][0]:box[0][1]] = (32767, 1)
    house.upload_tsdf(vol)
    print(f"doorway cut: voxels x {box[0]}, y {box[1]}, z {box[2]}")
    walk = house.default_clearance_params()
    pp = house.default_partition_params(walk, core_d2=min(hsk.clearance_d2(walk, args.core), walk.max_d2))
    rooms, st = house.build_partition(walk, pp)
    doors = house.partition_doors()
    relaxed, first, tiles = house.partition_tiles_relaxed()
    print(f"partition: core_d2 {pp.core_d2} ({args.core} m), min_core_voxels {pp.min_core_voxels}; {st['n_cores']} cores, {st['n_dropped']} dropped, "
          f"{st['n_rooms']} rooms, {st['n_doors']} doors; {st['n_assigned']} of {st['n_passable']} passable voxels assigned; {st['n_rounds']} rounds, "
          f"{relaxed} tile relaxations, {first} of {tiles} tiles on the first list, scratch {st['scratch_bytes'] / 2 ** 20:.0f} MiB")
    for i, r in enumerate(rooms):
        c = (r["sum"].astype(np.float64) / max(int(r["n_voxels"]), 1) + 0.5) * cell
        print(f"    room {i}: {int(r['n_voxels'])} voxels ({int(r['n_voxels']) * cell ** 3:.2f} m^3), {int(r['n_core_voxels'])} of them core; centroid "
              f"({c[0]:.2f}, {c[1]:.2f}, {c[2]:.2f}) m; box {tuple(round(float(v) * cell, 2) for v in r['lo'])} .. {tuple(round(float(v) * cell, 2) for v in r['hi'])} m")
    for d in doors:
        faces = int(d["n_faces"].sum())
        c = (d["sum2"].astype(np.float64) / (2.0 * max(faces, 1)) + 0.5) * cell
        width = 2.0 * float(hsk.clearance_metres(walk, int(d["max_d2"])))
        print(f"    door {int(d['a'])} - {int(d['b'])}: {faces} faces {d['n_faces'].tolist()} by axis, centre ({c[0]:.2f}, {c[1]:.2f}, {c[2]:.2f}) m, "
              f"at most {width:.2f} m wide (max_d2 {int(d['max_d2'])})")
    merged = hsk.merge_rooms(doors, len(rooms), pp.core_d2)
    print(f"    merge at core_d2: {len(set(merged.tolist()))} classes {merged.tolist()}")
    # the floor form
    floor_y = estimated_floor(house, e[3]) if args.estimate_floor else e[3]
    lo, hi = max(0, int(np.floor((floor_y - 1.8) / cell))), min(n, int(np.ceil((floor_y - 0.1) / cell)))
    fp = house.default_partition_params(walk, core_d2=pp.core_d2, min_core_voxels=int(np.ceil((0.25 / cell) ** 2)))          # (a square of edge 0.25 m, in columns)
    fmap, frooms, fdoors, fst = house.partition_floor(1, lo, hi, walk, fp)
    rgb = np.zeros(fmap.shape + (3,), np.uint8)
    rgb[fmap == hsk.kinfu.ROOM_UNASSIGNED] = 90
    held = fmap < hsk.kinfu.ROOM_NONE
    rgb[held] = COLOURS[fmap[held] % len(COLOURS)]
    path = os.path.join(args.out, "floor_rooms.ppm")
    write_ppm(path, rgb)
    print(f"floor form of the planes y = {lo} .. {hi - 1}: {fst['n_rooms']} rooms of {[int(v) for v in frooms['n_voxels']]} columns "
          f"({[round(int(v) * cell * cell, 2) for v in frooms['n_voxels']]} m^2), {fst['n_doors']} doors -> {path}")
    # the house cloud, labelled and written out room by room
    cloud, total = house.extract_cloud()
    ids = house.partition_at(cloud, radius=2)
    print(f"house cloud: {len(cloud)} points; " + ", ".join(f"room {i}: {int((ids == i).sum())}" for i in range(len(rooms))) +
          f"; no room within 2 voxels: {int((ids == hsk.kinfu.ROOM_NONE).sum())}")
    hs = H.House()
    for i in range(len(rooms)):
        pts = cloud[ids == i]
        if len(pts) < 1000:
            print(f"    room {i}: {len(pts)} points, no directory written")
            continue
        d = os.path.join(args.out, f"room{i}")
        planes, n_down = P.write_room_dir(d, pts, leaf=0.04, dist_thresh=0.025, min_fraction=0.03)
        rid = hs.load_room(d)
        print(f"    room {i}: {len(pts)} points, {n_down} downsampled, {len(planes)} planes -> {d}; hsh_load_room gives room id {rid}")
    house.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
