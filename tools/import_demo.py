#!/usr/bin/env python3
"""Cloud import: a room that exists only as a room directory's cloud_bin.pcd becomes a volume again, with carved free space.

Room 0 is scanned (its scripted scan, every `--stride`-th frame), its census printed, its floor plan written
(hsk_render_section -> floor_plan_original.ppm) and its cloud extracted and written as a room directory
(products.write_room_dir); the context is closed -- from here on the room is its directory.  A fresh context of the same size
imports the directory's cloud (house.import_room -> hsk_import_cloud) from a fan of virtual cameras at the room's middle:
hsk_pose_lattice(centre, 0, 0, step, n_rot), yaw x pitch from one standpoint.  Printed: the census before and after the import
beside the original's; the rooms hsk_build_partition finds in the imported volume; then the loop the coverage calls are for --
a lattice of further standpoints is scored (hsk_score_views) and ranked (hsk_rank_views), the best view is imported too, and
n_unseen falls.  The imported volume's floor plan is written as floor_plan_imported.ppm.

usage: python tools/import_demo.py [--n 128] [--stride 12] [--n-rot 4] [--core 0.25] [--out import_demo]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def census_line(c):
    return f"unseen {c['n_unseen']}, free {c['n_free']}, solid {c['n_solid']}, frontier {c['n_frontier']}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--stride", type=int, default=12)
    ap.add_argument("--n-rot", type=int, default=4, help="the fan holds (2 n_rot + 1)^2 views")
    ap.add_argument("--core", type=float, default=0.25, help="metres of clearance that make a voxel part of a room's core (a fan from one standpoint leaves "
                    "never-observed space, an obstacle, around the camera: less than a walked scan's 0.5 m)")
    ap.add_argument("--out", default="import_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from split_demo import floor_plan             # (beside this file)
    from housescan_amd import house as H
    from housescan_amd import products as P

    os.makedirs(args.out, exist_ok=True)
    n, cell = args.n, 3.0 / args.n
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 720, args.stride)]
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    original = trk.coverage()
    P.write_ppm(os.path.join(args.out, "floor_plan_original.ppm"), trk.render_section(**floor_plan(hsk))["rgb"])
    cloud, _ = trk.extract_cloud()
    room_dir = os.path.join(args.out, "room0")
    P.write_room_dir(room_dir, cloud, leaf=0.04, dist_thresh=0.025, min_fraction=0.03)
    trk.close()
    print(f"scanned: {len(poses)} frames at {n}^3, {len(cloud)} points -> {room_dir}; the context is closed")
    print(f"    original census: {census_line(original)}")

    e = hsk.synth_room_extents(0).astype(np.float64)
    centre = np.array(poses[0], np.float32).reshape(4, 4).copy()
    centre[:3, 3] = (0.5 * (e[0] + e[1]), 0.5 * (e[2] + e[3]), 0.5 * (e[4] + e[5]))
    step = float(np.pi / (2 * args.n_rot + 1))    # yaw over half a turn to either side, pitch likewise (the lattice turns both by the same step)
    fan = hsk.pose_lattice(centre, 0.0, 0, step, args.n_rot)
    new = hsk.KinfuTracker(n=n, init_pose=centre)
    params = dict(point_size_m=cell, max_half_px=32.0)      # the cloud's spacing is the scanned volume's cell
    print(f"    empty census:    {census_line(new.coverage())}")
    stats, xyz = H.import_room(room_dir, new, fan, **params)
    imported = new.coverage()
    print(f"imported {len(xyz)} points from {len(fan)} views at the room's middle: {int(stats['n_splatted'].sum())} point views splatted, "
          f"{int(stats['n_pixels'].sum())} pixels")
    print(f"    imported census: {census_line(imported)}")
    walk = new.default_clearance_params()
    pp = new.default_partition_params(walk, core_d2=min(hsk.clearance_d2(walk, args.core), walk.max_d2))
    rooms, st = new.build_partition(walk, pp)
    print(f"    partition (core {args.core} m): {st['n_rooms']} rooms, {st['n_doors']} doors; " + ", ".join(f"room {i}: {int(r['n_voxels']) * cell ** 3:.2f} m^3" for i, r in enumerate(rooms)))
    # where should the next virtual camera stand
    around = hsk.pose_lattice(centre, 0.5, 1, float(np.radians(60.0)), 1)
    sc = new.score_views(around)
    order = hsk.rank_views(sc)
    best = around[order[0]]
    print(f"    next view: {order[0]} of {len(around)}, {sc[order[0]]}")
    new.import_cloud(xyz, best[None], **params)
    after = new.coverage()
    print(f"    with that view:  {census_line(after)} (n_unseen {imported['n_unseen']} -> {after['n_unseen']})")
    path = os.path.join(args.out, "floor_plan_imported.ppm")
    P.write_ppm(path, new.render_section(**floor_plan(hsk))["rgb"])
    print(f"floor plans -> {os.path.join(args.out, 'floor_plan_original.ppm')}, {path}")
    new.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
