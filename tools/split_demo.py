#!/usr/bin/env python3
"""The scene split on a scanned room: structure, objects, and the room without them (hsk_split_scene, hsk_remove_objects).

Room 0 is scanned with a box composited into every depth frame (min(depth, the box's depth along the pixel's ray)), with the
tracker's own poses and the sensor model's noise, or at the script's poses without noise.  The planes come from
hsk_detect_planes_volume, the up direction from hsk_estimate_upright, the kinds from hsk_split_plane_kinds; the volume is split at
the default parameters.  Printed: the planes with their kinds, the kept objects in metres with their contacts and their heights
over the floor, whether the box is ONE kept object, and the kept objects away from the box (the walls' false objects).  Then the
objects are removed (the box alone, or with --remove all every kept object) and the mesh and the section floor plan are written
before and after (.ply, .ppm).

usage: python tools/split_demo.py [--n 256] [--stride 3] [--poses tracker|script] [--remove box|all] [--out split_demo]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOX = ((0.9, 2.1, 0.8), (1.3, 2.65, 1.2))      # free floor between the cupboard and the wardrobe of room 0, 5 cm above the floor
KINDS = {1: "floor", 2: "ceiling", 3: "wall", 4: "other"}


def scan(hsk, args):
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 720, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    lost = 0
    for p in poses:
        d = hsk.synth_sensor_depth(p, scene=0, seed=1234)[0] if args.poses == "tracker" else hsk.synth_room_depth(0, p)
        d = hsk.synth_box_depth(d, p, *BOX)
        if args.poses == "tracker":
            lost += 0 if trk.process_frame(d)[1] else 1
        else:
            trk.integrate(d, p)
    return trk, lost, len(poses)


def floor_plan(hsk, side=512):
    """KinfuTracker.render_section's keywords for room 0 from above, 3.2 m across, cut at mid height"""
    from housescan_amd import _lib
    x0, x1, y0, y1, z0, z1 = (float(v) for v in hsk.synth_room_extents(0))
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = [[-1, 0, 0], [0, 0, 1], [0, 1, 0]]          # x axis -x, y axis +z, looking along +y (down)
    pose[:3, 3] = (0.5 * (x0 + x1), -0.5, 0.5 * (z0 + z1))
    return dict(pose=pose, projection=_lib.HSK_PROJ_ORTHO, width=side, height=side, fx=side / 3.2, fy=side / 3.2, cx=(side - 1) / 2.0, cy=(side - 1) / 2.0,
                clip=[(0, 1, 0, -0.5 * (y0 + y1))], mode=_lib.HSK_VIEW_LAMBERT, light=(0.3, -1.0, 0.2), light_in_camera=0, light_directional=1)


def write_products(hsk, trk, out, tag):
    from housescan_amd.products import write_ply_indexed, write_ppm
    v, f, nrm = trk.extract_mesh_indexed(rgb=False)[:3]
    write_ply_indexed(os.path.join(out, f"mesh_{tag}.ply"), v, f, nrm)
    write_ppm(os.path.join(out, f"floor_plan_{tag}.ppm"), trk.render_section(**floor_plan(hsk))["rgb"])
    return len(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--stride", type=int, default=3)
    ap.add_argument("--poses", default="tracker", choices=("tracker", "script"))
    ap.add_argument("--remove", default="box", choices=("box", "all"))
    ap.add_argument("--out", default="split_demo")
    ap.add_argument("--json", default="", help="also write the figures to this file")
    args = ap.parse_args()
    import housescan_amd as hsk

    os.makedirs(args.out, exist_ok=True)
    cell = 3.0 / args.n
    trk, lost, n_frames = scan(hsk, args)
    print(f"room 0 with a box at {args.n}^3, {n_frames} frames, poses: {args.poses}; frames lost: {lost}")
    planes, _ = trk.detect_planes()
    up = -np.asarray(trk.estimate_upright()["level"], np.float64).reshape(4, 4)[1, :3]
    pl = hsk.split_plane_kinds(planes["abcd"], up)
    for i, p in enumerate(pl):
        print(f"  plane {i}: {KINDS[int(p['kind'])]:7s} {np.round(p['abcd'], 3).tolist()} ({int(planes[i]['n_inliers'])} inliers)")
    p = trk.default_split_params()
    recs, st = trk.split_scene(pl)
    print(f"hsk_split_scene, defaults dist_m {p.dist_m:.3f} back_m {p.back_m:.3f} cos_min {p.cos_min:.3f} min_voxels {p.min_voxels}: classes {st['n_class'].tolist()}, "
          f"{st['n_objects']} kept objects, {st['n_minor_objects']} MINOR objects, {st['n_edge']} voxels by the edge rule, {st['n_no_normal']} without a gradient")
    vlo = tuple(int(np.floor(BOX[0][i] / cell)) for i in range(3))
    vhi = tuple(int(np.ceil(BOX[1][i] / cell)) for i in range(3))
    print(f"the composited box: {BOX[0]} .. {BOX[1]} m, voxels {vlo} .. {vhi}")
    box_roots, false_kept, objects = [], [], []
    for c in recs:
        lo, hi = [int(v) for v in c["lo"]], [int(v) for v in c["hi"]]
        touches = all(lo[i] < vhi[i] + 2 and hi[i] > vlo[i] - 2 for i in range(3))
        inside = all(lo[i] >= vlo[i] - 3 and hi[i] <= vhi[i] + 3 for i in range(3))
        root = (int(c["root"][2]) * args.n + int(c["root"][1])) * args.n + int(c["root"][0])
        if touches and inside:
            box_roots.append(root)
        else:
            false_kept.append(int(c["n_voxels"]))
        centre = [round((int(c["sum"][i]) / int(c["n_voxels"]) + 0.5) * cell, 3) for i in range(3)]
        contacts = {KINDS[k + 1]: int(c["contact"][k]) for k in range(4) if c["contact"][k]}
        objects.append({"root": root, "n_voxels": int(c["n_voxels"]), "lo": lo, "hi": hi, "centre_m": centre, "contact": contacts, "plane_mask": int(c["plane_mask"]),
                        "height_m": [int(c["height_lo"]) / 65536.0, int(c["height_hi"]) / 65536.0], "is_box": touches and inside})
        print(f"  object at {tuple(round(v * cell, 3) for v in lo)} .. {tuple(round(v * cell, 3) for v in hi)} m, centre {centre}: {int(c['n_voxels'])} voxels, contacts "
              f"{contacts}, planes {int(c['plane_mask']):#x}, {int(c['height_lo']) / 65536.0:.3f} .. {int(c['height_hi']) / 65536.0:.3f} m over the floor"
              f"{' -- THE BOX' if touches and inside else ''}")
    print(f"by its coordinates in the script's frame the box is {len(box_roots)} kept object(s); kept objects away from it (false objects of the walls and the room's own furniture): {len(false_kept)} {false_kept}")
    faces_before = write_products(hsk, trk, args.out, "before")
    rst = trk.remove_objects(box_roots if args.remove == "box" else None)
    faces_after = write_products(hsk, trk, args.out, "after")
    comps = trk.download_components()[vlo[2]:vhi[2], vlo[1]:vhi[1], vlo[0]:vhi[0]]
    left = int((comps != 0xFFFFFFFF).sum())
    print(f"hsk_remove_objects ({args.remove}), defaults {dict((k, int(getattr(trk.default_remove_params(), k))) for k in hsk.kinfu.REMOVE_FIELDS)}: {rst}; "
          f"INSIDE voxels left in the box's voxels: {left}; meshes {faces_before} and {faces_after} faces")
    out = {"n": args.n, "frames": n_frames, "poses": args.poses, "frames_lost": lost, "build_id": hsk._lib.load().hsk_build_id().decode(),
           "planes": [{"abcd": [float(v) for v in q["abcd"]], "kind": int(q["kind"])} for q in pl], "n_class": st["n_class"].tolist(), "n_objects": st["n_objects"],
           "n_minor_objects": st["n_minor_objects"], "n_edge": st["n_edge"], "n_no_normal": st["n_no_normal"], "objects": objects, "box_voxels": [list(vlo), list(vhi)],
           "box_objects": len(box_roots), "false_kept_objects": false_kept, "remove": rst, "inside_left_in_box": left, "faces": [faces_before, faces_after]}
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    trk.close()
    if args.poses == "tracker":
        # (the volume's frame is the tracker's own, not the script's: the box cannot be named by its coordinates there; look for the
        # object whose heights over the floor are the box's, 0.05 .. 0.60 m)
        print("the tracker's frame is not the script's: the verdict by coordinates does not apply; see the objects' heights and sizes")
        return 0
    if len(box_roots) != 1:
        print("FAILED: the box is not one kept object")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
