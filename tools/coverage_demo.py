#!/usr/bin/env python3
"""Scan coverage on a half-scanned room: what has the scan not seen yet, and where should the camera go to see it.

Room 0 is scanned through the first of its three turns only (the level one).  The census of the room's box says what is open and
on which side; a lattice of candidate poses around the last pose is scored (hsk_score_views) and ranked (hsk_rank_views); the
coverage image of the last pose and of the best view are written as .ppm (hit grey by depth, FRONTIER red by gain, open blue,
blind black, outside dark green); the frame the sensor takes at the best view is integrated and the census taken again: n_unseen
inside the room's extents must have gone down.

usage: python tools/coverage_demo.py [--n 256] [--frames 240] [--stride 4] [--out coverage_demo]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FACES = ("-x", "+x", "-y", "+y", "-z", "+z")


def coverage_rgb(img):
    cls, depth, gain = img["cls"], img["depth"].astype(np.float32), img["gain"].astype(np.float32)
    rgb = np.zeros(cls.shape + (3,), np.uint8)
    grey = (255.0 - 200.0 * np.clip(depth / 4000.0, 0.0, 1.0)).astype(np.uint8)
    rgb[cls == 0] = grey[cls == 0][:, None]
    red = (120.0 + 135.0 * np.clip(gain / max(1.0, float(gain.max())), 0.0, 1.0)).astype(np.uint8)
    rgb[cls == 1, 0] = red[cls == 1]
    rgb[cls == 2] = (40, 60, 200)
    rgb[cls == 4] = (0, 60, 0)
    return rgb


def write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb).tobytes())


def show(name, c):
    total = c["n_unseen"] + c["n_free"] + c["n_solid"]
    print(f"{name}: unseen {c['n_unseen']} ({100.0 * c['n_unseen'] / total:.1f} %), free {c['n_free']}, solid {c['n_solid']}, frontier voxels {c['n_frontier']}")
    print("    open faces (free voxel, unseen neighbour): " + ", ".join(f"{d} {int(v)}" for d, v in zip(FACES, c["faces"])))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=240, help="frames of the 720-frame scan to fuse: 240 is the level turn")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--out", default="coverage_demo")
    args = ap.parse_args()
    import housescan_amd as hsk

    os.makedirs(args.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    e = hsk.synth_room_extents(0).astype(np.float64)
    cell = 3.0 / args.n
    box = (tuple(max(0, int(np.floor(e[2 * i] / cell))) for i in range(3)), tuple(min(args.n, int(np.ceil(e[2 * i + 1] / cell))) for i in range(3)))
    before = trk.coverage(box)
    show(f"room 0 after {len(poses)} frames of its level turn, voxels {box[0]} .. {box[1]}", before)
    last = poses[-1]
    lattice = hsk.pose_lattice(last, 0.4, 1, float(np.radians(35.0)), 1)
    scores = trk.score_views(lattice)
    order = hsk.rank_views(scores)
    best = lattice[order[0]]
    s = scores[order[0]]
    print(f"{len(lattice)} candidate views scored; {int((scores['eye_state'] == 0).sum())} of them stand in observed free space")
    print(f"best view: candidate {int(order[0])} at {np.round(best[:3, 3].astype(np.float64), 3).tolist()}: gain {int(s['gain'])}, frontier rays {int(s['n_frontier'])}, "
          f"hits {int(s['n_hit'])}, blind {int(s['n_blind'])}")
    here = trk.render_coverage(last)
    there = trk.render_coverage(best)
    print(f"the last pose itself: gain {int(here['score']['gain'])}, frontier rays {int(here['score']['n_frontier'])}")
    write_ppm(os.path.join(args.out, "coverage_last.ppm"), coverage_rgb(here))
    write_ppm(os.path.join(args.out, "coverage_best.ppm"), coverage_rgb(there))
    trk.integrate(hsk.synth_room_depth(0, best), best)
    after = trk.coverage(box)
    show("after the frame taken at the best view", after)
    print(f"n_unseen in the room: {before['n_unseen']} -> {after['n_unseen']} ({before['n_unseen'] - after['n_unseen']} voxels seen for the first time)")
    trk.close()
    if after["n_unseen"] >= before["n_unseen"]:
        print("FAILED: the suggested view revealed nothing")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
