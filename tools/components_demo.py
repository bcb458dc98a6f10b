#!/usr/bin/env python3
"""Surface components on a noisy room scan: what floats in free space, and the scan without it.

Room 0 is scanned through the sensor model's noise stream (hsk_synth_render_sensor: shadow bands at depth discontinuities, no return
from grazing rays, range noise).  The volume's components are labelled on the device (hsk_label_components); the head of the
table and the number of components below the default min_voxels are printed; hsk_prune_components erases those; the cloud's
point count before and after is printed and both clouds are written as .ply.

usage: python tools/components_demo.py [--n 256] [--frames 120] [--stride 2] [--sigma-mm 2.0] [--out components_demo]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--stride", type=int, default=2, help="every stride-th frame of the 720-frame scan")
    ap.add_argument("--sigma-mm", type=float, default=2.0)
    ap.add_argument("--out", default="components_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd import house
    os.makedirs(args.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames * args.stride, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    lost = 0
    for i, p in enumerate(poses):
        depth, _ = hsk.synth_sensor_depth(p, 0, 1234 + i, args.sigma_mm)
        _, ok = trk.process_frame(depth)
        lost += 0 if ok or i == 0 else 1
    print(f"room 0 at {args.n}^3: {len(poses)} frames, {lost} lost")
    rec, st = trk.label_components()
    p = trk.default_prune_params()
    print(f"{st['n_components']} components, {st['n_inside']} inside voxels, the largest {st['largest']}")
    print("rank  voxels     root             box")
    for i, r in enumerate(rec[:10]):
        print(f"{i:4d}  {int(r['n_voxels']):9d}  {tuple(int(v) for v in r['root'])!s:15s}  {tuple(int(v) for v in r['lo'])} .. {tuple(int(v) for v in r['hi'])}")
    small = rec["n_voxels"] < p.min_voxels
    print(f"{int(small.sum())} components ({int(rec['n_voxels'][small].sum())} voxels) lie below the default min_voxels = {p.min_voxels}")
    before, _ = trk.extract_cloud()
    house.write_ply_points(os.path.join(args.out, "cloud_before.ply"), before)
    got = trk.prune_components()
    after, _ = trk.extract_cloud()
    house.write_ply_points(os.path.join(args.out, "cloud_after.ply"), after)
    print(f"pruned {got['n_pruned']} components, {got['n_pruned_voxels']} voxels; {got['n_kept_voxels']} voxels kept")
    print(f"hsk_extract_cloud: {len(before)} points before, {len(after)} after; written to {args.out}/cloud_before.ply and cloud_after.ply")
    trk.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
