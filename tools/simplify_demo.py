#!/usr/bin/env python3
"""The simplified mesh read-out on a synthetic room: the indexed marching-cubes mesh and its reductions.

Room 0 is scanned at `--n`^3.  The indexed mesh (hsk_extract_mesh_indexed) and the simplified meshes at cluster sizes 2, 4 and 8
(hsk_extract_mesh_simplified: quadric vertex clustering on the GPU) are written as .ply with hsk_write_ply_indexed, and the
vertices and faces of each are printed, with the ranks of the simplified vertices (1: on a wall, 2: on an edge, 3: at a corner).

usage: python tools/simplify_demo.py [--n 256] [--frames 120] [--stride 2] [--mean] [--out simplify_demo]"""
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
    ap.add_argument("--mean", action="store_true", help="HSK_SIMPLIFY_MEAN instead of the quadric")
    ap.add_argument("--out", default="simplify_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd import products
    os.makedirs(args.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames * args.stride, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    lost = 0
    for i, p in enumerate(poses):
        _, ok = trk.process_frame(hsk.synth_room_depth(0, p))
        lost += 0 if ok or i == 0 else 1
    print(f"room 0 at {args.n}^3: {len(poses)} frames, {lost} lost")
    v, f, nrm, _, _ = trk.extract_mesh_indexed(normals=True, rgb=False)
    products.write_ply_indexed(os.path.join(args.out, "mesh_indexed.ply"), v, f, normals=nrm)
    print(f"indexed mesh     : {len(v):9d} vertices {len(f):9d} faces -> {args.out}/mesh_indexed.ply")
    mode = hsk.SIMPLIFY_MEAN if args.mean else hsk.SIMPLIFY_QUADRIC
    for c in (2, 4, 8):
        sv, sf, sn, _, st = trk.extract_mesh_simplified(cluster_voxels=c, mode=mode, normals=True, rgb=False)
        products.write_ply_indexed(os.path.join(args.out, f"mesh_c{c}.ply"), sv, sf, normals=sn)
        print(f"simplified, c = {c} : {len(sv):9d} vertices {len(sf):9d} faces ({100.0 * len(sf) / max(len(f), 1):5.1f} % of the faces); "
              f"by rank {st['n_rank']}, clamped {st['n_clamped']} -> {args.out}/mesh_c{c}.ply")
    trk.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
