#!/usr/bin/env python3
"""Hole filling on a half-scanned room: the gaps a scan leaves, closed by volumetric diffusion (hsk_fill_holes).

Room 0 is scanned through the first of its three turns only (the level one), which leaves real gaps: the floor and the ceiling
the level turn missed, the shadows of the furniture.  The census of the room's box, the indexed mesh's face count and its
boundary-edge count (edges used by exactly one triangle) are printed before and after the fill; both meshes are written as .ply,
and a view from the last pose as .ppm with the pixels that hit filled voxels (hsk_download_fill_mask) tinted orange.

usage: python tools/fill_demo.py [--n 256] [--frames 240] [--stride 4] [--iterations 0] [--out fill_demo]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb).tobytes())


def show(name, c):
    total = c["n_unseen"] + c["n_free"] + c["n_solid"]
    print(f"{name}: unseen {c['n_unseen']} ({100.0 * c['n_unseen'] / total:.1f} %), free {c['n_free']}, solid {c['n_solid']}, frontier voxels {c['n_frontier']}")


def boundary_edges(faces):
    if len(faces) == 0:
        return 0
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1).astype(np.int64)
    key = e[:, 0] * (int(e.max()) + 1) + e[:, 1]
    return int((np.unique(key, return_counts=True)[1] == 1).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=240, help="frames of the 720-frame scan to fuse: 240 is the level turn")
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=0, help="0: hsk_default_fill_params'")
    ap.add_argument("--out", default="fill_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd.products import write_ply_indexed

    os.makedirs(args.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    e = hsk.synth_room_extents(0).astype(np.float64)
    cell = 3.0 / args.n
    box = (tuple(max(0, int(np.floor(e[2 * i] / cell))) for i in range(3)), tuple(min(args.n, int(np.ceil(e[2 * i + 1] / cell))) for i in range(3)))
    show(f"room 0 after {len(poses)} frames of its level turn, voxels {box[0]} .. {box[1]}", trk.coverage(box))
    v0, f0, n0 = trk.extract_mesh_indexed(rgb=False)[:3]
    open0 = boundary_edges(f0)
    print(f"mesh before: {len(f0)} faces, {open0} boundary edges")
    write_ply_indexed(os.path.join(args.out, "before.ply"), v0, f0, n0)
    params = trk.default_fill_params() if args.iterations <= 0 else trk.default_fill_params(iterations=args.iterations)
    st = trk.fill_holes(params, box=box)
    print(f"hsk_fill_holes, {params.iterations} iterations, band {params.band}, inside the room's box: {st}")
    show("after the fill", trk.coverage(box))
    v1, f1, n1 = trk.extract_mesh_indexed(rgb=False)[:3]
    open1 = boundary_edges(f1)
    print(f"mesh after: {len(f1)} faces, {open1} boundary edges")
    write_ply_indexed(os.path.join(args.out, "after.ply"), v1, f1, n1)
    mask = trk.download_fill_mask()
    img = trk.render_view(pose=poses[-1], vmap=True, depth=False)
    rgb = img["rgb"].copy()
    idx = np.floor(np.nan_to_num(img["vmap"], nan=-1.0) / cell).astype(np.int64)
    ok = ((idx >= 0) & (idx < args.n)).all(axis=0)
    hit = np.zeros(ok.shape, bool)
    hit[ok] = mask[idx[2][ok], idx[1][ok], idx[0][ok]] == 1
    rgb[hit] = (0.5 * rgb[hit] + 0.5 * np.array((255, 128, 0))).astype(np.uint8)
    write_ppm(os.path.join(args.out, "filled_view.ppm"), rgb)
    print(f"view from the last pose: {int(hit.sum())} of {img['n_hit']} hit pixels show filled surface")
    trk.close()
    if st["n_written"] == 0 or len(f1) <= len(f0):
        print("FAILED: the fill added no surface")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
