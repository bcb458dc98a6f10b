#!/usr/bin/env python3
"""A textured mesh of a synthetic room: few triangles, and a colour atlas at the scan's own resolution.

Room 0 is scanned with colour at `--n`^3 and its mesh is simplified at `--cluster` voxels (hsk_extract_mesh_simplified).
hsk_bake_texture lays the faces out in an atlas and bakes it on the GPU; the mesh goes to room_textured.ply (hsk_write_ply_textured:
per-face texture coordinates, the form Meshlab reads) and the atlas to room_atlas.png (hsk_write_png_rgb), with the normal map and
the mask beside them.  Printed: the atlas's size and texel counts, and -- a report, not a test -- the mean colour error per channel
of `--samples` baked texels inside faces against hsk_synth_color_at at the same points, beside the error of the mesh's vertex
colours interpolated to the same points.

usage: python tools/texture_demo.py [--n 256] [--frames 120] [--stride 2] [--cluster 8] [--width 1024] [--samples 4000] [--out texture_demo]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def texel_points(bk, v, f, idx):
    """the points P0 on their faces and the barycentrics of the texels idx (flat indices into the atlas), from the charts alone"""
    W = bk["width"]
    own = np.full(bk["mask"].shape, -1, np.int64)
    for i, (x0, y0, s, hr) in enumerate(bk["charts"].tolist()):
        if s < 0:
            continue
        j, k = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        mine = (k + j <= s - 2) if (hr & 255) == 0 else (k + j > s - 2)
        own[y0:y0 + s, x0:x0 + s][mine] = i
    face = own.reshape(-1)[idx]
    ch = bk["charts"][face]
    x = (idx % W) - ch["x0"] + 0.5
    y = (idx // W) - ch["y0"] + 0.5
    half = (ch["half_rot"] & 255) == 1
    x, y = np.where(half, ch["s"] - x, x), np.where(half, ch["s"] - y, y)
    bu, bv = (x - 1) / (ch["s"] - 5), (y - 1) / (ch["s"] - 5)
    r = ch["half_rot"] >> 8
    corners = [f[face, (r + j) % 3] for j in range(3)]
    bary = np.stack([1 - bu - bv, bu, bv], axis=1)
    p = sum(bary[:, j:j + 1] * v[corners[j]] for j in range(3))
    return p, corners, bary


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--stride", type=int, default=2, help="every stride-th frame of the 720-frame scan")
    ap.add_argument("--cluster", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--out", default="texture_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd import products
    os.makedirs(args.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames * args.stride, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    trk.enable_color()
    lost = 0
    for i, p in enumerate(poses):
        _, ok = trk.process_frame_rgbd(hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0))
        lost += 0 if ok or i == 0 else 1
    print(f"room 0 at {args.n}^3 with colour: {len(poses)} frames, {lost} lost")
    v, f, nrm, vcol, _ = trk.extract_mesh_simplified(cluster_voxels=args.cluster, normals=True, rgb=True)
    bk = trk.bake_texture(v, f, atlas_width=args.width, normal_rgb=True)
    trk.close()
    products.write_ply_textured(os.path.join(args.out, "room_textured.ply"), v, f, bk["uv"], "room_atlas.png", normals=nrm)
    products.write_png_rgb(os.path.join(args.out, "room_atlas.png"), bk["rgb"])
    products.write_png_rgb(os.path.join(args.out, "room_normals.png"), bk["normal_rgb"])
    products.write_png_rgb(os.path.join(args.out, "room_mask.png"), np.repeat((bk["mask"] * 8)[:, :, None], 3, axis=2))
    n_tex = bk["width"] * bk["height"]
    print(f"simplified, c = {args.cluster}: {len(v)} vertices, {len(f)} faces ({bk['n_faces_skipped']} skipped) -> {args.out}/room_textured.ply")
    print(f"atlas {bk['width']} x {bk['height']}: blocks of 8/16/32/64 = {bk['n_blocks']}; owned {bk['n_owned']} ({100.0 * bk['n_owned'] / max(n_tex, 1):.1f} %), "
          f"inside {bk['n_inside']}, projected {bk['n_projected']}, coloured {bk['n_colored']}, with a normal {bk['n_normal']} -> {args.out}/room_atlas.png")
    want = hsk.TEXEL_INSIDE | hsk.TEXEL_PROJECTED | hsk.TEXEL_COLORED
    idx = np.flatnonzero((bk["mask"].reshape(-1) & want) == want)
    if len(idx) == 0:
        print("no texel is inside a face, projected and coloured: nothing to compare")
        return 0
    idx = np.random.default_rng(0).choice(idx, min(args.samples, len(idx)), replace=False)
    p, corners, bary = texel_points(bk, v.astype(np.float64), f, idx)
    truth = np.array([hsk.synth_color_at(q, 0) for q in p], np.float64)
    baked = bk["rgb"].reshape(-1, 3)[idx].astype(np.float64)
    interp = sum(bary[:, j:j + 1] * vcol[corners[j]].astype(np.float64) for j in range(3))
    print(f"mean |colour error| per channel over {len(idx)} texels, against hsk_synth_color_at at the texel's point on its face: "
          f"baked atlas {np.abs(baked - truth).mean():.2f} levels, interpolated vertex colours {np.abs(interp - truth).mean():.2f} levels")
    return 0


if __name__ == "__main__":
    sys.exit(main())
