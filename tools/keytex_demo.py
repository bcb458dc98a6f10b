#!/usr/bin/env python3
"""A textured mesh of a synthetic room from a depth-only scan: the atlas's colour comes from keyframes, not from a colour volume.

Room 0 is scanned WITHOUT hsk_enable_color at `--n`^3.  The frames' colour is hsk_synth_render_rgb with a fine pattern laid over
it -- a `--checker` m checker of the pixel's world point, computed from the clean depth and the pose; the synthetic colour alone is
too smooth to show anything --, and a frame is kept as a keyframe whenever hsk_keyframe_wanted says so (0.3 m / 20 degrees) at the
tracker's pose.  The mesh is simplified at `--cluster` voxels and baked by hsk_bake_texture_keyframes; it goes to room_keytex.ply
and the atlas to room_keytex_atlas.png.  Printed -- a report, not a test --: the keyframes kept, the share of inside-and-projected
texels keyed, and the mean colour error per channel of `--samples` keyed texels against the same pattern at the texels' points on
their faces; beside it the error of hsk_bake_texture at the same texels on a second context that scanned the same frames with
colour.

usage: python tools/keytex_demo.py [--n 256] [--frames 120] [--stride 2] [--cluster 8] [--width 1024] [--samples 4000] [--checker 0.02] [--mode 0] [--out keytex_demo]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from texture_demo import texel_points  # noqa: E402

AMPLITUDE = 40      # the checker adds or takes this many levels
INTR = (525.0, 525.0, 319.5, 239.5)


def checker_sign(p, period):
    """+1 / -1 per world point [..., 3]: a 3-D checker of cells `period` metres wide, shifted by a quarter of a cell: room 0's walls
    lie at odd and even multiples of 1 cm, and a wall on the border between two cells would get whichever the depth's last bit says"""
    c = np.floor(p / period + 0.25).astype(np.int64).sum(axis=-1)
    return np.where(c & 1, 1, -1)


def patterned(rgb, depth_mm, pose, period):
    """the frame's colour with the checker of every pixel's world point laid over it (pixels without depth stay as they are)"""
    h, w = depth_mm.shape
    fx, fy, cx, cy = INTR
    z = depth_mm.astype(np.float64) * 0.001
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cam = np.stack([(i - cx) / fx * z, (j - cy) / fy * z, z], axis=-1)
    m = np.asarray(pose, np.float64).reshape(4, 4)
    world = cam @ m[:3, :3].T + m[:3, 3]
    out = rgb.astype(np.int64) + AMPLITUDE * checker_sign(world, period)[..., None]
    return np.where((depth_mm > 0)[..., None], np.clip(out, 0, 255), rgb).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--stride", type=int, default=2, help="every stride-th frame of the 720-frame scan")
    ap.add_argument("--cluster", type=int, default=8)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--checker", type=float, default=0.02)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--mode", type=int, default=0, help="0: HSK_KEYTEX_BEST, 1: HSK_KEYTEX_BLEND")
    ap.add_argument("--texels-per-metre", type=float, default=0.0, help="0: one texel per voxel")
    ap.add_argument("--out", default="keytex_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd import products
    os.makedirs(args.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, args.frames * args.stride, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])          # depth only: no colour volume
    ref = hsk.KinfuTracker(n=args.n, init_pose=poses[0])          # the same frames with colour, for hsk_bake_texture
    ref.enable_color()
    trk.enable_keyframes(args.cap)
    kept, lost = [], 0
    for i, p in enumerate(poses):
        d = hsk.synth_room_depth(0, p)
        c = patterned(hsk.synth_rgb(p, 0), d, p, args.checker)
        pose, ok = trk.process_frame(d)
        ref.process_frame_rgbd(d, c)
        lost += 0 if ok or i == 0 else 1
        if (ok or i == 0) and len(kept) < args.cap and hsk.keyframe_wanted(kept, pose):
            trk.add_keyframe(d, c, pose)                            # the tracker's pose, in the volume's frame
            kept.append(np.array(pose, np.float32).reshape(4, 4))
    kc = trk.keyframe_count()
    print(f"room 0 at {args.n}^3 without colour: {len(poses)} frames, {lost} lost, {kc['n']} keyframes kept of {kc['cap']} slots "
          f"({kc['bytes'] / 2**20:.1f} MiB; a colour volume would be {4 * args.n**3 / 2**20:.0f} MiB)")
    v, f, nrm, _, _ = trk.extract_mesh_simplified(cluster_voxels=args.cluster, normals=True, rgb=False)
    bk = trk.bake_texture_keyframes(v, f, atlas_width=args.width, texels_per_metre=args.texels_per_metre, mode=args.mode)
    rb = ref.bake_texture(v, f, atlas_width=args.width, texels_per_metre=args.texels_per_metre)
    trk.close()
    ref.close()
    products.write_ply_textured(os.path.join(args.out, "room_keytex.ply"), v, f, bk["uv"], "room_keytex_atlas.png", normals=nrm)
    products.write_png_rgb(os.path.join(args.out, "room_keytex_atlas.png"), bk["rgb"])
    products.write_png_rgb(os.path.join(args.out, "room_volume_atlas.png"), rb["rgb"])
    ip = hsk.TEXEL_INSIDE | hsk.TEXEL_PROJECTED
    inside = (bk["mask"] & ip) == ip
    keyed = (bk["mask"] & hsk.TEXEL_KEYFRAME) != 0
    print(f"simplified, c = {args.cluster}: {len(v)} vertices, {len(f)} faces -> {args.out}/room_keytex.ply")
    print(f"atlas {bk['width']} x {bk['height']}: owned {bk['n_owned']}, keyed {bk['n_keyed']}, uncoloured {bk['n_uncolored']}; "
          f"{100.0 * (keyed & inside).sum() / max(inside.sum(), 1):.1f} % of the {inside.sum()} inside-and-projected texels keyed; "
          f"pairs seen {bk['n_pairs_seen']} ({bk['n_pairs_seen'] / max(bk['n_owned'], 1):.2f} a texel), occluded {bk['n_pairs_occluded']} "
          f"-> {args.out}/room_keytex_atlas.png")
    both = keyed & inside & ((rb["mask"] & hsk.TEXEL_COLORED) != 0)
    idx = np.flatnonzero(both.reshape(-1))
    if len(idx) == 0:
        print("no texel is keyed and coloured by the volume: nothing to compare")
        return 0
    idx = np.random.default_rng(0).choice(idx, min(args.samples, len(idx)), replace=False)
    p, _, _ = texel_points(bk, v.astype(np.float64), f, idx)
    truth = np.array([hsk.synth_color_at(q, 0) for q in p], np.int64) + AMPLITUDE * checker_sign(p, args.checker)[:, None]
    truth = np.clip(truth, 0, 255).astype(np.float64)
    e_key = np.abs(bk["rgb"].reshape(-1, 3)[idx].astype(np.float64) - truth).mean()
    e_vol = np.abs(rb["rgb"].reshape(-1, 3)[idx].astype(np.float64) - truth).mean()
    flat = np.abs(np.array([hsk.synth_color_at(q, 0) for q in p], np.float64) - truth).mean()
    print(f"mean |colour error| per channel over {len(idx)} texels, against the synthetic colour with the {args.checker * 100:.0f} cm checker at the "
          f"texel's point on its face: keyframe atlas {e_key:.2f} levels, colour-volume atlas (hsk_bake_texture) {e_vol:.2f} levels, "
          f"the pattern left out altogether {flat:.2f} levels")
    return 0


if __name__ == "__main__":
    sys.exit(main())
