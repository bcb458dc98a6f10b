#!/usr/bin/env python3
"""Pictures of a scan, for a person to look at: room 0 scanned with colour (256^3, 150 frames), then
  follow.ppm            what the sensor's camera sees of the model at the tracker's pose (Lambert)
  orbit_NN_<mode>.ppm   a free 1280 x 960 camera on a circle round the room's centre, looking at it, in all four modes
  depth.pgm             the depth image (16-bit millimetres) of the follow view
  floorplan.ppm / floorplan_heights.pgm   the room from above, orthographic, the ceiling side cut away at mid height: wall outlines
                        in the cut colour, and the depth image as a height map (hsk_render_section)
  elevation.ppm         the far wall seen square on, orthographic, the near half of the room cut away
  dollhouse.ppm         a pinhole camera obliquely above the room, the ceiling side cut away

usage: python tools/view_demo.py [--out view_demo_out] [--n 256] [--frames 150] [--orbit 8]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import housescan_amd as hsk  # noqa: E402
from housescan_amd import _lib, products  # noqa: E402

MODES = (("lambert", _lib.HSK_VIEW_LAMBERT), ("normals", _lib.HSK_VIEW_NORMALS), ("color", _lib.HSK_VIEW_COLOR),
         ("color_lit", _lib.HSK_VIEW_COLOR_LIT))


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """cam->world pose of a camera at `eye` whose z axis points at `target` (y down, as the sensor's)"""
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(-np.asarray(up, np.float64), z)
    x /= np.linalg.norm(x)
    p = np.eye(4, dtype=np.float32)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = x, np.cross(z, x), z, eye
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="view_demo_out")
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--orbit", type=int, default=8)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(a.frames)]
    trk = hsk.KinfuTracker(n=a.n, init_pose=poses[0])
    trk.enable_color()
    for k, p in enumerate(poses):
        trk.submit_frame_rgbd(hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0))
        if k >= 1:
            trk.wait_frame()
    trk.wait_frame()
    r = trk.render_view()
    products.write_ppm(os.path.join(a.out, "follow.ppm"), r["rgb"])
    products.write_pgm16(os.path.join(a.out, "depth.pgm"), r["depth"])
    print(f"follow: {r['n_hit']} of {r['rgb'].shape[0] * r['rgb'].shape[1]} pixels hit")
    e = hsk.synth_room_extents(0)
    centre = np.array([(e[0] + e[1]) / 2, (e[2] + e[3]) / 2, (e[4] + e[5]) / 2])
    radius = 0.35 * min(e[1] - e[0], e[5] - e[4])
    for i in range(a.orbit):
        ang = 2 * np.pi * i / a.orbit
        eye = centre + radius * np.array([np.cos(ang), 0.0, np.sin(ang)])
        pose = look_at(eye, centre)
        for name, mode in MODES:
            r = trk.render_view(pose=pose, mode=mode, width=1280, height=960, fx=700.0, fy=700.0, cx=639.5, cy=479.5, depth=False)
            products.write_ppm(os.path.join(a.out, f"orbit_{i:02d}_{name}.ppm"), r["rgb"])
    # sections: the whole scan is needed for these (the first 150 frames have not looked at floor or ceiling), so what is there is shown
    x0, x1, y0, y1, z0, z1 = (float(v) for v in e)
    y_cut = 0.5 * (y0 + y1)
    sun = dict(light=(0.3, -1.0, 0.2), light_in_camera=0, light_directional=1, background=(255, 255, 255))
    mode = _lib.HSK_VIEW_COLOR_LIT
    ortho = dict(projection=_lib.HSK_PROJ_ORTHO, width=1024, height=1024, fx=320.0, fy=320.0, cx=511.5, cy=511.5)   # 3.2 m across
    above = look_at(np.array([centre[0], -0.5, centre[2]]), np.array([centre[0], 0.5, centre[2]]), up=(0.0, 0.0, -1.0))
    r = trk.render_section(pose=above, clip=[(0, 1, 0, -y_cut)], mode=mode, **ortho, **sun)
    products.write_ppm(os.path.join(a.out, "floorplan.ppm"), r["rgb"])
    products.write_pgm16(os.path.join(a.out, "floorplan_heights.pgm"), r["depth"])
    print(f"floor plan: {r['n_hit']} hits, {r['n_cut']} cut pixels")
    front = look_at(np.array([centre[0], centre[1], -0.5]), np.array([centre[0], centre[1], 1.0]))
    r = trk.render_section(pose=front, clip=[(0, 0, 1, -centre[2])], mode=mode, depth=False, **ortho, **sun)
    products.write_ppm(os.path.join(a.out, "elevation.ppm"), r["rgb"])
    print(f"elevation: {r['n_hit']} hits, {r['n_cut']} cut pixels")
    eye = np.array([centre[0] - 2.6, y0 - 2.0, centre[2] - 2.6])
    r = trk.render_section(pose=look_at(eye, centre), clip=[(0, 1, 0, -(y0 + 0.4 * (y1 - y0)))], mode=mode, depth=False, width=1280,
                           height=960, fx=1100.0, fy=1100.0, cx=639.5, cy=479.5, **sun)
    products.write_ppm(os.path.join(a.out, "dollhouse.ppm"), r["rgb"])
    print(f"dollhouse: {r['n_hit']} hits, {r['n_cut']} cut pixels")
    trk.close()
    print("written to", a.out)


if __name__ == "__main__":
    main()
