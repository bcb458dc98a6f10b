#!/usr/bin/env python3
"""Cloud normals: a room that exists only as a room directory's cloud_bin.pcd -- xyz and nothing else -- gets oriented normals, and
with them the better mode of every cloud call.

Room 0 is scanned (its scripted scan, every `--stride`-th frame), its cloud written as a room directory (products.write_room_dir)
and the context closed; its TSDF is kept on the host only to judge the results against.  The directory's cloud is read
(house.read_pcd_xyz) and its normals estimated (hsk_estimate_normals) with the import fan's standpoint, the room's middle, as the
viewpoint.  Then, for HSK_SPLAT_DISC and for HSK_SPLAT_SURFEL with the estimated normals: the cloud is imported into a fresh context
from the fan (hsk_import_cloud), the census printed, and the imported volume's surface points (hsk_extract_cloud) looked up in the
ORIGINAL volume's TSDF -- trilinear, in millimetres; their RMS says how far the imported surface lies from the scanned one.  Last,
the planes of the xyz-only cloud: hsk_detect_planes (host, unoriented) beside hsk_detect_planes_oriented with the estimated normals.

usage: python tools/normals_demo.py [--n 128] [--stride 12] [--n-rot 4] [--out normals_demo]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def census_line(c):
    return f"unseen {c['n_unseen']}, free {c['n_free']}, solid {c['n_solid']}, frontier {c['n_frontier']}"


def tsdf_mm(vol, cell, tau, xyz):
    """the volume's TSDF [Z, Y, X, 2] at the points, trilinear between voxel centres ((g + 0.5) cell), in millimetres; NaN where one
    of the eight voxels was never observed or lies outside"""
    g = xyz.astype(np.float64) / cell - 0.5
    g0 = np.floor(g).astype(np.int64)
    f = g - g0
    Z, Y, X, _ = vol.shape
    ok = ((g0 >= 0) & (g0 + 1 < np.array([X, Y, Z]))).all(axis=1)
    g0 = np.where(ok[:, None], g0, 0)
    out = np.zeros(len(xyz))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                v = vol[g0[:, 2] + dz, g0[:, 1] + dy, g0[:, 0] + dx]
                ok &= v[:, 1] != 0
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                out += w * v[:, 0].astype(np.float64) / 32767.0
    return np.where(ok, out * tau * 1000.0, np.nan)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--stride", type=int, default=12)
    ap.add_argument("--n-rot", type=int, default=4, help="the fan holds (2 n_rot + 1)^2 views")
    ap.add_argument("--out", default="normals_demo")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd import house as H
    from housescan_amd import products as P

    os.makedirs(args.out, exist_ok=True)
    n, cell = args.n, 3.0 / args.n
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 720, args.stride)]
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    cloud, _ = trk.extract_cloud()
    original, vol = trk.coverage(), trk.download_tsdf()
    tau = max(float(trk.cfg.trunc_dist_m), 2.1 * cell)
    room_dir = os.path.join(args.out, "room0")
    P.write_room_dir(room_dir, cloud, leaf=0.04, dist_thresh=0.025, min_fraction=0.03)
    trk.close()
    print(f"scanned: {len(poses)} frames at {n}^3, {len(cloud)} points -> {room_dir}; the context is closed")
    print(f"    original census: {census_line(original)}")

    e = hsk.synth_room_extents(0).astype(np.float64)
    centre = np.array(poses[0], np.float32).reshape(4, 4).copy()
    centre[:3, 3] = (0.5 * (e[0] + e[1]), 0.5 * (e[2] + e[3]), 0.5 * (e[4] + e[5]))
    fan = hsk.pose_lattice(centre, 0.0, 0, float(np.pi / (2 * args.n_rot + 1)), args.n_rot)
    xyz = H.read_pcd_xyz(os.path.join(room_dir, "cloud_bin.pcd"))
    new = hsk.KinfuTracker(n=n, init_pose=centre)
    nrm, curv, cnt, cls, st = new.estimate_normals(xyz, centre[:3, 3][None])
    radius = hsk.default_normal_params(new).radius_m
    new.close()
    print(f"normals of {len(xyz)} points, radius {radius * 1000:.1f} mm, viewpoint the room's middle: {st}")
    print(f"    neighbours {int(cnt.min())} .. {int(cnt.max())} (median {int(np.median(cnt))}), curvature median {float(np.median(curv[cls == 0])):.4f}")
    for mode, name, normals in ((hsk.SPLAT_DISC, "DISC", None), (hsk.SPLAT_SURFEL, "SURFEL with the estimated normals", nrm)):
        t = hsk.KinfuTracker(n=n, init_pose=centre)
        stats = t.import_cloud(xyz, fan, normals, mode=mode, point_size_m=cell, max_half_px=32.0)
        back, _ = t.extract_cloud()
        d = tsdf_mm(vol, cell, tau, back)
        seen = ~np.isnan(d)
        print(f"import, {name}: {int(stats['n_splatted'].sum())} point views, {int(stats['n_backfacing'].sum())} back-facing")
        print(f"    census: {census_line(t.coverage())}")
        print(f"    {len(back)} surface points, {int(seen.sum())} inside the original's observed space: the original's TSDF there has RMS "
              f"{float(np.sqrt(np.mean(d[seen] ** 2))):.2f} mm, mean {float(d[seen].mean()):+.2f} mm")
        if normals is not None:
            recs, labels, bad = t.detect_planes_cloud(xyz, normals)
            print(f"planes of the xyz-only cloud, hsk_detect_planes_oriented with the estimated normals: {len(recs)} planes, "
                  f"{int((labels >= 0).sum())} of {len(xyz)} points labelled, {bad} invalid; inliers {[int(r['n_inliers']) for r in recs]}")
        t.close()
    planes, labels = P.detect_planes(xyz)
    print(f"planes of the xyz-only cloud, hsk_detect_planes (host, unoriented): {len(planes)} planes, {int((labels >= 0).sum())} points labelled; "
          f"inliers {[int((labels == i).sum()) for i in range(len(planes))]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
