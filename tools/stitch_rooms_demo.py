#!/usr/bin/env python3
"""End to end on one MI355X: scan closed synthetic rooms with the KinFu core, write the room directories HouseScan
loads, run the host-side stitching chain on them and export one .xf per room plus the stitched cloud as .ply.

  python tools/stitch_rooms_demo.py --rooms 2 --volume 256 --frames 720 --out gpurun_out/stitch

This is BASELINE configs[0] (two rooms -> cuboid fit + translation optimiser -> export) fed by configs[2]-style
scans; with --rooms 4 it is the single-GPU form of configs[4].  The "user" who clicks corners in HouseScan is
emulated: of the suggested corners, the 8 nearest to the true room corners are accepted.

--indexed-mesh: each room's mesh comes off the GPU indexed, with normals (hsk_extract_mesh_indexed), is written as
<room_dir>/mesh.ply, and house_mesh.ply concatenates the rooms' meshes moved by their .xf (positions by transform_cloud,
normals by transform_normals, faces offset by each room's vertex base) -- no host weld.

--floorplan: behind the stitch, one top-down orthographic section of the whole house, cut at mid height, is taken into every
room's frame by its .xf (hsk_section_in_room), rendered from the room's volume on the GPU (hsk_render_section) and the rooms'
images are composited (hsk_composite_views): house_floorplan.ppm (walls as outlines in the cut colour) and house_heights.pgm
(16-bit millimetres below the camera's plane: a height map).

--fuse-house: behind the stitch, ONE house volume is made on the GPU -- a context sized to the placed rooms' extents at the
rooms' cell -- and every room's volume is fused into it by T_offset . xf (hsk_fuse_volume; T_offset moves the house into the
context's positive octant).  house_fused_mesh.ply is one hsk_extract_mesh_indexed of that volume (in house coordinates: where
rooms overlap there is one surface, not two), house_fused_floorplan.ppm one hsk_render_section of it (--floorplan's camera);
report.json gets a "fused_house" block with the statistics of every fuse and the milliseconds.

--simplify C (with --fuse-house): the fused house's mesh once more, reduced on the GPU by quadric vertex clustering on cells of C
voxels (2, 4, 8 or 16; hsk_extract_mesh_simplified), as house_fused_mesh_simplified.ply; the "fused_house" block gets its counts,
statistics and milliseconds beside the full-resolution mesh's.

--refine (with --fuse-house): every room after the first is first registered against the house volume fused so far, starting
from its stitched .xf (hsk_align_volume: the room's cloud and normals against the house's TSDF), and fused by the refined matrix,
which is written as <room>.refined.xf; both matrices and every iteration's n_used / rms are printed.  A registration that does
not end CONVERGED keeps the stitched matrix.

--device-planes: each room's planes are detected on the GPU from its volume's own cloud and normals (hsk_detect_planes_volume:
oriented, on every point, the cloud never leaves the device for it) instead of by the host RANSAC on the downsampled cloud;
write_room_dir takes them with their labels, planes.txt and the hulls come from the labelled full-resolution points.

--save-volumes: behind each scan the room's volume is written to <room dir>/volume.hskv (hsk_save_volume: a sparse image packed
on the GPU) and the room's context is closed.  --floorplan and --fuse-house then load one room at a time from its file into a
single scratch context (hsk_load_volume), so at most two contexts are alive at once however many rooms the house has.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scan_room(hsk, variant, n, frames, device_id=0, with_mesh=False, indexed=False, keep=False, planes_out=None):
    """the three-turn scan inside room `variant`; returns (cloud, worst translation error [m], lost frames, fps).
    (Round 6: the frames go through the pipelined pair and the clock covers the tracker only -- the poses and the errors are
    computed outside it; the synchronous call with a pose and a norm per frame inside the loop made "2050 frames/s" of a
    scan that runs at 4900.)"""
    gts = [hsk.synth_room_pose(variant, k, frames) for k in range(frames + 1)]
    trk = hsk.KinfuTracker(n=n, init_pose=gts[0], device_id=device_id)
    with ThreadPoolExecutor(8) as ex:   # (the renderer releases the GIL)
        depth = list(ex.map(lambda p: hsk.synth_room_depth(variant, p), gts))
    got = []
    t0 = time.perf_counter()
    trk.submit_frame(depth[0])
    for d in depth[1:]:
        trk.submit_frame(d)
        got.append(trk.wait_frame())
    got.append(trk.wait_frame())
    trk.synchronize()
    dt = time.perf_counter() - t0
    lost = sum(1 for k, (_, ok) in enumerate(got) if k > 0 and not ok)   # frame 0 only seeds the model
    worst = max(float(np.linalg.norm(pose[:3, 3] - gt[:3, 3])) for (pose, _), gt in zip(got, gts))
    cloud, total = trk.extract_cloud()
    if planes_out is not None:   # (--device-planes: the labels are in this cloud's order)
        t1 = time.perf_counter()
        rec, labels = trk.detect_planes(dist_m=0.025, min_fraction=0.03)
        planes_out.append((rec, labels, 1e3 * (time.perf_counter() - t1)))
    if with_mesh and indexed:
        mesh = trk.extract_mesh_indexed(normals=True, rgb=False)[:3]   # (vertices, faces, normals)
    else:
        mesh = trk.extract_mesh(cubes=True)[0] if with_mesh else None   # marching cubes: the form upstream's .ply export has
    if keep:   # (the volume stays on the device for --floorplan; the caller closes the tracker)
        return cloud, worst, lost, len(depth) / dt, mesh, trk
    trk.close()
    if with_mesh:
        return cloud, worst, lost, len(depth) / dt, mesh
    return cloud, worst, lost, len(depth) / dt


class RoomVolumes:
    """the rooms' volumes for what follows the stitch, in room order: the scans' own contexts, or (--save-volumes) their
    volume files, loaded one at a time into a single scratch context when they are iterated over"""

    def __init__(self, hsk):
        self.hsk, self.items, self.scratch = hsk, [], None

    def add(self, item):            # a KinfuTracker, or the path of a volume file
        self.items.append(item)

    def __iter__(self):
        for item in self.items:
            if not isinstance(item, str):
                yield item
            elif self.scratch is None:
                self.scratch = self.hsk.KinfuTracker.from_volume_file(item)
                yield self.scratch
            else:
                self.scratch.load_volume(item)
                yield self.scratch

    def close(self):
        for item in self.items + [self.scratch]:
            if item is not None and not isinstance(item, str):
                item.close()


def true_corners(extents):
    x0, x1, y0, y1, z0, z1 = [float(v) for v in extents]
    return np.array([[x, y, z] for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)], np.float64)


def stitch(hsk, room_dirs, variants, log=print):
    from housescan_amd import house as H
    hs = H.House()
    rooms = []
    for d, v in zip(room_dirs, variants):
        rid = hs.loadRoom(d)
        hs.rotateKinfuRoom(rid)
        hs.autoAlignFloor(rid)
        n, adopted = hs.suggestPoints(rid)
        if not adopted:
            # the user's clicks: accept the suggestion nearest to each true corner
            M = hs.room_projection(rid).astype(np.float64)
            want = true_corners(hsk.synth_room_extents(v)) @ M[:3, :3].T + M[:3, 3]
            ids, xyz = hs.room_corners(rid, suggested=True)
            picked = []
            for c in want:
                k = int(np.argmin(np.linalg.norm(xyz - c, axis=1)))
                if ids[k] not in picked:
                    picked.append(ids[k])
                    hs.acceptCornerSuggestion(rid, ids[k])
        p, steps, rmse = hs.fitCuboidToRoom(rid)
        log(f"room {rid} ({os.path.basename(os.path.dirname(d))}): {n} corner suggestions, cuboid {np.round(np.abs(p[3:6]), 3)} "
            f"in {steps} steps, RMSE {rmse:.4f}")
        rooms.append(rid)

    def wall(room, axis, sign):
        ids, _ = hs.room_planes(room)
        return max(ids, key=lambda q: sign * hs.plane_bounds(q).mean(axis=0)[axis])

    # a row of rooms along x: shared walls 10 cm thick, floors level, the low-z walls flush
    for a, b in zip(rooms[:-1], rooms[1:]):
        hs.connectWalls(wall(a, 0, +1), wall(b, 0, -1), H.OPPOSITE, 0.1)
        hs.connectWalls(wall(a, 1, -1), wall(b, 1, -1), H.SAME)
        hs.connectWalls(wall(a, 2, -1), wall(b, 2, -1), H.SAME)
    rm = hs.optimizeRoomPositions()
    log(f"placement RMSE per axis: {rm}")
    return hs, rooms, rm


def house_section(hsk, variants, Ms, px_per_m):
    """the top-down orthographic section of the whole house, cut at mid height, in house coordinates -> (section, W, H)"""
    from housescan_amd import _lib
    Ms = [np.asarray(M, np.float64) for M in Ms]
    corners = np.concatenate([true_corners(hsk.synth_room_extents(v)) @ M[:3, :3].T + M[:3, 3] for v, M in zip(variants, Ms)])
    up = Ms[0][:3, :3] @ np.array([0.0, -1.0, 0.0])          # a scan's y axis points down
    up /= np.linalg.norm(up)
    z = -up
    x = np.eye(3)[int(np.argmin(np.abs(up)))]
    x = x - (x @ z) * z
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    u, v, h = corners @ x, corners @ y, corners @ up
    margin = 0.2
    W = min(4096, int(np.ceil((u.max() - u.min() + 2 * margin) * px_per_m)))
    H = min(4096, int(np.ceil((v.max() - v.min() + 2 * margin) * px_per_m)))
    eye = 0.5 * (u.max() + u.min()) * x + 0.5 * (v.max() + v.min()) * y + (h.max() + 0.5) * up
    house = _lib.HskSection()
    _lib.load().hsk_default_section(None, house)
    hv = house.view
    hv.width, hv.height, hv.fx, hv.fy, hv.cx, hv.cy = W, H, px_per_m, px_per_m, (W - 1) / 2.0, (H - 1) / 2.0
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    hv.pose[:] = [float(a) for a in pose.astype(np.float32).reshape(16)]
    hv.follow, hv.mode, hv.light_in_camera = 0, _lib.HSK_VIEW_LAMBERT, 0
    light = up + 0.3 * x + 0.2 * y
    hv.light[:] = [float(a) for a in light]
    hv.background[:] = [255, 255, 255]
    house.projection, house.light_directional, house.n_clip = _lib.HSK_PROJ_ORTHO, 1, 1
    mid = 0.5 * (h.max() + h.min())
    house.clip[0][:] = [float(-up[0]), float(-up[1]), float(-up[2]), float(mid)]     # keep what lies below mid height
    return house, W, H


def floorplan(hsk, trackers, variants, Ms, out, px_per_m=100.0):
    """the house from above: one section in house coordinates, each room's share rendered in the room's own frame"""
    from housescan_amd import products as P
    t0 = time.perf_counter()
    house, W, H = house_section(hsk, variants, Ms, px_per_m)
    Ms = [np.asarray(M, np.float64) for M in Ms]
    rgbs, deps, counts = [], [], []
    for trk, M in zip(trackers, Ms):
        r = trk.render_section(P.section_in_room(house, M.astype(np.float32)))
        rgbs.append(r["rgb"])
        deps.append(r["depth"])
        counts.append({"hit": r["n_hit"], "cut": r["n_cut"]})
    rgb, dep, idx = P.composite_views(rgbs, deps, (255, 255, 255))
    ms = 1e3 * (time.perf_counter() - t0)
    P.write_ppm(os.path.join(out, "house_floorplan.ppm"), rgb)
    P.write_pgm16(os.path.join(out, "house_heights.pgm"), dep)
    return {"width": W, "height": H, "px_per_m": px_per_m, "rooms": counts, "pixels_per_room": [int((idx == i).sum()) for i in range(len(Ms))],
            "end_to_end_ms": round(ms, 2)}


def fuse_house(hsk, trackers, variants, Ms, out, volume, px_per_m=100.0, margin=0.25, refine=False, simplify=0):
    """one house volume on the GPU: every room fused into it by its .xf (with `refine`: by the .xf registered against the house
    so far); one mesh and one floor plan of the whole"""
    from housescan_amd import products as P
    Ms = [np.asarray(M, np.float64) for M in Ms]
    cell = 3.0 / volume                                       # the rooms' cell (a room's context is volume^3 over 3 m)
    corners = np.concatenate([true_corners(hsk.synth_room_extents(v)) @ M[:3, :3].T + M[:3, 3] for v, M in zip(variants, Ms)])
    lo, hi = corners.min(axis=0) - margin, corners.max(axis=0) + margin
    dims = [int(-(-(hi[i] - lo[i]) // (64 * cell))) * 64 for i in range(3)]   # (multiples of 64: the brick bitfield's rule)
    size = [d * cell for d in dims]
    T = np.eye(4)
    T[:3, 3] = -lo
    t0 = time.perf_counter()
    house = hsk.KinfuTracker(hsk.default_config(dims[2], vol_x=dims[0], vol_y=dims[1], vol_z=dims[2], vol_size_m=size))
    make_ms = 1e3 * (time.perf_counter() - t0)
    rooms = []
    for i, (trk, M) in enumerate(zip(trackers, Ms)):
        m = (T @ M).astype(np.float32)
        align = None
        if refine and i > 0:
            t0 = time.perf_counter()
            m_ref, a = house.align_from(trk, m)
            align = {"status": a["status"], "iterations": a["iterations"], "n_points": a["n_points"], "stride": a["stride"],
                     "n_used": a["n_used"], "rms_mm": [round(1e3 * float(v), 4) for v in a["rms_m"]],
                     "ms": round(1e3 * (time.perf_counter() - t0), 3)}
            xf = (np.linalg.inv(T) @ m_ref.astype(np.float64)).astype(np.float32)       # room -> house, as the stitched .xf is
            print(f"room{variants[i]}: stitched .xf\n{M.astype(np.float32)}\nrefined ({a['status']}, {a['iterations']} iterations)\n{xf}")
            for k, (nu, rms) in enumerate(zip(a["n_used"], a["rms_m"])):
                print(f"  iteration {k}: n_used {nu} of {a['n_points']}, rms {1e3 * float(rms):.3f} mm")
            if a["status"] == "converged":
                m = m_ref
                P.write_xf(os.path.join(out, f"room{variants[i]}.refined.xf"), xf)
            else:
                print(f"room{variants[i]}: the registration ended {a['status']}: the stitched matrix is kept")
            align["used"] = a["status"] == "converged"
        t0 = time.perf_counter()
        st = house.fuse_from(trk, m)
        st["ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        if align is not None:
            st["align"] = align
        st["box"] = list(st["box"])
        rooms.append(st)
    t0 = time.perf_counter()
    verts, faces, normals, _, _ = house.extract_mesh_indexed(normals=True, rgb=False)
    mesh_ms = 1e3 * (time.perf_counter() - t0)
    P.write_ply_indexed(os.path.join(out, "house_fused_mesh.ply"), P.transform_cloud(verts, np.linalg.inv(T).astype(np.float32)), faces,
                        normals=normals)
    simplified = None
    if simplify:
        t0 = time.perf_counter()
        sv, sf, sn, _, st = house.extract_mesh_simplified(cluster_voxels=simplify, normals=True, rgb=False)
        simplified = {"cluster_voxels": simplify, "vertices": int(len(sv)), "faces": int(len(sf)), "ms": round(1e3 * (time.perf_counter() - t0), 2), "stats": st}
        P.write_ply_indexed(os.path.join(out, "house_fused_mesh_simplified.ply"), P.transform_cloud(sv, np.linalg.inv(T).astype(np.float32)), sf, normals=sn)
        print(f"fused house: {len(verts)} vertices, {len(faces)} faces; simplified at c = {simplify}: {len(sv)} vertices, {len(sf)} faces")
    t0 = time.perf_counter()
    sec, W, H = house_section(hsk, variants, Ms, px_per_m)
    r = house.render_section(P.section_in_room(sec, np.linalg.inv(T).astype(np.float32)), depth=False)   # (the context sits at T^-1 in the house)
    plan_ms = 1e3 * (time.perf_counter() - t0)
    P.write_ppm(os.path.join(out, "house_fused_floorplan.ppm"), r["rgb"])
    house.close()
    return {"dims": dims, "size_m": [round(x, 6) for x in size], "rooms": rooms, "create_ms": round(make_ms, 2),
            "mesh": {"vertices": int(len(verts)), "faces": int(len(faces)), "ms": round(mesh_ms, 2)}, "mesh_simplified": simplified,
            "floorplan": {"width": W, "height": H, "hit": r["n_hit"], "cut": r["n_cut"], "ms": round(plan_ms, 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=2)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--frames", type=int, default=720, help="frames of the three-turn room trajectory")
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "stitch"))
    ap.add_argument("--indexed-mesh", action="store_true", help="rooms' meshes indexed with normals: <room_dir>/mesh.ply, no host weld")
    ap.add_argument("--floorplan", action="store_true", help="house_floorplan.ppm + house_heights.pgm: a top-down section of the stitched house")
    ap.add_argument("--fuse-house", action="store_true", help="house_fused_mesh.ply + house_fused_floorplan.ppm: the rooms' volumes fused into one house volume on the GPU")
    ap.add_argument("--refine", action="store_true", help="with --fuse-house: register every room after the first against the house fused so far (<room>.refined.xf)")
    ap.add_argument("--simplify", type=int, default=0, choices=(0, 2, 4, 8, 16), metavar="C",
                    help="with --fuse-house: house_fused_mesh_simplified.ply, the fused house's mesh clustered on cells of C voxels on the GPU")
    ap.add_argument("--device-planes", action="store_true", help="the rooms' planes from hsk_detect_planes_volume (oriented, on the GPU) instead of the host RANSAC")
    ap.add_argument("--save-volumes", action="store_true", help="<room dir>/volume.hskv behind each scan, the room's context closed; --floorplan / --fuse-house load them one at a time")
    args = ap.parse_args()

    import housescan_amd as hsk
    from housescan_amd import house as H
    from housescan_amd import products as P

    os.makedirs(args.out, exist_ok=True)
    report = {"rooms": []}
    dirs, variants, meshes, trackers = [], list(range(args.rooms)), [], RoomVolumes(hsk)
    for v in variants:
        found = [] if args.device_planes else None
        res = scan_room(hsk, v, args.volume, args.frames, with_mesh=True, indexed=args.indexed_mesh,
                        keep=args.floorplan or args.fuse_house or args.save_volumes, planes_out=found)
        cloud, worst, lost, fps, mesh = res[:5]
        if args.save_volumes:
            os.makedirs(os.path.join(args.out, f"room{v}"), exist_ok=True)
            path = os.path.join(args.out, f"room{v}", "volume.hskv")
            t0 = time.perf_counter()
            info = res[5].save_volume(path)
            res[5].close()
            trackers.add(path)
            report.setdefault("volumes", []).append({"path": os.path.relpath(path, args.out), "bytes": int(info["total_bytes"]),
                                                     "share_of_raw": info["total_bytes"] / (4.0 * args.volume ** 3),
                                                     "tsdf_bricks": [int(x) for x in info["tsdf_bricks"]],
                                                     "save_ms": round(1e3 * (time.perf_counter() - t0), 2)})
        elif args.floorplan or args.fuse_house:
            trackers.add(res[5])
        meshes.append(mesh)
        d = os.path.join(args.out, f"room{v}", "walls")
        if args.device_planes:
            rec, labels, ms = found[0]
            planes, n_down = P.write_room_dir(d, cloud, leaf=0.04, planes=(rec["abcd"], labels, cloud))
            resid = [float(r["sum_abs"]) / 65536.0 / max(1, int(r["n_inliers"])) * 1e3 for r in rec]
            print(f"room{v}: {len(rec)} planes on the device in {ms:.1f} ms, {int((labels >= 0).sum())} of {len(labels)} points on them, "
                  f"mean residuals {[round(x, 2) for x in resid]} mm")
        else:
            planes, n_down = P.write_room_dir(d, cloud, leaf=0.04, dist_thresh=0.025, min_fraction=0.03)
        if args.indexed_mesh:
            P.write_ply_indexed(os.path.join(d, "mesh.ply"), mesh[0], mesh[1], normals=mesh[2])
        print(f"room{v}: {len(cloud)} points, {n_down} downsampled, {len(planes)} planes, worst pose error {worst * 1000:.1f} mm, "
              f"lost {lost}, {fps:.0f} frames/s incl. upload")
        report["rooms"].append({"variant": v, "points": int(len(cloud)), "planes": int(len(planes)), "worst_pose_error_mm": worst * 1000,
                                "lost": int(lost), "fps_host_frames": fps})
        dirs.append(d)
    hs, rooms, rm = stitch(hsk, dirs, variants)
    merged = []
    for rid, d in zip(rooms, dirs):
        M = hs.room_projection(rid)
        base = os.path.basename(os.path.dirname(d))
        with open(os.path.join(args.out, base + ".xf"), "w") as f:
            f.write(hs.roomProjectionToXfFormat(rid))
        full = H.read_pcd_xyz(os.path.join(os.path.dirname(d), "walls", "cloud_bin.pcd"))
        merged.append(P.transform_cloud(full, M))
        print(f"{base}: pcl_transform_point_cloud -matrix {hs.roomProjectionToString(rid)}")
    merged = np.concatenate(merged)
    H.write_ply_points(os.path.join(args.out, "house.ply"), merged)
    # the README's last step (plyxform on KinFu's mesh): every room's mesh moved by its .xf, one welded .ply
    if args.indexed_mesh:
        vs, fs, ns, base = [], [], [], 0
        for (v, f, nrm), rid in zip(meshes, rooms):
            M = hs.room_projection(rid)
            vs.append(P.transform_cloud(v, M))
            ns.append(P.transform_normals(nrm, M))
            fs.append(f + base)
            base += len(v)
        P.write_ply_indexed(os.path.join(args.out, "house_mesh.ply"), np.concatenate(vs), np.concatenate(fs), normals=np.concatenate(ns))
        nv, nf = base, sum(len(f) for f in fs)
    else:
        moved = [P.transform_cloud(m.reshape(-1, 3), hs.room_projection(rid)).reshape(-1, 3, 3) for m, rid in zip(meshes, rooms)]
        nv, nf = P.write_ply_mesh(os.path.join(args.out, "house_mesh.ply"), np.concatenate(moved))
    report["house_mesh"] = {"vertices": nv, "faces": nf}
    if args.floorplan:
        report["floorplan"] = floorplan(hsk, trackers, variants, [hs.room_projection(rid) for rid in rooms], args.out)
    if args.fuse_house:
        report["fused_house"] = fuse_house(hsk, trackers, variants, [hs.room_projection(rid) for rid in rooms], args.out, args.volume,
                                            refine=args.refine, simplify=args.simplify)
    trackers.close()
    report["placement_rmse"] = [None if np.isnan(x) else float(x) for x in rm]
    report["house_points"] = int(len(merged))
    with open(os.path.join(args.out, "report.json"), "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
