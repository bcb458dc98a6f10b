#!/usr/bin/env python3
"""Volume differencing on a room scanned twice: what changed, and a merge without ghosts (hsk_diff_volume, hsk_adopt_diff).

Room 0 is scanned twice with the tracker's own poses and the sensor model's noise (hsk_synth_render_sensor, two seeds); for the
second scan a box is composited into every depth frame (min(depth, the box's depth along the pixel's ray)).  The second volume
is registered against the first (hsk_align_volume), resampled onto its grid (hsk_fuse_volume into an empty context) and diffed.
Printed: the kept regions in metres, the kept and MINOR regions away from the box (the false changes of a noisy pair), the
second scan's mesh with changed vertices tinted (APPEARED orange, VANISHED blue; written as .ply), and the merge of both scans
by plain hsk_fuse_volume -- the box at half weight: a ghost -- beside adopt-then-fuse, each measured against the second scan on
the voxels of the box's shell.

usage: python tools/diff_demo.py [--n 256] [--stride 3] [--poses tracker|script] [--out diff_demo]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BOX = ((0.9, 2.1, 0.8), (1.3, 2.65, 1.2))      # free floor between the cupboard and the wardrobe of room 0, 5 cm above the floor


def scan(hsk, args, seed, box):
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 720, args.stride)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    lost = 0
    for p in poses:
        d, _ = hsk.synth_sensor_depth(p, scene=0, seed=seed)
        if box is not None:
            d = hsk.synth_box_depth(d, p, *box)
        if args.poses == "tracker":
            lost += 0 if trk.process_frame(d)[1] else 1
        else:
            trk.integrate(d, p)
    return trk, lost, len(poses)


def away_from(lo, hi, vlo, vhi, margin):
    return any(hi[i] <= vlo[i] - margin or lo[i] >= vhi[i] + margin for i in range(3))


def shell_error(vol, cur, shell):
    """mean |raw difference| in units of the truncation distance, and the voxels not observed, over the shell cur observed"""
    seen = vol[..., 1][shell] != 0
    d = np.abs(vol[..., 0][shell].astype(np.int64) - cur[..., 0][shell].astype(np.int64))[seen]
    return round(float(d.mean()) / 32767.0, 4) if seen.any() else None, int((~seen).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--stride", type=int, default=3)
    ap.add_argument("--poses", default="tracker", choices=("tracker", "script"))
    ap.add_argument("--out", default="diff_demo")
    ap.add_argument("--json", default="", help="also write the figures to this file")
    args = ap.parse_args()
    import housescan_amd as hsk
    from housescan_amd.products import write_ply_indexed
    from scipy import ndimage

    os.makedirs(args.out, exist_ok=True)
    cell = 3.0 / args.n
    ref, lost_a, n_frames = scan(hsk, args, 1234, None)
    cur, lost_b, _ = scan(hsk, args, 4321, BOX)
    print(f"two scans of room 0 at {args.n}^3, {n_frames} frames each, poses: {args.poses}; frames lost: {lost_a}, {lost_b}")
    m, ast = ref.align_from(cur, np.eye(4, dtype=np.float32))
    rms = float(ast["rms_m"][-1]) if len(ast["rms_m"]) else float("nan")
    if ast["status"] != "converged":
        m = np.eye(4, dtype=np.float32)              # (do not trust the matrix: both scans started from the same pose)
    print(f"hsk_align_volume: {ast['status']}, {ast['iterations']} iterations, rms {rms * 1000:.2f} mm, shift {np.linalg.norm(m[:3, 3]) * 1000:.2f} mm")
    res = cur.resampled_like(ref, m)
    recs, st = ref.diff_volume(res)
    vlo = tuple(int(np.floor(BOX[0][i] / cell)) for i in range(3))
    vhi = tuple(int(np.ceil(BOX[1][i] / cell)) for i in range(3))
    margin = 4                                   # voxels: the truncation band about the box at the default 3 cm
    print(f"hsk_diff_volume, defaults {dict((k, int(getattr(ref.default_diff_params(), k))) for k in hsk.kinfu.DIFF_FIELDS)}: "
          f"classes {st['n_class'].tolist()}, {st['n_regions']} kept regions, {st['n_minor_regions']} MINOR regions")
    print(f"the composited box: {BOX[0]} .. {BOX[1]} m, voxels {vlo} .. {vhi}")
    false_kept = []
    for c in recs:
        lo, hi = tuple(int(v) for v in c["lo"]), tuple(int(v) for v in c["hi"])
        away = away_from(lo, hi, vlo, vhi, margin)
        false_kept += [int(c["n_voxels"])] if away else []
        print(f"  region at {tuple(round(v * cell, 3) for v in lo)} .. {tuple(round(v * cell, 3) for v in hi)} m: {int(c['n_voxels'])} voxels "
              f"({int(c['n_appeared'])} appeared, {int(c['n_vanished'])} vanished){' -- AWAY FROM THE BOX' if away else ''}")
    cls, _ = ref.download_diff(region=False)
    minor = cls == hsk.DIFF_MINOR
    near = np.zeros_like(minor)
    near[max(vlo[2] - margin, 0):vhi[2] + margin, max(vlo[1] - margin, 0):vhi[1] + margin, max(vlo[0] - margin, 0):vhi[0] + margin] = True
    lab, n_lab = ndimage.label(minor)
    minor_away = int(n_lab - len(np.unique(lab[near & minor])))
    print(f"false changes away from the box: {len(false_kept)} kept regions {false_kept}, {minor_away} MINOR regions ({int((minor & ~near).sum())} voxels)")
    # the second scan's mesh, changed vertices tinted
    v, f, nrm = res.extract_mesh_indexed(rgb=False)[:3]
    vc, _ = ref.diff_at(v, radius=1)
    rgb = np.full((len(v), 3), 190, np.uint8)
    rgb[vc == hsk.DIFF_APPEARED] = (255, 128, 0)
    rgb[vc == hsk.DIFF_VANISHED] = (40, 90, 255)
    write_ply_indexed(os.path.join(args.out, "second_scan_tinted.ply"), v, f, nrm, rgb)
    print(f"second scan's mesh: {len(f)} faces, {int((vc == hsk.DIFF_APPEARED).sum())} vertices tinted appeared, {int((vc == hsk.DIFF_VANISHED).sum())} vanished")
    # plain fuse beside adopt-then-fuse, against the second scan on the box's shell
    cur_vol, ref_vol = res.download_tsdf(), ref.download_tsdf()
    box_mask = np.zeros(cls.shape, bool)
    box_mask[max(vlo[2] - 2, 0):vhi[2] + 2, max(vlo[1] - 2, 0):vhi[1] + 2, max(vlo[0] - 2, 0):vhi[0] + 2] = True
    shell = box_mask & (cur_vol[..., 1] != 0) & (np.abs(cur_vol[..., 0].astype(np.int32)) < 32767)
    plain = hsk.KinfuTracker(ref.cfg)
    plain.upload_tsdf(ref_vol)
    plain.fuse_from(res, np.eye(4, dtype=np.float32))
    v_p, f_p, n_p = plain.extract_mesh_indexed(rgb=False)[:3]
    write_ply_indexed(os.path.join(args.out, "plain_fuse.ply"), v_p, f_p, n_p)
    err_plain = shell_error(plain.download_tsdf(), cur_vol, shell)
    adopt = ref.adopt_diff(res)
    ref.fuse_from(res, np.eye(4, dtype=np.float32))
    v_a, f_a, n_a = ref.extract_mesh_indexed(rgb=False)[:3]
    write_ply_indexed(os.path.join(args.out, "adopt_then_fuse.ply"), v_a, f_a, n_a)
    err_adopt = shell_error(ref.download_tsdf(), cur_vol, shell)
    print(f"hsk_adopt_diff: {adopt}")
    print(f"on the {int(shell.sum())} shell voxels of the box: plain fuse departs from the second scan by {err_plain[0]} tau on average (the ghost), "
          f"adopt-then-fuse by {err_adopt[0]} tau; meshes {len(f_p)} and {len(f_a)} faces")
    out = {"n": args.n, "frames": n_frames, "poses": args.poses, "frames_lost": [lost_a, lost_b], "align": {"status": ast["status"], "rms_m": rms, "shift_m": float(np.linalg.norm(m[:3, 3]))},
           "n_class": st["n_class"].tolist(), "n_regions": st["n_regions"], "n_minor_regions": st["n_minor_regions"],
           "regions": [{"lo": [int(x) for x in c["lo"]], "hi": [int(x) for x in c["hi"]], "n_voxels": int(c["n_voxels"]), "n_appeared": int(c["n_appeared"]),
                        "n_vanished": int(c["n_vanished"])} for c in recs],
           "box_voxels": [list(vlo), list(vhi)], "false_kept_regions": false_kept, "false_minor_regions": minor_away, "adopt": adopt,
           "shell_voxels": int(shell.sum()), "plain_fuse_mean_abs_tau": err_plain[0], "adopt_then_fuse_mean_abs_tau": err_adopt[0]}
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    for t in (ref, cur, res, plain):
        t.close()
    named = [c for c in recs if not away_from(tuple(c["lo"]), tuple(c["hi"]), vlo, vhi, 0)]
    if not named:
        print("FAILED: no kept region names the box")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
