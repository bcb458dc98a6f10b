#!/usr/bin/env python3
"""Lost -> relocalise -> resume on a synthetic room: scan room 0 under HSK_LOSS_HOLD, feed a blank frame (tracking is lost, the
volume stays), then a frame from a camera that has swung back to where it looked `--back` frames ago (30 degrees at the
default, well out of the ICP's reach) and stands a few centimetres beside that, find it with hsk_relocalize over a lattice of
candidates around the last tracked pose, resume the scan there and track on.  Prints the pose errors.

usage: python tools/reloc_demo.py [--n 256] [--frames 240] [--back 20] [--shift 0.04 -0.03 0.05] [--yaw 3] [--pitch -2]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCAN = 720


def moved(pose, shift, yaw_deg, pitch_deg):
    """pose . T(shift) . Ry(yaw) . Rx(pitch): the camera moved in its own frame"""
    a, b = np.radians(yaw_deg), np.radians(pitch_deg)
    t = np.eye(4)
    t[:3, 3] = shift
    ry = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    rx = np.array([[1, 0, 0, 0], [0, np.cos(b), -np.sin(b), 0], [0, np.sin(b), np.cos(b), 0], [0, 0, 0, 1]])
    return (np.asarray(pose, np.float64) @ t @ ry @ rx).astype(np.float32)


def pose_error(a, b):
    """(millimetres between the camera centres, degrees between the orientations)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3]) * 1e3), float(np.degrees(np.arccos(min(1.0, max(-1.0, c)))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--frames", type=int, default=240, help="frames of the 720-frame scripted scan fused before the loss")
    ap.add_argument("--back", type=int, default=20, help="the displaced camera looks where the scan looked this many frames ago")
    ap.add_argument("--shift", type=float, nargs=3, default=(0.04, -0.03, 0.05), help="metres beside that pose, in its camera's frame")
    ap.add_argument("--yaw", type=float, default=3.0)
    ap.add_argument("--pitch", type=float, default=-2.0)
    args = ap.parse_args()
    import housescan_amd as hsk

    poses = [hsk.synth_room_pose(0, k, SCAN) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    trk.set_loss_policy("hold")
    last = None
    for p in poses:
        last, ok = trk.process_frame(hsk.synth_room_depth(0, p))
    print(f"scanned {args.frames} frames at {args.n}^3; the last pose is {pose_error(last, poses[-1])[0]:.1f} mm from its truth")
    pose, ok = trk.process_frame(np.zeros((trk.hgt, trk.w), np.uint16))
    assert not ok and np.array_equal(pose, last), "a blank frame is lost and reports the last tracked pose"
    truth = moved(poses[-1 - args.back], args.shift, args.yaw, args.pitch)
    depth = hsk.synth_room_depth(0, truth)
    pose, ok = trk.process_frame(depth)
    mm, deg = pose_error(truth, last)
    print(f"the camera swings {deg:.1f} degrees and {mm:.0f} mm away: tracked = {ok}")
    cands = hsk.pose_lattice(last, 0.2, 3, float(np.radians(20.0)), 2)
    t0 = time.perf_counter()
    found, st = trk.relocalize(depth, cands)
    ms = (time.perf_counter() - t0) * 1e3
    print(f"hsk_relocalize over {len(cands)} candidates: {st['status']} in {ms:.1f} ms; " +
          "; ".join(f"{c['align_status']} ({c['n_used']} of {st['n_valid']} points, rms {float(c['rms_m']) * 1e3:.1f} mm)" for c in st["candidates"]))
    mm, deg = pose_error(found, truth)
    print(f"the pose found is {mm:.1f} mm and {deg:.3f} degrees from the truth")
    if st["status"] != "found":
        return 1
    trk.resume_scan(found)
    onward = moved(truth, (0.02, 0.0, 0.0), 1.0, 0.0)
    pose, ok = trk.process_frame(hsk.synth_room_depth(0, onward))
    mm, deg = pose_error(pose, onward)
    print(f"resumed: the next frame (2 cm, 1 degree on) is tracked = {ok}, {mm:.1f} mm and {deg:.3f} degrees from its truth")
    trk.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
