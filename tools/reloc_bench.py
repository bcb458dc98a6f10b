#!/usr/bin/env python3
"""Pose scoring and relocalisation at 512^3, 640 x 480, level 2 (160 x 120 = 19 200 points), prints one JSON object.

  scan        the first `--frames` frames of room 0's scripted scan fused at `--n`^3; the frame searched for is the next one
  score       hsk_score_cloud on that frame's level-2 cloud for n_poses in {1, 343, 8575, 65536}: host time of the call (ms,
              median of `--reps`; upload, two launches and the scores' read-back included), samples (points x poses) and
              gathers (x 8) per second
  relocalize  hsk_relocalize with the same candidates: host time of the call (preprocessing, scoring, four refinements)
  No bar is set: nobody has measured any of this.

usage: python tools/reloc_bench.py [--reps 5] [--n 512] [--frames 60]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def candidates(hsk, centre, count):
    """`count` poses around `centre`: a lattice of 0.2 m and 20 degrees (1: the centre; 343: shifts only; 8575: the default
    search), beyond that one of 0.1 m and 10 degrees repeated up to the count"""
    if count == 1:
        return hsk.pose_lattice(centre, 0.2, 0, 0.0, 0)
    if count == 343:
        return hsk.pose_lattice(centre, 0.2, 3, 0.0, 0)
    if count == 8575:
        return hsk.pose_lattice(centre, 0.2, 3, float(np.radians(20.0)), 2)
    base = hsk.pose_lattice(centre, 0.1, 3, float(np.radians(10.0)), 6)      # 57 967
    return np.concatenate([base] * (count // len(base) + 1))[:count]


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    args = ap.parse_args()
    import housescan_amd as hsk

    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames + 1)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses[:-1]:
        last, _ = trk.process_frame(hsk.synth_room_depth(0, p))
    depth = hsk.synth_room_depth(0, poses[-1])
    trk.preprocess(depth)
    cloud = np.ascontiguousarray(trk.download_map(0, 2).reshape(3, -1).T)
    out = {"volume": args.n, "frame": [trk.w, trk.hgt], "level": 2, "points": len(cloud), "build_id": hsk._lib.load().hsk_build_id().decode(), "runs": []}
    for count in (1, 343, 8575, 65536):
        c = candidates(hsk, last, count)
        ms = median_ms(lambda: trk.score_cloud(cloud, c), args.reps)
        found = {}

        def reloc():
            found["st"] = trk.relocalize(depth, c)[1]
        ms_r = median_ms(reloc, max(1, args.reps // 2))
        out["runs"].append({"n_poses": len(c), "score_cloud_ms": round(ms, 3), "samples_per_s": round(len(c) * len(cloud) / (ms * 1e-3)),
                            "gathers_per_s": round(8 * len(c) * len(cloud) / (ms * 1e-3)), "relocalize_ms": round(ms_r, 3),
                            "relocalize_status": found["st"]["status"]})
    trk.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
