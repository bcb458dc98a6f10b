#!/usr/bin/env python3
"""The room partition on the fused two-room scan; writes profiles/r22/partition_bench.json and prints it as one JSON object.

  scan     rooms 0 and 1, `--frames` frames of the 720-frame scripted scan each with stride `--stride`, each at `--n`^3 over 3 m,
           fused side by side into one house volume of 2 `--n` x `--n` x `--n` voxels over 6 x 3 x 3 m (tools/partition_demo.py's)
  calls    host time (ms, median of `--reps`, the first call reported apart, ending in the call's own wait) of hsk_build_partition
           behind a volume change (the clearance field is rebuilt with it; hsk_build_clearance behind the same change is reported
           beside it) and again (reused), of hsk_partition_at for 4096 points with radius 2 and of hsk_partition_floor; beside them
           hsk_build_reach seeded once in each room and hsk_label_components behind a volume change: the yardstick is their sum.
           Per build the rounds, the tiles relaxed, the first worklist's length and the scratch bytes.  Clearance flags 0.
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace --stats` child (no counters in that run): medians and sums (us)
           of the k_part_* kernels beside k_reach_round and the components' kernels
  No bar is set: nothing here had been measured before.

usage: python tools/partition_bench.py [--reps 3] [--n 512] [--frames 720] [--stride 8] [--skip kernels] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_part_label_tile(", "k_part_label_faces(", "k_part_flatten_count(", "k_part_roots(", "k_part_init(", "k_part_round(", "k_part_records(",
           "k_part_doors(", "k_part_gather(", "k_part_box(", "k_reach_init(", "k_reach_round(", "k_comp_")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"first_ms": round(v[0], 3), "median_ms": round(float(np.median(v[1:])), 3)}


def work(args):
    """the scan and every measured call, 1 + reps times each"""
    import housescan_amd as hsk
    n = args.n
    house = hsk.KinfuTracker(hsk.default_config(n, vol_x=2 * n, vol_size_m=(6.0, 3.0, 3.0)))
    for room in (0, 1):
        poses = [hsk.synth_room_pose(room, k, 720) for k in range(0, args.frames, args.stride)]
        if room == 0:
            pose0, d0 = poses[0], hsk.synth_room_depth(0, poses[0])
        trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
        for p in poses:
            trk.integrate(hsk.synth_room_depth(room, p), p)
        move = np.eye(4, dtype=np.float32)
        move[0, 3] = 3.0 * room
        house.fuse_from(trk, move)
        trk.close()
    walk = house.default_clearance_params(flags=0)
    pp = house.default_partition_params(walk)
    rp = house.default_reach_params(walk)
    out = {"volume": [2 * n, n, n], "frames": args.frames, "stride": args.stride, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(),
           "params": {"weight": list(walk.weight), "max_d2": int(walk.max_d2), "unit_m": float(walk.unit_m), "core_d2": int(pp.core_d2), "min_d2": int(pp.min_d2),
                      "min_core_voxels": int(pp.min_core_voxels), "reach_min_d2": int(rp.min_d2)}}

    def changed(fn):
        house.integrate(d0, pose0)          # (a volume change -- room 0's first frame once more: cached fields are void)
        house.synchronize()
        return timed(fn)
    reps = args.reps + 1
    out["build_clearance"] = stat([changed(lambda: house.build_clearance(walk)) for _ in range(reps)])
    out["build_partition"] = stat([changed(lambda: house.build_partition(walk, pp)) for _ in range(reps)])
    rooms, st = house.build_partition(walk, pp)
    out["build_partition_reused"] = stat([timed(lambda: house.build_partition(walk, pp)) for _ in range(reps)])
    relaxed, first, tiles = house.partition_tiles_relaxed()
    house.integrate(d0, pose0)
    rooms, st = house.build_partition(walk, pp)
    out["stats"] = st
    out["tiles"], out["tiles_relaxed"], out["first_list"] = tiles, relaxed, first
    out["rooms"] = [{"n_voxels": int(r["n_voxels"]), "n_core_voxels": int(r["n_core_voxels"]), "lo": r["lo"].tolist(), "hi": r["hi"].tolist()} for r in rooms[:8]]
    out["doors"] = [{"a": int(d["a"]), "b": int(d["b"]), "n_faces": d["n_faces"].tolist(), "lo": d["lo"].tolist(), "hi": d["hi"].tolist(), "max_d2": int(d["max_d2"])}
                    for d in house.partition_doors()[:8]]
    cell = 3.0 / n
    seeds = [tuple((float(r["sum"][i]) / float(r["n_voxels"]) + 0.5) * cell for i in range(3)) for r in rooms[:2]]          # (a room's centroid)
    pts = np.random.default_rng(1).uniform(0.0, 3.0, (4096, 3)).astype(np.float32) * np.array([2.0, 1.0, 1.0], np.float32)
    out["at_4096_radius_2"] = stat([timed(lambda: house.partition_at(pts, 2)) for _ in range(reps)])
    lo, hi = int(n * 0.3), int(n * 0.8)
    out["floor"] = stat([timed(lambda: house.partition_floor(1, lo, hi, walk, pp)) for _ in range(reps)])
    out["floor_stats"] = house.partition_floor(1, lo, hi, walk, pp)[3]
    # the yardstick: the reach field seeded once in each room, with the partition's min_d2, and the components' labelling
    out["reach_seeds"] = seeds
    out["build_reach"] = stat([changed(lambda: house.build_reach(seeds, walk, min_d2=int(pp.min_d2))) for _ in range(reps)])
    out["reach_stats"] = house.build_reach(seeds, walk, min_d2=int(pp.min_d2))
    out["reach_tiles_relaxed"] = house.reach_tiles_relaxed()[0]
    out["label_components"] = stat([changed(house.label_components) for _ in range(reps)])
    c = out["build_clearance"]["median_ms"]
    out["partition_alone_ms"] = round(out["build_partition"]["median_ms"] - c, 3)
    out["yardstick_ms"] = round(out["build_reach"]["median_ms"] - c + out["label_components"]["median_ms"], 3)
    out["partition_over_yardstick"] = round(out["partition_alone_ms"] / max(out["yardstick_ms"], 1e-9), 3)
    out["scratch_bytes"] = st["scratch_bytes"]
    out["scratch_over_volume"] = round(st["scratch_bytes"] / (4.0 * 2 * n ** 3), 4)
    house.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "partition",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", "1", "--frames", str(args.frames),
               "--stride", str(args.stride)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for name in KERNELS:
        v = [us(r) for r in rows if name in r["Kernel_Name"]]
        out[name.rstrip("(") + "_us"] = ({"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2), "sum": round(sum(v), 1), "n": len(v)}
                                         if v else None)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=720)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the profiled child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "partition_bench.json"))
    args = ap.parse_args()
    if args.stage == "child":
        work(args)
        return 0
    out = work(args)
    if "kernels" not in args.skip.split(","):
        try:
            out["kernels"] = kernels(args)
        except RuntimeError as e:
            out["kernels"] = {"error": str(e)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
