#!/usr/bin/env python3
"""Cloud normals on a room's whole cloud; writes profiles/r35/normals_bench.json and prints it as one JSON object.

  clouds   the import bench's room cloud (the first `--frames` frames of room 0's scripted scan fused at `--n`^3, about 208 k points
           at 512^3), and the same room at about 2 M points: every point `--dense` times, jittered by up to half a cell per axis
  calls    host time (ms, median of `--reps`, the upload and the copies out included) of hsk_estimate_normals at radii of 2, 3 and 5
           cells with one viewpoint, max_neighbours 2^20 so that no point is CROWDED; the pairs (the sum of the neighbour counts) per
           second; beside them, on the room cloud: hsk_extract_cloud_attrs (the volume's own normals) in the scanned context and
           hsk_detect_planes_oriented with the estimated normals
  kernels  the same calls once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) of k_normal_keys,
           k_normal_scatter, k_normal_gather per cloud and radius, and the gather's pairs per second
  host     tests/normal_point_harness.cpp built without sanitizers (-O2), one thread, the room cloud at 3 cells: its pairs per second
           (the file reads and writes included)
  No bar is set: nothing exists to compare against.

usage: python tools/normals_bench.py [--reps 5] [--n 512] [--frames 60] [--dense 10] [--skip kernels,host]"""
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
RADII = (2, 3, 5)


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def work(args):
    """the scan and every measured call, 1 + reps times each in a fixed order -> (the results, the room cloud)"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    trk.prepare_readout()
    cloud, _ = trk.extract_cloud()
    cell = 3.0 / args.n
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(), "cell_m": cell}
    out["extract_cloud_attrs"] = {"call_ms": round(median_ms(lambda: trk.extract_cloud_attrs(rgb=False), args.reps), 3), "points": len(cloud)}
    rng = np.random.default_rng(1)
    dense = (np.repeat(cloud, args.dense, axis=0) + rng.uniform(-0.5 * cell, 0.5 * cell, (len(cloud) * args.dense, 3))).astype(np.float32)
    e = hsk.synth_room_extents(0).astype(np.float64)
    view = np.array([[0.5 * (e[0] + e[1]), 0.5 * (e[2] + e[3]), 0.5 * (e[4] + e[5])]], np.float32)
    got = {}
    for name, pts in (("room", cloud), ("dense", dense)):
        rows = []
        for cells in RADII:
            def call():
                got["r"] = trk.estimate_normals(pts, view, radius_m=cells * cell, max_neighbours=1 << 20)
            ms = median_ms(call, args.reps)
            st = got["r"][4]
            rows.append({"radius_cells": cells, "call_ms": round(ms, 3), "pairs": st["n_pairs"], "pairs_per_s": round(st["n_pairs"] / (ms * 1e-3)),
                         "mean_neighbours": round(st["n_pairs"] / max(len(pts), 1), 1), "stats": st})
            if name == "room" and cells == 3:
                got["nrm"] = got["r"][0]
        out[name] = {"points": len(pts), "radii": rows}
    out["detect_planes_oriented"] = {"call_ms": round(median_ms(lambda: trk.detect_planes_cloud(cloud, got["nrm"]), args.reps), 3)}
    trk.close()
    return out, cloud


def kernels(args, calls):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "normals",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames),
               "--dense", str(args.dense)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    # every estimate launches each kernel once: 1 + reps launches per cloud and radius, in the order of work()
    out = {}
    per = 1 + args.reps
    for kname in ("k_normal_keys", "k_normal_scatter", "k_normal_gather"):
        v = [us(r) for r in rows if kname in r["Kernel_Name"]]
        if len(v) != per * 2 * len(RADII):
            raise RuntimeError(f"{kname}: {len(v)} launches in the trace, {per * 2 * len(RADII)} expected")
        for ci, cloud in enumerate(("room", "dense")):
            for ri, cells in enumerate(RADII):
                at = (ci * len(RADII) + ri) * per
                out[f"{kname}_{cloud}_{cells}_us"] = round(float(np.median(v[at + 1:at + per])), 2)
    for cloud in ("room", "dense"):
        for row in calls[cloud]["radii"]:
            t = out[f"k_normal_gather_{cloud}_{row['radius_cells']}_us"]
            out[f"gather_pairs_per_s_{cloud}_{row['radius_cells']}"] = round(row["pairs"] / (t * 1e-6))
    return out


def host_rate(args, cloud):
    cell = 3.0 / args.n
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "normal_point")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "normal_point_harness.cpp"), "-o", exe])
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([len(cloud), 0, 8, 1 << 20], np.uint32).tobytes())
            f.write(np.array([3 * cell, 1e-3], np.float32).tobytes())
            f.write(np.ascontiguousarray(cloud, np.float32).tobytes())
        t0 = time.perf_counter()
        subprocess.check_call([exe, src, dst])
        s = time.perf_counter() - t0
        pairs = int(np.fromfile(dst, np.uint8)[-8:].view(np.uint64)[0])
    return {"seconds": round(s, 3), "pairs": pairs, "pairs_per_s": round(pairs / s)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--dense", type=int, default=10)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=240, help="seconds the profiled child may take")
    args = ap.parse_args()
    if args.stage == "child":
        work(args)
        return 0
    out, cloud = work(args)
    skip = args.skip.split(",")
    if "kernels" not in skip:
        try:
            out["kernels"] = kernels(args, out)
        except RuntimeError as e:
            out["kernels"] = {"error": str(e)}
    if "host" not in skip:
        out["host_harness"] = host_rate(args, cloud)
    os.makedirs(os.path.join(ROOT, "profiles", "r35"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r35", "normals_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
