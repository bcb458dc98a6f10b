#!/usr/bin/env python3
"""Cloud import at 512^3 with a room's whole cloud; writes profiles/r34/import_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused at `--n`^3; its cloud is extracted and the context closed
  calls    host time (ms, median of `--reps`, ending in the call's own wait) in a fresh context of the same size:
           hsk_splat_cloud (one view, the cloud uploaded by the call), hsk_import_cloud over the `--views` views of a fan at the
           room's middle (hsk_pose_lattice(centre, 0, 0, step, 4) gives 81), hsk_integrate of one sensor frame; the import's time
           per view, and points per second = points x views / time
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) of
           k_splat_points and k_splat_resolve beside the integrate's kernels (k_integrate, k_integrate_detail3), and
           k_splat_points' points per second
  No bar is set: nobody has measured any of this.

usage: python tools/import_bench.py [--reps 5] [--n 512] [--frames 60] [--n-rot 4] [--skip kernels]"""
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


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def work(args):
    """the scan and every measured call, 1 + reps times each in a fixed order"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    cloud, _ = trk.extract_cloud()
    trk.close()
    e = hsk.synth_room_extents(0).astype(np.float64)
    centre = np.array(poses[0], np.float32).reshape(4, 4).copy()
    centre[:3, 3] = (0.5 * (e[0] + e[1]), 0.5 * (e[2] + e[3]), 0.5 * (e[4] + e[5]))
    fan = hsk.pose_lattice(centre, 0.0, 0, float(np.pi / (2 * args.n_rot + 1)), args.n_rot)
    new = hsk.KinfuTracker(n=args.n, init_pose=centre)
    new.prepare_readout()
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(),
           "points": len(cloud), "views": len(fan)}
    got = {}

    def splat():
        got["splat"] = new.splat_cloud(cloud, poses[0])
    ms = median_ms(splat, args.reps)
    out["splat_cloud"] = {"call_ms": round(ms, 3), "points_per_s": round(len(cloud) / (ms * 1e-3)), "stats": got["splat"][1]}

    def imp():
        got["import"] = new.import_cloud(cloud, fan)
    ms = median_ms(imp, args.reps)
    st = got["import"]
    out["import_cloud"] = {"call_ms": round(ms, 3), "per_view_ms": round(ms / len(fan), 4), "points_per_s": round(len(cloud) * len(fan) / (ms * 1e-3)),
                           "n_splatted": int(st["n_splatted"].astype(np.int64).sum()), "n_pixels": int(st["n_pixels"].astype(np.int64).sum())}
    depth = hsk.synth_room_depth(0, poses[0])
    out["integrate"] = {"call_ms": round(median_ms(lambda: new.integrate(depth, poses[0]), args.reps), 3)}
    c = new.coverage()
    out["census"] = {k: int(c[k]) for k in ("n_unseen", "n_free", "n_solid", "n_frontier")}
    new.close()
    return out


def kernels(args, calls):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "import",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames),
               "--n-rot", str(args.n_rot)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))

    def med(name, tail=None):
        v = [us(r) for r in rows if name in r["Kernel_Name"]]
        v = v[-tail:] if tail else v
        return round(float(np.median(v)), 2) if v else None
    # (the import's launches are the last reps x views of k_splat_points; before them the single views' 1 + reps)
    n_imp = args.reps * calls["views"]
    out = {"k_splat_points_us": med("k_splat_points", n_imp), "k_splat_resolve_us": med("k_splat_resolve", n_imp), "k_splat_pose_us": med("k_splat_pose"),
           "k_integrate_us": med("k_integrate<"), "k_integrate_detail3_us": med("k_integrate_detail3"), "k_scale_depth_us": med("k_scale_depth")}
    if out["k_splat_points_us"]:
        out["k_splat_points_points_per_s"] = round(calls["points"] / (out["k_splat_points_us"] * 1e-6))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--n-rot", type=int, default=4)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=240, help="seconds the profiled child may take")
    args = ap.parse_args()
    if args.stage == "child":
        work(args)
        return 0
    out = work(args)
    if "kernels" not in args.skip.split(","):
        try:
            out["kernels"] = kernels(args, out)
        except RuntimeError as e:
            out["kernels"] = {"error": str(e)}
    os.makedirs(os.path.join(ROOT, "profiles", "r34"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r34", "import_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
