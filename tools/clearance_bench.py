#!/usr/bin/env python3
"""The clearance field at 512^3 on room 0's scan; writes profiles/r20/clearance_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused at `--n`^3
  calls    host time (ms, median of `--reps`, the first call reported apart, ending in the call's own wait) of hsk_build_clearance
           behind a volume change and again (reused), of hsk_clearance_at for 4096 points, of hsk_clearance_floor and of
           hsk_download_clearance of the box 0.3 n .. 0.8 n on every axis (a partial box: through k_box_rows), beside
           hsk_label_components behind a volume change and hsk_coverage_census on the same volume; the scratch bytes
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace --stats` child (no counters in that run): medians (us) of the
           k_clear_* kernels and k_box_rows beside k_comp_local and k_pack_classify, which stream the same words
  No bar is set: nothing here had been measured before.

usage: python tools/clearance_bench.py [--reps 10] [--n 512] [--frames 60] [--skip kernels] [--out FILE]"""
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
KERNELS = ("k_clear_rows(", "k_clear_axis<1>", "k_clear_axis<2>", "k_clear_project(", "k_clear_axis_plain(", "k_clear_gather(", "k_box_rows<", "k_comp_local(", "k_pack_classify(",
           "k_cover_census(")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"first_ms": round(v[0], 3), "median_ms": round(float(np.median(v[1:])), 3)}


def work(args):
    """the scan and every measured call, 1 + reps times each"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.process_frame(hsk.synth_room_depth(0, p))
    trk.prepare_readout()
    d0 = hsk.synth_room_depth(0, poses[0])
    par = trk.default_clearance_params()
    pts = np.random.default_rng(1).uniform(0.0, 3.0, (4096, 3)).astype(np.float32)
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(),
           "params": {"weight": list(par.weight), "max_d2": int(par.max_d2), "flags": int(par.flags), "unit_m": float(par.unit_m)}}

    def changed(fn):
        trk.integrate(d0, poses[0])          # (a volume change: cached passes are void)
        trk.synchronize()
        return timed(fn)
    n = args.reps + 1
    out["build"] = stat([changed(trk.build_clearance) for _ in range(n)])
    out["stats"] = trk.build_clearance()
    out["build_reused"] = stat([timed(trk.build_clearance) for _ in range(n)])
    out["build_without_unknown"] = stat([changed(lambda: trk.build_clearance(flags=0)) for _ in range(n)])
    out["stats_without_unknown"] = trk.build_clearance(flags=0)
    trk.build_clearance()
    out["at_4096"] = stat([timed(lambda: trk.clearance_at(pts)) for _ in range(n)])
    lo, hi = int(args.n * 0.3), int(args.n * 0.8)
    out["floor"] = stat([timed(lambda: trk.clearance_floor(1, lo, hi)) for _ in range(n)])
    out["download_box"] = stat([timed(lambda: trk.download_clearance(box=((lo, lo, lo), (hi, hi, hi)))) for _ in range(n)])
    out["label_components"] = stat([changed(trk.label_components) for _ in range(n)])
    out["coverage_census"] = stat([timed(trk.coverage) for _ in range(n)])
    out["pack_volume"] = stat([changed(trk.pack_volume) for _ in range(n)])
    out["scratch_bytes"] = out["stats"]["scratch_bytes"]
    out["scratch_over_volume"] = round(out["scratch_bytes"] / (4.0 * args.n ** 3), 4)
    trk.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "clear",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames)]
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
        out[name.rstrip("(") + "_us"] = {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2), "n": len(v)} if v else None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the profiled child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "clearance_bench.json"))
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
