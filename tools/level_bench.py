#!/usr/bin/env python3
"""The upright-frame estimate on a room scan at 512^3, prints one JSON object.

  scan      `--frames` frames spread over room 0's whole scripted scan -- its level turn alone shows neither floor nor ceiling --
            fused at `--n`^3 at their scripted poses (every stage scans again: a few seconds)
  calls     host time (ms, median of `--reps`) of hsk_estimate_upright -- the first call behind a change of the volume, which counts
            the cloud, and the calls behind it, which find the count pass in place -- beside hsk_detect_planes_volume and
            hsk_extract_cloud_attrs from the same build, and beside the hsk_fuse_volume call that levels (hsk_level_config's
            destination, made once); the estimate itself
  kernels   from ONE `rocprofv3 --kernel-trace` child run of `--reps` + 1 calls of hsk_estimate_upright: per k_level_* kernel, the
            gather and the cloud's write pass the launches per call, the median time of a launch and the time per call (us); and
            level_us_per_call against cloud_pass_us_per_call -- the estimate's own kernels should cost less than the pass that feeds them
  No bar is set beyond that.

Every GPU stage is a child process under its own time limit; the first failure ends the run.
usage: python tools/level_bench.py [--reps 5] [--n 512] [--frames 120]"""
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
LEVEL_KERNELS = ("k_level_hist", "k_level_sums", "k_level_extents", "k_cloud_fold", "k_plane_gather")
CLOUD_KERNELS = ("k_extract_attrs",)


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def scanned(hsk, args):
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 720, 720 // args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.integrate(hsk.synth_room_depth(0, p), p)
    return trk, poses


def stage_calls(args):
    import housescan_amd as hsk

    trk, poses = scanned(hsk, args)
    out = {"volume": args.n, "frames": args.frames, "build_id": hsk._lib.load().hsk_build_id().decode()}
    first = []
    for _ in range(args.reps):                       # a frame changes the volume: the next estimate counts the cloud again
        trk.integrate(hsk.synth_room_depth(0, poses[-1]), poses[-1])
        trk.synchronize()
        t0 = time.perf_counter()
        up = trk.estimate_upright()
        first.append((time.perf_counter() - t0) * 1e3)
    ms_reused = median_ms(lambda: trk.estimate_upright(), args.reps)
    ms_planes = median_ms(lambda: trk.detect_planes(), max(1, args.reps // 2))
    ms_attrs = median_ms(lambda: trk.extract_cloud_attrs(rgb=False), args.reps)
    cfg, M = trk.level_config(up)
    dst = hsk.KinfuTracker(cfg)
    fuse = []
    for _ in range(max(1, args.reps // 2)):
        dst.reset()
        t0 = time.perf_counter()
        st = dst.fuse_from(trk, M)
        fuse.append((time.perf_counter() - t0) * 1e3)
    lev = dst.estimate_upright()
    L = up["level"][:3, :3].astype(np.float64)
    out["calls"] = {"points": up["n_points"], "estimate_upright_first_ms": round(float(np.median(first)), 3), "estimate_upright_reused_ms": round(ms_reused, 3),
                    "detect_planes_volume_ms": round(ms_planes, 3), "extract_cloud_attrs_ms": round(ms_attrs, 3),
                    "fuse_volume_levelling_ms": round(float(np.median(fuse)), 3), "levelled_dims": [cfg.vol_x, cfg.vol_y, cfg.vol_z],
                    "n_fused": st["n_fused"]}
    out["estimate"] = {"found": up["found"], "up_off_volume_y_deg": round(float(np.degrees(np.arccos(min(1.0, L[1, 1])))), 4),
                       "yaw_off_volume_x_deg": round(float(np.degrees(np.arccos(min(1.0, L[0, 0])))), 4), "floor_m": round(float(up["floor_m"]), 4),
                       "ceiling_m": round(float(up["ceiling_m"]), 4), "n_axis": up["n_axis"], "n_walls": up["n_walls"], "n_invalid": up["n_invalid"],
                       "levelled_found": lev["found"], "levelled_floor_m": round(float(lev["floor_m"]), 4)}
    dst.close()
    trk.close()
    print(json.dumps(out))


def stage_trace_child(args):
    """what the parent looks for in the trace: reps + 1 calls of hsk_estimate_upright, each behind a change of the volume"""
    import housescan_amd as hsk
    trk, poses = scanned(hsk, args)
    for _ in range(args.reps + 1):
        trk.integrate(hsk.synth_room_depth(0, poses[-1]), poses[-1])
        up = trk.estimate_upright()
    trk.close()
    print("TRACE_CHILD " + json.dumps({"calls": args.reps + 1, "points": up["n_points"], "found": up["found"]}))


def stage_trace(args, limit):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "level", "--", sys.executable, os.path.abspath(__file__),
               "--stage", "trace-child", "--n", str(args.n), "--reps", str(min(args.reps, 5)), "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-800:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("TRACE_CHILD ")]
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not line or not files:
            raise RuntimeError("the traced child left no result or no *kernel_trace.csv: " + p.stdout[-800:])
        rows = list(csv.DictReader(open(files[0])))
    out = json.loads(line[0][len("TRACE_CHILD "):])
    for key, names in (("level_us_per_call", LEVEL_KERNELS), ("cloud_pass_us_per_call", CLOUD_KERNELS)):
        per_call = 0.0
        for name in names:
            t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
            if not t:
                continue
            out[name] = {"launches_per_call": round(len(t) / out["calls"], 2), "median_us": round(float(np.median(t)), 2), "max_us": round(max(t), 2),
                         "us_per_call": round(sum(t) / out["calls"], 2)}
            per_call += sum(t) / out["calls"]
        out[key] = round(per_call, 2)
    if "k_level_hist" not in out:
        raise RuntimeError("no k_level_hist launches in the trace")
    return out


def child(args, stage, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--stage", stage, "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    if p.returncode != 0:
        raise RuntimeError(f"stage {stage} exited {p.returncode}: " + p.stdout[-800:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--stage")
    args = ap.parse_args()
    if args.stage:
        {"calls": stage_calls, "trace-child": stage_trace_child}[args.stage](args)
        return 0
    out = {}
    try:
        out.update(child(args, "calls", 300))
        out["kernels"] = stage_trace(args, 300)
    except (RuntimeError, OSError, subprocess.SubprocessError, ValueError) as e:
        out["error"] = f"{type(e).__name__}: {e}"
    print(json.dumps(out))
    return 1 if "error" in out else 0


if __name__ == "__main__":
    sys.exit(main())
