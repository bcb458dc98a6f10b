#!/usr/bin/env python3
"""Plane detection on a room scan at 512^3, prints one JSON object.

  scan      the first `--frames` frames of room 0's scripted scan fused at `--n`^3 (every stage scans again: a few seconds)
  device    hsk_detect_planes_volume on the volume's own cloud (every point, oriented): host time of the call (ms, median of
            `--reps`; the cloud's write pass, the gather, every round's launches and read-backs included), the rounds' share
            alone (hsk_detect_planes_oriented on the downloaded cloud, its upload included) and one scoring stage
            (hsk_score_planes, 512 hypotheses); the planes, their points and mean residuals
  host      the path it replaces, on the same cloud: hsk_extract_cloud, hsk_voxel_downsample (3 cm), hsk_detect_planes
            (unoriented, on at most 20 000 of the downsampled points per hypothesis), each timed; the planes, their points
            and mean residuals
  kernels   from ONE `rocprofv3 --kernel-trace` child run of `--reps` + 1 calls of hsk_detect_planes_volume: per k_plane_* kernel
            (and the cloud's write pass) the launches per call, the median time of a launch and the time per call (us)
  No bar is set: the feature's claim is the oriented result on the whole cloud, not a speed-up.

Every GPU stage is a child process under its own time limit; the first failure ends the run.
usage: python tools/planes_bench.py [--reps 5] [--n 512] [--frames 120]"""
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
KERNELS = ("k_plane_seed", "k_plane_score", "k_plane_count_sum", "k_plane_moments", "k_plane_label", "k_cloud_fold", "k_plane_unlabel",
           "k_plane_gather", "k_extract_attrs")


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def scanned(hsk, args):
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.process_frame(hsk.synth_room_depth(0, p))
    return trk


def stage_calls(args):
    import housescan_amd as hsk
    from housescan_amd import products as P

    trk = scanned(hsk, args)
    out = {"volume": args.n, "frames": args.frames, "build_id": hsk._lib.load().hsk_build_id().decode()}

    # the device path
    keep = {}

    def device():
        keep["rec"], keep["labels"] = trk.detect_planes()
    ms_volume = median_ms(device, args.reps)
    rec, labels = keep["rec"], keep["labels"]
    xyz, nrm, _, total, _ = trk.extract_cloud_attrs(rgb=False)
    ms_cloud = median_ms(lambda: trk.detect_planes_cloud(xyz, nrm), max(1, args.reps // 2))
    with np.errstate(all="ignore"):
        hyp = np.concatenate([nrm[:512], -np.einsum("ij,ij->i", nrm[:512], xyz[:512])[:, None]], axis=1).astype(np.float32)
    ms_score = median_ms(lambda: trk.score_planes(xyz, nrm, hyp), max(1, args.reps // 2))
    out["device"] = {"points": int(total), "detect_planes_volume_ms": round(ms_volume, 3), "detect_planes_oriented_ms": round(ms_cloud, 3),
                     "score_planes_512_ms": round(ms_score, 3), "planes": int(len(rec)), "points_on_planes": int((labels >= 0).sum()),
                     "inliers": [int(v) for v in rec["n_inliers"]],
                     "mean_residual_mm": [round(float(r["sum_abs"]) / 65536.0 / max(1, int(r["n_inliers"])) * 1e3, 3) for r in rec],
                     "mean_residual_all_mm": round(float(rec["sum_abs"].sum()) / 65536.0 / max(1, int(rec["n_inliers"].sum())) * 1e3, 3)}

    # the path it replaces
    ms_extract = median_ms(lambda: trk.extract_cloud(), args.reps)
    cloud, _ = trk.extract_cloud()
    ms_down = median_ms(lambda: P.voxel_downsample(cloud, 0.03), 1)
    down = P.voxel_downsample(cloud, 0.03)
    t0 = time.perf_counter()
    planes, hl = P.detect_planes(down)
    ms_host = (time.perf_counter() - t0) * 1e3
    resid, counts = [], []
    for k, eq in enumerate(planes):
        pts = down[hl == k].astype(np.float64)
        counts.append(int(len(pts)))
        resid.append(float(np.abs(pts @ eq[:3].astype(np.float64) + float(eq[3])).mean()) * 1e3 if len(pts) else 0.0)
    out["host"] = {"points": int(len(cloud)), "downsampled": int(len(down)), "extract_cloud_ms": round(ms_extract, 3),
                   "voxel_downsample_ms": round(ms_down, 3), "detect_planes_ms": round(ms_host, 3),
                   "total_ms": round(ms_extract + ms_down + ms_host, 3), "planes": int(len(planes)), "inliers": counts,
                   "mean_residual_mm": [round(r, 3) for r in resid],
                   "mean_residual_all_mm": round(float(np.dot(resid, counts)) / max(1, sum(counts)), 3)}
    trk.close()
    print(json.dumps(out))


def stage_trace_child(args):
    """what the parent looks for in the trace: reps + 1 calls of hsk_detect_planes_volume"""
    import housescan_amd as hsk
    trk = scanned(hsk, args)
    for _ in range(args.reps + 1):
        rec, labels = trk.detect_planes()
    trk.close()
    print("TRACE_CHILD " + json.dumps({"calls": args.reps + 1, "planes": int(len(rec)), "points": int(len(labels))}))


def stage_trace(args, limit):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "planes", "--", sys.executable, os.path.abspath(__file__),
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
    per_call = 0.0
    for name in KERNELS:
        t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not t:
            continue
        out[name] = {"launches_per_call": round(len(t) / out["calls"], 2), "median_us": round(float(np.median(t)), 2), "max_us": round(max(t), 2),
                     "us_per_call": round(sum(t) / out["calls"], 2)}
        per_call += sum(t) / out["calls"]
    if "k_plane_score" not in out:
        raise RuntimeError("no k_plane_score launches in the trace")
    out["kernel_us_per_call"] = round(per_call, 2)
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
