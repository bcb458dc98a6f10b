#!/usr/bin/env python3
"""Scene views against the tracker's own raycast, one JSON line (profiles/r10/view_bench.json).

  kernels    median kernel time (us) over `--reps` launches each of k_render_view and of k_raycast on the same volume,
             camera and pose, from ONE `rocprofv3 --kernel-trace` run of a child process: the headline state (512^3 after
             60 frames of the scripted stream) with the sensor's camera -- the bar is view <= 1.10 x raycast -- and the view
             alone at 1280 x 960 and 1920 x 1080; the same at 1024^3 (10 frames) with the sensor's camera
  calls      end-to-end host time (ms, median) of hsk_render_view for rgb + depth against hsk_raycast's for the same camera
             (which moves 7.4 MB of float maps and overwrites the tracker's maps: timed on a context of its own)
  pipelined  frames/s of the scripted stream at 512^3 through the pipelined pair, without and with a `follow` view (rgb +
             depth) behind every submission

usage: python tools/view_bench.py [--reps 20] [--frames 60] [--no-rocprof] [--skip-1024]"""
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
import housescan_amd as hsk  # noqa: E402

SENSOR = dict(width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5)
CAMERAS = {"640x480": SENSOR, "1280x960": dict(width=1280, height=960, fx=1050.0, fy=1050.0, cx=639.5, cy=479.5),
           "1920x1080": dict(width=1920, height=1080, fx=1000.0, fy=1000.0, cx=959.5, cy=539.5)}


def scan(n, frames):
    trk = hsk.KinfuTracker(n=n)
    trk.submit_frame(hsk.synth_depth(hsk.synth_pose(0)))
    for k in range(1, frames):
        trk.submit_frame(hsk.synth_depth(hsk.synth_pose(k)))
        trk.wait_frame()
    pose, ok = trk.wait_frame()
    assert ok
    trk.synchronize()
    trk.prepare_readout()
    return trk, pose


def child(n, frames, reps, cams):
    """the launches the parent looks for in the trace, in this order: per camera `reps` views, then `reps` stage raycasts"""
    trk, pose = scan(n, frames)
    for name in cams:
        for _ in range(reps + 1):   # (one more: the first launch of a shape is left out)
            trk.render_view(pose=pose, **CAMERAS[name])
    for _ in range(reps + 1):
        trk.raycast(pose)
    trk.close()


def kernel_medians(n, frames, reps, cams):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "view", "--", sys.executable,
               os.path.abspath(__file__), "--child", str(n), "--frames", str(frames), "--reps", str(reps), "--cams", ",".join(cams)]
        try:
            p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=500)
        except (OSError, subprocess.SubprocessError) as e:
            return {"error": f"{type(e).__name__}: {e}"}
        if p.returncode != 0:
            return {"error": f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return {"error": "no *kernel_trace.csv written: " + p.stdout[-600:]}
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
        us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
        views = [us(r) for r in rows if "k_render_view" in r["Kernel_Name"]]
        rays = [us(r) for r in rows if "k_raycast" in r["Kernel_Name"]]
        if len(views) != len(cams) * (reps + 1) or len(rays) < reps + 1:
            return {"error": f"{len(views)} view and {len(rays)} raycast launches in the trace"}
        out = {}
        for i, name in enumerate(cams):
            t = views[i * (reps + 1) + 1:(i + 1) * (reps + 1)]
            P = CAMERAS[name]["width"] * CAMERAS[name]["height"]
            out["view_" + name] = {"median_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
                                   "rays_per_s": round(P / (np.median(t) * 1e-6))}
        t = rays[-reps:]   # (the stage calls come last; the scan's own raycasts before them)
        out["raycast_640x480"] = {"median_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
                                  "rays_per_s": round(640 * 480 / (np.median(t) * 1e-6))}
        out["view_over_raycast"] = round(out["view_640x480"]["median_us"] / out["raycast_640x480"]["median_us"], 3)
        return out


def call_times(n, frames, reps):
    trk, pose = scan(n, frames)
    own, _ = scan(n, frames)
    out = {}
    for name, cam in CAMERAS.items():
        trk.render_view(pose=pose, **cam)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            trk.render_view(pose=pose, **cam)
            t.append(1e3 * (time.perf_counter() - t0))
        out["render_view_" + name + "_ms"] = round(float(np.median(t)), 3)
    own.raycast(pose)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        own.raycast(pose)
        t.append(1e3 * (time.perf_counter() - t0))
    out["raycast_640x480_ms"] = round(float(np.median(t)), 3)
    trk.close()
    own.close()
    return out


def pipelined(n, count, with_view):
    frames = [hsk.synth_depth(hsk.synth_pose(k)) for k in range(count)]
    trk = hsk.KinfuTracker(n=n)
    trk.prepare_readout()
    trk.submit_frame(frames[0])
    trk.submit_frame(frames[1])
    trk.wait_frame()
    t0 = time.perf_counter()
    for k in range(2, count):
        trk.submit_frame(frames[k])
        if with_view:
            trk.render_view()
        trk.wait_frame()
    trk.wait_frame()
    trk.synchronize()
    dt = time.perf_counter() - t0
    trk.close()
    return round((count - 2) / dt, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--skip-1024", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--cams", default="640x480")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.frames, a.reps, a.cams.split(","))
        return
    out = {"reps": a.reps, "frames": a.frames, "build_id": hsk._lib.load().hsk_build_id().decode()}
    if not a.no_rocprof:
        out["kernels_512"] = kernel_medians(512, a.frames, a.reps, list(CAMERAS))
        if not a.skip_1024:
            out["kernels_1024"] = kernel_medians(1024, 10, a.reps, ["640x480"])
    out["calls_512"] = call_times(512, a.frames, a.reps)
    out["pipelined_512_fps"] = {"without_view": pipelined(512, 150, False), "with_follow_view": pipelined(512, 150, True)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
