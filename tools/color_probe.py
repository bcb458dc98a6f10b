#!/usr/bin/env python3
"""The cost of colour (hsk_enable_color) at 512^3, one JSON line: frames/s with colour off and on from host frames (pipelined
submit / wait, one process, the same frames) on the scripted stream and on room 0 as a sensor sees it; the colour kernel's
mean time from `rocprofv3 --kernel-trace --stats --output-format csv` (a child process; on failure the error's tail is
reported instead); the host's time per submission by phase (hsk_submit_host_us: staging copies, upload + preprocessing
enqueue, the wait for them, the main chain's enqueue); extract_cloud against extract_cloud_attrs after the scan, in ms.

usage: python tools/color_probe.py [--frames 200] [--n 512] [--no-rocprof]"""
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


def frames_of(stream, count):
    if stream == "scripted":
        poses = [hsk.synth_pose(k) for k in range(count)]
        return poses, [hsk.synth_depth(p) for p in poses], [hsk.synth_rgb(p) for p in poses]
    poses, depth = hsk.synth_sensor_frames(count, room=0, scan=720)
    return poses, depth, [hsk.synth_rgb(p, 0) for p in poses]


def scan(n, poses, depth, rgb, color):
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    if color:
        trk.enable_color()
    # (frame 0 and a first tracked frame outside the clock: the scan's start is synchronous)
    for k in range(2):
        trk.process_frame_rgbd(depth[k], rgb[k]) if color else trk.process_frame(depth[k])
    trk.synchronize()
    trk.submit_host_us(reset=True)
    t0 = time.perf_counter()
    waited = 0
    for k in range(2, len(depth)):
        trk.submit_frame_rgbd(depth[k], rgb[k]) if color else trk.submit_frame(depth[k])
        if k >= 4:
            trk.wait_frame()
            waited += 1
    for _ in range(len(depth) - 2 - waited):
        trk.wait_frame()
    trk.synchronize()
    fps = (len(depth) - 2) / (time.perf_counter() - t0)
    us, subs = trk.submit_host_us()
    trk.host_us_per_frame = [round(u / max(subs, 1), 2) for u in us]
    return trk, fps


def readout_ms(trk, reps=5):
    trk.prepare_readout()
    trk.extract_cloud()
    trk.extract_cloud_attrs()
    a, b = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        trk.extract_cloud()
        a.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        trk.extract_cloud_attrs()
        b.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(a)), 1e3 * float(np.median(b))


def kernel_stats(args, stream):
    """k_color_integrate's calls and mean / min / max duration (us) in a child run under rocprofv3 (colour on), with the
    integrate's kernels beside it for scale; {"error": ...} when the run or its statistics file fails"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "probe", "--", sys.executable,
               os.path.abspath(__file__), "--child", stream, "--frames", str(args.frames), "--n", str(args.n)]
        try:
            p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        except (OSError, subprocess.SubprocessError) as e:
            return {"error": f"{type(e).__name__}: {e}"}
        if p.returncode != 0:
            return {"error": f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no *kernel_stats.csv written: " + p.stdout[-600:]}
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            for key, pat in (("color", "k_color_integrate"), ("integrate_pass_a", "k_integrate<"), ("integrate_pass_b", "k_integrate_detail3"),
                             ("column_zrange", "k_column_zrange"), ("raycast", "k_raycast")):
                if pat in name and key not in out:
                    out[key] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                                "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
        return out if "color" in out else {"error": "k_color_integrate not in " + files[0], **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        poses, depth, rgb = frames_of(a.child, a.frames)
        scan(a.n, poses, depth, rgb, True)[0].close()
        return
    out = {"n": a.n, "frames": a.frames, "build_id": hsk._lib.load().hsk_build_id().decode()}
    for stream in ("scripted", "room0_sensor"):
        poses, depth, rgb = frames_of(stream, a.frames)
        off, fps_off = scan(a.n, poses, depth, rgb, False)
        host_off = off.host_us_per_frame
        off.close()
        on, fps_on = scan(a.n, poses, depth, rgb, True)
        host_on = on.host_us_per_frame
        cloud_ms, attrs_ms = readout_ms(on)
        on.close()
        out[stream] = {"fps_color_off": round(fps_off, 1), "fps_color_on": round(fps_on, 1), "on_over_off": round(fps_on / fps_off, 4),
                       "host_us_per_frame_off": host_off, "host_us_per_frame_on": host_on,
                       "extract_cloud_ms": round(cloud_ms, 3), "extract_cloud_attrs_ms": round(attrs_ms, 3),
                       "kernels": None if a.no_rocprof else kernel_stats(a, stream)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
