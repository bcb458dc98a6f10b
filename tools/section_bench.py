#!/usr/bin/env python3
"""Section views against scene views, one JSON line (profiles/r11/section_bench.json).

  ratio      median kernel time (us) over `--reps` launches each of k_render_section and of k_render_view for the SAME image:
             the sensor's camera, pinhole, no planes, 512^3 after 60 frames of the scripted stream, from ONE
             `rocprofv3 --kernel-trace` run of a child process -- the bar is section <= 1.10 x view
  sections   recorded, no bar: the top-down orthographic section of room 0's whole scan, cut at mid height, 1024 x 1024 and
             2048 x 2048, at 512^3 and 1024^3 -- kernel medians from one traced child per volume, and hsk_render_section's
             end-to-end host time (ms, median) for rgb + depth from an untraced scan in this process

usage: python tools/section_bench.py [--reps 20] [--frames 60] [--no-rocprof] [--skip-1024]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import housescan_amd as hsk  # noqa: E402
from housescan_amd import _lib  # noqa: E402

SENSOR = dict(width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5)
SIDES = (1024, 2048)
SCAN = 720


def scan_synth(n, frames):
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


def scan_room(n):
    """room 0's whole three-turn scan, RGB-D, pipelined (the frames are rendered eight at a time)"""
    poses = [hsk.synth_room_pose(0, k, SCAN) for k in range(SCAN)]
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    trk.enable_color()
    sent = 0
    with ThreadPoolExecutor(8) as ex:
        for lo in range(0, SCAN, 48):
            for d, c in ex.map(lambda p: (hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0)), poses[lo:lo + 48]):
                trk.submit_frame_rgbd(d, c)
                sent += 1
                if sent >= 2:
                    trk.wait_frame()
    trk.wait_frame()
    trk.synchronize()
    trk.prepare_readout(64 << 20)
    return trk


def floor_plan(side):
    """the keywords of KinfuTracker.render_section for room 0 from above, 3.2 m across, cut at mid height"""
    x0, x1, y0, y1, z0, z1 = (float(v) for v in hsk.synth_room_extents(0))
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = [[-1, 0, 0], [0, 0, 1], [0, 1, 0]]          # x axis -x, y axis +z, looking along +y (down)
    pose[:3, 3] = (0.5 * (x0 + x1), -0.5, 0.5 * (z0 + z1))
    return dict(pose=pose, projection=_lib.HSK_PROJ_ORTHO, width=side, height=side, fx=side / 3.2, fy=side / 3.2, cx=(side - 1) / 2.0,
                cy=(side - 1) / 2.0, clip=[(0, 1, 0, -0.5 * (y0 + y1))], mode=_lib.HSK_VIEW_COLOR_LIT, light=(0.3, -1.0, 0.2),
                light_in_camera=0, light_directional=1)


def child_ratio(n, frames, reps):
    """the launches the parent looks for in the trace: reps + 1 views, then reps + 1 degenerate sections of the same image"""
    trk, pose = scan_synth(n, frames)
    for _ in range(reps + 1):   # (one more: the first launch of a shape is left out)
        trk.render_view(pose=pose, **SENSOR)
    for _ in range(reps + 1):
        trk.render_section(pose=pose, **SENSOR)
    trk.close()


def child_room(n, reps):
    trk = scan_room(n)
    for side in SIDES:
        for _ in range(reps + 1):
            trk.render_section(**floor_plan(side))
    trk.close()


def traced(args, name):
    """the rows of one traced child's kernel trace, in launch order -> (rows, error)"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", name, "--", sys.executable,
               os.path.abspath(__file__)] + args
        try:
            p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=500)
        except (OSError, subprocess.SubprocessError) as e:
            return None, f"{type(e).__name__}: {e}"
        if p.returncode != 0:
            return None, f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:]
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return None, "no *kernel_trace.csv written: " + p.stdout[-600:]
        return sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"])), None


def stats(t, pixels):
    return {"median_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
            "rays_per_s": round(pixels / (np.median(t) * 1e-6))}


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def ratio(n, frames, reps):
    rows, err = traced(["--child", "ratio", "--n", str(n), "--frames", str(frames), "--reps", str(reps)], "ratio")
    if err:
        return {"error": err}
    views = [us(r) for r in rows if "k_render_view" in r["Kernel_Name"]]
    secs = [us(r) for r in rows if "k_render_section" in r["Kernel_Name"]]
    if len(views) != reps + 1 or len(secs) != reps + 1:
        return {"error": f"{len(views)} view and {len(secs)} section launches in the trace"}
    out = {"view_640x480": stats(views[1:], 640 * 480), "section_640x480": stats(secs[1:], 640 * 480)}
    out["section_over_view"] = round(out["section_640x480"]["median_us"] / out["view_640x480"]["median_us"], 3)
    return out


def room_kernels(n, reps):
    rows, err = traced(["--child", "room", "--n", str(n), "--reps", str(reps)], "room")
    if err:
        return {"error": err}
    secs = [us(r) for r in rows if "k_render_section" in r["Kernel_Name"]]
    if len(secs) != len(SIDES) * (reps + 1):
        return {"error": f"{len(secs)} section launches in the trace"}
    return {f"floorplan_{side}x{side}": stats(secs[i * (reps + 1) + 1:(i + 1) * (reps + 1)], side * side) for i, side in enumerate(SIDES)}


def room_calls(n, reps):
    trk = scan_room(n)
    out = {}
    for side in SIDES:
        kw = floor_plan(side)
        r = trk.render_section(**kw)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            trk.render_section(**kw)
            t.append(1e3 * (time.perf_counter() - t0))
        P = side * side
        out[f"render_section_{side}x{side}_ms"] = round(float(np.median(t)), 3)
        out[f"classes_{side}x{side}"] = {"hit": round(r["n_hit"] / P, 4), "cut": round(r["n_cut"] / P, 4)}
    trk.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--skip-1024", action="store_true")
    ap.add_argument("--child", default="")
    ap.add_argument("--n", type=int, default=512)
    a = ap.parse_args()
    if a.child == "ratio":
        child_ratio(a.n, a.frames, a.reps)
        return
    if a.child == "room":
        child_room(a.n, a.reps)
        return
    out = {"reps": a.reps, "frames": a.frames, "build_id": _lib.load().hsk_build_id().decode()}
    sizes = (512,) if a.skip_1024 else (512, 1024)
    if not a.no_rocprof:
        out["ratio_512"] = ratio(512, a.frames, a.reps)
        for n in sizes:
            out[f"kernels_room_{n}"] = room_kernels(n, a.reps)
    for n in sizes:
        out[f"calls_room_{n}"] = room_calls(n, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
