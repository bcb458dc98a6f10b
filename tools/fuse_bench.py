#!/usr/bin/env python3
"""Volume fusion against the host round trip it replaces, one JSON line (profiles/r12/fuse_bench.json).

  fuse_512       median host time (ms) of `--reps` hsk_fuse_volume calls: room 0's whole RGB-D scan at 512^3 into an EMPTY 512^3
                 destination under a general rotation with a sub-cell shift; the destination is reset between the calls, the
                 resets outside the clock
  round_trip_ms  the yardstick, NOT the code under test: what a host pays to move the two volumes before it resamples anything --
                 hsk_download_tsdf(src) + hsk_download_tsdf(dst) + hsk_upload_tsdf(dst), same process, same contexts, the
                 second call of each.  The bar: fuse_512.median_ms <= round_trip_ms.total ("fuse_not_slower")
  recorded, no bar: chunks_swept / chunks_total; the identity fuse; the same fuse into a 1024 x 512 x 512 house volume over
                 6 x 3 x 3 m; the kernels' own medians (the pre-pass, the sweep, the two rebuilds) from ONE
                 `rocprofv3 --kernel-trace --stats` run of a child process

usage: python tools/fuse_bench.py [--reps 10] [--n 512] [--no-rocprof] [--skip-house]"""
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

SCAN = 720


def scan_room(n, frames=SCAN):
    """room 0's three-turn scan, RGB-D, pipelined (the frames are rendered eight at a time)"""
    poses = [hsk.synth_room_pose(0, k, SCAN) for k in range(frames)]
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    trk.enable_color()
    sent = 0
    with ThreadPoolExecutor(8) as ex:
        for lo in range(0, frames, 48):
            for d, c in ex.map(lambda p: (hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0)), poses[lo:lo + 48]):
                trk.submit_frame_rgbd(d, c)
                sent += 1
                if sent >= 2:
                    trk.wait_frame()
    trk.wait_frame()
    trk.synchronize()
    return trk


def rot(axis, deg, centre):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    R = np.array({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                  "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis])
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = np.asarray(centre) - R @ np.asarray(centre)
    return m


def general(n, offset=(0.0, 0.0, 0.0)):
    """no axis of the rotation is a grid axis; a sub-cell shift on top (tests/test_fuse_host.py: general)"""
    c = (1.5, 1.5, 1.5)
    m = rot("y", 25.0, c) @ rot("x", -13.0, c) @ rot("z", 8.0, c)
    m[:3, 3] += 0.37 * 3.0 / n * np.array([1.0, -0.6, 0.3]) + np.asarray(offset)
    return m.astype(np.float32)


def house_ctx(n):
    cfg = hsk.default_config(n, vol_x=2 * n, vol_size_m=(6.0, 3.0, 3.0))
    trk = hsk.KinfuTracker(cfg)
    trk.enable_color()
    return trk


def timed_fuses(dst, src, m, reps):
    st = dst.fuse_from(src, m)   # (the first call makes the scratch)
    t = []
    for _ in range(reps):
        dst.reset()
        dst.synchronize()
        t0 = time.perf_counter()
        st = dst.fuse_from(src, m)
        t.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
            "n_fused": st["n_fused"], "n_colored": st["n_colored"], "chunks_total": st["chunks_total"],
            "chunks_swept": st["chunks_swept"], "swept_share": round(st["chunks_swept"] / max(1, st["chunks_total"]), 4),
            "box": list(st["box"])}


def round_trip(src, dst):
    """second call of each transfer, as bench.py's readout_ms does"""
    a, b = src.download_tsdf(), dst.download_tsdf()
    out = {}
    t0 = time.perf_counter()
    src.download_tsdf(out=a)
    out["download_src"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    dst.download_tsdf(out=b)
    out["download_dst"] = 1e3 * (time.perf_counter() - t0)
    dst.upload_tsdf(b)
    t0 = time.perf_counter()
    dst.upload_tsdf(b)
    out["upload_dst"] = 1e3 * (time.perf_counter() - t0)
    out["total"] = out["download_src"] + out["download_dst"] + out["upload_dst"]
    return {k: round(v, 3) for k, v in out.items()}


def child(n, reps):
    """what the parent looks for in the trace: reps + 1 fuses of the general rotation into a 512^3 destination"""
    src = scan_room(n)
    dst = hsk.KinfuTracker(n=n)
    dst.enable_color()
    m = general(n)
    for _ in range(reps + 1):
        dst.reset()
        dst.fuse_from(src, m)
    dst.close()
    src.close()


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def kernels(n, reps):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "fuse", "--", sys.executable,
               os.path.abspath(__file__), "--child", "--n", str(n), "--reps", str(reps)]
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
    first = next((i for i, r in enumerate(rows) if "k_fuse_bricks" in r["Kernel_Name"]), None)
    if first is None:
        return {"error": "no k_fuse_bricks launch in the trace"}
    out = {}
    # (from the first fuse on; k_summaries<false, ..> is the rebuild, <true, ..> the write-back of deferred weights)
    for key, name in (("bricks_prepass", "k_fuse_bricks"), ("sweep", "k_fuse_sweep"), ("rebuild_flags", "k_rebuild_flags"),
                      ("rebuild_summaries", "k_summaries<false")):
        t = [us(r) for r in rows[first:] if name in r["Kernel_Name"]][1:]
        if not t:
            return {"error": f"no {name} launches in the trace"}
        out[key] = {"median_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "launches": len(t)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--skip-house", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.n, a.reps)
        return
    n = a.n
    out = {"n": n, "reps": a.reps, "scan_frames": SCAN, "build_id": _lib.load().hsk_build_id().decode()}
    src = scan_room(n)
    dst = hsk.KinfuTracker(n=n)
    dst.enable_color()
    out[f"fuse_{n}"] = timed_fuses(dst, src, general(n), a.reps)
    out[f"fuse_{n}_identity"] = timed_fuses(dst, src, np.eye(4, dtype=np.float32), a.reps)
    out["round_trip_ms"] = round_trip(src, dst)
    out["fuse_not_slower"] = bool(out[f"fuse_{n}"]["median_ms"] <= out["round_trip_ms"]["total"])
    dst.close()
    if not a.skip_house:
        house = house_ctx(n)
        out[f"fuse_house_{2 * n}x{n}x{n}"] = timed_fuses(house, src, general(n, offset=(1.2, 0.0, 0.0)), a.reps)
        house.close()
    src.close()
    if not a.no_rocprof:
        out["kernels_us"] = kernels(n, min(a.reps, 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
