#!/usr/bin/env python3
"""Volume alignment at 512^3 with a room's whole cloud, writes profiles/r15/align_bench.json (one JSON object).

  scan           room 0's scripted scan fused at 512^3, saved as a volume file; every later stage loads that file
  calls          host time (ms, median of `--reps`) of hsk_align_cloud with the defaults: the room's own cloud (hsk_extract_cloud_attrs)
                 against the room's volume from a start 1 degree and (30, -20, 25) mm off; of one iteration alone (max_iters = 1);
                 of hsk_align_volume (the cloud's extraction and its way through host memory included)
  kernels        from ONE `rocprofv3 --kernel-trace` child run: the median time of k_align_iter (one iteration's kernel) and, in
                 the same process on the same volume, of k_fuse_sweep (tools/fuse_bench.py's general rotation into an empty volume)
  tap rates      gathers per second: points x probes x 8 for the alignment; voxels of the swept chunks x 8 for the sweep (every
                 voxel of a swept chunk gathers; a few lanes of clipped chunks do not: an upper bound of the sweep's rate by < 1 %)
  No bar is set: the ratio is recorded.

Every GPU stage is a child process under its own time limit; the first failure ends the run.
usage: python tools/align_bench.py [--reps 10] [--n 512] [--frames 720] [--out profiles/r15/align_bench.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

SCAN = 720


def start_matrix():
    """1 degree about (1, 2, 3) through the volume's centre, then (30, -20, 25) mm"""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    a = np.radians(1.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    c = np.array([1.5, 1.5, 1.5])
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = c - R @ c + np.array([0.030, -0.020, 0.025])
    return m.astype(np.float32)


def scan_room(hsk, n, frames):
    """the first `frames` frames of room 0's three-turn scan, depth only, pipelined (the frames are rendered eight at a time)"""
    from concurrent.futures import ThreadPoolExecutor
    poses = [hsk.synth_room_pose(0, k, SCAN) for k in range(frames)]
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    sent = 0
    with ThreadPoolExecutor(8) as ex:
        for lo in range(0, frames, 48):
            for d in ex.map(lambda p: hsk.synth_room_depth(0, p), poses[lo:lo + 48]):
                trk.submit_frame(d)
                sent += 1
                if sent >= 2:
                    trk.wait_frame()
    trk.wait_frame()
    trk.synchronize()
    return trk


def stage_scan(a):
    import housescan_amd as hsk
    trk = scan_room(hsk, a.n, a.frames)
    info = trk.save_volume(a.volume)
    trk.close()
    print(json.dumps({"frames": a.frames, "file_bytes": int(info["total_bytes"])}))


def loaded(hsk, a):
    trk = hsk.KinfuTracker(n=a.n)
    trk.load_volume(a.volume)
    return trk


def timed(call, reps):
    call()   # (the first call makes the scratch)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = call()
        t.append(1e3 * (time.perf_counter() - t0))
    return res, {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def stage_calls(a):
    import housescan_amd as hsk
    src, dst = loaded(hsk, a), loaded(hsk, a)
    xyz, nrm, _, total, _ = src.extract_cloud_attrs(rgb=False)
    m0 = start_matrix()
    out = {"build_id": hsk._lib.load().hsk_build_id().decode(), "cloud_points": int(total)}
    (m, st), out["align_cloud"] = timed(lambda: dst.align_cloud(xyz, nrm, m0), a.reps)
    err = np.abs(m.astype(np.float64) - np.eye(4)).max()
    out["align_cloud"].update(status=st["status"], iterations=st["iterations"], n_points=st["n_points"], stride=st["stride"], n_used=st["n_used"],
                              rms_mm=[round(1e3 * float(v), 4) for v in st["rms_m"]], max_abs_matrix_minus_identity=float(err))
    (_, st1), out["align_cloud_one_iteration"] = timed(lambda: dst.align_cloud(xyz, nrm, m0, max_iters=1), a.reps)
    out["align_cloud_one_iteration"]["n_used"] = st1["n_used"]
    (_, stv), out["align_volume"] = timed(lambda: dst.align_from(src, m0), a.reps)
    out["align_volume"].update(status=stv["status"], iterations=stv["iterations"])
    src.close()
    dst.close()
    print(json.dumps(out))


def stage_trace_child(a):
    """what the parent looks for in the trace: reps + 1 alignments, then reps + 1 fuses into an empty volume"""
    import fuse_bench
    import housescan_amd as hsk
    src, dst = loaded(hsk, a), loaded(hsk, a)
    xyz, nrm, _, _, _ = src.extract_cloud_attrs(rgb=False)
    m0 = start_matrix()
    for _ in range(a.reps + 1):
        _, st = dst.align_cloud(xyz, nrm, m0)
    dst.close()
    empty = hsk.KinfuTracker(n=a.n)
    for _ in range(a.reps + 1):
        empty.reset()
        fs = empty.fuse_from(src, fuse_bench.general(a.n))
    empty.close()
    src.close()
    print("TRACE_CHILD " + json.dumps({"n_points": st["n_points"], "iterations": st["iterations"], "chunks_swept": fs["chunks_swept"],
                                       "chunks_total": fs["chunks_total"], "n_fused": fs["n_fused"]}))


def us(r):
    return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3


def stage_trace(a, limit):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "align", "--", sys.executable, os.path.abspath(__file__),
               "--stage", "trace-child", "--n", str(a.n), "--reps", str(min(a.reps, 5)), "--volume", a.volume]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-800:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("TRACE_CHILD ")]
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not line or not files:
            raise RuntimeError("the traced child left no result or no *kernel_trace.csv: " + p.stdout[-800:])
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    out = json.loads(line[0][len("TRACE_CHILD "):])
    for key, name in (("align_iter", "k_align_iter"), ("fuse_sweep", "k_fuse_sweep")):
        t = [us(r) for r in rows if name in r["Kernel_Name"]]
        skip = out["iterations"] if key == "align_iter" else 1     # (the first call's launches)
        t = t[skip:]
        if not t:
            raise RuntimeError(f"no {name} launches in the trace")
        out[key + "_us"] = {"median": round(float(np.median(t)), 2), "min": round(min(t), 2), "max": round(max(t), 2), "launches": len(t)}
    return out


def child(a, stage, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--stage", stage, "--n", str(a.n), "--reps", str(a.reps), "--frames", str(a.frames),
           "--volume", a.volume]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    if p.returncode != 0:
        raise RuntimeError(f"stage {stage} exited {p.returncode}: " + p.stdout[-800:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=SCAN)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "align_bench.json"))
    ap.add_argument("--stage")
    ap.add_argument("--volume")
    a = ap.parse_args()
    if a.stage:
        {"scan": stage_scan, "calls": stage_calls, "trace-child": stage_trace_child}[a.stage](a)
        return
    with tempfile.TemporaryDirectory() as d:
        a.volume = os.path.join(d, "room0.hskv")
        out = {"n": a.n, "reps": a.reps}
        try:
            out["scan"] = child(a, "scan", 420)
            out.update(child(a, "calls", 300))
            k = stage_trace(a, 300)
            out["kernels"] = k
            probes = 2 * 3 + 1     # (the default: 3 to either side)
            align_rate = k["n_points"] * probes * 8 / (k["align_iter_us"]["median"] * 1e-6)
            sweep_rate = k["chunks_swept"] * 4096 * 8 / (k["fuse_sweep_us"]["median"] * 1e-6)
            out["taps_per_s"] = {"align_iter": round(align_rate / 1e9, 3), "fuse_sweep": round(sweep_rate / 1e9, 3), "unit": "1e9 gathers / s",
                                 "align_over_sweep": round(align_rate / sweep_rate, 3)}
        except (RuntimeError, OSError, subprocess.SubprocessError, ValueError) as e:
            out["error"] = f"{type(e).__name__}: {e}"
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text + "\n")
    print(text)
    sys.exit(1 if "error" in out else 0)


if __name__ == "__main__":
    main()
