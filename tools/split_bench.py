#!/usr/bin/env python3
"""The scene split at 512^3 on a scan of room 0 with a box composited into its depth frames (the scene of tools/diff_bench.py);
writes profiles/r28/split_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused twice at `--n`^3 at the script's poses, once with the box
  calls    host time (ms, ending in the call's own wait) of hsk_split_scene -- the first call, which makes the scratch, by itself,
           then the median of `--reps` with the scratch reused and the volume uploaded afresh before each (not in its time), then
           of a call answered from the held split --, hsk_download_split (classes alone, all three), hsk_split_at (2^18 cloud
           points, radius 1) and hsk_remove_objects (uploaded afresh and split: neither is in its time); in the same run
           hsk_diff_volume against the scan without the box and hsk_label_components behind a volume change
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) and launch
           counts of the k_split_* kernels and k_mask_dilate beside the labelling's and k_diff_classify
  No bar is set: nobody has measured this before.

usage: python tools/split_bench.py [--reps 10] [--n 512] [--frames 60] [--skip kernels]"""
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
KERNELS = ("k_split_classify", "k_split_records", "k_split_box", "k_split_gather", "k_split_mark", "k_mask_dilate", "k_split_restore", "k_comp_local", "k_comp_merge",
           "k_comp_flatten", "k_comp_roots", "k_comp_records", "k_comp_prune", "k_diff_classify")
BOX = ((1.3, 1.3, 2.1), (1.7, 1.7, 2.4))       # hangs in front of the wall the first frames look at


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return round(float(np.median(v)), 3)


def work(args):
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    ref, cur = hsk.KinfuTracker(n=args.n, init_pose=poses[0]), hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        d = hsk.synth_room_depth(0, p)
        ref.integrate(d, p)
        cur.integrate(hsk.synth_box_depth(d, p, *BOX), p)
    for t in (ref, cur):
        t.prepare_readout()
    vol = cur.download_tsdf()
    planes, _ = cur.detect_planes()
    up = -np.asarray(cur.estimate_upright()["level"], np.float64).reshape(4, 4)[1, :3]
    pl = hsk.split_plane_kinds(planes["abcd"], up)
    words = args.n * args.n * ((args.n + 3) & ~3)
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(), "volume_bytes": 4 * words,
           "planes": len(pl), "kinds": pl["kind"].tolist(),
           # split.hip's split_layout: the class words, the labelling's parents, two byte volumes, the rows' counts (the rest is below 16 KiB)
           "scratch_bytes": 8 * words + 2 * args.n ** 3 + 4 * (args.n * args.n + 1)}
    # (KinfuTracker.split_scene is a size query and a fill: the second call is answered from the held split, so one device split a
    # timed call -- provided the volume changed since the last one: it is uploaded afresh before each, outside the time)
    first = timed(lambda: cur.split_scene(pl))
    ms = []
    for _ in range(args.reps):
        cur.upload_tsdf(vol)
        ms.append(timed(lambda: cur.split_scene(pl)))
    held = [timed(lambda: cur.split_scene(pl)) for _ in range(args.reps)]
    recs, st = cur.split_scene(pl)
    out["split"] = {"first_ms": round(first, 3), "ms": med(ms), "held_ms": med(held), "n_class": st["n_class"].tolist(), "n_objects": st["n_objects"],
                    "n_minor_objects": st["n_minor_objects"], "largest": st["largest"], "n_edge": st["n_edge"], "n_no_normal": st["n_no_normal"]}
    out["download_cls_ms"] = med([timed(lambda: cur.download_split(plane=False, object=False)) for _ in range(args.reps + 1)][1:])
    out["download_all_ms"] = med([timed(cur.download_split) for _ in range(args.reps + 1)][1:])
    pts = cur.extract_cloud(cap=1 << 18)[0]
    out["split_at"] = {"points": len(pts), "radius": 1, "ms": med([timed(lambda: cur.split_at(pts, 1)) for _ in range(args.reps + 1)][1:])}
    n = args.n
    roots = [(int(c["root"][2]) * n + int(c["root"][1])) * n + int(c["root"][0]) for c in recs[:256]]          # (a call takes 256 objects)
    remove, rst = [], None
    for _ in range(args.reps + 1):
        cur.upload_tsdf(vol)
        cur.split_scene(pl)
        t0 = time.perf_counter()
        rst = cur.remove_objects(roots)
        remove.append((time.perf_counter() - t0) * 1e3)
    out["remove"] = {"ms": med(remove[1:]), "stats": rst}
    label, diff = [], []
    for _ in range(args.reps + 1):
        cur.upload_tsdf(vol)
        label.append(timed(cur.label_components))
        diff.append(timed(lambda: cur.diff_volume(ref)))
    out.update({"label_ms": med(label[1:]), "diff_ms": med(diff[1:])})
    cur.release_split()
    ref.close()
    cur.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "split",
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
        v = [us(r) for r in rows if r["Kernel_Name"].startswith(name + "(") or r["Kernel_Name"].startswith(name + "<") or (" " + name + "(") in r["Kernel_Name"]
             or (" " + name + "<") in r["Kernel_Name"]]
        out[name] = {"launches": len(v), "median_us": round(float(np.median(v)), 2), "max_us": round(float(np.max(v)), 2),
                     "sum_ms": round(float(np.sum(v)) / 1e3, 3)} if v else None
    nominal = 2 * 4 * args.n * args.n * ((args.n + 3) & ~3)          # one read and one write of a volume
    if out.get("k_split_classify"):
        out["k_split_classify"]["nominal_GBps"] = round(nominal / (out["k_split_classify"]["median_us"] * 1e-6) / 1e9, 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the profiled child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28", "split_bench.json"))
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
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
