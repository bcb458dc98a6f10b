#!/usr/bin/env python3
"""Volume differencing at 512^3 on two scans of room 0 (the scene of tools/components_bench.py and tools/fill_bench.py), the second
with a box composited into its depth frames; writes profiles/r27/diff_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused twice at `--n`^3 at the script's poses
  calls    host time (ms, ending in the call's own wait) of hsk_diff_volume -- the first call, which makes the scratch, by itself,
           then the median of `--reps` with the scratch reused and ref uploaded afresh before each (not in its time), then of a
           call answered from the held diff --, hsk_download_diff (classes alone, classes and labels),
           hsk_diff_at (2^18 cloud points, radius 1) and hsk_adopt_diff (ref uploaded afresh and diffed: neither is in its time);
           in the same run hsk_label_components behind a volume change, hsk_prune_components and hsk_fuse_volume (cur into ref
           with the identity) on the same volumes
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) and launch
           counts of the k_diff_* kernels and k_mask_dilate beside the labelling's and k_fuse_sweep; the classification sweep's and the fuse
           sweep's GB/s over the same nominal traffic (two reads and one write of a volume)
  No bar is set: nobody has measured this before.

usage: python tools/diff_bench.py [--reps 10] [--n 512] [--frames 60] [--skip kernels]"""
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
KERNELS = ("k_diff_classify", "k_diff_records", "k_diff_box", "k_diff_gather", "k_diff_mark", "k_mask_dilate", "k_diff_adopt", "k_comp_local", "k_comp_merge",
           "k_comp_flatten", "k_comp_roots", "k_comp_records", "k_comp_prune", "k_fuse_sweep", "k_fuse_bricks")
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
    vol = ref.download_tsdf()
    words = args.n * args.n * ((args.n + 3) & ~3)
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(), "volume_bytes": 4 * words,
           # diff.hip's diff_layout: the class words, the labelling's parents, two byte volumes, the rows' counts (the rest is below 1 KiB)
           "scratch_bytes": 8 * words + 2 * args.n ** 3 + 4 * (args.n * args.n + 1)}
    # (KinfuTracker.diff_volume is a size query and a fill: the second call is answered from the held diff, so one device diff a
    # timed call -- provided the volume changed since the last one: ref is uploaded afresh before each, outside the time)
    first = timed(lambda: ref.diff_volume(cur))
    ms = []
    for _ in range(args.reps):
        ref.upload_tsdf(vol)
        ms.append(timed(lambda: ref.diff_volume(cur)))
    held = [timed(lambda: ref.diff_volume(cur)) for _ in range(args.reps)]
    recs, st = ref.diff_volume(cur)
    out["diff"] = {"first_ms": round(first, 3), "ms": med(ms), "held_ms": med(held), "n_class": st["n_class"].tolist(), "n_regions": st["n_regions"],
                   "n_minor_regions": st["n_minor_regions"], "largest": st["largest"]}
    out["download_cls_ms"] = med([timed(lambda: ref.download_diff(region=False)) for _ in range(args.reps + 1)][1:])
    out["download_cls_region_ms"] = med([timed(ref.download_diff) for _ in range(args.reps + 1)][1:])
    pts = cur.extract_cloud(cap=1 << 18)[0]
    out["diff_at"] = {"points": len(pts), "radius": 1, "ms": med([timed(lambda: ref.diff_at(pts, 1)) for _ in range(args.reps + 1)][1:])}
    adopt, ast = [], None
    for _ in range(args.reps + 1):
        ref.upload_tsdf(vol)
        ref.diff_volume(cur)
        t0 = time.perf_counter()
        ast = ref.adopt_diff(cur)
        adopt.append((time.perf_counter() - t0) * 1e3)
    out["adopt"] = {"ms": med(adopt[1:]), "stats": ast}
    label, prune, fuse = [], [], []
    eye = np.eye(4, dtype=np.float32)
    for _ in range(args.reps + 1):
        ref.upload_tsdf(vol)
        label.append(timed(ref.label_components))
        prune.append(timed(ref.prune_components))
        ref.upload_tsdf(vol)
        fuse.append(timed(lambda: ref.fuse_from(cur, eye)))
    out.update({"label_ms": med(label[1:]), "prune_ms": med(prune[1:]), "fuse_ms": med(fuse[1:])})
    ref.release_diff()
    ref.close()
    cur.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "diff",
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
    nominal = 3 * 4 * args.n * args.n * ((args.n + 3) & ~3)
    for name in ("k_diff_classify", "k_fuse_sweep"):
        if out.get(name):
            out[name]["nominal_GBps"] = round(nominal / (out[name]["median_us"] * 1e-6) / 1e9, 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the profiled child may take")
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
    os.makedirs(os.path.join(ROOT, "profiles", "r27"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r27", "diff_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
