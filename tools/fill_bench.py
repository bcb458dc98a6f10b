#!/usr/bin/env python3
"""Hole filling at 512^3 on room 0's scan (the scene of tools/components_bench.py); writes profiles/r26/fill_bench.json and prints
it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused at `--n`^3
  calls    host time (ms, ending in the call's own wait) of hsk_fill_holes on the volume uploaded afresh -- HSK_FILL_SURFACE and
           HSK_FILL_ALL at 8 iterations and at the default --, the first call (which makes the scratch) reported by itself, then the
           median of `--reps`; in the same run hsk_prune_components (the volume uploaded afresh and labelled: the labelling is not
           in its time), hsk_label_components behind a volume change and hsk_coverage_census
  work     tile_visits beside candidates x iterations (the candidates counted on the host from the download: the 16 x 16 x 8 tiles
           that hold a never-observed voxel) and the scratch's size (fill.hip's fill_layout: two int16 states per stored voxel, 259
           bytes per tile, the counters)
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) and launch
           counts of the k_fill_* kernels and k_mask_dilate beside k_comp_prune, k_pack_classify and k_cover_census
  No bar is set: nobody has measured this before.

usage: python tools/fill_bench.py [--reps 10] [--n 512] [--frames 60] [--skip kernels]"""
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
FILL_KERNELS = ("k_fill_init", "k_fill_round", "k_fill_cross", "k_mask_dilate", "k_fill_count", "k_fill_commit")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def candidates(vol):
    """the 16 x 16 x 8 tiles that hold a never-observed voxel"""
    Z, Y, X = vol.shape[:3]
    unseen = np.zeros(((Z + 7) // 8 * 8, (Y + 15) // 16 * 16, (X + 15) // 16 * 16), bool)
    unseen[:Z, :Y, :X] = vol[..., 1] == 0
    t = unseen.reshape(unseen.shape[0] // 8, 8, unseen.shape[1] // 16, 16, unseen.shape[2] // 16, 16)
    return int(t.any(axis=(1, 3, 5)).sum()), int(t.shape[0] * t.shape[2] * t.shape[4])


def work(args):
    """the scan and every measured call, 1 + reps times each"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.process_frame(hsk.synth_room_depth(0, p))
    trk.prepare_readout()
    d0 = hsk.synth_room_depth(0, poses[0])
    vol = trk.download_tsdf()
    n_cand, n_tiles = candidates(vol)
    default_it = int(trk.default_fill_params().iterations)
    words = args.n * args.n * ((args.n + 3) & ~3)
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(),
           "default_iterations": default_it, "tiles": n_tiles, "candidate_tiles": n_cand,
           "scratch_bytes": 4 * words + 259 * n_tiles + 4 * (16 + 256), "volume_bytes": 4 * words, "fills": {}}
    for keep, kname in ((hsk.FILL_SURFACE, "surface"), (hsk.FILL_ALL, "all")):
        for it in (8, default_it):
            ms, st = [], None
            for _ in range(args.reps + 1):
                trk.upload_tsdf(vol)
                t0 = time.perf_counter()
                st = trk.fill_holes(iterations=it, keep=keep)
                ms.append((time.perf_counter() - t0) * 1e3)
            out["fills"][f"{kname}_{it}"] = {"first_ms": round(ms[0], 3), "ms": round(float(np.median(ms[1:])), 3), "stats": st,
                                             "candidates_x_iterations": n_cand * it,
                                             "visits_over_candidates_x_iterations": round(st["tile_visits"] / max(1, n_cand * it), 4)}
    prune = []
    for _ in range(args.reps + 1):
        trk.upload_tsdf(vol)
        trk.label_components()
        prune.append(timed(trk.prune_components))
    trk.upload_tsdf(vol)

    def changed(fn):
        trk.integrate(d0, poses[0])          # (a volume change: cached passes are void)
        trk.synchronize()
        return timed(fn)
    label = [changed(trk.label_components) for _ in range(args.reps + 1)][1:]
    census = [timed(trk.coverage) for _ in range(args.reps + 1)][1:]
    out.update({"prune_ms": round(float(np.median(prune[1:])), 3), "label_first_ms": round(float(np.median(label)), 3),
                "census_ms": round(float(np.median(census)), 3)})
    trk.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "fill",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for name in FILL_KERNELS + ("k_comp_prune", "k_pack_classify", "k_cover_census"):
        v = [us(r) for r in rows if r["Kernel_Name"].startswith(name + "(") or r["Kernel_Name"].startswith(name + "<") or (" " + name + "(") in r["Kernel_Name"]
             or (" " + name + "<") in r["Kernel_Name"]]
        out[name] = {"launches": len(v), "median_us": round(float(np.median(v)), 2), "max_us": round(float(np.max(v)), 2),
                     "sum_ms": round(float(np.sum(v)) / 1e3, 3)} if v else None
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
    os.makedirs(os.path.join(ROOT, "profiles", "r26"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r26", "fill_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
