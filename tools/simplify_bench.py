#!/usr/bin/env python3
"""The simplified mesh at 512^3 on room 0's scan; writes profiles/r19/simplify_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused at `--n`^3 (the components bench's volume)
  calls    host time (ms, median of `--reps`, the first call of each kind left out and reported on its own as *_first_call_ms; a
           call ends in its own wait) of hsk_extract_mesh_simplified -- counts only then the fill, as the wrapper does -- at
           c = 2, 4, 8, 16 in both modes: behind a volume change (`first`: the indexed mesh's count pass runs again) and again
           (`repeat`: both count passes are found in place), beside hsk_extract_mesh_indexed on the same context, likewise.
           over_indexed = the simplified call over the indexed mesh's, which reads the same volume and writes more
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) of the
           k_simp_* kernels per cluster size (the launches are told apart by their order), beside the indexed mesh's kernels
  No bar is set: nobody has measured a simplifier on this volume.

usage: python tools/simplify_bench.py [--reps 10] [--n 512] [--frames 60] [--skip kernels]"""
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
CLUSTERS = (2, 4, 8, 16)
SIMP_KERNELS = ("k_simp_faces<false>", "k_simp_rows", "k_simp_list", "k_simp_gather<", "k_simp_solve", "k_simp_faces<true>")
INDEXED_KERNELS = ("k_mesh_index_mark", "k_mesh_index_rows", "k_mesh_index_verts", "k_mesh_index_faces")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def work(args):
    """the scan and every measured call, 1 + reps times each"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.process_frame(hsk.synth_room_depth(0, p))
    trk.prepare_readout()
    d0 = hsk.synth_room_depth(0, poses[0])
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode()}

    def changed(fn):
        trk.integrate(d0, poses[0])          # (a volume change: the cached count pass is void)
        trk.synchronize()
        return timed(fn)

    def series(fn):
        first = [changed(fn) for _ in range(args.reps + 1)]
        repeat = [timed(fn) for _ in range(args.reps + 1)]
        return {"first_call_ms": round(first[0], 3), "first_ms": round(float(np.median(first[1:])), 3),
                "repeat_ms": round(float(np.median(repeat[1:])), 3)}

    def indexed():
        return trk.extract_mesh_indexed(normals=True, rgb=False)
    v, f, _, _, _ = indexed()
    out["indexed"] = dict(series(indexed), vertices=int(len(v)), faces=int(len(f)))
    out["simplified"] = {}
    for c in CLUSTERS:
        for mode, name in ((hsk.SIMPLIFY_QUADRIC, "quadric"), (hsk.SIMPLIFY_MEAN, "mean")):
            def call():
                return trk.extract_mesh_simplified(cluster_voxels=c, mode=mode, normals=True, rgb=False)
            sv, sf, _, _, st = call()
            row = dict(series(call), vertices=int(len(sv)), faces=int(len(sf)), stats=st)
            row["first_over_indexed"] = round(row["first_ms"] / out["indexed"]["first_ms"], 3)
            row["repeat_over_indexed"] = round(row["repeat_ms"] / out["indexed"]["repeat_ms"], 3)
            out["simplified"][f"c{c}_{name}"] = row
    trk.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "simp",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))

    def med(v):
        return round(float(np.median(v)), 2) if len(v) else None
    out = {"indexed": {name + "_us": med([us(r) for r in rows if name + "(" in r["Kernel_Name"]]) for name in INDEXED_KERNELS}}
    # the child runs the cluster sizes one after the other, both modes each: a launch's size is its place among the launches of
    # its kernel.  The gather and the solve run in every call (2 per wrapper call), the write pass of the faces once per wrapper call
    # (k_simp_gather<WAVES>: whichever form the cluster size takes)
    per_kernel = {name.rstrip("<"): [us(r) for r in rows if (name if name.endswith("<") else name + "(") in r["Kernel_Name"]] for name in SIMP_KERNELS}
    for i, c in enumerate(CLUSTERS):
        block = {}
        for name, v in per_kernel.items():
            n = len(v) // len(CLUSTERS)
            block[name + "_us"] = med(v[i * n:(i + 1) * n]) if n else None
            if name == "k_simp_solve" and n >= 2:   # (the first half of a size's launches solve the quadric, the second take the mean)
                block["k_simp_solve_quadric_us"] = med(v[i * n:i * n + n // 2])
                block["k_simp_solve_mean_us"] = med(v[i * n + n // 2:(i + 1) * n])
        if block.get("k_simp_solve_quadric_us") is not None:
            block["k_simp_solve_us"] = block["k_simp_solve_quadric_us"]   # (sum_us: one quadric call with every array)
        have = [v for v in (block[k.rstrip("<") + "_us"] for k in SIMP_KERNELS) if v is not None]
        block["sum_us"] = round(sum(have), 2) if have else None
        out[f"c{c}"] = block
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=400, help="seconds the profiled child may take")
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
    os.makedirs(os.path.join(ROOT, "profiles", "r19"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r19", "simplify_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
