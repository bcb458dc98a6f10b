#!/usr/bin/env python3
"""The reach field at 512^3 on room 0's scan; writes profiles/r21/reach_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused at `--n`^3 (the clearance bench's volume); the seed is the
           centre of the voxel with the most clearance
  calls    host time (ms, median of `--reps`, the first call reported apart, ending in the call's own wait) of hsk_build_reach
           behind a volume change (the clearance field is rebuilt with it) and again (reused), of hsk_reach_at for 4096 points, of
           hsk_reach_path to the farthest reached voxel and of hsk_reach_floor, beside hsk_build_clearance and
           hsk_label_components behind a volume change; per build the rounds, the tiles relaxed in all and their share of all
           tiles x rounds; the scratch bytes.  With and without HSK_CLEAR_UNKNOWN (without it the never-observed space is walkable
           and the field fills the whole grid: the large case)
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace --stats` child (no counters in that run): medians (us) of the
           k_reach_* kernels beside the k_clear_* passes they follow
  No bar is set: nothing here had been measured before.

usage: python tools/reach_bench.py [--reps 5] [--n 512] [--frames 60] [--skip kernels] [--out FILE]"""
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
KERNELS = ("k_reach_init(", "k_reach_seed(", "k_reach_round(", "k_reach_stats(", "k_reach_path(", "k_clear_rows(", "k_clear_axis<1>", "k_clear_axis<2>",
           "k_clear_gather(", "k_comp_local(")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def stat(v):
    return {"first_ms": round(v[0], 3), "median_ms": round(float(np.median(v[1:])), 3)}


def work(args):
    """the scan and every measured call, 1 + reps times each"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    for p in poses:
        trk.process_frame(hsk.synth_room_depth(0, p))
    trk.prepare_readout()
    d0 = hsk.synth_room_depth(0, poses[0])
    par = trk.default_clearance_params()
    rp = trk.default_reach_params(par)
    # the seed: the roomiest voxel of the default clearance field.  (The camera's own position will not do with HSK_CLEAR_UNKNOWN: it
    # lies inside the sensor's near range, in space no frame of a turn on the spot has observed.)
    fld = trk.download_clearance(par)
    far = np.unravel_index(int(np.argmax(fld)), fld.shape)
    seed = [tuple((float(far[2 - i]) + 0.5) * 3.0 / args.n for i in range(3))]
    del fld
    pts = np.random.default_rng(1).uniform(0.0, 3.0, (4096, 3)).astype(np.float32)
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(), "seed": seed[0],
           "params": {"weight": list(par.weight), "max_d2": int(par.max_d2), "unit_m": float(par.unit_m), "min_d2": int(rp.min_d2), "max_cost": int(rp.max_cost)}}

    def changed(fn):
        trk.integrate(d0, poses[0])          # (a volume change: cached fields are void)
        trk.synchronize()
        return timed(fn)
    n = args.reps + 1
    cell = 3.0 / args.n
    for name, flags in (("unknown_blocks", par.flags), ("solids_only", 0)):
        o = {}
        o["build_clearance"] = stat([changed(lambda: trk.build_clearance(flags=flags)) for _ in range(n)])
        o["build_reach"] = stat([changed(lambda: trk.build_reach(seed, flags=flags)) for _ in range(n)])
        st = trk.build_reach(seed, flags=flags)
        trk.integrate(d0, poses[0])
        st = trk.build_reach(seed, flags=flags)
        relaxed, tiles = trk.reach_tiles_relaxed()
        o["stats"] = st
        o["tiles"], o["tiles_relaxed"] = tiles, relaxed
        o["share_of_tiles_x_rounds"] = round(relaxed / float(tiles * max(st["n_rounds"], 1)), 5)
        o["build_reach_reused"] = stat([timed(lambda: trk.build_reach(seed, flags=flags)) for _ in range(n)])
        o["at_4096"] = stat([timed(lambda: trk.reach_at(pts)) for _ in range(n)])
        g = trk.download_reach()
        val = np.where(g <= hsk.kinfu.REACH_MAX_COST, g, 0)
        far = np.unravel_index(int(np.argmax(val)), g.shape)
        goal = tuple((float(far[2 - i]) + 0.5) * cell for i in range(3))
        o["farthest_m"] = float(hsk.reach_metres(par, int(val[far])))
        o["path_voxels"] = int(len(trk.reach_path(goal, cap=1 << 16)))
        o["path"] = stat([timed(lambda: trk.reach_path(goal, cap=1 << 16)) for _ in range(n)])
        lo, hi = int(args.n * 0.3), int(args.n * 0.8)
        o["floor"] = stat([timed(lambda: trk.reach_floor(1, lo, hi, seed, flags=flags)) for _ in range(n)])
        o["floor_stats"] = trk.reach_floor(1, lo, hi, seed, flags=flags)[1]
        out[name] = o
    out["label_components"] = stat([changed(trk.label_components) for _ in range(n)])
    out["scratch_bytes"] = out["unknown_blocks"]["stats"]["scratch_bytes"]
    out["scratch_over_volume"] = round(out["scratch_bytes"] / (4.0 * args.n ** 3), 4)
    trk.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "reach",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", "1", "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for name in KERNELS:
        v = [us(r) for r in rows if name in r["Kernel_Name"]]
        out[name.rstrip("(") + "_us"] = ({"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2), "sum": round(sum(v), 1), "n": len(v)}
                                         if v else None)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=300, help="seconds the profiled child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "reach_bench.json"))
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
