#!/usr/bin/env python3
"""Surface components at 512^3 on room 0's scan; writes profiles/r18/components_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused at `--n`^3
  calls    host time (ms, median of `--reps`, the first left out, ending in the call's own wait) of hsk_label_components behind a
           volume change (first) and again (cached), of hsk_prune_components with the default parameters on the volume uploaded
           afresh and labelled (the labelling is not in its time), beside hsk_coverage_census (it caches nothing: every call
           sweeps) and hsk_pack_volume behind a volume change (its class pass runs again)
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) of the
           k_comp_* kernels beside k_pack_classify and k_cover_census, which stream the same words; label_over_classify = the five
           labelling kernels' sum over k_pack_classify (the three small launches of the row scan are not in it)
  No bar is set: nobody has measured a union-find on this volume.

usage: python tools/components_bench.py [--reps 10] [--n 512] [--frames 60] [--skip kernels]"""
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
LABEL_KERNELS = ("k_comp_local", "k_comp_merge", "k_comp_flatten", "k_comp_roots", "k_comp_records")


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
    rec, st = trk.label_components()
    p = trk.default_prune_params()
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(), "stats": st,
           "min_voxels": int(p.min_voxels), "below_min_voxels": int((rec["n_voxels"] < p.min_voxels).sum()), "head": [int(v) for v in rec["n_voxels"][:5]]}

    def changed(fn):
        trk.integrate(d0, poses[0])          # (a volume change: cached passes are void)
        trk.synchronize()
        return timed(fn)
    first = [changed(trk.label_components) for _ in range(args.reps + 1)][1:]
    cached = [timed(trk.label_components) for _ in range(args.reps + 1)][1:]
    census = [timed(trk.coverage) for _ in range(args.reps + 1)][1:]
    pack = [changed(trk.pack_volume) for _ in range(args.reps + 1)][1:]
    vol = trk.download_tsdf()
    prune, got = [], None
    for _ in range(args.reps + 1):
        trk.upload_tsdf(vol)
        trk.label_components()
        t0 = time.perf_counter()
        got = trk.prune_components()
        prune.append((time.perf_counter() - t0) * 1e3)
    out.update({"label_first_ms": round(float(np.median(first)), 3), "label_cached_ms": round(float(np.median(cached)), 3),
                "prune_ms": round(float(np.median(prune[1:])), 3), "prune": got, "census_ms": round(float(np.median(census)), 3),
                "pack_volume_ms": round(float(np.median(pack)), 3)})
    trk.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "comp",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = list(csv.DictReader(open(files[0])))

    def med(name):
        v = [us(r) for r in rows if name in r["Kernel_Name"]]
        return round(float(np.median(v)), 2) if v else None
    out = {name + "_us": med(name + "(") for name in LABEL_KERNELS}
    out.update({"k_comp_prune_us": med("k_comp_prune<"), "k_pack_classify_us": med("k_pack_classify("), "k_cover_census_us": med("k_cover_census(")})
    if all(out[name + "_us"] for name in LABEL_KERNELS) and out["k_pack_classify_us"]:
        out["label_kernels_us"] = round(sum(out[name + "_us"] for name in LABEL_KERNELS), 2)
        out["label_over_classify"] = round(out["label_kernels_us"] / out["k_pack_classify_us"], 2)
        if out["k_cover_census_us"]:
            out["label_over_census"] = round(out["label_kernels_us"] / out["k_cover_census_us"], 2)
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
    os.makedirs(os.path.join(ROOT, "profiles", "r18"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r18", "components_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
