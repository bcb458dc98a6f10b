#!/usr/bin/env python3
"""The keyframe bake at 512^3 on room 0's scan; writes profiles/r30/keytex_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused with colour at `--n`^3 (the colour volume is there for
           hsk_bake_texture's side of the comparison and as the keyframe bake's fallback)
  store    640 x 480 keyframes taken from the scan's frames at equal spacing, n = 1, 8, 32, 128 (a scan shorter than n repeats its
           frames: a repeated keyframe passes wherever its twin does, which is the expensive case)
  calls    host time (ms, median of `--reps`, the first call left out and reported on its own; a call ends in its own wait) of
           hsk_bake_texture_keyframes with rgb + mask + source in both modes for every n, at the default density (one texel per
           voxel) on the mesh simplified at c = `--cluster`, beside hsk_bake_texture (rgb + mask) on the same mesh; the time of
           one hsk_add_keyframe; n_pairs_seen per owned texel; the store's bytes
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) of
           k_bake_keytex per (n, mode) beside k_bake_texture
  No bar is set: nothing comparable has been measured on this volume.

usage: python tools/keytex_bench.py [--reps 10] [--n 512] [--frames 60] [--cluster 4] [--skip kernels]"""
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
COUNTS = (1, 8, 32, 128)
MODES = (("best", 0), ("blend", 1))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def work(args):
    """the scan and every measured call, 1 + reps times each, in a fixed order (the kernel trace is read by position)"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    trk.enable_color()
    frames = []
    for p in poses:
        d, c = hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0)
        pose, _ = trk.process_frame_rgbd(d, c)
        frames.append((d, c, np.array(pose, np.float32)))
    trk.prepare_readout()
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "cluster_voxels": args.cluster, "keyframe_size": [640, 480],
           "build_id": hsk._lib.load().hsk_build_id().decode()}

    def series(fn):
        t = [timed(fn) for _ in range(args.reps + 1)]
        return {"first_call_ms": round(t[0], 3), "ms": round(float(np.median(t[1:])), 3)}

    v, f, _, _, _ = trk.extract_mesh_simplified(cluster_voxels=args.cluster, normals=False, rgb=False)
    out["mesh"] = {"vertices": int(len(v)), "faces": int(len(f))}
    out["bake_texture"] = series(lambda: trk.bake_texture(v, f, rgb=True, normal_rgb=False, mask=True))
    out["keyframes"] = {}
    for n in COUNTS:
        trk.release_keyframes()
        trk.enable_keyframes(n)
        picks = [frames[(i * len(frames)) // n if n <= len(frames) else i % len(frames)] for i in range(n)]
        t_add = [timed(lambda fr=fr: trk.add_keyframe(*fr)) for fr in picks]
        rec = {"store_bytes": trk.keyframe_count()["bytes"], "add_keyframe_ms": round(float(np.median(t_add)), 3)}
        for name, mode in MODES:
            bk = trk.bake_texture_keyframes(v, f, rgb=True, normal_rgb=False, mask=True, source=True, mode=mode)
            rec[name] = dict(series(lambda mode=mode: trk.bake_texture_keyframes(v, f, rgb=True, normal_rgb=False, mask=True, source=True, mode=mode)),
                             **{k: bk[k] for k in ("n_keyed", "n_fallback", "n_uncolored", "n_pairs_seen", "n_pairs_occluded")},
                             pairs_seen_per_texel=round(bk["n_pairs_seen"] / max(bk["n_owned"], 1), 3))
        out["atlas"] = {k: bk[k] for k in ("width", "height", "n_owned", "n_inside", "n_projected", "n_normal")}
        out["keyframes"][str(n)] = rec
    trk.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "keytex",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames),
               "--cluster", str(args.cluster)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))

    def med(v):
        return round(float(np.median(v)), 2) if len(v) else None
    key = [us(r) for r in rows if "k_bake_keytex" in r["Kernel_Name"]]
    per = args.reps + 2                                           # the child bakes once for the counts, then 1 + reps times, per (n, mode)
    out = {"k_bake_texture_us": med([us(r) for r in rows if "k_bake_texture" in r["Kernel_Name"]][1:]), "launches": len(key)}
    at = 0
    for n in COUNTS:
        for name, _ in MODES:
            out[f"k_bake_keytex_n{n}_{name}_us"] = med(key[at + 2:at + per])
            at += per
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--cluster", type=int, default=4)
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
    os.makedirs(os.path.join(ROOT, "profiles", "r30"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r30", "keytex_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
