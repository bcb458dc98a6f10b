#!/usr/bin/env python3
"""Scan coverage at 512^3 on a room scan; writes profiles/r17/coverage_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused at `--n`^3 (the level turn: floor and ceiling stay open)
  calls    host time (ms, median of `--reps`, ending in the call's own wait) of hsk_coverage_census, of hsk_pack_volume behind
           a volume change (its class pass runs again), of hsk_score_views with the default probe for 1, 64, 1024 and 4096
           poses around the last pose, and of hsk_score_cloud on the next frame's level-2 cloud under 1024 poses
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) of
           k_cover_census + k_cover_census_sum beside k_pack_classify, of k_cover_rays per pose count, of k_reloc_score
  Samples per second of hsk_score_views: NOMINAL ones -- poses x rays x samples per ray -- and WALKED ones: a ray that has
  ended gathers nothing more, and the samples the rays take before they end are counted by the numpy twin (tests/cover_twin.py)
  on the downloaded volume for `--twin-poses` evenly spaced poses of each count (their scores must equal the device's) and
  scaled to the count.  hsk_score_cloud's are points x poses (8 taps each).  No bar is set: nobody has measured any of this.

usage: python tools/coverage_bench.py [--reps 10] [--n 512] [--frames 60] [--twin-poses 12] [--skip kernels]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
COUNTS = (1, 64, 1024, 4096)
CLOUD_POSES = 1024


def candidates(hsk, centre, count):
    """`count` poses around `centre`: a lattice of 0.15 m and 20 degrees, repeated up to the count"""
    if count == 1:
        return hsk.pose_lattice(centre, 0.15, 0, 0.0, 0)
    base = hsk.pose_lattice(centre, 0.15, 2, float(np.radians(20.0)), 2)      # 3125
    return np.concatenate([base] * (count // len(base) + 1))[:count]


def median_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def walked_fraction(vol, size, probe, poses, scores, n_twin):
    """the share of the nominal samples that the rays of `n_twin` evenly spaced poses take before they end, on the twin"""
    import cover_twin as CT
    pr = CT.probe(probe.width, probe.height, probe.fx, probe.fy, probe.cx, probe.cy, probe.near_m, probe.far_m, probe.step_m)
    pick = np.unique(np.linspace(0, len(poses) - 1, min(n_twin, len(poses))).astype(int))
    walked = 0
    for j in range(0, len(pick), 4):
        sel = pick[j:j + 4]
        r = CT.ray_walk(vol, size, pr, poses[sel])
        for i, k in enumerate(sel):      # (the twin walks what the device walked: the same classes and gain)
            assert [int((r["cls"][i] == c).sum()) for c in range(5)] == [int(scores[k][n]) for n in CT.CLASSES] and int(r["gain"][i].sum()) == int(scores[k]["gain"])
        walked += int(r["walked"].sum())
    return walked / (len(pick) * pr["width"] * pr["height"] * CT.n_samples(pr)), len(pick)


def work(args, twin=False):
    """the scan and every measured call, 1 + reps times each in a fixed order (the kernel trace is cut by that order)"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames + 1)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    last = poses[0]
    for p in poses[:-1]:
        last, _ = trk.process_frame(hsk.synth_room_depth(0, p))
    depth = hsk.synth_room_depth(0, poses[-1])
    trk.preprocess(depth)
    cloud = np.ascontiguousarray(trk.download_map(0, 2).reshape(3, -1).T)
    trk.prepare_readout()
    probe = hsk.default_probe(trk)
    n_samples = int(min(4096.0, np.floor((float(probe.far_m) - float(probe.near_m)) / float(probe.step_m)) + 1.0))
    rays = probe.width * probe.height
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "build_id": hsk._lib.load().hsk_build_id().decode(),
           "probe": {"width": probe.width, "height": probe.height, "near_m": probe.near_m, "far_m": probe.far_m, "step_m": probe.step_m,
                     "samples_per_ray": n_samples},
           "census": trk.coverage()}
    out["census"]["faces"] = [int(v) for v in out["census"]["faces"]]
    out["census_ms"] = round(median_ms(trk.coverage, args.reps), 3)
    d0 = hsk.synth_room_depth(0, poses[0])

    def pack():
        trk.integrate(d0, poses[0])          # (a volume change: the class pass of the next pack runs again)
        trk.synchronize()
        t0 = time.perf_counter()
        trk.pack_volume()
        return (time.perf_counter() - t0) * 1e3
    pack()
    out["pack_volume_ms"] = round(float(np.median([pack() for _ in range(args.reps)])), 3)
    out["score_views"] = []
    vol = trk.download_tsdf() if twin and args.twin_poses > 0 else None
    for count in COUNTS:
        c = candidates(hsk, last, count)
        got = {}

        def score():
            got["s"] = trk.score_views(c)
        ms = median_ms(score, args.reps)
        s = got["s"]
        out["score_views"].append({"n_poses": len(c), "call_ms": round(ms, 3), "nominal_samples": len(c) * rays * n_samples,
                                   "nominal_samples_per_s": round(len(c) * rays * n_samples / (ms * 1e-3)),
                                   "rays_by_class": {k: int(s[k].astype(np.int64).sum()) for k in ("n_hit", "n_frontier", "n_open", "n_blind", "n_outside")},
                                   "gain": int(s["gain"].sum())})
        if vol is not None:
            frac, n_twin = walked_fraction(vol, tuple(trk.cfg.vol_size_m), probe, c.reshape(-1, 4, 4), s, args.twin_poses)
            out["score_views"][-1].update({"twin_poses": n_twin, "walked_fraction": round(frac, 4),
                                           "walked_samples_per_s": round(frac * len(c) * rays * n_samples / (ms * 1e-3))})
    c = candidates(hsk, last, CLOUD_POSES)
    ms = median_ms(lambda: trk.score_cloud(cloud, c), args.reps)
    out["score_cloud"] = {"n_poses": len(c), "points": len(cloud), "call_ms": round(ms, 3), "samples": len(c) * len(cloud),
                          "samples_per_s": round(len(c) * len(cloud) / (ms * 1e-3)), "taps_per_s": round(8 * len(c) * len(cloud) / (ms * 1e-3))}
    trk.close()
    return out


def kernels(args, calls):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "cover",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(args.n), "--reps", str(args.reps), "--frames", str(args.frames)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))

    def of(name):
        return [us(r) for r in rows if name in r["Kernel_Name"]]

    def med(v):
        return round(float(np.median(v)), 2) if len(v) else None
    per = args.reps + 1
    out = {"k_cover_census_us": med(of("k_cover_census(")), "k_cover_census_sum_us": med(of("k_cover_census_sum")),
           "k_pack_classify_us": med(of("k_pack_classify(")), "k_reloc_score_us": med(of("k_reloc_score")), "k_cover_rays": []}
    rays = of("k_cover_rays<false>")      # (1 + reps launches per pose count, in COUNTS' order)
    if len(rays) == per * len(COUNTS):
        for i, sv in enumerate(calls["score_views"]):
            k_us = med(rays[i * per + 1:(i + 1) * per])
            out["k_cover_rays"].append({"n_poses": sv["n_poses"], "kernel_us": k_us, "nominal_samples_per_s": round(sv["nominal_samples"] / (k_us * 1e-6))})
            if "walked_fraction" in sv:
                out["k_cover_rays"][-1]["walked_samples_per_s"] = round(sv["walked_fraction"] * sv["nominal_samples"] / (k_us * 1e-6))
    else:
        out["k_cover_rays_error"] = f"{len(rays)} launches in the trace, {per * len(COUNTS)} expected"
    if out["k_reloc_score_us"]:
        out["k_reloc_score_samples_per_s"] = round(calls["score_cloud"]["samples"] / (out["k_reloc_score_us"] * 1e-6))
    if out["k_cover_census_us"] and out["k_pack_classify_us"]:
        out["census_over_classify"] = round((out["k_cover_census_us"] + (out["k_cover_census_sum_us"] or 0.0)) / out["k_pack_classify_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--skip", default="")
    ap.add_argument("--twin-poses", type=int, default=12, help="poses of each count whose walked samples the twin counts (0: none)")
    ap.add_argument("--stage", default="all", choices=("all", "child"))
    ap.add_argument("--limit", type=int, default=240, help="seconds the profiled child may take")
    args = ap.parse_args()
    if args.stage == "child":
        work(args)
        return 0
    out = work(args, twin=True)
    if "kernels" not in args.skip.split(","):
        try:
            out["kernels"] = kernels(args, out)
        except RuntimeError as e:
            out["kernels"] = {"error": str(e)}
    os.makedirs(os.path.join(ROOT, "profiles", "r17"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r17", "coverage_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
