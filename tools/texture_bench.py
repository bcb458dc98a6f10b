#!/usr/bin/env python3
"""The texture bake at 512^3 on room 0's scan; writes profiles/r29/texture_bench.json and prints it as one JSON object.

  scan     the first `--frames` frames of room 0's scripted scan fused with colour at `--n`^3
  calls    host time (ms, median of `--reps`, the first call left out and reported on its own; a call ends in its own wait) of
           hsk_bake_texture with rgb alone and with rgb + normal_rgb + mask, at the default density (one texel per voxel) on the
           mesh simplified at c = `--cluster`; of the layout alone (hsk_texture_layout, host only); beside hsk_render_view (rgb
           alone) at the atlas's pixel count and hsk_extract_mesh_simplified on the same context.  texels_per_s: the owned texels
           over the bake's kernel time; owned_share: the owned texels over the atlas's
  kernels  the same work once more in ONE `rocprofv3 --kernel-trace` child (no counters in that run): medians (us) of
           k_bake_texture beside k_render_view
  No bar is set: nothing comparable has been measured on this volume.

usage: python tools/texture_bench.py [--reps 10] [--n 512] [--frames 60] [--cluster 4] [--skip kernels]"""
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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def work(args):
    """the scan and every measured call, 1 + reps times each"""
    import housescan_amd as hsk
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(args.frames)]
    trk = hsk.KinfuTracker(n=args.n, init_pose=poses[0])
    trk.enable_color()
    for p in poses:
        trk.process_frame_rgbd(hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0))
    trk.prepare_readout()
    out = {"volume": args.n, "frames": args.frames, "reps": args.reps, "cluster_voxels": args.cluster,
           "build_id": hsk._lib.load().hsk_build_id().decode()}

    def series(fn):
        t = [timed(fn) for _ in range(args.reps + 1)]
        return {"first_call_ms": round(t[0], 3), "ms": round(float(np.median(t[1:])), 3)}

    def simplified():
        return trk.extract_mesh_simplified(cluster_voxels=args.cluster, normals=False, rgb=False)
    v, f, _, _, _ = simplified()
    out["simplified"] = dict(series(simplified), vertices=int(len(v)), faces=int(len(f)))
    tpm = float(1.0 / (np.float32(trk.cfg.vol_size_m[0]) / np.float32(args.n)))
    out["layout"] = series(lambda: hsk.texture_layout(v, f, tpm))
    bk = trk.bake_texture(v, f, normal_rgb=True)
    W, H = bk["width"], bk["height"]
    out["atlas"] = {k: bk[k] for k in ("width", "height", "n_faces_charted", "n_faces_skipped", "n_blocks", "n_owned", "n_inside", "n_projected",
                                       "n_colored", "n_normal")}
    out["atlas"]["owned_share"] = round(bk["n_owned"] / max(W * H, 1), 4)
    out["bake_rgb"] = series(lambda: trk.bake_texture(v, f, rgb=True, normal_rgb=False, mask=False))
    out["bake_all"] = series(lambda: trk.bake_texture(v, f, rgb=True, normal_rgb=True, mask=True))
    # a view of as many pixels as the atlas has texels, from the scan's first pose
    vw = 1024
    vh = max(1, (W * H) // vw)
    out["render_view"] = dict(series(lambda: trk.render_view(pose=poses[0], width=vw, height=vh, fx=525.0 * vw / 640, fy=525.0 * vw / 640,
                                                             cx=vw / 2 - 0.5, cy=vh / 2 - 0.5, mode=hsk._lib.HSK_VIEW_COLOR, rgb=True, depth=False)),
                              width=vw, height=vh)
    trk.close()
    return out


def kernels(args):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(args.limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "tex",
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
    bakes = [us(r) for r in rows if "k_bake_texture" in r["Kernel_Name"]]
    n = args.reps + 1
    # the child bakes once with every output, then 1 + reps times rgb alone, then 1 + reps times every output
    return {"k_bake_texture_rgb_us": med(bakes[1:1 + n]), "k_bake_texture_all_us": med(bakes[1 + n:1 + 2 * n]), "launches": len(bakes),
            "k_render_view_us": med([us(r) for r in rows if "k_render_view" in r["Kernel_Name"]])}


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
            k = out["kernels"].get("k_bake_texture_all_us")
            if k:
                out["texels_per_s"] = round(out["atlas"]["n_owned"] / (k * 1e-6))
        except RuntimeError as e:
            out["kernels"] = {"error": str(e)}
    os.makedirs(os.path.join(ROOT, "profiles", "r29"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r29", "texture_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
