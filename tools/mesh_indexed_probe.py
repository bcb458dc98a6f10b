#!/usr/bin/env python3
"""The indexed marching-cubes mesh at 512^3, one JSON line.  Two scans with colour (the scripted stream, and room 0 as a
sensor sees it), then per scan, as medians over a few repetitions in ms:
  cubes_ms          hsk_extract_mesh_cubes, query + fill (the triangle soup)
  indexed_geom_ms   hsk_extract_mesh_indexed, vertices + faces (query + fill)
  indexed_attrs_ms  hsk_extract_mesh_indexed with normals and colour
  soup_ply_ms       the soup + hsk_write_ply_mesh (the host weld and the file)
  indexed_ply_ms    indexed with normals and colour + hsk_write_ply_indexed
Each timed read-out runs its own count pass (the call before it counted another product).  The kernels' times come from
`rocprofv3 --kernel-trace --stats --output-format csv` around a child process that does the same read-outs (on failure
the error's tail is reported instead).

usage: python tools/mesh_indexed_probe.py [--frames 200] [--n 512] [--reps 5] [--no-rocprof]"""
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
import housescan_amd as hsk  # noqa: E402
from housescan_amd import products as P  # noqa: E402


def frames_of(stream, count):
    if stream == "scripted":
        poses = [hsk.synth_pose(k) for k in range(count)]
        return poses, [hsk.synth_depth(p) for p in poses], [hsk.synth_rgb(p) for p in poses]
    poses, depth = hsk.synth_sensor_frames(count, room=0, scan=720)
    return poses, depth, [hsk.synth_rgb(p, 0) for p in poses]


def scan(n, stream, count):
    poses, depth, rgb = frames_of(stream, count)
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    trk.enable_color()
    trk.submit_frame_rgbd(depth[0], rgb[0])
    for k in range(1, len(depth)):
        trk.submit_frame_rgbd(depth[k], rgb[k])
        trk.wait_frame()
    trk.wait_frame()
    trk.prepare_readout()
    return trk


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return 1e3 * (time.perf_counter() - t0), r


def readouts(trk, reps, tmp):
    """the five timings (ms, medians) and the mesh's sizes"""
    t = {k: [] for k in ("cubes_ms", "indexed_geom_ms", "indexed_attrs_ms", "soup_ply_ms", "indexed_ply_ms")}
    soup_path, idx_path = os.path.join(tmp, "soup.ply"), os.path.join(tmp, "indexed.ply")
    trk.extract_mesh(cubes=True)
    trk.extract_mesh_indexed()   # (first use: allocations, the code object)
    for _ in range(reps):
        ms, (soup, n_tri) = timed(lambda: trk.extract_mesh(cubes=True))
        t["cubes_ms"].append(ms)
        ms, geom = timed(lambda: trk.extract_mesh_indexed(normals=False, rgb=False))
        t["indexed_geom_ms"].append(ms)
        trk.extract_cloud()      # (another product counted: the next call counts again)
        ms, mesh = timed(lambda: trk.extract_mesh_indexed())
        t["indexed_attrs_ms"].append(ms)
        ms, _ = timed(lambda: P.write_ply_mesh(soup_path, trk.extract_mesh(cubes=True)[0]))
        t["soup_ply_ms"].append(ms)

        def indexed_ply():
            v, f, nrm, col, _ = trk.extract_mesh_indexed()
            P.write_ply_indexed(idx_path, v, f, normals=nrm, rgb=col)
        ms, _ = timed(indexed_ply)
        t["indexed_ply_ms"].append(ms)
    v, f, nrm, col, unc = mesh
    wv, _ = P.weld_triangles(soup)
    out = {k: round(float(np.median(x)), 3) for k, x in t.items()}
    out.update({"triangles": int(n_tri), "vertices": len(v), "welded_vertices": len(wv), "n_uncolored": int(unc),
                "soup_ply_bytes": os.path.getsize(soup_path), "indexed_ply_bytes": os.path.getsize(idx_path),
                "soup_bytes": 36 * int(n_tri), "indexed_bytes": 12 * len(v) + 12 * len(f)})
    out["indexed_geom_over_cubes"] = round(out["indexed_geom_ms"] / out["cubes_ms"], 3)
    out["indexed_attrs_over_cubes"] = round(out["indexed_attrs_ms"] / out["cubes_ms"], 3)
    out["soup_ply_over_indexed_ply"] = round(out["soup_ply_ms"] / out["indexed_ply_ms"], 2)
    return out


KERNELS = (("mark", "k_mesh_index_mark"), ("rows", "k_mesh_index_rows"), ("verts", "k_mesh_index_verts"),
           ("faces", "k_mesh_index_faces"), ("cubes_count", "k_extract_mesh_mc<false>"), ("cubes_write", "k_extract_mesh_mc<true>"),
           ("scan_rows_sum", "k_scan_rows_sum"), ("scan_rows_top", "k_scan_rows_top"), ("scan_rows_fill", "k_scan_rows_fill"))


def kernel_stats(a, stream):
    """calls and mean / min / max (us) of the read-out kernels in a child run under rocprofv3; {"error": ...} on failure"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "probe", "--", sys.executable,
               os.path.abspath(__file__), "--child", stream, "--frames", str(a.frames), "--n", str(a.n), "--reps", str(a.reps)]
        try:
            p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
        except (OSError, subprocess.SubprocessError) as e:
            return {"error": f"{type(e).__name__}: {e}"}
        if p.returncode != 0:
            return {"error": f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no *kernel_stats.csv written: " + p.stdout[-600:]}
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            for key, pat in KERNELS:
                if pat in name and key not in out:
                    out[key] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                                "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
        return out if "mark" in out else {"error": "k_mesh_index_mark not in " + files[0], **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        trk = scan(a.n, a.child, a.frames)
        with tempfile.TemporaryDirectory() as tmp:
            readouts(trk, a.reps, tmp)
        trk.close()
        return
    out = {"n": a.n, "frames": a.frames, "reps": a.reps, "build_id": hsk._lib.load().hsk_build_id().decode()}
    for stream in ("scripted", "room0_sensor"):
        trk = scan(a.n, stream, a.frames)
        with tempfile.TemporaryDirectory() as tmp:
            out[stream] = readouts(trk, a.reps, tmp)
        trk.close()
        out[stream]["kernels"] = None if a.no_rocprof else kernel_stats(a, stream)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
