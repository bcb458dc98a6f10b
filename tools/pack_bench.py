#!/usr/bin/env python3
"""Volume images against the raw transfers they replace (profiles/r13/pack_bench.json, profiles/r13/pack_notes.md).

Every GPU step is a child process of its own under its own time limit; the steps run in turn and the first that fails ends the
run (nothing more is started on the GPU behind it).

  main      room 0's whole RGB-D scan at 512^3.  Median of `--reps`, the second call of each function and later:
            pack      hsk_pack_volume (size query + fill) behind a volume change -- one frame integrated outside the clock, so
                      the call pays its class / offset pass and the write-back of the deferred weights
            download  the only path the parent commit offers for the same data, NOT the code under test: hsk_download_tsdf +
                      hsk_download_color into preallocated arrays, behind the same volume change.  The bar: pack <= download
            pack_warm the same call with the pass of the previous one in place (no volume change)
            unpack    hsk_unpack_volume of that image;  upload: hsk_upload_tsdf + hsk_upload_color.  The bar: unpack <= upload
            save / load  hsk_save_volume / hsk_load_volume on the local disk (reported only)
            and the packed share, the class counts
  stream    SURVEY.md 8(d)'s scripted stream, depth only, at 1024^3: pack / unpack / the raw pair, share, counts (reported only)
  kernels   per-kernel medians from ONE `rocprofv3 --kernel-trace --stats` child (no counters in that run)

usage: python tools/pack_bench.py [--reps 10] [--n 512] [--stream-n 1024] [--stream-frames 120] [--skip stream,kernels]"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT_DIR = os.path.join(ROOT, "profiles", "r13")
SCAN = 720


def scan_room(hsk, n, frames=SCAN):
    """room 0's three-turn scan, RGB-D, pipelined (the frames are rendered eight at a time)"""
    poses = [hsk.synth_room_pose(0, k, SCAN) for k in range(frames)]
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    trk.enable_color()
    sent = 0
    with ThreadPoolExecutor(8) as ex:
        for lo in range(0, frames, 48):
            for d, c in ex.map(lambda p: (hsk.synth_room_depth(0, p), hsk.synth_rgb(p, 0)), poses[lo:lo + 48]):
                trk.submit_frame_rgbd(d, c)
                sent += 1
                if sent >= 2:
                    trk.wait_frame()
    trk.wait_frame()
    trk.synchronize()
    return trk


def stats(t):
    return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def info_block(info, raw_bytes):
    return {"bytes": int(info["total_bytes"]), "share_of_raw": round(info["total_bytes"] / raw_bytes, 4),
            "tsdf_bricks": [int(x) for x in info["tsdf_bricks"]], "color_bricks": [int(x) for x in info["color_bricks"]],
            "n_bricks": int(info["n_bricks"])}


class Packer:
    """hsk_pack_volume into one preallocated buffer (what a host that saves behind every scan would keep)"""

    def __init__(self, hsk, trk):
        self.hsk, self.trk, self.lib = hsk, trk, trk.lib
        self.n, self.info = C.c_size_t(), hsk._lib.HskVolumeInfo()
        self.buf = np.empty(0, np.uint8)

    def __call__(self):
        trk = self.trk
        trk._ck(self.lib.hsk_pack_volume(trk.h, None, 0, C.byref(self.n), C.byref(self.info)))
        if self.buf.size < self.n.value:
            self.buf = np.empty(self.n.value + (self.n.value >> 3), np.uint8)
            self.buf[:] = 0     # (pages faulted in outside any clock that matters: the first call is never timed)
        trk._ck(self.lib.hsk_pack_volume(trk.h, self.buf.ctypes.data, self.buf.size, C.byref(self.n), C.byref(self.info)))
        return self.buf[:self.n.value]


def bench_volume(hsk, trk, reps, change, color, tmp):
    """the timings of one context; change(): a small volume change outside the clocks"""
    from housescan_amd.kinfu import _info_dict
    lib = trk.lib
    tsdf = trk.download_tsdf()
    col = trk.download_color() if color else None
    raw_bytes = tsdf.nbytes + (col.nbytes if color else 0)
    pack = Packer(hsk, trk)
    pack()
    out = {}

    def timed(fn, before=None):
        t = []
        for _ in range(reps):
            if before:
                before()
                trk.synchronize()
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return stats(t)

    def download():
        trk.download_tsdf(out=tsdf)
        if color:
            trk._ck(lib.hsk_download_color(trk.h, col.ctypes.data))

    def upload():
        trk.upload_tsdf(tsdf)
        if color:
            trk.upload_color(col)

    out["pack"] = timed(pack, change)
    out["download_pair"] = timed(download, change)
    out["pack_warm"] = timed(pack)
    out["download_pair_warm"] = timed(download)
    img = pack().tobytes()
    out["image"] = info_block(_info_dict(pack.info), raw_bytes)
    download()
    upload()
    trk.unpack_volume(img)
    out["unpack"] = timed(lambda: trk.unpack_volume(img))
    out["upload_pair"] = timed(upload)
    path = os.path.join(tmp, "volume.hskv")
    trk.save_volume(path)
    out["save"] = timed(lambda: trk.save_volume(path), change)
    out["load"] = timed(lambda: trk.load_volume(path))
    out["pack_not_slower"] = bool(out["pack"]["median_ms"] <= out["download_pair"]["median_ms"])
    out["unpack_not_slower"] = bool(out["unpack"]["median_ms"] <= out["upload_pair"]["median_ms"])
    return out


def stage_main(a):
    import housescan_amd as hsk
    trk = scan_room(hsk, a.n)
    pose = hsk.synth_room_pose(0, 40, SCAN)
    depth, rgb = hsk.synth_room_depth(0, pose), hsk.synth_rgb(pose, 0)

    def change():
        trk.integrate(depth, pose)
        trk.integrate_color(depth, rgb, pose)

    with tempfile.TemporaryDirectory() as tmp:
        out = bench_volume(hsk, trk, a.reps, change, True, tmp)
    out["build_id"] = hsk._lib.load().hsk_build_id().decode()
    trk.close()
    return out


def stage_stream(a):
    import housescan_amd as hsk
    trk = hsk.KinfuTracker(n=a.stream_n)
    poses = [hsk.synth_pose(k) for k in range(a.stream_frames)]
    lost = 0
    with ThreadPoolExecutor(8) as ex:
        for k, d in enumerate(ex.map(hsk.synth_depth, poses)):
            lost += 0 if (trk.process_frame(d)[1] or k == 0) else 1
    d0 = hsk.synth_depth(poses[-1])

    with tempfile.TemporaryDirectory() as tmp:
        out = bench_volume(hsk, trk, max(3, a.reps // 2), lambda: trk.integrate(d0, poses[-1]), False, tmp)
    out["frames"], out["lost"] = a.stream_frames, lost
    trk.close()
    return out


def stage_child(a):
    """what the kernels stage looks for in the trace: packs behind a volume change, and unpacks"""
    import housescan_amd as hsk
    trk = scan_room(hsk, a.n, frames=240)
    pose = hsk.synth_room_pose(0, 40, SCAN)
    depth = hsk.synth_room_depth(0, pose)
    pack = Packer(hsk, trk)
    for _ in range(min(a.reps, 5) + 1):
        trk.integrate(depth, pose)
        img = pack()
    img = img.tobytes()
    for _ in range(min(a.reps, 5) + 1):
        trk.unpack_volume(img)
    trk.close()
    return {}


def stage_kernels(a):
    def us(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    with tempfile.TemporaryDirectory() as d:
        # (timeout(1) leads a process group of its own and signals the whole group: the profiled child goes with rocprofv3)
        cmd = ["timeout", "-k", "10", str(a.limit - 30), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "pack",
               "--", sys.executable, os.path.abspath(__file__), "--stage", "child", "--n", str(a.n), "--reps", str(a.reps)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exited {p.returncode}: " + p.stdout[-600:])
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("no *kernel_trace.csv written: " + p.stdout[-600:])
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for key, name in (("classify", "k_pack_classify("), ("classify_color", "k_pack_classify_color"), ("scan_sums", "k_pack_scan_sums"),
                      ("scan_blocks", "k_pack_scan_blocks"), ("scan_final", "k_pack_scan_final"), ("gather_tsdf", "k_pack_gather<false"),
                      ("gather_color", "k_pack_gather<true"), ("scatter_tsdf", "k_pack_scatter<false"),
                      ("scatter_color", "k_pack_scatter<true"), ("sizes", "k_pack_sizes")):
        t = [us(r) for r in rows if name in r["Kernel_Name"]][1:]
        out[key] = ({"median_us": round(float(np.median(t)), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "launches": len(t)}
                    if t else {"error": "no launch in the trace"})
    return out


STAGES = {"main": (stage_main, 420), "stream": (stage_stream, 420), "kernels": (stage_kernels, 300), "child": (stage_child, 280)}


def notes(out):
    m = out.get("main", {})
    lines = ["# Volume images: what was measured (tools/pack_bench.py)", ""]
    if "image" in m:
        im = m["image"]
        lines += [f"Room 0's whole RGB-D scan at {out['n']}^3 (build {m.get('build_id')}): the image is {im['bytes']} bytes, "
                  f"{im['share_of_raw']} of the raw TSDF + colour; TSDF bricks ZERO / UNIFORM / SPLIT / RAW {im['tsdf_bricks']}, "
                  f"colour bricks ZERO / RAW {im['color_bricks']}.", "",
                  "| call | median ms | against | median ms |", "|---|---|---|---|",
                  f"| hsk_pack_volume (behind a volume change) | {m['pack']['median_ms']} | download_tsdf + download_color | {m['download_pair']['median_ms']} |",
                  f"| hsk_pack_volume (pass in place) | {m['pack_warm']['median_ms']} | the pair, no change in front | {m['download_pair_warm']['median_ms']} |",
                  f"| hsk_unpack_volume | {m['unpack']['median_ms']} | upload_tsdf + upload_color | {m['upload_pair']['median_ms']} |",
                  f"| hsk_save_volume | {m['save']['median_ms']} | | |", f"| hsk_load_volume | {m['load']['median_ms']} | | |", "",
                  f"The bar: pack <= download pair: {m['pack_not_slower']}; unpack <= upload pair: {m['unpack_not_slower']}.", ""]
    s = out.get("stream", {})
    if "image" in s:
        im = s["image"]
        lines += [f"The scripted stream, depth only, {s['frames']} frames at {out['stream_n']}^3 ({s['lost']} lost): {im['bytes']} bytes, "
                  f"{im['share_of_raw']} of the raw TSDF; bricks {im['tsdf_bricks']}; pack {s['pack']['median_ms']} ms against "
                  f"{s['download_pair']['median_ms']} ms for hsk_download_tsdf; unpack {s['unpack']['median_ms']} ms against "
                  f"{s['upload_pair']['median_ms']} ms for hsk_upload_tsdf; save {s['save']['median_ms']} ms, load {s['load']['median_ms']} ms.", ""]
    k = out.get("kernels", {})
    if k and "error" not in k:
        lines += ["Kernels (one rocprofv3 --kernel-trace --stats child, medians in us): " +
                  ", ".join(f"{key} {v.get('median_us', '-')}" for key, v in k.items()) + ".", ""]
    for key in ("main", "stream", "kernels"):
        if isinstance(out.get(key), dict) and "error" in out[key]:
            lines += [f"Stage `{key}` did not complete: {out[key]['error']}", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--stream-n", type=int, default=1024)
    ap.add_argument("--stream-frames", type=int, default=120)
    ap.add_argument("--skip", default="")
    ap.add_argument("--stage", default=None)
    ap.add_argument("--limit", type=int, default=300)
    a = ap.parse_args()
    if a.stage:      # a child: one stage, its result as the last line of its output
        print("RESULT " + json.dumps(STAGES[a.stage][0](a)))
        return
    out = {"n": a.n, "stream_n": a.stream_n, "reps": a.reps, "scan_frames": SCAN}
    skip = set(x for x in a.skip.split(",") if x)
    for key in ("main", "stream", "kernels"):
        if key in skip:
            continue
        limit = STAGES[key][1]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--stage", key, "--n", str(a.n), "--reps", str(a.reps),
               "--stream-n", str(a.stream_n), "--stream-frames", str(a.stream_frames), "--limit", str(limit)]
        print(f"[pack_bench] stage {key} (limit {limit} s)", flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            out[key] = {"error": f"exit status {p.returncode}: " + p.stdout[-800:]}
            print(f"[pack_bench] stage {key} failed; nothing more is started on the GPU", flush=True)
            break
        out[key] = json.loads(res[-1][7:])
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(os.path.join(OUT_DIR, "pack_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.join(OUT_DIR, "pack_notes.md"), "w") as f:
        f.write(notes(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
