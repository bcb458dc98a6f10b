"""bench.py's single-GPU line: a plain run does the timed region only, --full adds the rest, --dump-outputs writes what
the last timed step computed, and the frames a run times are make_frames' frames however they are generated."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kit import ROOT


@pytest.mark.parametrize("first", [0, 75])
def test_bench_frames_are_the_rendered_stream(hsk, first):
    """synth_frames / make_frames render each distinct pose once: every frame must still be synth_depth(synth_pose(k))"""
    from bench_common import make_frames, synth_frames
    count = 330   # past the first repeat of the scripted poses (frame 300)
    poses, distinct, index = synth_frames(hsk, first, count)
    poses2, frames = make_frames(hsk, first, count)
    assert len(distinct) < count and index.shape == (count,) and distinct.dtype == np.uint16
    for k in range(count):
        want_pose = hsk.synth_pose(first + k)
        want = hsk.synth_depth(want_pose)
        assert np.array_equal(poses[k].view(np.uint32), want_pose.view(np.uint32)), k
        assert np.array_equal(poses2[k].view(np.uint32), want_pose.view(np.uint32)), k
        assert np.array_equal(distinct[index[k]], want) and np.array_equal(frames[k], want), k


def test_dump_outputs_is_refused_for_more_than_one_gpu(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dump-outputs", str(tmp_path / "d")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_plain_line_and_dump_outputs(tmp_path):
    """a plain run: the contract's keys, exactly --steps timed steps, none of --full's blocks; its dump: float32 / float64
    arrays within 64 MB that agree with the line, and the same bits from a second run with the same arguments"""
    def run(d):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "3", "--volume", "256", "--dump-outputs", str(d)],
                           cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    line = run(tmp_path / "a")
    assert line["steps"] == 8 and line["warmup"] == 3 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"].startswith("f32") and line["metric"].startswith("frames/sec fused")
    assert abs(line["ms_per_step"] * line["value"] / 1000.0 - 1.0) < 0.01
    for key in ("roofline", "stage_us", "cpu_baseline", "readout_ms", "room_256", "concurrent_rooms_one_gpu", "trajectory_256"):
        assert key not in line, key
    assert line["host_frames_pipelined_fps"] is None and line["sync_process_frame_fps"] is None
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in ("pose", "tracked", "model_vertex_l0", "model_normal_l0", "model_valid_l0", "tsdf_sample_index",
                                                "tsdf_sample_value", "tsdf_sample_weight"))
    arrays = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values()), [n for n, a in arrays.items() if not np.isfinite(a).all()]
    valid = arrays["model_valid_l0"]
    assert valid.shape == (480, 640) and set(np.unique(valid)) <= {0.0, 1.0} and valid.mean() > 0.5
    assert not arrays["model_vertex_l0"][:, valid == 0].any() and not arrays["model_normal_l0"][:, valid == 0].any()
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["pose"][:3, :4].astype(np.float32).tobytes().hex() == line["tracking"]["final_pose_f32_hex"]
    assert line["tracking"]["lost_frames"] == 0 and arrays["tracked"][0] == 1.0
    assert arrays["model_vertex_l0"].shape == (3, 480, 640) and (arrays["tsdf_sample_weight"] > 0).any()
    run(tmp_path / "b")
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "a" / f)), f
