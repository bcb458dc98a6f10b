"""Colour and normals on the host side (no GPU): the XYZRGBNormal PCD, the attribute downsample, the synthetic colour
renders, write_room_dir's defaults and the argument checks of the colour entry points."""
import ctypes as C
import os

import numpy as np
import pytest

import housescan_amd as hsk
from housescan_amd import _lib, products

from color_cases import read_pcd_xyzrgbnormal

NEW_SYMBOLS = ["hsk_enable_color", "hsk_process_frame_rgbd", "hsk_submit_frame_rgbd", "hsk_integrate_color", "hsk_download_color",
               "hsk_upload_color", "hsk_extract_cloud_attrs", "hsk_voxel_downsample_attrs", "hsk_write_pcd_xyzrgbnormal",
               "hsk_synth_render_rgb", "hsk_synth_color_at"]


def test_new_symbols_bound():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert getattr(lib, name) is not None


def test_pcd_xyzrgbnormal_roundtrip(tmp_path):
    rng = np.random.default_rng(7)
    n = 1000
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm[::7] = np.nan
    path = str(tmp_path / "c.pcd")
    products.write_pcd_xyzrgbnormal(path, xyz, rgb, nrm)
    head, x2, bits, n2, curv = read_pcd_xyzrgbnormal(path)
    assert head["VERSION"] == "0.7"
    assert head["FIELDS"] == "x y z rgb normal_x normal_y normal_z curvature"
    assert head["SIZE"] == " ".join(["4"] * 8) and head["TYPE"] == " ".join(["F"] * 8) and head["COUNT"] == " ".join(["1"] * 8)
    assert head["WIDTH"] == str(n) and head["HEIGHT"] == "1" and head["DATA"] == "binary"
    assert np.array_equal(x2.view(np.uint32), xyz.view(np.uint32))
    want = (rgb[:, 0].astype(np.uint32) << 16) | (rgb[:, 1].astype(np.uint32) << 8) | rgb[:, 2].astype(np.uint32)
    assert np.array_equal(bits, want)
    assert np.array_equal(np.isnan(n2), np.isnan(nrm))
    ok = ~np.isnan(nrm)
    assert np.array_equal(n2[ok], nrm[ok])
    assert not curv.any()
    # no normals: NaN; and an empty cloud
    products.write_pcd_xyzrgbnormal(path, xyz[:3], rgb[:3])
    assert np.isnan(read_pcd_xyzrgbnormal(path)[3]).all()
    products.write_pcd_xyzrgbnormal(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    head, x2, _, _, _ = read_pcd_xyzrgbnormal(path)
    assert head["POINTS"] == "0" and len(x2) == 0


def test_voxel_downsample_attrs():
    rng = np.random.default_rng(3)
    xyz = rng.uniform(0, 1, size=(5000, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(5000, 3), dtype=np.uint8)
    nrm = rng.normal(size=(5000, 3)).astype(np.float32)
    nrm[::3] = np.nan
    d0 = products.voxel_downsample(xyz, 0.1)
    d1, r1, n1 = products.voxel_downsample_attrs(xyz, 0.1, rgb, nrm)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    assert r1.shape == d1.shape and n1.shape == d1.shape
    d2, r2, n2 = products.voxel_downsample_attrs(xyz, 0.1)
    assert np.array_equal(d2.view(np.uint32), d0.view(np.uint32)) and r2 is None and n2 is None
    # a hand-built cloud: leaf (0,0,0) holds three points, leaf (1,0,0) one with a NaN normal
    pts = np.array([[0.01, 0.01, 0.01], [0.02, 0.02, 0.02], [0.03, 0.01, 0.02], [0.15, 0.01, 0.01]], np.float32)
    col = np.array([[10, 20, 30], [11, 20, 31], [11, 21, 31], [200, 100, 0]], np.uint8)
    nn = np.array([[1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.nan, np.nan, np.nan]], np.float32)
    d, r, n = products.voxel_downsample_attrs(pts, 0.1, col, nn)
    assert len(d) == 2
    assert r.tolist() == [[11, 20, 31], [200, 100, 0]]   # (32 + 1) // 3 = 11, (61 + 1) // 3 = 20, (92 + 1) // 3 = 31
    assert np.allclose(n[0], [np.sqrt(0.5), np.sqrt(0.5), 0.0], atol=1e-6)
    assert np.isnan(n[1]).all()


@pytest.mark.parametrize("scene", [-1, 0, 2])
def test_synth_rgb_matches_depth(scene):
    pose = hsk.synth_pose(5) if scene < 0 else hsk.synth_room_pose(scene, 30, 720)
    depth = hsk.synth_depth(pose) if scene < 0 else hsk.synth_room_depth(scene, pose)
    rgb = hsk.synth_rgb(pose, scene)
    assert rgb.shape == (480, 640, 3) and rgb.dtype == np.uint8
    assert np.array_equal(rgb, hsk.synth_rgb(pose, scene)), "not deterministic"
    assert np.array_equal((rgb == 0).all(axis=2), depth == 0)
    lit = rgb[depth != 0]
    assert lit.min() >= 28 and lit.max() <= 228


def test_synth_color_at_range():
    rng = np.random.default_rng(1)
    for p in rng.uniform(-5, 5, size=(200, 3)):
        c = hsk.synth_color_at(p)
        want = np.rint(128.0 + 100.0 * np.sin(2.0 * np.pi * p.astype(np.float32).astype(np.float64) / 1.2))
        assert np.array_equal(c, want.astype(np.uint8)), (p, c, want)
        assert 28 <= c.min() and c.max() <= 228


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "room_dir_defaults")


def test_write_room_dir_defaults_unchanged(tmp_path):
    """default arguments: the same files, byte for byte, as before colour existed -- tests/golden/room_dir_defaults/files is
    what write_room_dir wrote for cloud_in.npy (two walls and a floor) at the commit before colour was added"""
    xyz = np.load(os.path.join(GOLDEN, "cloud_in.npy"))
    files = sorted(os.listdir(os.path.join(GOLDEN, "files")))
    assert "cloud_bin.pcd" in files and "cloud_downsampled.pcd" in files and "planes.txt" in files
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    products.write_room_dir(d1, xyz)
    products.write_room_dir(d2, xyz, cloud_rgb=None, cloud_normals=None)
    for d in (d1, d2):
        assert sorted(os.listdir(d)) == files
        for f in files:
            assert open(os.path.join(d, f), "rb").read() == open(os.path.join(GOLDEN, "files", f), "rb").read(), (d, f)
    rng = np.random.default_rng(11)
    # the XYZ files are what write_pcd writes
    ref = str(tmp_path / "ref.pcd")
    products.write_pcd(ref, xyz)
    assert open(ref, "rb").read() == open(os.path.join(d1, "cloud_bin.pcd"), "rb").read()
    # coloured: cloud_bin.pcd becomes XYZRGBNormal, the downsampled cloud and the planes stay as they are
    d3 = str(tmp_path / "c")
    rgb = rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(xyz), 1))
    products.write_room_dir(d3, xyz, cloud_rgb=rgb, cloud_normals=nrm)
    for f in files:
        if f != "cloud_bin.pcd":
            assert open(os.path.join(d1, f), "rb").read() == open(os.path.join(d3, f), "rb").read(), f
    _, x2, bits, _, _ = read_pcd_xyzrgbnormal(os.path.join(d3, "cloud_bin.pcd"))
    assert np.array_equal(x2, xyz)
    d4 = str(tmp_path / "d")
    products.write_room_dir(d4, xyz, cloud_rgb=rgb, cloud_normals=nrm, colored_downsampled=True)
    head, xd, _, nd, _ = read_pcd_xyzrgbnormal(os.path.join(d4, "cloud_downsampled.pcd"))
    assert np.array_equal(xd, products.voxel_downsample(xyz, 0.03))
    assert open(os.path.join(d1, "planes.txt"), "rb").read() == open(os.path.join(d4, "planes.txt"), "rb").read()
    # colour without normals: XYZRGBNormal with NaN normals; normals (or a coloured downsample) without colour: refused
    d5 = str(tmp_path / "e")
    products.write_room_dir(d5, xyz, cloud_rgb=rgb)
    _, x5, bits5, n5, _ = read_pcd_xyzrgbnormal(os.path.join(d5, "cloud_bin.pcd"))
    assert np.array_equal(x5, xyz) and np.array_equal(bits5, bits) and np.isnan(n5).all()
    with pytest.raises(ValueError):
        products.write_room_dir(str(tmp_path / "f"), xyz, cloud_normals=nrm)
    with pytest.raises(ValueError):
        products.write_room_dir(str(tmp_path / "g"), xyz, colored_downsampled=True)
    assert not os.path.exists(str(tmp_path / "f")) and not os.path.exists(str(tmp_path / "g"))


def test_null_and_argument_errors(tmp_path):
    lib = _lib.load()
    n = C.c_size_t()
    assert lib.hsk_enable_color(None, 0, C.c_float(0)) == -1
    assert lib.hsk_process_frame_rgbd(None, None, None, 640, 480, None, None) == -1
    assert lib.hsk_submit_frame_rgbd(None, None, None, 640, 480) == -1
    assert lib.hsk_integrate_color(None, None, None, 640, 480, None) == -1
    assert lib.hsk_download_color(None, None) == -1
    assert lib.hsk_upload_color(None, None) == -1
    assert lib.hsk_extract_cloud_attrs(None, None, None, None, 0, C.byref(n), None) == -1
    assert lib.hsk_write_pcd_xyzrgbnormal(None, None, None, None, 0) == -1
    assert lib.hsk_write_pcd_xyzrgbnormal(os.fsencode(str(tmp_path / "x.pcd")), None, None, None, 3) == -1
    assert lib.hsk_voxel_downsample_attrs(None, None, None, 0, C.c_float(0.1), None, None, None, 0, None) == -1
    assert lib.hsk_voxel_downsample_attrs(None, None, None, 0, C.c_float(0.0), None, None, None, 0, C.byref(n)) == -1
    assert lib.hsk_voxel_downsample_attrs(None, None, None, 0, C.c_float(0.1), None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    p = np.eye(4, dtype=np.float32).reshape(16)
    buf = np.empty(3 * 16, np.uint8)
    fp = p.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.hsk_synth_render_rgb(0, None, 4, 4, 1, 1, 1, 1, buf.ctypes.data) == -1
    assert lib.hsk_synth_render_rgb(0, fp, 4, 4, 1, 1, 1, 1, None) == -1
    assert lib.hsk_synth_render_rgb(4, fp, 4, 4, 1, 1, 1, 1, buf.ctypes.data) == -1
    assert lib.hsk_synth_color_at(0, None, buf.ctypes.data) == -1
    assert lib.hsk_synth_color_at(0, fp, None) == -1
    with pytest.raises(ValueError):
        products.write_pcd_xyzrgbnormal(str(tmp_path / "y.pcd"), np.zeros((3, 3), np.float32), np.zeros((2, 3), np.uint8))
