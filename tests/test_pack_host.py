"""The sparse volume image on the host: the numpy twin (tests/pack_twin.py) round-trips volumes that hold every class; the
library's host-only header readers agree with the twin field for field; malformed images are refused with a message;
hsk_config_from_volume reproduces the fields; a scanned room packs to well under the raw size because of the SPLIT class."""
import ctypes as C
import struct

import numpy as np
import pytest

import pack_twin as PT

f32 = np.float32
SCAN_FRAMES = 720     # the scripted three-turn room scan

CASES = {
    "cube32": ((32, 32, 32), True),
    "z20": ((16, 24, 20), True),          # vol_z not a multiple of 8: the last brick layer is padded
    "flat": ((64, 16, 8), False),         # non-cubic, no colour
    "tall": ((8, 40, 36), True),
}


def fields_for(dims, color, **over):
    f = PT.default_fields(dims, size_m=(3.0, 1.5, 2.25), trunc_dist_m=0.03, trunc_eff_m=0.2953125, width=320, height=240, fx=262.5, fy=263.0,
                          cx=159.5, cy=119.25, pose=tuple(np.arange(16, dtype=f32) * f32(0.37) - f32(1.1)), frame=17,
                          color_max_weight=64 if color else 0, color_band_m=0.0625 if color else 0.0)
    f.update(over)
    return f


def image_for(name):
    dims, color = CASES[name]
    tsdf, col = PT.crafted_volume(dims, seed=sum(dims), color=color)
    return tsdf, col, PT.pack(tsdf, col, fields_for(dims, color))


@pytest.mark.parametrize("name", list(CASES))
def test_the_twin_round_trips_every_class(name):
    dims, color = CASES[name]
    tsdf, col, img = image_for(name)
    assert (tsdf[..., 1] == 256).any(), "no weight of 256 in the crafted volume"
    assert ((tsdf[..., 1] == 0) & (tsdf[..., 0] != 0)).any(), "no tsdf != 0 under weight 0"
    f = PT.info(img)
    assert all(n > 0 for n in f["tsdf_bricks"]), f"a class is missing: {f['tsdf_bricks']}"
    assert sum(f["tsdf_bricks"]) == f["n_bricks"] == (dims[0] // 8) * (dims[1] // 8) * ((dims[2] + 7) // 8)
    assert f["total_bytes"] == len(img) and len(img) % 4 == 0
    assert f["tsdf_payload_bytes"] == 4 * f["tsdf_bricks"][1] + 516 * f["tsdf_bricks"][2] + 2048 * f["tsdf_bricks"][3]
    if color:
        assert f["flags"] == 1 and f["color_bricks"][0] > 0 and f["color_bricks"][1] > 0
        assert f["color_payload_bytes"] == 2048 * f["color_bricks"][1]
    else:
        assert f["flags"] == 0 and f["color_table_bytes"] == 0 and f["color_payload_bytes"] == 0
    t2, c2, _ = PT.unpack(img)
    assert np.array_equal(t2, tsdf)
    assert (c2 is None) if col is None else np.array_equal(c2, col)
    assert PT.pack(t2, c2, fields_for(dims, color)) == img


def test_a_weight_of_256_forces_raw_and_a_bare_tsdf_is_not_zero():
    t = np.zeros((8, 8, 8, 2), np.int16)
    assert PT.classify_tsdf(PT.bricks_of(PT.words_of(t)))[0] == PT.ZERO
    t[..., 0] = 5
    assert PT.classify_tsdf(PT.bricks_of(PT.words_of(t)))[0] == PT.UNIFORM      # weight 0 everywhere, the word is not 0
    t[..., 1] = 255
    t[2, 3, 4, 1] = 7
    assert PT.classify_tsdf(PT.bricks_of(PT.words_of(t)))[0] == PT.SPLIT
    t[2, 3, 4, 1] = 256
    assert PT.classify_tsdf(PT.bricks_of(PT.words_of(t)))[0] == PT.RAW
    t[2, 3, 4, 1] = -1                                                           # a negative weight is not a byte either
    assert PT.classify_tsdf(PT.bricks_of(PT.words_of(t)))[0] == PT.RAW
    # a uniform volume whose last layer is partial: the padding words are 0, so that layer's bricks are not UNIFORM
    u = np.empty((12, 8, 8, 2), np.int16)
    u[...] = (9, 3)
    assert PT.classify_tsdf(PT.bricks_of(PT.words_of(u))).tolist() == [PT.UNIFORM, PT.RAW]


# ---- the library's header readers against the twin -------------------------------------------------------------------
SCALARS = ("version", "header_bytes", "flags", "z0", "nz", "trunc_dist_m", "trunc_eff_m", "width", "height", "fx", "fy", "cx", "cy", "frame",
           "color_max_weight", "color_band_m", "n_bricks", "tsdf_table_bytes", "tsdf_payload_bytes", "color_table_bytes",
           "color_payload_bytes", "total_bytes")
ARRAYS = ("dims", "size_m", "tsdf_bricks", "color_bricks")


def assert_same_header(got, want):
    for key in SCALARS:
        a, b = got[key], want[key]
        same = (f32(a).view(np.uint32) == f32(b).view(np.uint32)) if isinstance(b, float) else (int(a) == int(b))
        assert same, f"{key}: {a} != {b}"
    for key in ARRAYS:
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), f"{key}: {got[key]} != {want[key]}"
    assert np.array_equal(np.asarray(got["pose"], f32).reshape(-1).view(np.uint32), np.asarray(want["pose"], f32).view(np.uint32)), "pose"


@pytest.mark.parametrize("name", list(CASES))
def test_the_header_readers_agree_with_the_twin(hsk, tmp_path, name):
    _, _, img = image_for(name)
    want = PT.info(img)
    assert_same_header(hsk.volume_image_info(img), want)
    path = tmp_path / "volume.hskv"
    path.write_bytes(img)
    assert_same_header(hsk.volume_file_info(path), want)


def patched(img, at, fmt, value):
    b = bytearray(img)
    struct.pack_into("<" + fmt, b, at, value)
    return bytes(b)


def bad_images():
    _, _, img = image_for("cube32")
    f = PT.info(img)
    cls = np.frombuffer(img, np.uint8, f["n_bricks"], f["at"][0])
    first_raw = f["at"][0] + int(np.flatnonzero(cls == PT.RAW)[0])
    first_zero = f["at"][0] + int(np.flatnonzero(cls == PT.ZERO)[0])
    ccls = np.frombuffer(img, np.uint8, f["n_bricks"], f["at"][2])
    first_craw = f["at"][2] + int(np.flatnonzero(ccls == PT.RAW)[0])
    return img, {
        "truncated by one byte": img[:-1],
        "one byte too long": img + b"\0",
        "bad magic": b"HSKW" + img[4:],
        "version 2": patched(img, 4, "I", 2),
        "version 0": patched(img, 4, "I", 0),
        "header size": patched(img, 8, "I", 512),
        "class byte 4": patched(img, first_raw, "B", 4),
        "colour class 1": patched(img, first_craw, "B", 1),
        "colour class 2": patched(img, first_craw, "B", 2),
        "a RAW brick called ZERO (payload longer than the table says)": patched(img, first_raw, "B", 0),
        "a ZERO brick called UNIFORM (payload shorter than the table says)": patched(img, first_zero, "B", 1),
        "tsdf payload length + 4": patched(img, 224, "Q", f["tsdf_payload_bytes"] + 4),
        "colour payload length - 2048 and total with it": patched(patched(img, 240, "Q", f["color_payload_bytes"] - 2048), 248, "Q", f["total_bytes"] - 2048)[:-2048],
        "brick count": patched(img, 160, "Q", f["n_bricks"] + 1),
        "dims not a multiple of 8": patched(img, 16, "i", 36),
        "unknown flag": patched(img, 12, "I", 3),
        "vol_x near 2^31 (the brick count would wrap)": patched(img, 16, "i", 0x7FFFFFF8),
        "vol_z and nz of INT_MAX": patched(patched(img, 24, "i", 0x7FFFFFFF), 32, "i", 0x7FFFFFFF),
        "shorter than a header": img[:100],
        "empty": b"",
    }


def test_malformed_images_are_refused_with_a_message(hsk, tmp_path):
    lib = hsk._lib.load()
    good, bad = bad_images()
    assert hsk.volume_image_info(good)["total_bytes"] == len(good)
    for what, img in bad.items():
        a = np.frombuffer(img, np.uint8)
        info = hsk._lib.HskVolumeInfo()
        rc = lib.hsk_volume_image_info(a.ctypes.data if a.size else None, a.size, C.byref(info))
        msg = lib.hsk_last_error(None).decode()
        assert rc == -1, f"{what}: accepted (rc {rc})"
        assert len(msg) > 10, f"{what}: no message"
        path = tmp_path / "bad.hskv"
        path.write_bytes(img)
        rc = lib.hsk_volume_file_info(str(path).encode(), C.byref(info))
        assert rc == -1 and len(lib.hsk_last_error(None).decode()) > 10, f"{what}: the file form accepted it (rc {rc})"
    with pytest.raises(hsk.KinfuError, match="truncated"):
        hsk.volume_image_info(bad["truncated by one byte"])
    with pytest.raises(hsk.KinfuError, match="magic"):
        hsk.volume_image_info(bad["bad magic"])
    with pytest.raises(hsk.KinfuError, match="version"):
        hsk.volume_image_info(bad["version 2"])
    with pytest.raises(hsk.KinfuError, match="class byte"):
        hsk.volume_image_info(bad["class byte 4"])
    with pytest.raises(hsk.KinfuError, match="cannot open"):
        hsk.volume_file_info(tmp_path / "missing.hskv")
    assert lib.hsk_volume_image_info(None, 0, None) == -1 and lib.hsk_volume_file_info(None, None) == -1
    assert lib.hsk_config_from_volume(None, None) == -1


def test_config_from_volume_reproduces_the_fields(hsk):
    for name in CASES:
        dims, color = CASES[name]
        _, _, img = image_for(name)
        want = PT.info(img)
        info = hsk.volume_image_info(img)
        cfg = hsk.config_from_volume(info)
        assert (cfg.vol_x, cfg.vol_y, cfg.vol_z) == tuple(dims)
        assert np.array_equal(np.array(cfg.vol_size_m[:], f32), np.array(want["size_m"], f32))
        assert f32(cfg.trunc_dist_m) == f32(want["trunc_dist_m"])
        assert (cfg.width, cfg.height) == (want["width"], want["height"])
        assert [f32(cfg.fx), f32(cfg.fy), f32(cfg.cx), f32(cfg.cy)] == [f32(want[k]) for k in ("fx", "fy", "cx", "cy")]
        assert np.array_equal(np.array(cfg.init_pose[:], f32), np.array(want["pose"], f32))
        assert (cfg.own_z0, cfg.own_z1, cfg.halo) == (0, dims[2], 0)
        base = hsk.default_config(dims[0])
        assert list(cfg.icp_iters) == list(base.icp_iters) and cfg.use_graph == base.use_graph == 0
        assert f32(cfg.icp_dist_thresh_m) == f32(base.icp_dist_thresh_m)


def test_a_scanned_room_packs_to_under_sixty_percent(hsk, oracle):
    """room 0 at 128^3, every third frame of its scripted scan, depth only, integrated by the oracle at the script's poses.
    The cap is the share WITHOUT the SPLIT class (0.60): it fails if free space stops packing as SPLIT."""
    n = 128
    cfg = oracle.default_config(n)
    vol = np.zeros((n, n, n, 2), np.int16)
    for k in range(0, 720, 3):
        pose = hsk.synth_room_pose(0, k, SCAN_FRAMES)
        oracle.integrate(cfg, vol, oracle.scale_depth(cfg, hsk.synth_room_depth(0, pose)), pose)
    img = PT.pack(vol, None, PT.default_fields((n, n, n), trunc_eff_m=oracle.tau(cfg)))
    f = PT.info(img)
    raw_bytes = vol.nbytes
    share = len(img) / raw_bytes
    no_split = (len(img) + f["tsdf_bricks"][PT.SPLIT] * (2048 - 516)) / raw_bytes
    print(f"bricks {f['tsdf_bricks']}, packed share {share:.3f}, without SPLIT {no_split:.3f}")
    assert f["tsdf_bricks"][PT.ZERO] > 0 and f["tsdf_bricks"][PT.SPLIT] > 0 and f["tsdf_bricks"][PT.RAW] > 0, f["tsdf_bricks"]
    assert share <= 0.60, f"packed share {share:.3f} of the raw bytes"
    t2, _, _ = PT.unpack(img)
    assert np.array_equal(t2, vol)
    assert hsk.volume_image_info(img)["total_bytes"] == len(img)
