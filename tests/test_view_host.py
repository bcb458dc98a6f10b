"""Scene views without a GPU: the new symbols and their argument checks, the image writers, the hsk_view layout, and the
numpy restatement of the shading rule (tests/view_twin.py) on volumes the CPU oracle integrates -- where depth, brightness
and normal colour have known values."""
import ctypes as C
import os

import numpy as np

import view_twin as VT
from kit import c_values
from pins_cases import CX, CY, FX, H, W, small_cfg, small_depth


def test_symbols_and_argument_checks(hsk, tmp_path):
    from housescan_amd import _lib
    lib = _lib.load()
    for name in ("hsk_default_view", "hsk_render_view", "hsk_write_ppm", "hsk_write_pgm16"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    v = _lib.HskView()
    assert lib.hsk_render_view(None, C.byref(v), None, None, None, None, None, None) == -1
    assert lib.hsk_render_view(None, None, None, None, None, None, None, None) == -1
    # hsk_default_view is void (as hsk_default_config): without a context the default sensor camera, without a view nothing
    lib.hsk_default_view(None, None)
    lib.hsk_default_view(None, C.byref(v))
    assert (v.width, v.height, v.fx, v.fy, v.cx, v.cy) == (640, 480, 525.0, 525.0, 319.5, 239.5)
    assert (v.follow, v.mode, v.light_in_camera, list(v.light), list(v.background)) == (1, _lib.HSK_VIEW_LAMBERT, 1, [0.0] * 3, [0] * 3)
    assert np.array_equal(np.array(v.pose, np.float32).reshape(4, 4), np.eye(4, dtype=np.float32))
    rgb = np.zeros((4, 5, 3), np.uint8)
    dep = np.zeros((4, 5), np.uint16)
    path = os.fsencode(str(tmp_path / "x"))
    for fn, a in ((lib.hsk_write_ppm, rgb), (lib.hsk_write_pgm16, dep)):
        assert fn(None, a.ctypes.data, 5, 4) == -1
        assert fn(path, None, 5, 4) == -1
        for w, h in ((0, 4), (5, 0), (-1, 4), (4097, 4), (5, 4097)):
            assert fn(path, a.ctypes.data, w, h) == -1
        assert not os.path.exists(path)
        assert fn(os.fsencode(str(tmp_path / "nodir" / "x")), a.ctypes.data, 5, 4) == -3


def read_pnm(path):
    """a reader of its own: magic, width, height, maxval as ASCII tokens, one whitespace byte, then the samples"""
    raw = open(path, "rb").read()
    tokens, pos = [], 0
    while len(tokens) < 4:
        while raw[pos:pos + 1].isspace():
            pos += 1
        start = pos
        while not raw[pos:pos + 1].isspace():
            pos += 1
        tokens.append(raw[start:pos])
    pos += 1
    magic, w, h, maxval = tokens[0], int(tokens[1]), int(tokens[2]), int(tokens[3])
    return magic, w, h, maxval, raw[pos:]


def test_writers_round_trip(hsk, tmp_path):
    from housescan_amd import products
    rng = np.random.default_rng(7)
    for w, h in ((1, 1), (7, 3), (333, 217)):
        rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        dep = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
        dep.reshape(-1)[:2] = (0x0102, 0xFF00)[:dep.size]
        p, g = str(tmp_path / f"v{w}.ppm"), str(tmp_path / f"d{w}.pgm")
        products.write_ppm(p, rgb)
        products.write_pgm16(g, dep)
        magic, rw, rh, mx, body = read_pnm(p)
        assert (magic, rw, rh, mx) == (b"P6", w, h, 255) and body == rgb.tobytes()
        assert open(p, "rb").read().startswith(b"P6\n%d %d\n255\n" % (w, h))
        magic, rw, rh, mx, body = read_pnm(g)
        assert (magic, rw, rh, mx) == (b"P5", w, h, 65535) and len(body) == 2 * w * h
        assert np.array_equal(np.frombuffer(body, ">u2").reshape(h, w), dep)
        assert body[:2] == bytes([dep[0, 0] >> 8, dep[0, 0] & 255])        # most significant byte first


def test_view_struct_layout_matches_c(tmp_path, hsk):
    from housescan_amd import _lib
    fields = [n for n, _ in _lib.HskView._fields_]
    nums = c_values(tmp_path, ["sizeof(hsk_view)"] + [f"offsetof(hsk_view, {f})" for f in fields])
    assert nums[0] == C.sizeof(_lib.HskView)
    assert nums[1:] == [getattr(_lib.HskView, f).offset for f in fields]


def test_twin_on_analytic_scene(oracle, hsk):
    """the scene of test_oracle_pins.test_analytic_scene_and_raycast (wall + block, one frame, 96^3) through the view rule with
    the sensor's camera: (a) the rendered depth against the input depth -- that test's own mask and bound; (b) Lambert with the
    light at the camera: the fronto-parallel wall's centre pixel is lit fully, no hit is darker than the ambient term;
    (c) the normal colour of that pixel is that of a normal facing the camera, -z."""
    n = 96
    cfg = small_cfg(oracle, n)
    pose = hsk.synth_pose(0)
    d = small_depth(hsk, 0)
    vol = np.zeros((n, n, n, 2), np.int16)
    oracle.integrate(cfg, vol, oracle.scale_depth(cfg, d), pose)
    cell = 3.0 / n
    vm, nm = VT.geometry(oracle, VT.view_config(oracle, (n, n, n), W, H, FX, FX, CX, CY), vol, pose, omp=False)
    lam = VT.shade(vm, nm, pose, VT.LAMBERT, light=(0, 0, 0), light_in_camera=True, background=(1, 2, 3))
    hit = ~np.isnan(vm[0])
    assert lam["n_hit"] == hit.sum()
    # (a)
    valid = hit & (d > 0)
    assert valid.mean() > 0.5
    assert np.median(np.abs(lam["depth"][valid].astype(np.float64) - d[valid])) < 0.5 * cell * 1000
    assert (lam["depth"][~hit] == 0).all() and (lam["rgb"][~hit] == (1, 2, 3)).all()
    # (b)
    cy, cx = H // 2, W // 2
    assert hit[cy, cx] and lam["rgb"][cy, cx, 0] in (254, 255)
    assert (lam["rgb"][cy, cx] == lam["rgb"][cy, cx, 0]).all()
    assert lam["rgb"][hit].min() >= 50
    # the same light given in world coordinates: the camera's position
    lam_w = VT.shade(vm, nm, pose, VT.LAMBERT, light=pose[:3, 3], light_in_camera=False, background=(1, 2, 3))
    assert np.array_equal(lam_w["rgb"], lam["rgb"])
    # (c)
    nrm = VT.shade(vm, nm, pose, VT.NORMALS)
    assert np.abs(nrm["rgb"][cy, cx].astype(int) - (128, 128, 0)).max() <= 1
    assert np.array_equal(nrm["depth"], lam["depth"])


def test_twin_colour_modes(oracle, hsk):
    """COLOR looks the hit's voxel up (uncoloured voxels: black, counted), COLOR_LIT scales it by the Lambert term"""
    n = 96
    cfg = small_cfg(oracle, n)
    pose = hsk.synth_pose(0)
    vol = np.zeros((n, n, n, 2), np.int16)
    oracle.integrate(cfg, vol, oracle.scale_depth(cfg, small_depth(hsk, 0)), pose)
    vm, nm = VT.geometry(oracle, VT.view_config(oracle, (n, n, n), W, H, FX, FX, CX, CY), vol, pose, omp=False)
    hit = ~np.isnan(vm[0])
    z, y, x = np.mgrid[0:n, 0:n, 0:n]
    col = np.stack([x, y, z, 1 + (x % 3)], axis=-1).astype(np.uint8)   # a voxel's colour is its index
    col[:, :, ::5, 3] = 0                                              # every fifth column of voxels has none
    c = VT.shade(vm, nm, pose, VT.COLOR, color=col)
    g = np.floor(np.nan_to_num(vm) / np.float32(3.0 / n)).astype(np.int64)
    unc = hit & (g[0] % 5 == 0)
    assert c["n_uncolored"] == unc.sum() > 100 and (c["rgb"][unc] == 0).all()
    ok = hit & ~unc
    assert np.array_equal(c["rgb"][ok], np.stack([g[0], g[1], g[2]], axis=-1)[ok].astype(np.uint8))
    lit = VT.shade(vm, nm, pose, VT.COLOR_LIT, color=col)
    br = VT.brightness(vm, nm, pose, (0, 0, 0), True)
    assert np.array_equal(lit["rgb"][ok], ((c["rgb"][ok].astype(int) * br[ok][:, None] + 127) // 255).astype(np.uint8))
    assert lit["n_uncolored"] == c["n_uncolored"] and (lit["rgb"][unc] == 0).all()


def test_twin_hits_without_a_normal(oracle, hsk):
    """a volume written in numpy whose surface lies in the outer cell layers (view_twin.plane_volume), seen from the scripted
    pose 0 by the sensor's camera: hits whose normal is NaN get the ambient 50 under LAMBERT and the background under NORMALS
    -- the branch no scanned input reaches"""
    vol = VT.plane_volume(64, 3.5)
    pose = hsk.synth_pose(0)
    vm, nm = VT.geometry(oracle, VT.view_config(oracle, (64, 64, 64), 640, 480, 525.0, 525.0, 319.5, 239.5), vol, pose, omp=False)
    hit = ~np.isnan(vm[0])
    bare = hit & np.isnan(nm[0])
    assert hit.mean() > 0.2 and bare.sum() > 1000            # (measured: 28 % hits, 4164 of them without a normal)
    lam = VT.shade(vm, nm, pose, VT.LAMBERT)
    assert (lam["rgb"][bare] == 50).all() and lam["rgb"][hit & ~bare].min() > 50
    nrm = VT.shade(vm, nm, pose, VT.NORMALS, background=(9, 8, 7))
    assert (nrm["rgb"][bare] == (9, 8, 7)).all() and (nrm["rgb"][~hit] == (9, 8, 7)).all()
    assert (nrm["depth"][bare] > 0).all()
    lit = VT.shade(vm, nm, pose, VT.COLOR_LIT, color=np.full((64, 64, 64, 4), 200, np.uint8))
    assert (lit["rgb"][bare] == (200 * 50 + 127) // 255).all()
