"""Section views without a GPU: the new symbols, the hsk_section layout, the defaults, the numpy restatement of the rule
(tests/section_twin.py) pinned against the CPU oracle's raycast and against volumes with known answers, and the two host-side
calls -- hsk_section_in_room and hsk_composite_views -- against numpy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import section_twin as ST
import view_twin as VT
from kit import ROOT, c_values, same_bits_nan

f32 = np.float32
SIZE, TRUNC = (3.0, 3.0, 3.0), 0.03
W, H, FX, CX, CY = 160, 120, 131.25, 79.5, 59.5


def test_symbols_defaults_and_null_checks(hsk):
    from housescan_amd import _lib
    lib = _lib.load()
    for name in ("hsk_default_section", "hsk_render_section", "hsk_section_in_room", "hsk_composite_views"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert (_lib.HSK_PROJ_PINHOLE, _lib.HSK_PROJ_ORTHO, _lib.HSK_MAX_CLIP) == (0, 1, 4)
    lib.hsk_default_section(None, None)
    s = _lib.HskSection()
    C.memset(C.byref(s), 0xAB, C.sizeof(s))
    lib.hsk_default_section(None, C.byref(s))
    v = _lib.HskView()
    lib.hsk_default_view(None, C.byref(v))
    assert bytes(s.view) == bytes(v), "the view part is hsk_default_view's"
    assert (s.projection, s.light_directional, s.n_clip, list(s.cut_rgb)) == (_lib.HSK_PROJ_PINHOLE, 0, 0, [255, 96, 0])
    assert all(x == 0.0 for pl in s.clip for x in pl)
    # the argument checks that need no device: a NULL context is refused before anything else is looked at
    assert lib.hsk_render_section(None, C.byref(s), None, None, None, None, None, None, None) == -1
    assert lib.hsk_render_section(None, None, None, None, None, None, None, None, None) == -1


def test_section_struct_layout_matches_c(tmp_path, hsk):
    from housescan_amd import _lib
    fields = [n for n, _ in _lib.HskSection._fields_]
    nums = c_values(tmp_path, ["sizeof(hsk_section)"] + [f"offsetof(hsk_section, {f})" for f in fields] +
                    ["sizeof(hsk_view)", "HSK_PROJ_PINHOLE", "HSK_PROJ_ORTHO", "HSK_MAX_CLIP"])
    assert nums[0] == C.sizeof(_lib.HskSection)
    assert nums[1:1 + len(fields)] == [getattr(_lib.HskSection, f).offset for f in fields]
    assert nums[1 + len(fields):] == [C.sizeof(_lib.HskView), 0, 1, 4]


def test_header_with_sections_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "hskinfu.h"\nint main(void){hsk_section s; hsk_section r; float m[16] = {0};\n'
                   'hsk_default_section(0, &s); (void)hsk_section_in_room(&s, m, &r);\n'
                   '(void)hsk_render_section(0, &s, 0, 0, 0, 0, 0, 0, 0); (void)hsk_composite_views(0, 0, 0, 1, 1, 0, 0, 0, 0); return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "c.o")])


@pytest.fixture(scope="module")
def room_volume(hsk, oracle):
    """room 0 at 64^3, integrated by the ORACLE at the scripted poses (every 12th of the 720), a small sensor camera"""
    n = 64
    cfg = oracle.default_config(n, W=W, H=H, fx=FX, fy=FX, cx=CX, cy=CY)
    vol = np.zeros((n, n, n, 2), np.int16)
    for k in range(0, 720, 12):
        p = hsk.synth_room_pose(0, k, 720)
        oracle.integrate(cfg, vol, oracle.scale_depth(cfg, hsk.synth_room_depth(0, p, W, H, FX, FX, CX, CY)), p)
    return n, vol


def test_twin_is_pinned_to_the_oracle(hsk, oracle, room_volume):
    """pinhole rays, no planes, a point light: the twin's maps are oracle.raycast's and its images view_twin's, bit for bit"""
    n, vol = room_volume
    for k, mode in ((30, VT.LAMBERT), (200, VT.NORMALS), (415, VT.COLOR_LIT)):
        pose = hsk.synth_room_pose(0, k, 720)
        vm, nm = VT.geometry(oracle, VT.view_config(oracle, (n, n, n), W, H, FX, FX, CX, CY), vol, pose, omp=False)
        assert (~np.isnan(vm[0])).mean() > 0.5, "the pin needs hits"
        z, y, x = np.mgrid[0:n, 0:n, 0:n]
        col = np.stack([x * 3, y * 3, z * 3, 1 + (x % 3)], axis=-1).astype(np.uint8)
        col[:, :, ::7, 3] = 0
        light, in_cam, bg = (0.1, -0.2, 0.05), True, (3, 4, 5)
        ref = VT.shade(vm, nm, pose, mode, light, in_cam, bg, color=col)
        sec = ST.section(W, H, FX, FX, CX, CY, pose, ST.PINHOLE, (), mode, light, in_cam, False, bg)
        got = ST.render(vol, SIZE, TRUNC, sec, color=col)
        assert same_bits_nan(got["vmap"], vm) and same_bits_nan(got["nmap"], nm), f"frame {k}"
        assert np.array_equal(got["rgb"], ref["rgb"]) and np.array_equal(got["depth"], ref["depth"])
        assert (got["n_hit"], got["n_cut"], got["n_uncolored"]) == (ref["n_hit"], 0, ref["n_uncolored"])


def wall_camera(n, px_per_m=16.0, side=64):
    """an orthographic camera outside the volume's z = 0 face, facing +z, exactly axis aligned (two direction components are
    0 -> 1e-15: step 1), `side` pixels over side / px_per_m metres centred on the volume's axis"""
    pose = np.eye(4, dtype=f32)
    pose[:3, 3] = (1.5, 1.5, -0.5)
    c = (side - 1) / 2.0
    return dict(width=side, height=side, fx=px_per_m, fy=px_per_m, cx=c, cy=c, pose=pose, projection=ST.ORTHO)


def test_twin_orthographic_wall(hsk):
    """view_twin.plane_volume: a wall 3.3 cells before the far z face (not 3.5: a layer of voxels that hold exactly 0 hides the
    crossing from a march whose samples fall into it -- A.6 asks for a strictly positive and a strictly negative voxel).  (a) an orthographic camera facing it: every hit's depth
    is the wall's distance from the camera's plane within half a cell, and the rays beside the volume are background.  (b) a
    directional light along the axis, towards the camera: every hit with a normal has brightness 254 or 255 -- the normal is
    (0, 0, -1) up to the rounding of its normalisation, so w is 1 or 1 - 2^-24 and 50 + trunc(205 w) is 255 or 254.  (c) a clip plane one cell behind the wall, inside its negative band: every marching pixel is CUT, and its depth is
    the plane's."""
    n = 64
    cell = 3.0 / n
    vol = VT.plane_volume(n, 3.3)
    wall_z = 3.0 - 3.3 * cell
    cam = wall_camera(n)
    o, _ = ST.rays(ST.section(**cam))
    footprint = (o[0] > 0) & (o[0] < 3) & (o[1] > 0) & (o[1] < 3)      # the rays that march
    assert 0.4 < footprint.mean() < 0.7
    # (a ray inside the outermost layer of voxels finds no vertex: the trilinear sample is NaN on the grid's shell, A.6)
    inner = (o[0] > cell) & (o[0] < 3 - cell) & (o[1] > cell) & (o[1] < 3 - cell)
    assert 0 < (footprint & ~inner).sum() < 0.2 * footprint.sum()
    # (a), (b)
    sec = ST.section(**cam, mode=VT.LAMBERT, light=(0, 0, -1), light_in_camera=False, light_directional=True, background=(1, 2, 3))
    r = ST.render(vol, SIZE, TRUNC, sec)
    hit = r["cls"] == ST.HIT
    assert r["n_cut"] == 0 and r["n_hit"] == hit.sum()
    assert np.array_equal(hit, inner), "every ray through the volume's inner voxels meets the wall, no other does"
    want_mm = (wall_z + 0.5) * 1000
    assert np.abs(r["depth"][hit].astype(np.float64) - want_mm).max() <= 0.5 * cell * 1000
    assert (r["depth"][~hit] == 0).all() and (r["rgb"][~hit] == (1, 2, 3)).all()
    has_n = hit & ~np.isnan(r["nmap"][0])
    assert has_n.sum() > 0.5 * hit.sum()
    assert np.isin(r["rgb"][has_n], (254, 255)).all(), np.unique(r["rgb"][has_n])
    assert (r["rgb"][hit & ~has_n] == 50).all()
    # the same light given in camera coordinates (the pose is the identity rotation): the same image
    sec_c = ST.section(**cam, mode=VT.LAMBERT, light=(0, 0, -1), light_in_camera=True, light_directional=True, background=(1, 2, 3))
    assert np.array_equal(ST.render(vol, SIZE, TRUNC, sec_c)["rgb"], r["rgb"])
    # a light from behind the wall: ambient only
    sec_b = ST.section(**cam, mode=VT.LAMBERT, light=(0, 0, 1), light_in_camera=False, light_directional=True)
    assert (ST.render(vol, SIZE, TRUNC, sec_b)["rgb"][hit] == 50).all()
    # (c)
    zc = wall_z + cell
    sec = ST.section(**cam, clip=[(0, 0, 1, -zc)], cut_rgb=(9, 8, 7), background=(1, 2, 3))
    r = ST.render(vol, SIZE, TRUNC, sec)
    cut = r["cls"] == ST.CUT
    assert np.array_equal(cut, footprint) and r["n_cut"] == cut.sum() and r["n_hit"] == 0
    assert (r["rgb"][cut] == (9, 8, 7)).all() and (r["rgb"][~cut] == (1, 2, 3)).all()
    assert np.abs(r["depth"][cut].astype(np.float64) - (zc + 0.5) * 1000).max() <= 1.0
    assert np.isnan(r["vmap"]).all() and np.isnan(r["nmap"]).all()
    # the plane in front of the wall, the far side kept away (z <= wall + cell is kept: a no-op for the hits): the wall again
    sec = ST.section(**cam, clip=[(0, 0, 1, -1.0), (0, 0, -1, zc)])
    r = ST.render(vol, SIZE, TRUNC, sec)
    assert np.array_equal(r["cls"] == ST.HIT, inner) and r["n_cut"] == 0
    # ... and with the far-side plane in FRONT of the wall the hits lie beyond it: not shown (step 5)
    sec = ST.section(**cam, clip=[(0, 0, -1, wall_z - 2 * cell)])
    r = ST.render(vol, SIZE, TRUNC, sec)
    assert r["n_hit"] == 0 and r["n_cut"] == 0
    assert np.array_equal(r["raw_hit"], inner), "the march does not end at t_exit: it still finds the wall"


def test_twin_room_floor_plan(hsk, room_volume):
    """room 0 from above, the ceiling side cut away at mid height (64^3): a floor plan -- hits, cut outlines and background are
    all there, the hits lie on the floor side of the plane, and without the plane the same camera sees fewer hits"""
    n, vol = room_volume
    x0, x1, y0, y1, z0, z1 = hsk.synth_room_extents(0)
    cxw, czw = 0.5 * (x0 + x1), 0.5 * (z0 + z1)
    pose = ST.look((cxw, -0.5, czw), (cxw, 0.5, czw), (0, 0, 1))
    yc = 0.5 * (y0 + y1)
    cam = dict(width=100, height=100, fx=100 / 3.2, fy=100 / 3.2, cx=49.5, cy=49.5, pose=pose, projection=ST.ORTHO)
    r = ST.render(vol, SIZE, TRUNC, ST.section(**cam, clip=[(0, 1, 0, -yc)]))
    share = {k: (r["cls"] == v).mean() for k, v in (("hit", ST.HIT), ("cut", ST.CUT), ("bg", ST.BACKGROUND))}
    print("floor plan 64^3:", share)
    assert share["hit"] >= 0.05 and share["cut"] >= 0.01 and share["bg"] >= 0.05, share
    hit = r["cls"] == ST.HIT
    assert (r["vmap"][1][hit] >= yc).all()
    bare = ST.render(vol, SIZE, TRUNC, ST.section(**cam))
    assert bare["n_hit"] < r["n_hit"], (bare["n_hit"], r["n_hit"])


def test_composite_views_against_numpy(hsk):
    from housescan_amd import _lib, products
    lib = _lib.load()
    rng = np.random.default_rng(11)
    for n, (w, h) in ((1, (5, 4)), (2, (33, 17)), (4, (64, 48))):
        deps = [rng.integers(0, 6, size=(h, w)).astype(np.uint16) * 500 for _ in range(n)]    # many ties, many zeros
        deps[0][0, 0] = 0
        for d in deps:
            d[1, :] = 0                                                                       # a row without depth anywhere
        cols = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(n)]
        want = ST.composite(cols, deps, (7, 8, 9))
        got = products.composite_views(cols, deps, (7, 8, 9))
        for a, b, what in zip(got, want, ("rgb", "depth", "index")):
            assert np.array_equal(a, b), (n, what)
        assert (got[2][1, :] == -1).all() and (got[1][1, :] == 0).all() and (got[0][1, :] == (7, 8, 9)).all()
        if n > 1:
            tie = (deps[0] == deps[1]) & (deps[0] > 0) & (got[1] == deps[0])
            assert tie.any() and (got[2][tie] == 0).all(), "the lowest index wins a tie"
        # NULL outputs, one at a time and all at once
        dp = (C.c_void_p * n)(*[d.ctypes.data for d in deps])
        cp = (C.c_void_p * n)(*[c.ctypes.data for c in cols])
        bg = np.array((7, 8, 9), np.uint8)
        assert lib.hsk_composite_views(n, cp, dp, w, h, bg.ctypes.data, None, None, None) == 0
        idx = np.empty((h, w), np.int32)
        assert lib.hsk_composite_views(n, None, dp, w, h, None, None, None, idx.ctypes.data) == 0
        assert np.array_equal(idx, want[2])
        dep = np.empty((h, w), np.uint16)
        assert lib.hsk_composite_views(n, None, dp, w, h, None, None, dep.ctypes.data, None) == 0
        assert np.array_equal(dep, want[1])
        _, d2, i2 = products.composite_views(None, deps, want_rgb=False)
        assert np.array_equal(d2, want[1]) and np.array_equal(i2, want[2])
        # refusals
        rgb = np.empty((h, w, 3), np.uint8)
        assert lib.hsk_composite_views(0, cp, dp, w, h, bg.ctypes.data, rgb.ctypes.data, None, None) == -1
        assert lib.hsk_composite_views(n, cp, None, w, h, bg.ctypes.data, rgb.ctypes.data, None, None) == -1
        assert lib.hsk_composite_views(n, None, dp, w, h, bg.ctypes.data, rgb.ctypes.data, None, None) == -1
        assert lib.hsk_composite_views(n, cp, dp, w, h, None, rgb.ctypes.data, None, None) == -1
        assert lib.hsk_composite_views(n, cp, dp, 0, h, bg.ctypes.data, rgb.ctypes.data, None, None) == -1
        assert lib.hsk_composite_views(n, cp, dp, w, 4097, bg.ctypes.data, rgb.ctypes.data, None, None) == -1


def rigid(deg_y, t, deg_x=0.0):
    a, b = np.radians(deg_y), np.radians(deg_x)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    M = np.eye(4)
    M[:3, :3] = Ry @ Rx
    M[:3, 3] = t
    return M.astype(f32)


def house_section(light_in_camera, directional):
    pose = ST.look((2.3, -0.7, 1.9), (2.0, 1.0, 1.6), (0.1, 0, 1))
    return ST.section(200, 150, 62.5, 60.0, 99.5, 74.5, pose, ST.ORTHO, [(0.1, 0.9, -0.2, -1.3), (1, 0, 0, 0.25), (0, 0, -1, 4.5)],
                      VT.COLOR_LIT, (0.3, -2.0, 0.7), light_in_camera, directional, (1, 2, 3), (4, 5, 6))


def test_section_in_room_against_numpy(hsk):
    """equal bits with a binary64 numpy computation rounded once (the twin sums left to right, as the library does: no ulp is
    needed); a point of the house plane, mapped into the room, lies on the room's plane; the refusals"""
    from housescan_amd import _lib, products
    lib = _lib.load()
    for M in (rigid(0, (0, 0, 0)), rigid(90, (2.6, 0.0, 0.1)), rigid(37.5, (-1.2, 0.4, 3.3), 11.0)):
        for in_cam, directional in ((False, False), (False, True), (True, False), (True, True)):
            sec = house_section(in_cam, directional)
            want = ST.in_room(sec, M)
            got = ST.from_struct(products.section_in_room(ST.to_struct(sec, _lib), M))
            assert same_bits_nan(got["pose"], want["pose"]), (M, got["pose"], want["pose"])
            assert same_bits_nan(np.array(got["clip"], f32), np.array(want["clip"], f32))
            assert same_bits_nan(np.array(got["light"], f32), np.array(want["light"], f32))
            if in_cam:
                assert same_bits_nan(np.array(got["light"], f32), np.array(sec["light"], f32))
            for key in ("width", "height", "fx", "fy", "cx", "cy", "projection", "mode", "light_in_camera", "light_directional",
                        "background", "cut_rgb"):
                assert got[key] == sec[key], key
            # physically: p_house = M p_room; a point on the house plane <-> a point on the room plane; the camera's centre too
            M64 = M.astype(np.float64)
            for ph, pr in zip(sec["clip"], got["clip"]):
                nrm = np.array(ph[:3], np.float64)
                p_house = -ph[3] * nrm / (nrm @ nrm) + np.cross(nrm, (0.3, 0.2, 0.9))
                p_room = np.linalg.solve(M64, np.append(p_house, 1.0))[:3]
                assert abs(np.array(pr[:3], np.float64) @ p_room + pr[3]) < 1e-5
            back = M64 @ got["pose"].astype(np.float64)
            assert np.abs(back - sec["pose"]).max() < 1e-5
    # in place (room == house)
    sec = house_section(False, False)
    s = ST.to_struct(sec, _lib)
    M = rigid(90, (2.6, 0.0, 0.1)).reshape(16)
    mp = M.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.hsk_section_in_room(C.byref(s), mp, C.byref(s)) == 0
    assert same_bits_nan(ST.from_struct(s)["pose"], ST.in_room(sec, M)["pose"])
    # the three refusals (and NULL pointers)
    s = ST.to_struct(sec, _lib)
    out = _lib.HskSection()
    s.view.follow = 1
    assert lib.hsk_section_in_room(C.byref(s), mp, C.byref(out)) == -1
    s.view.follow = 0
    bad = M.copy()
    bad[12] = 0.5
    assert lib.hsk_section_in_room(C.byref(s), bad.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)) == -1
    bad = M.copy()
    bad[15] = 2.0
    assert lib.hsk_section_in_room(C.byref(s), bad.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)) == -1
    bad = M.copy()
    bad[0] += f32(1e-3)          # a scale: R^T R - I = 2e-3 on one diagonal entry
    bad[5] = f32(1.001)
    assert lib.hsk_section_in_room(C.byref(s), bad.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)) == -1
    ok = M.copy()
    ok[5] = f32(1.00001)         # |R^T R - I| = 2e-5: inside the bound
    assert lib.hsk_section_in_room(C.byref(s), ok.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out)) == 0
    assert lib.hsk_section_in_room(None, mp, C.byref(out)) == -1
    assert lib.hsk_section_in_room(C.byref(s), None, C.byref(out)) == -1
    assert lib.hsk_section_in_room(C.byref(s), mp, None) == -1
