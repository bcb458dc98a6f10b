"""Baked textures without a GPU: the layout and the texel rule (housescan_amd/csrc/hsk_texture_point.h, the text the ABI's layout
and every lane of the kernel run) compiled for the host with the sanitizers into a program of its own and compared with the numpy
twin (tests/texture_twin.py) byte for byte; the layout's properties; the analytic wall; failed projections; the PNG and PLY
writers; the C layout of the structs; the argument errors that need no device.  The cases are the GPU tests' too
(tests/texture_cases.py)."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import kit
import simplify_twin as ST
import texture_cases as TC
import texture_twin as TT
from kit import blocked
from simplify_cases import twin_of
from texture_cases import check_failed, check_wall, differing, resolved

f32 = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """hsk_texture_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program, which is run as a program)"""
    exe = kit.build_harness("texture_point", tmp_path_factory.mktemp("texture"))
    return exe


def run_harness(exe, tmp_path, vol, col, size, v, f, **params):
    Z, Y, X, _ = vol.shape
    tpm, W, n_iter, f_tol, mo = resolved(vol, size, **params)
    v, f = np.ascontiguousarray(v, f32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as o:
        o.write(np.array([X, Y, Z, 0 if col is None else 1, len(v), len(f), W, n_iter], np.int32).tobytes())
        o.write(np.array(list(size) + [tpm, f_tol, mo], f32).tobytes())
        o.write(v.tobytes())
        o.write(f.tobytes())
        o.write(blocked(vol).tobytes())
        if col is not None:
            o.write(np.ascontiguousarray(col, np.uint8).tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    info = [int(x) for x in np.frombuffer(raw, np.uint64, 13)]
    out = dict(info=dict(width=info[0], height=info[1], n_faces_charted=info[2], n_faces_skipped=info[3], n_blocks=info[4:8], n_owned=info[8],
                         n_inside=info[9], n_projected=info[10], n_colored=info[11], n_normal=info[12]))
    if info[1] > TT.MAX_SIDE:
        assert len(raw) == 104
        return out
    W, H, m, off = info[0], info[1], len(f), 104
    for name, dtype, count, shape in (("charts", np.int32, 4 * m, (m, 4)), ("uv", f32, 6 * m, (m, 3, 2)), ("rgb", np.uint8, 3 * W * H, (H, W, 3)),
                                      ("normal_rgb", np.uint8, 3 * W * H, (H, W, 3)), ("mask", np.uint8, W * H, (H, W)), ("points", f32, 3 * W * H, (H, W, 3))):
        out[name] = np.frombuffer(raw, dtype, count, off).reshape(shape)
        off += count * np.dtype(dtype).itemsize
    assert off == len(raw)
    return out


def box_meshes(oracle):
    return {c: (twin_of(oracle, "box with colour", c, ST.QUADRIC)["vertices"], twin_of(oracle, "box with colour", c, ST.QUADRIC)["faces"]) for c in (4, 8)}


# ---- 1. the kernel's text against the twin -------------------------------------------------------------------------------------
def test_the_shared_text_equals_the_twin_on_the_host(harness, tmp_path, oracle):
    vol, col, size = TC.box_case()
    cases = {}
    for c, (v, f) in box_meshes(oracle).items():
        for W in (64, 256):
            cases[("box", c, W)] = (vol, col, size, v, f, dict(atlas_width=W))
    hv, hf = TC.hand_mesh()
    cases[("hand", 0, 64)] = (vol, col, size, hv, hf, dict(atlas_width=64))
    cases[("hand, no colour", 0, 128)] = (vol, None, size, hv, hf, dict(atlas_width=128, n_iter=0))
    cases[("hand, long projection", 0, 64)] = (vol, col, size, hv, hf, dict(atlas_width=64, n_iter=16, f_tol=0.0, max_offset_m=0.02, texels_per_metre=40.0))
    cases[("empty mesh", 0, 64)] = (vol, col, size, np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), dict(atlas_width=64))
    for key, (vo, co, sz, v, f, params) in cases.items():
        got = run_harness(harness, tmp_path, vo, co, sz, v, f, **params)
        tw = TC.twin_bake(key, vo, co, sz, v, f, **params)
        assert differing(got, tw) == 0, key
        assert np.array_equal(got["points"].view(np.uint32), tw["points"].view(np.uint32)), key
        print(key, tw["info"])
    # the list is not trivial: unowned tiles, blocks of several sizes, more than one row of super-tiles, every mask bit and its absence
    box = TC.twin_bake(("box", 4, 64), None, None, None, None, None)
    assert box["H"] > 64 and sum(n > 0 for n in TC.twin_bake(("box", 8, 64), None, None, None, None, None)["info"]["n_blocks"]) >= 2
    assert (box["mask"].reshape(box["H"] // 8, 8, 8, 8).max(axis=(1, 3)) == 0).any()
    inside = (box["mask"] & 3) == 3
    assert 0 < box["info"]["n_colored"] < box["info"]["n_owned"] and (box["mask"][inside] & 4).mean() > 0.9
    hand = TC.twin_bake(("hand", 0, 64), None, None, None, None, None)
    assert all(n > 0 for n in hand["info"]["n_blocks"]) and hand["info"]["n_faces_skipped"] == 5
    assert 0 < hand["info"]["n_projected"] < hand["info"]["n_owned"] and 0 < hand["info"]["n_colored"] < hand["info"]["n_owned"]
    assert TC.twin_bake(("empty mesh", 0, 64), None, None, None, None, None)["mask"].shape == (0, 64)


# ---- 2. the layout's properties ------------------------------------------------------------------------------------------------------
def test_layout_properties(hsk, oracle):
    rng = np.random.default_rng(29)
    hv, hf = TC.hand_mesh()
    meshes = {"hand": (hv, hf, 1.0 / 0.0375)}
    for c, (v, f) in box_meshes(oracle).items():
        meshes[f"box {c}"] = (v, f, 1.0 / 0.0375)
    for name, (v, f, tpm) in meshes.items():
        for W in (64, 256):
            lay = TT.layout(v, f, f32(tpm), W)
            got = hsk.texture_layout(v, f, tpm, W)
            assert np.array_equal(got["uv"].view(np.uint32), lay["uv"].view(np.uint32)) and np.array_equal(got["charts"], lay["charts"]), (name, W)
            assert TC.info_list(got) == TC.info_list(lay["info"]), (name, W)
            H, blocks = lay["H"], lay["blocks"]
            taken = np.zeros((H // 8, W // 8), np.int64)
            sides = [b[2] for b in blocks]
            assert sides == sorted(sides, reverse=True)                                          # descending sizes
            for (x0, y0, s, fa, fb, _, _) in blocks:
                assert x0 % s == 0 and y0 % s == 0 and x0 + s <= W and y0 + s <= H                 # aligned to its size, inside the atlas
                taken[y0 // 8:(y0 + s) // 8, x0 // 8:(x0 + s) // 8] += 1
                assert fa >= 0
            assert taken.max() == 1                                                               # no two blocks overlap
            if W == 64:
                assert all(b[0] + b[2] <= 64 for b in blocks) and H == 64 * -(-int(taken.sum()) // 64)   # one column of super-tiles
            # per size, the faces in ascending order, two to a block; only the last block of a size may lack its half B
            for s in TT.SIDES:
                ids = [i for b in blocks if b[2] == s for i in b[3:5]]
                assert all(i >= 0 for i in ids[:-1]) and [i for i in ids if i >= 0] == sorted(i for i in ids if i >= 0)
            # a bilinear look-up anywhere inside a face's uv triangle touches only texels that the face owns
            own = TC.owner_of_texels(dict(mask=np.zeros((H, W), np.uint8), charts=lay["charts"]))
            for i in np.flatnonzero(lay["charts"]["s"] > 0)[:40]:
                bary = rng.dirichlet((1, 1, 1), 200)
                bary[:3] = np.eye(3)                                                             # (the corners themselves)
                uv = bary @ lay["uv"][i].astype(np.float64)
                x, y = uv[:, 0] * W - 0.5, (1.0 - uv[:, 1]) * H - 0.5
                for dx in (0, 1):
                    for dy in (0, 1):
                        px, py = np.floor(x + 1e-9).astype(int) + dx, np.floor(y + 1e-9).astype(int) + dy
                        assert (own[py, px] == i).all(), (name, W, i)
    # an odd bucket leaves half B unowned
    lay = TT.layout(hv, hf, f32(1.0 / 0.0375), 64)
    b32 = [b for b in lay["blocks"] if b[2] == 32]
    assert len(b32) == 1 and b32[0][4] == -1
    tw = TC.twin_bake(("hand", 0, 64), *TC.box_case(), hv, hf, atlas_width=64)
    x0, y0 = b32[0][:2]
    j, k = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    blk = tw["mask"][y0:y0 + 32, x0:x0 + 32]
    assert (blk[k + j > 30] == 0).all() and (blk[k + j <= 30] & 1).all()
    # skipped faces: no chart, uv 0
    skipped = lay["charts"]["s"] < 0
    assert skipped.sum() == 5 and (lay["uv"][skipped] == 0).all() and lay["info"]["n_faces_skipped"] == 5
    # rotation: the corner opposite the longest edge sits at the chart's right angle, whichever corner the face starts with
    assert [int(h) >> 8 for h in lay["charts"]["half_rot"][[0, 6, 8]]] == [0, 2, 1]


def test_a_mesh_that_needs_too_high_an_atlas_is_refused(hsk):
    """4200 faces of side 64 at W = 64: 2100 blocks, one to a super-tile -> H = 134400"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    f = np.tile(np.array([[0, 1, 2]], np.int32), (4200, 1))
    with pytest.raises(TT.TooHigh) as e:
        TT.layout(v, f, f32(100.0), 64)
    assert e.value.height == 64 * 2100
    lib, L = hsk._lib.load(), hsk._lib
    info = L.HskTextureInfo()
    uv = np.full((4200, 6), 7.0, f32)
    assert lib.hsk_texture_layout(v.ctypes.data, 3, f.ctypes.data, 4200, 100.0, 64, uv.ctypes.data, None, C.byref(info)) == -1
    assert (info.width, info.height, info.n_faces_charted, info.n_blocks[3]) == (64, 64 * 2100, 4200, 2100) and (uv == 7.0).all()
    assert b"16384" in lib.hsk_last_error(None)
    with pytest.raises(hsk.KinfuError):
        hsk.texture_layout(v, f, 100.0, 64)
    assert hsk.texture_layout(v, f, 100.0, 16384)["height"] == 64 * 9             # 2100 super-tiles, 256 to a row


# ---- 3. the analytic wall, and projections that fail ---------------------------------------------------------------------------------


def test_the_analytic_wall_on_the_host(harness, tmp_path):
    vol, col = TC.wall_volume(), TC.wall_colour()
    v, f = TC.wall_mesh(0.3)
    got = run_harness(harness, tmp_path, vol, col, TC.WALL_SIZE, v, f, atlas_width=128)
    tw = TC.twin_bake("wall", vol, col, TC.WALL_SIZE, v, f, atlas_width=128)
    assert differing(got, tw) == 0 and got["info"]["n_blocks"] == [0, 0, 0, 1]
    check_wall(got)
    check_wall(tw)
    # the mesh starts 0.3 voxel off: further than f_tol tau, so the texels moved
    assert 0.3 > 0.01 * TC.WALL_TAU_VOXELS
    assert (np.abs(got["points"][(got["mask"] & 3) == 3][:, 0] - v[0, 0]) > 0.2 * TC.WALL_CELL).all()


def test_failed_projections_on_the_host(harness, tmp_path):
    col = TC.wall_colour()
    # ten voxels off: the stored TSDF is clipped there, its gradient is 0 -- the texel keeps P0 and its colour
    v, f = TC.wall_mesh(10.0)
    got = run_harness(harness, tmp_path, TC.wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)
    assert differing(got, TC.twin_bake("wall, 10 off", TC.wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)) == 0
    check_failed(got, v, colored=True)
    assert ((got["mask"][(got["mask"] & 1) != 0] & 16) == 0).all()                  # (no gradient: no normal)
    # never observed there: the same, and the colour volume is still read at P0
    got = run_harness(harness, tmp_path, TC.unseen_wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)
    assert differing(got, TC.twin_bake("wall, unseen", TC.unseen_wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)) == 0
    check_failed(got, v, colored=True)
    # no colour there either: uncoloured
    none = col.copy()
    none[..., 3] = 0
    got = run_harness(harness, tmp_path, TC.unseen_wall_volume(), none, TC.WALL_SIZE, v, f, atlas_width=128)
    check_failed(got, v, colored=False)
    # a projection that would have to move further than max_offset_m fails, too
    v, f = TC.wall_mesh(2.0)
    got = run_harness(harness, tmp_path, TC.wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128, max_offset_m=float(TC.WALL_CELL))
    check_failed(got, v, colored=True)
    got = run_harness(harness, tmp_path, TC.wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)
    assert (got["mask"][(got["mask"] & 3) == 3] & 4).all()


# ---- 4. the files --------------------------------------------------------------------------------------------------------------------
def read_png(path):
    """a PNG's image through Python's own zlib, every chunk's crc checked -> (h, w, 3) uint8, the zlib stream"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    off, chunks = 8, []
    while off < len(raw):
        n, kind = struct.unpack(">I4s", raw[off:off + 8])
        data = raw[off + 8:off + 8 + n]
        assert struct.unpack(">I", raw[off + 8 + n:off + 12 + n])[0] == zlib.crc32(kind + data)
        chunks.append((kind, data))
        off += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3), chunks[1][1]


def test_png_files_load(tmp_path, hsk):
    from housescan_amd import products
    rng = np.random.default_rng(3)
    # 1 x 1; a row of 1 + 3 * 7000 = 21001 bytes, so the first stored block (65535 bytes) ends inside the fourth row; exactly one
    # block and one byte (65536 = 1 + 3 * 21845)
    for h, w in ((1, 1), (9, 7000), (1, 21845), (64, 64)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        path = tmp_path / f"{h}x{w}.png"
        products.write_png_rgb(path, img)
        back, z = read_png(path)
        assert np.array_equal(back, img), (h, w)
        raw_bytes = h * (1 + 3 * w)
        assert len(z) == 2 + raw_bytes + 5 * -(-raw_bytes // 65535) + 4 and z[2] == (1 if raw_bytes <= 65535 else 0)
    assert 65535 % 21001 != 0
    lib = hsk._lib.load()
    assert lib.hsk_write_png_rgb(None, img.ctypes.data, 4, 4) == -1 and lib.hsk_write_png_rgb(b"x.png", None, 4, 4) == -1
    assert lib.hsk_write_png_rgb(os.fsencode(tmp_path / "z.png"), img.ctypes.data, 0, 4) == -1 and not (tmp_path / "z.png").exists()
    assert lib.hsk_write_png_rgb(os.fsencode(tmp_path / "no" / "dir.png"), img.ctypes.data, 4, 4) == -3
    with pytest.raises(ValueError):
        products.write_png_rgb(tmp_path / "bad.png", np.zeros((4, 4), np.uint8))


def test_textured_ply_files_load(tmp_path, hsk):
    from housescan_amd import products
    hv, hf = TC.hand_mesh()
    keep = [i for i in range(len(hf)) if 0 <= hf[i].min() and hf[i].max() < len(hv)]
    v, f = np.nan_to_num(hv), hf[keep]
    uv = hsk.texture_layout(v, f, 26.0, 64)["uv"]
    nrm = np.tile(np.array([[1.0, 0.0, np.nan]], f32), (len(v), 1))
    for normals in (None, nrm):
        path = tmp_path / "m.ply"
        products.write_ply_textured(path, v, f, uv, "atlas.png", normals=normals)
        raw = open(path, "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        lines = head.decode().split("\n")
        assert lines[:3] == ["ply", "format binary_little_endian 1.0", "comment TextureFile atlas.png"]
        want = [f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
        want += ["property float nx", "property float ny", "property float nz"] if normals is not None else []
        want += [f"element face {len(f)}", "property list uchar int vertex_indices", "property list uchar float texcoord", ""]
        assert lines[3:] == want
        vrec = 24 if normals is not None else 12
        assert len(body) == vrec * len(v) + 38 * len(f)
        vb = np.frombuffer(body, f32, (vrec // 4) * len(v)).reshape(len(v), -1)
        assert np.array_equal(vb[:, :3], v) and (normals is None or np.array_equal(vb[:, 3:], np.nan_to_num(nrm)))
        faces = np.frombuffer(body, np.dtype([("n", "u1"), ("i", "<i4", 3), ("m", "u1"), ("uv", "<f4", 6)]), len(f), vrec * len(v))
        assert (faces["n"] == 3).all() and (faces["m"] == 6).all() and np.array_equal(faces["i"], f)
        assert np.array_equal(faces["uv"].view(np.uint32), uv.reshape(-1, 6).view(np.uint32))
    lib = hsk._lib.load()
    args = (v.ctypes.data, None, len(v), f.ctypes.data, len(f))
    assert lib.hsk_write_ply_textured(os.fsencode(tmp_path / "a.ply"), *args, uv.ctypes.data, b"two\nlines.png") == -1
    assert lib.hsk_write_ply_textured(os.fsencode(tmp_path / "a.ply"), *args, uv.ctypes.data, b"") == -1
    assert lib.hsk_write_ply_textured(os.fsencode(tmp_path / "a.ply"), *args, uv.ctypes.data, None) == -1
    assert lib.hsk_write_ply_textured(os.fsencode(tmp_path / "a.ply"), *args, None, b"a.png") == -1
    bad = f.copy()
    bad[0, 0] = len(v)
    assert lib.hsk_write_ply_textured(os.fsencode(tmp_path / "a.ply"), v.ctypes.data, None, len(v), bad.ctypes.data, len(f), uv.ctypes.data, b"a.png") == -1
    assert not (tmp_path / "a.ply").exists()
    # and the untextured writer's file is what it was: no comment line, 13 bytes a face
    products.write_ply_indexed(tmp_path / "i.ply", v, f)
    raw = open(tmp_path / "i.ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    assert b"TextureFile" not in head and b"texcoord" not in head and len(body) == 12 * len(v) + 13 * len(f)


# ---- 5. C layout, Python mirror, errors without a device ---------------------------------------------------------------------------------
def test_texture_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, Ch, I = _lib.HskTextureParams, _lib.HskTextureChart, _lib.HskTextureInfo
    assert (C.sizeof(P), C.sizeof(Ch), C.sizeof(I)) == (20, 16, 104)
    assert (TT.OWNED, TT.INSIDE, TT.PROJECTED, TT.COLORED, TT.NORMAL) == (1, 2, 4, 8, 16) == (
        hsk.TEXEL_OWNED, hsk.TEXEL_INSIDE, hsk.TEXEL_PROJECTED, hsk.TEXEL_COLORED, hsk.TEXEL_NORMAL) == (
        _lib.HSK_TEXEL_OWNED, _lib.HSK_TEXEL_INSIDE, _lib.HSK_TEXEL_PROJECTED, _lib.HSK_TEXEL_COLORED, _lib.HSK_TEXEL_NORMAL)
    assert tuple(n for n, _ in I._fields_) == hsk.kinfu.TEXTURE_INFO_FIELDS == TT.INFO_FIELDS
    assert hsk.kinfu.TEXTURE_CHART_DTYPE == TT.CHART_DTYPE and TT.CHART_DTYPE.itemsize == 16


def test_argument_errors_that_need_no_device(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    p = L.HskTextureParams(9.0, 9, 9, 9.0, 9.0)
    lib.hsk_default_texture_params(None, C.byref(p))
    assert (p.texels_per_metre, p.atlas_width, p.n_iter, p.f_tol, p.max_offset_m) == (0.0, 0, 4, f32(0.01), 0.0)
    lib.hsk_default_texture_params(None, None)
    info = L.HskTextureInfo(width=77)
    assert lib.hsk_bake_texture(None, None, 0, None, 0, None, None, None, None, 0, None, None, C.byref(info)) == -1 and info.width == 77
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    f = np.array([[0, 1, 2]], np.int32)
    assert hsk.texture_layout(v, f, 10.0)["width"] == 1024                        # (0: the default width)
    for bad in (dict(texels_per_metre=0.0), dict(texels_per_metre=-1.0), dict(texels_per_metre=float("nan")), dict(texels_per_metre=float("inf")),
                dict(atlas_width=32), dict(atlas_width=100), dict(atlas_width=-64), dict(atlas_width=16448)):
        with pytest.raises(hsk.KinfuError):
            hsk.texture_layout(v, f, **dict(dict(texels_per_metre=10.0), **bad))
    assert lib.hsk_texture_layout(None, 3, f.ctypes.data, 1, 10.0, 64, None, None, None) == -1
    assert lib.hsk_texture_layout(v.ctypes.data, 3, None, 1, 10.0, 64, None, None, None) == -1
    assert lib.hsk_texture_layout(None, 0, None, 0, 10.0, 64, None, None, C.byref(info)) == 0 and (info.width, info.height) == (64, 0)
    assert callable(hsk.KinfuTracker.bake_texture)
