"""Keyframe textures without a GPU: the rule (housescan_amd/csrc/hsk_keytex_point.h, the text every lane of the kernel runs)
compiled for the host with the sanitizers into a program of its own and compared with the numpy twin (tests/keytex_twin.py) byte
for byte on the cases of tests/keytex_cases.py, in both modes; the analytic checks on the wall -- the colour against a binary64
projection, the occluder, the hole and the column where two depths meet, the tie, the cameras that must fail --; the empty store;
hsk_keyframe_wanted; the C layout of the structs; the argument errors that need no device."""
import ctypes as C

import numpy as np
import pytest

import keytex_cases as KC
import keytex_twin as KT
import kit
import texture_cases as TC
import texture_twin as TT
from keytex_cases import differing
from kit import blocked
from texture_cases import resolved

f32 = np.float32
MODES = (KT.BEST, KT.BLEND)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """hsk_keytex_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program, which is run as a program)"""
    exe = kit.build_harness("keytex_point", tmp_path_factory.mktemp("keytex"))
    return exe


def run_harness(exe, tmp_path, vol, col, size, v, f, kfs, keytex, tex):
    Z, Y, X, _ = vol.shape
    tpm, W, n_iter, f_tol, mo = resolved(vol, size, **tex)
    kp = KT.default_params(max(TT.cells((X, Y, Z), size)))
    kp.update(keytex)
    v, f = np.ascontiguousarray(v, f32).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    kh, kw = kfs[0]["depth"].shape if kfs else (2, 2)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as o:
        o.write(np.array([X, Y, Z, 0 if col is None else 1, len(v), len(f), W, n_iter, len(kfs), kw, kh, kp["mode"], kp["fallback_volume"]], np.int32).tobytes())
        o.write(np.array(list(size) + [tpm, f_tol, mo] + [kp[n] for n in ("z_min_m", "z_max_m", "cos_min", "border_px", "occlusion_tol_m", "blend_floor")],
                         f32).tobytes())
        o.write(v.tobytes())
        o.write(f.tobytes())
        o.write(blocked(vol).tobytes())
        if col is not None:
            o.write(np.ascontiguousarray(col, np.uint8).tobytes())
        for kf in kfs:
            o.write(np.concatenate([kf["pose"][:3, :3].reshape(-1), kf["pose"][:3, 3], kf["intr"]]).astype(f32).tobytes())
            o.write(kf["rgb"].tobytes())
            o.write(kf["depth"].tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    info = [int(x) for x in np.frombuffer(raw, np.uint64, 13)]
    out = dict(info=dict(width=info[0], height=info[1], n_faces_charted=info[2], n_faces_skipped=info[3], n_blocks=info[4:8], n_owned=info[8],
                         n_inside=info[9], n_projected=info[10], n_colored=info[11], n_normal=info[12]),
               kinfo=dict(zip(KT.KINFO_FIELDS, (int(x) for x in np.frombuffer(raw, np.uint64, 6, 104)))))
    W, H, m, off = info[0], info[1], len(f), 152
    for name, dtype, count, shape in (("charts", np.int32, 4 * m, (m, 4)), ("uv", f32, 6 * m, (m, 3, 2)), ("rgb", np.uint8, 3 * W * H, (H, W, 3)),
                                      ("normal_rgb", np.uint8, 3 * W * H, (H, W, 3)), ("mask", np.uint8, W * H, (H, W)), ("source", np.uint8, W * H, (H, W)),
                                      ("points", f32, 3 * W * H, (H, W, 3))):
        out[name] = np.frombuffer(raw, dtype, count, off).reshape(shape)
        off += count * np.dtype(dtype).itemsize
    assert off == len(raw)
    return out


def inside_projected(tw):
    return (tw["mask"] & 7) == 7


# ---- 1. the kernel's text against the twin -------------------------------------------------------------------------------------
def test_the_shared_text_equals_the_twin_on_the_host(harness, tmp_path, oracle):
    for key, case in KC.all_cases(oracle).items():
        for mode in MODES:
            tw = KC.twin_bake(key, mode, *case)
            got = run_harness(harness, tmp_path, *case[:6], dict(case[6], mode=mode), case[7])
            assert differing(got, tw) == 0, (key, mode, got["kinfo"], tw["kinfo"])
            assert np.array_equal(got["points"].view(np.uint32), tw["points"].view(np.uint32)), key
            k = tw["kinfo"]
            assert k["n_keyed"] + k["n_fallback"] + k["n_uncolored"] == tw["info"]["n_owned"]
            print(key, mode, k)
    # the list is not trivial: keyed and unkeyed texels, occluded pairs, every source of the competing cameras that can win, a
    # blend that differs from the best, and more keyframes than any staging would hold
    comp = KC.twin_bake("competing", KT.BEST, None, None, None, None, None, None, None, None)
    assert set(np.unique(comp["source"])) == {0, 1, 5, KT.NONE}
    ring = [KC.twin_bake("ring of 70", m, None, None, None, None, None, None, None, None) for m in MODES]
    assert ring[0]["kinfo"]["n_keyframes"] == 70 and ring[0]["source"][ring[0]["source"] != KT.NONE].max() >= 64
    assert (ring[0]["rgb"] != ring[1]["rgb"]).any() and np.array_equal(ring[0]["source"], ring[1]["source"])
    box = KC.twin_bake("box", KT.BEST, None, None, None, None, None, None, None, None)
    k = box["kinfo"]
    assert k["n_keyed"] > 1000 and k["n_fallback"] > 100 and k["n_uncolored"] > 100 and 0 < k["n_pairs_occluded"] < k["n_pairs_seen"]
    assert len(np.unique(box["source"])) == 4


# ---- 2. the analytic wall ------------------------------------------------------------------------------------------------------
def test_the_frontal_camera_colours_the_wall_from_the_photograph(harness, tmp_path):
    """For every keyed texel the colour is within 1 level of the bilinear value of the stripes at the pixel obtained by projecting
    the twin's float32 point in binary64.  The bound: the rule projects in binary32 -- d = q - t of magnitude 2 (an ulp of 2.4e-7),
    three dot products, one division and a multiply-add by fx = 40 at u below 64 (an ulp of 3.8e-6) -- so its pixel is within 1e-3
    of the binary64 one with a wide margin; the stripes change by at most 128 levels per pixel, so the value moves by less than
    0.13 level, the binary32 interpolation adds some 1e-4, and the rounding to a level at most 0.5: below 1.  No keyed texel's
    pixel changes its integer part under an error of 1e-3 often enough to matter, and where it does the bilinear form is continuous.

    The frontal camera alone keys at least half of the wall's inside-and-projected texels (measured: 0.69)."""
    case = KC.wall_cases()["frontal"]
    kf = case[5][0]
    for mode in MODES:
        tw = KC.twin_bake("frontal", mode, *case)
        got = run_harness(harness, tmp_path, *case[:6], dict(case[6], mode=mode), case[7])
        assert differing(got, tw) == 0
        ip = inside_projected(tw)
        keyed = (got["mask"] & KT.KEYFRAME) != 0
        share = (keyed & ip).sum() / ip.sum()
        print("share of inside-and-projected texels keyed:", share)
        assert ip.sum() > 1500 and share >= 0.5
        u, v, zc = KC.project64(kf, tw["points"][keyed])
        iu, iv = np.minimum(np.floor(u).astype(int), KC.KW - 2), np.minimum(np.floor(v).astype(int), KC.KH - 2)
        a, b = (u - iu)[:, None], (v - iv)[:, None]
        img = kf["rgb"].astype(np.float64)
        top, bot = img[iv, iu] + a * (img[iv, iu + 1] - img[iv, iu]), img[iv + 1, iu] + a * (img[iv + 1, iu + 1] - img[iv + 1, iu])
        want = top + b * (bot - top)
        err = np.abs(got["rgb"][keyed].astype(np.float64) - want).max()
        print("largest colour error in levels:", err)
        assert err <= 1.0
        assert (got["source"][keyed] == 0).all() and (got["source"][~keyed] == KT.NONE).all() and (got["rgb"][~keyed] == 0).all()
        assert ((got["mask"][keyed] & TT.COLORED) == 0).all() and np.abs(zc - KC.FRONT_M).max() < 0.01
        # the pattern is in the atlas: both stripe levels and values between them, which no colour voxel of 94 mm could hold
        assert got["rgb"][keyed][:, 0].min() == 64 and got["rgb"][keyed][:, 0].max() == 192
        # every pair that passed steps 1 to 3 saw the wall: nothing is occluded, and n = 1 makes the blend the best
        assert tw["kinfo"]["n_pairs_occluded"] == 0 and tw["kinfo"]["n_pairs_seen"] == tw["kinfo"]["n_keyed"] == keyed.sum()
    assert np.array_equal(KC.twin_bake("frontal", KT.BEST, *case)["rgb"], KC.twin_bake("frontal", KT.BLEND, *case)["rgb"])


def test_occluder_hole_and_meeting_column(harness, tmp_path):
    """the edited depth image: no texel whose four taps touch the occluder's columns, the D = 0 block or the column where the two
    depths meet is keyed; every other texel the unedited image keyed still is"""
    case, plain = KC.wall_cases()["edited depth"], KC.wall_cases()["frontal"]
    kf = case[5][0]
    for mode in MODES:
        tw = KC.twin_bake("edited depth", mode, *case)
        got = run_harness(harness, tmp_path, *case[:6], dict(case[6], mode=mode), case[7])
        assert differing(got, tw) == 0
        ref = KC.twin_bake("frontal", mode, *plain)
        was = (ref["mask"] & KT.KEYFRAME) != 0
        u, v, _ = KC.project64(kf, tw["points"].reshape(-1, 3))
        u, v = u.reshape(was.shape), v.reshape(was.shape)
        keyed = (got["mask"] & KT.KEYFRAME) != 0
        eps = 1e-3                                                    # (the binary32 pixel is within this of the binary64 one)
        behind = was & (u < KC.LEFT_COLS - eps)                       # taps in columns <= 16: the occluder, or where it meets the wall
        rows, cols = KC.HOLE
        hole = was & (u > cols.start - 1 + eps) & (u < cols.stop - eps) & (v > rows.start - 1 + eps) & (v < rows.stop - eps)
        clear = was & (u > KC.LEFT_COLS + eps) & ~((u > cols.start - 1 - eps) & (u < cols.stop + eps) & (v > rows.start - 1 - eps) & (v < rows.stop + eps))
        assert behind.sum() > 300 and hole.sum() > 50 and clear.sum() > 500
        assert not keyed[behind].any() and not keyed[hole].any() and keyed[clear].all()
        meeting = was & (u > KC.LEFT_COLS - 1 + eps) & (u < KC.LEFT_COLS - eps)    # iu = 16: taps in columns 16 and 17
        assert meeting.sum() > 20 and not keyed[meeting].any()
        assert tw["kinfo"]["n_pairs_occluded"] == was.sum() - keyed.sum() > 0 and tw["kinfo"]["n_pairs_seen"] == was.sum()
        assert (got["rgb"][~keyed] == 0).all() and tw["kinfo"]["n_fallback"] == 0
    # with a colour volume, what the photograph does not show falls back to it and says so
    case = KC.wall_cases()["edited depth, fallback"]
    tw = KC.twin_bake("edited depth, fallback", KT.BEST, *case)
    base = TC.twin_bake("wall", case[0], case[1], case[2], case[3], case[4], atlas_width=128)
    keyed = (tw["mask"] & KT.KEYFRAME) != 0
    assert np.array_equal(tw["rgb"][~keyed], base["rgb"][~keyed]) and np.array_equal(tw["mask"][~keyed], base["mask"][~keyed])
    assert ((tw["mask"][keyed] & TT.COLORED) == 0).all() and tw["kinfo"]["n_fallback"] == int(((base["mask"] & TT.COLORED) != 0)[~keyed].sum()) > 0


def test_competing_cameras(harness, tmp_path):
    case = KC.wall_cases()["competing"]
    kfs = case[5]
    tw = KC.twin_bake("competing", KT.BEST, *case)
    got = run_harness(harness, tmp_path, *case[:6], dict(case[6], mode=KT.BEST), case[7])
    assert differing(got, tw) == 0
    src = got["source"]
    # the identical pair reports source 0; the camera behind the wall and the one too near never win
    assert (src == 0).sum() > 300 and not np.isin(src, (2, 3, 4)).any()
    # the near frontal camera wins wherever it sees the texel (it is closer: the weight is c / r2), and nowhere else
    u, v, _ = KC.project64(kfs[5], tw["points"].reshape(-1, 3))
    u, v = u.reshape(src.shape), v.reshape(src.shape)
    has_n = (tw["mask"] & TT.NORMAL) != 0
    well_in = has_n & (u > 4 + 1e-3) & (u < KC.KW - 5 - 1e-3) & (v > 4 + 1e-3) & (v < KC.KH - 5 - 1e-3)
    out = (u < 4 - 1e-3) | (u > KC.KW - 5 + 1e-3) | (v < 4 - 1e-3) | (v > KC.KH - 5 + 1e-3)
    assert well_in.sum() > 300 and (src[well_in] == 5).all() and not (src[out] == 5).any() and (src[has_n & out] != KT.NONE).mean() > 0.9
    # the oblique camera colours what the frontal one's image does not reach
    assert (src == 1).sum() > 300
    # each camera alone: behind the wall the view angle fails before anything is counted, too near z_min_m does
    for k in (3, 4):
        alone = KT.bake(*case[:5], [kfs[k]], dict(case[6], mode=KT.BEST), **case[7])
        assert alone["kinfo"]["n_keyed"] == 0 and alone["kinfo"]["n_pairs_seen"] == 0
    # the blend mixes the frontal and the oblique where both see the texel, and names the better of them
    bl = KC.twin_bake("competing", KT.BLEND, *case)
    assert np.array_equal(bl["source"], tw["source"]) and (bl["rgb"] != tw["rgb"]).any()


def test_an_empty_store_is_the_colour_volume(harness, tmp_path):
    case = KC.wall_cases()["empty store"]
    base = TC.twin_bake("wall", case[0], case[1], case[2], case[3], case[4], atlas_width=128)
    for mode in MODES:
        got = run_harness(harness, tmp_path, *case[:6], dict(case[6], mode=mode), case[7])
        for name in ("rgb", "normal_rgb", "mask"):
            assert np.array_equal(got[name], base[name]), name
        assert (got["source"] == KT.NONE).all() and got["info"] == base["info"]
        assert got["kinfo"] == dict(n_keyframes=0, n_keyed=0, n_fallback=base["info"]["n_colored"], n_uncolored=base["info"]["n_owned"] - base["info"]["n_colored"],
                                    n_pairs_seen=0, n_pairs_occluded=0)
    # without the fallback, or without a colour volume: black
    for col, fb in ((case[1], 0), (None, 1)):
        got = run_harness(harness, tmp_path, case[0], col, *case[2:6], dict(fallback_volume=fb), case[7])
        assert (got["rgb"] == 0).all() and np.array_equal(got["mask"], base["mask"] & ~np.uint8(TT.COLORED)) and got["kinfo"]["n_uncolored"] == base["info"]["n_owned"]


# ---- 3. the selection rule -------------------------------------------------------------------------------------------------------
def rot_z(deg):
    a = np.radians(deg)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return m


def test_keyframe_wanted(hsk):
    def at(x, deg=0.0):
        m = rot_z(deg)
        m[0, 3] = x
        return m.astype(f32)
    stored = [at(0.0), at(1.0, 90.0)]
    rad = np.radians
    assert hsk.keyframe_wanted([], at(0.0)) is True
    assert hsk.keyframe_wanted(stored, at(0.1), 0.3, rad(20)) is False               # near pose 0 in both
    assert hsk.keyframe_wanted(stored, at(0.5), 0.3, rad(20)) is True                # far from both in position
    assert hsk.keyframe_wanted(stored, at(0.1, 30.0), 0.3, rad(20)) is True          # near pose 0 in position, but turned by 30 degrees
    assert hsk.keyframe_wanted(stored, at(0.1, 30.0), 0.3, rad(31)) is False
    assert hsk.keyframe_wanted(stored, at(0.9, 80.0), 0.3, rad(20)) is False         # near pose 1 in both
    assert hsk.keyframe_wanted(stored, at(0.9, 80.0), 0.05, rad(20)) is True
    assert hsk.keyframe_wanted(stored, at(0.9, 80.0), 0.3, rad(5)) is True
    assert hsk.keyframe_wanted(stored, at(0.0), 0.0, 0.0) is False                   # "more than": the same pose is never wanted
    assert hsk.keyframe_wanted([at(0.0, 180.0)], at(0.0), 10.0, 3.0) is True         # trace -1: the cosine is clamped, the angle pi
    assert hsk.keyframe_wanted([at(0.0, 180.0)], at(0.0), 10.0, 3.2) is False
    lib = hsk._lib.load()
    p = at(0.0)
    for mt, ma in ((-0.1, 0.1), (0.1, -0.1), (float("nan"), 0.1), (0.1, float("inf"))):
        assert lib.hsk_keyframe_wanted(p.ctypes.data, 1, p.ctypes.data, mt, ma) == -1
        with pytest.raises(hsk.KinfuError):
            hsk.keyframe_wanted(stored, p, mt, ma)
    assert lib.hsk_keyframe_wanted(None, 1, p.ctypes.data, 0.3, 0.3) == -1 and lib.hsk_keyframe_wanted(p.ctypes.data, 1, None, 0.3, 0.3) == -1
    assert lib.hsk_keyframe_wanted(None, 0, p.ctypes.data, 0.3, 0.3) == 1


# ---- 4. C layout, Python mirror, errors without a device ---------------------------------------------------------------------------------
def test_keytex_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, I = _lib.HskKeytexParams, _lib.HskKeytexInfo
    assert (C.sizeof(P), C.sizeof(I)) == (32, 48) and [hsk.TEXEL_KEYFRAME, hsk.KEYTEX_BEST, hsk.KEYTEX_BLEND, hsk.KEYTEX_NONE] == [
        _lib.HSK_TEXEL_KEYFRAME, _lib.HSK_KEYTEX_BEST, _lib.HSK_KEYTEX_BLEND, _lib.HSK_KEYTEX_NONE] == [32, 0, 1, 255] == [KT.KEYFRAME, KT.BEST, KT.BLEND, KT.NONE]
    assert tuple(n for n, _ in I._fields_) == hsk.kinfu.KEYTEX_INFO_FIELDS == KT.KINFO_FIELDS
    assert tuple(n for n, _ in P._fields_) == tuple(KT.default_params(0.01))


def test_argument_errors_that_need_no_device(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    p = L.HskKeytexParams(9, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9)
    lib.hsk_default_keytex_params(None, C.byref(p))
    want = KT.default_params(0.01)
    assert [getattr(p, n) for n, _ in p._fields_] == [want["mode"], f32(0.3), 4.0, f32(0.2), 4.0, f32(0.03), 0.5, 1]
    lib.hsk_default_keytex_params(None, None)
    kinfo = L.HskKeytexInfo(n_keyed=77)
    assert lib.hsk_bake_texture_keyframes(None, None, 0, None, 0, None, None, None, None, None, None, 0, None, None, None, C.byref(kinfo)) == -1
    assert kinfo.n_keyed == 77
    assert lib.hsk_enable_keyframes(None, 4, 16, 12) == -1 and lib.hsk_add_keyframe(None, None, None, 16, 12, None, None, None) == -1
    assert lib.hsk_keyframe_count(None, None, None, None, None, None) == -1 and lib.hsk_get_keyframe(None, 0, None, None, None, None) == -1
    assert lib.hsk_clear_keyframes(None) == -1 and lib.hsk_release_keyframes(None) == -1
    for name in ("enable_keyframes", "add_keyframe", "keyframe_count", "get_keyframe", "clear_keyframes", "release_keyframes", "bake_texture_keyframes"):
        assert callable(getattr(hsk.KinfuTracker, name))
