"""The clearance field without a GPU: the numpy twin's separable capped form (tests/clearance_twin.py) against the literal minimum over
all obstacles on random small volumes; the kernels' shared text (housescan_amd/csrc/hsk_clear_point.h) compiled for the host with
the sanitizers, making whole fields, against the twin -- zero differences; the default parameters of the project's test scene;
hsk_clearance_d2 and hsk_rank_views_clear; the C layout of the new structs and their Python mirror; the argument errors that need
no device.  The volumes and constants here are the GPU tests' too."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_twin as AT
import clearance_twin as CL
import kit
from clearance_cases import AXIS_SEG, MASK_BITS, SCENE_DEFAULTS, lookup_points, twin_field
from components_cases import speckled
from cover_cases import carved_volume
from kit import ROOT, blocked

f32 = np.float32


def header_constant(name):
    src = open(os.path.join(ROOT, "housescan_amd", "csrc", "hsk_clear_point.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, src).group(1))


def random_states(rng, dims, p_solid=0.03, p_unseen=0.1):
    """a small volume [z, y, x, 2] of FREE voxels with a few SOLID (tsdf <= 0) and UNSEEN ones"""
    X, Y, Z = dims
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[..., 0], vol[..., 1] = 32767, 3
    r = rng.random((Z, Y, X))
    solid, unseen = r < p_solid, (r >= p_solid) & (r < p_solid + p_unseen)
    vol[solid, 0] = rng.choice(np.array([0, -1, -32767], np.int16), int(solid.sum()))
    vol[unseen] = (rng.integers(-5, 5), 0)
    return vol


# ---- 1. the twin: separable and capped == literal -----------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [(1, 1, 1), (16, 25, 44), (1024, 1, 1)])
def test_the_separable_capped_form_equals_the_literal_minimum(weight):
    rng = np.random.default_rng(sum(weight))
    n_checked = 0
    for trial in range(6):
        dims = tuple(int(v) for v in rng.integers(1, 15, 3))
        vol = random_states(rng, dims, p_solid=(0.0 if trial == 0 else 0.03))
        for cap in (0, 1, 100, 255 * 255 * min(weight)):
            for flags in (0, CL.UNKNOWN):
                got = CL.field(vol, weight, cap, flags)
                want = CL.literal(CL.obstacles(vol, flags), weight, cap, flags)
                assert got.dtype == np.uint32 and int((got != want).sum()) == 0, (dims, weight, cap, flags)
                assert ((got == 0) == CL.obstacles(vol, flags)).all()
                n_checked += 1
    assert n_checked == 48


def test_the_twin_on_a_hand_written_case():
    vol = np.zeros((1, 3, 8, 2), np.int16)
    vol[..., 0], vol[..., 1] = 32767, 1
    vol[0, 1, 2] = (-5, 1)
    vol[0, 0, 7] = (9, 0)                                      # UNSEEN: an obstacle only with the flag
    got = CL.field(vol, (1, 4, 9), 9, 0)
    assert got[0, 1].tolist() == [4, 1, 0, 1, 4, 9, CL.FAR, CL.FAR] and got[0, 0].tolist() == [8, 5, 4, 5, 8, CL.FAR, CL.FAR, CL.FAR]
    flagged = CL.field(vol, (1, 4, 9), 9, CL.UNKNOWN)
    assert flagged[0, 1].tolist() == [1, 1, 0, 1, 4, 8, 4, 1] and flagged[0, 0].tolist() == [1, 4, 4, 4, 4, 4, 1, 0]   # the borders: x, then y (4), z (9)
    assert CL.stats(vol, got, 0) == {"n_obstacle": 1, "n_far": 2 + 3 + 3, "max_d2_seen": 9}
    assert [CL.reach(11378, w) for w in (16, 25, 44)] == [26, 21, 16] and CL.reach(0, 7) == 0 and CL.reach(255 * 255, 1) == 255


# ---- 2. the kernels' shared text on the host --------------------------------------------------------------------------------------------
def host_cases():
    sp = speckled(carved_volume(), 46)
    return {"carved": carved_volume(), "speckled 46 planes": np.ascontiguousarray(sp[:46]),
            "speckled 72 x 56 x 41": np.ascontiguousarray(speckled(carved_volume(), 41)[:41, :56, :72])}


def run_harness(exe, tmp_path, vol, weight, max_d2, flags, size_m, pts):
    Z, Y, X = vol.shape[:3]
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for part in (np.array([X, Y, Z], np.int32), np.array(list(weight) + [max_d2, flags], np.uint32), np.array(size_m, f32), np.uint32(len(pts)), pts,
                     blocked(vol)):
            f.write(np.ascontiguousarray(part).tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    n = X * Y * Z
    fld = np.frombuffer(raw, np.uint32, n).reshape(Z, Y, X)
    st = np.frombuffer(raw, np.uint64, 3, n * 4)
    return fld, {"n_obstacle": int(st[0]), "n_far": int(st[1]), "max_d2_seen": int(st[2])}, np.frombuffer(raw, np.uint32, len(pts), n * 4 + 24)


def test_the_kernels_text_makes_the_twins_field_on_the_host(tmp_path):
    """hsk_clear_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program): row masks, nearest bits, windowed minima and the point lookup against the twin, zero differences"""
    assert (header_constant("CLEAR_MASK_BITS"), header_constant("CLEAR_AXIS_SEG"), header_constant("CLEAR_MAX_REACH")) == (MASK_BITS, AXIS_SEG, CL.MAX_REACH)
    exe = kit.build_harness("clear_point", tmp_path)
    for name, vol in host_cases().items():
        Z, Y, X = vol.shape[:3]
        size = (3.0 * X / 80, 3.0 * Y / 64, 3.0 * Z / 48)
        d = CL.default_params(size, (X, Y, Z))
        pts = lookup_points(size, (X, Y, Z))
        for weight, max_d2, flags in ((d["weight"], d["max_d2"], CL.UNKNOWN), (d["weight"], d["max_d2"], 0), ((1, 1, 1), 255 * 255, 0), ((1, 1, 1024), 255 * 255, CL.UNKNOWN),
                                      ((1, 1, 1), 0, CL.UNKNOWN)):
            fld, st, at = run_harness(exe, tmp_path, vol, weight, max_d2, flags, size, pts)
            ref = twin_field(name, vol, weight, max_d2, flags)
            print(f"{name} {weight} {max_d2} {flags}: {st}")
            assert int((fld != ref).sum()) == 0, (name, weight, max_d2, flags)
            assert st == CL.stats(vol, ref, flags)
            assert np.array_equal(at, CL.lookup(ref, size, pts))
    ref = twin_field("carved", carved_volume(), SCENE_DEFAULTS["weight"], SCENE_DEFAULTS["max_d2"], CL.UNKNOWN)
    assert int(ref[ref != CL.FAR].max()) > 16 * 9, "the carved room has clear space three voxels from anything"


def test_the_lookup_points_cover_every_case():
    pts = lookup_points(AT.DST_SIZE, AT.DST_DIMS)
    at = CL.lookup(np.arange(80 * 64 * 48, dtype=np.uint32).reshape(48, 64, 80), AT.DST_SIZE, pts)
    assert (at[:85] != CL.OUTSIDE).sum() == 83 and (at[-7:] == CL.OUTSIDE).all() and at[80] == 0 and at[81] == CL.OUTSIDE and at[82] == CL.OUTSIDE
    assert at[83] == 26 + 16 * 64 * 80 and at[84] == 79 + (21 + 16 * 64) * 80          # -0.0 is voxel 0 on its axis


# ---- 3. defaults, d2, ranking, layout, errors without a device ------------------------------------------------------------------------
def test_default_parameters(hsk):
    got = CL.default_params(AT.DST_SIZE, AT.DST_DIMS)
    assert got == SCENE_DEFAULTS and got["unit_m"].dtype == np.float32
    assert got["max_d2"] == int(np.ceil((1.0 / np.float64(f32(0.009375))) ** 2)) == 11378
    cube = CL.default_params((3.0, 3.0, 3.0), (256, 256, 256))
    assert cube == {"weight": (1, 1, 1), "max_d2": 7282, "flags": CL.UNKNOWN, "unit_m": f32(3.0) / f32(256)}
    p = hsk.default_clearance_params()
    assert (tuple(p.weight), p.max_d2, p.flags, f32(p.unit_m)) == (cube["weight"], cube["max_d2"], cube["flags"], cube["unit_m"])
    assert CL.default_params((0.5, 0.5, 0.5), (512, 512, 512))["max_d2"] == 255 * 255          # a metre is beyond the reach: capped
    q = hsk.default_clearance_params(weight=(2, 3, 4), max_d2=9, flags=0, unit_m=0.5)
    assert (tuple(q.weight), q.max_d2, q.flags, q.unit_m) == ((2, 3, 4), 9, 0, 0.5)
    with pytest.raises(TypeError, match="no field"):
        hsk.default_clearance_params(reach=3)
    hsk._lib.load().hsk_default_clearance_params(None, None)


def test_clearance_d2(hsk):
    p = hsk.default_clearance_params(unit_m=0.009375)
    assert hsk.clearance_d2(p, 0.3) == CL.d2_of_metres(0.009375, 0.3) in (1024, 1025) and hsk.clearance_d2(p, 1.0) == CL.d2_of_metres(0.009375, 1.0) == 11378
    assert hsk.clearance_d2(p, 0.0) == 0 and hsk.clearance_d2(p, -1.0) == 0 and hsk.clearance_d2(p, 0.009375) == 1
    assert hsk.clearance_d2(p, 1e6) == CL.FAR and hsk.clearance_d2(p, float("inf")) == CL.FAR and hsk.clearance_d2(p, float("nan")) == CL.FAR
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert hsk.clearance_d2(hsk.default_clearance_params(unit_m=bad), 0.3) == CL.FAR
    assert hsk._lib.load().hsk_clearance_d2(None, 0.3) == CL.FAR
    m = hsk.clearance_metres(p, np.array([0, 1024, CL.FAR, CL.OUTSIDE], np.uint32))
    assert m[0] == 0 and abs(m[1] - 0.3) < 1e-6 and np.isinf(m[2]) and np.isnan(m[3])


def test_rank_views_clear(hsk):
    rng = np.random.default_rng(8)
    n = 60
    s = np.zeros(n, hsk.kinfu.VIEW_SCORE_DTYPE)
    s["gain"], s["n_frontier"] = rng.integers(0, 6, n), rng.integers(0, 3, n)
    s["eye_state"] = rng.choice([0, 0, 0, 1, 2, 3], n)
    d = rng.choice(np.array([0, 5, 99, 100, 101, CL.FAR, CL.OUTSIDE], np.uint32), n)
    got = hsk.rank_views_clear(s, d, 100)
    assert np.array_equal(got, CL.rank_views_clear(s, d, 100)) and sorted(got.tolist()) == list(range(n))
    behind = (s["eye_state"] != 0) | (d < 100) | (d == CL.OUTSIDE)
    k = int((~behind).sum())
    assert 0 < k < n and not behind[got[:k]].any() and behind[got[k:]].all()
    assert np.array_equal(hsk.rank_views_clear(s, d, 0)[:int((s["eye_state"] == 0).sum() - ((s["eye_state"] == 0) & (d == CL.OUTSIDE)).sum())],
                          [i for i in hsk.rank_views(s) if s["eye_state"][i] == 0 and d[i] != CL.OUTSIDE])
    assert len(hsk.rank_views_clear(s[:0], d[:0], 5)) == 0
    lib = hsk._lib.load()
    order = np.full(n, 7, np.uint32)
    assert lib.hsk_rank_views_clear(None, d.ctypes.data_as(C.POINTER(C.c_uint32)), 1, n, order.ctypes.data_as(C.POINTER(C.c_uint32))) == -1
    assert lib.hsk_rank_views_clear(s.ctypes.data_as(C.POINTER(hsk._lib.HskViewScore)), None, 1, n, order.ctypes.data_as(C.POINTER(C.c_uint32))) == -1
    assert (order == 7).all()
    with pytest.raises(ValueError):
        hsk.rank_views_clear(s, d[:3], 5)


def test_clearance_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, S = _lib.HskClearanceParams, _lib.HskClearanceStats
    assert (C.sizeof(P), C.sizeof(S)) == (24, 32)
    assert (CL.FAR, CL.OUTSIDE, CL.UNKNOWN, CL.MAX_REACH) == (_lib.HSK_CLEARANCE_FAR, _lib.HSK_CLEARANCE_OUTSIDE, _lib.HSK_CLEAR_UNKNOWN, _lib.HSK_CLEAR_MAX_REACH)
    assert (hsk.kinfu.CLEARANCE_FAR, hsk.kinfu.CLEARANCE_OUTSIDE, hsk.kinfu.CLEAR_UNKNOWN) == (CL.FAR, CL.OUTSIDE, CL.UNKNOWN)
    assert tuple(n for n, _ in P._fields_) == hsk.kinfu.CLEARANCE_FIELDS


def test_null_contexts_are_refused(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    p = hsk.default_clearance_params()
    st = L.HskClearanceStats(n_far=77)
    out = np.full(8, 9, np.uint32)
    pts = np.zeros((2, 3), f32)
    assert lib.hsk_build_clearance(None, C.byref(p), C.byref(st)) == -1 and st.n_far == 77
    assert lib.hsk_download_clearance(None, C.byref(p), None, out.ctypes.data) == -1
    assert lib.hsk_clearance_at(None, C.byref(p), pts.ctypes.data, 2, out.ctypes.data) == -1
    assert lib.hsk_clearance_floor(None, C.byref(p), 1, 0, 1, out.ctypes.data, C.byref(st)) == -1 and st.n_far == 77
    assert lib.hsk_release_clearance(None) == -1 and (out == 9).all()
    for name in ("default_clearance_params", "build_clearance", "download_clearance", "clearance_at", "clearance_floor", "release_clearance"):
        assert callable(getattr(hsk.KinfuTracker, name))
