"""Cloud normals on the GPU: hsk_estimate_normals against the numpy restatement of the rule (tests/normals_twin.py) on every case of
tests/normals_cases.py -- normals, curvature, neighbour counts, classes and stats EQUAL to the bits, each call made twice; the
scratch growing and shrinking between calls; NULL optional outputs; the context left as it was, also with deferred weights and
between two frames of a scan; every error; and the chain it is for: a thin wall's faces kept apart by hsk_detect_planes_oriented,
an oblique plane imported in SURFEL mode from a cloud that had no normals."""
import ctypes as C

import numpy as np
import pytest

import kit
import normals_cases as NC
import normals_twin as NT
import splat_cases as SC
import splat_twin as ST

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
SIZE = (3.0, 3.0, 3.0)


def as_kwargs(p):
    return {k: (float(v) if k in ("radius_m", "line_rel") else int(v)) for k, v in p.items()}


@pytest.fixture(scope="module")
def trk(hsk):
    t = kit.volume_ctx(hsk, (32, 32, 32), SIZE)
    yield t
    t.close()


def device(t, c):
    return t.estimate_normals(c["xyz"], c["viewpoints"], **as_kwargs(c["params"]))


def assert_equal(got, ref, name):
    for what, a, b in zip(("normals", "curvature", "neighbours", "classes"), ref, got):
        assert kit.same_bits(a, b), f"{name}: {what} differ at {np.argwhere(np.asarray(a != b))[:5].tolist()}"
    assert got[4] == ref[4], f"{name}: {got[4]} != {ref[4]}"


GROUPS = {"counts": NC.count_cases, "boundary": NC.boundary_cases, "classes": NC.class_cases, "cells": NC.cell_cases,
          "orientation": NC.orientation_cases, "shapes": NC.shape_cases}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_estimate_normals_equals_the_twin(trk, group):
    for c in GROUPS[group]():
        ref = NC.twin(c)
        got = device(trk, c)
        assert got[0].dtype == f32 and got[2].dtype == np.uint32 and got[3].dtype == np.uint8
        assert_equal(got, ref, c["name"])
        assert_equal(device(trk, c), ref, c["name"] + ", again")    # (the scratch and the table are left fit for the next call)


def test_the_scratch_grows_and_is_reused(trk):
    """a large call, then a small one, then a larger one"""
    big, small, bigger = NC.case("6000", SC.random_cloud(6000, 3)[0], NT.params(0.25)), NC.count_cases()[5], NC.shape_cases()[0]
    for c in (big, small, bigger, small):
        assert_equal(device(trk, c), NC.twin(c), c["name"])


def test_null_optional_outputs_and_the_defaults(hsk, trk):
    lib, L = hsk._lib.load(), hsk._lib
    c = NC.shape_cases()[2]
    ref = NC.twin(c)
    p = hsk.default_normal_params(trk, **as_kwargs(c["params"]))
    nrm = np.zeros((len(c["xyz"]), 3), f32)
    assert lib.hsk_estimate_normals(trk.h, c["xyz"].ctypes.data, len(c["xyz"]), None, 0, C.byref(p), nrm.ctypes.data, None, None, None, None) == 0
    assert kit.same_bits(nrm, ref[0])
    # 0 in a field and no parameters at all are the defaults as values: 3 cells of 3 / 32 m are beyond the range, so 0.25 m
    d = hsk.default_normal_params(trk)
    assert d.radius_m == 0.25 and (d.min_neighbours, d.max_neighbours, f32(d.line_rel)) == (8, 4096, f32(1e-3))
    ref = NT.estimate(c["xyz"], None, NT.params(0.25))
    for params in (None, L.HskNormalParams()):
        nrm, st = np.zeros((len(c["xyz"]), 3), f32), L.HskNormalStats()
        assert lib.hsk_estimate_normals(trk.h, c["xyz"].ctypes.data, len(c["xyz"]), None, 0, None if params is None else C.byref(params),
                                        nrm.ctypes.data, None, None, None, C.byref(st)) == 0
        assert kit.same_bits(nrm, ref[0]) and {k: getattr(st, k) for k in NT.STATS} == ref[4]
    cells = hsk.KinfuTracker(n=64)
    try:
        assert f32(hsk.default_normal_params(cells).radius_m) == f32(3.0) * (f32(3.0) / f32(64.0))
    finally:
        cells.close()


def test_a_crowded_call_says_what_to_do(hsk, trk):
    c = NC.class_cases()[3]
    st = device(trk, c)[4]
    assert st["n_crowded"] == 300 and b"hsk_voxel_downsample" in trk.lib.hsk_last_error(trk.h)


def test_the_context_is_left_as_it_was(hsk, synth_frames):
    """on a volume that holds deferred weights (frames integrated, nothing downloaded in between), and between two frames of a scan"""
    c = NC.shape_cases()[3]
    t = hsk.KinfuTracker(n=64)
    try:
        for k in range(3):
            t.process_frame(synth_frames(k)[1])
        ref = NC.twin(c)
        got = device(t, c)                                      # before any download flushes the weights
        assert_equal(got, ref, "between two frames")
        _, ok = t.process_frame(synth_frames(3)[1])
        assert ok
        before = kit.state_of(t, True)
        assert_equal(device(t, c), ref, "after a download")
        kit.assert_state(t, before, "hsk_estimate_normals moved the pose, the volume or a model map")
        plain = hsk.KinfuTracker(n=64)
        try:
            for k in range(4):
                plain.process_frame(synth_frames(k)[1])
            for a, b in zip(kit.state_of(t, True), kit.state_of(plain, True)):
                assert kit.same_bits_nan(a, b), "the call between two frames changed the scan"
        finally:
            plain.close()
    finally:
        t.close()


def test_errors_leave_the_outputs_untouched_and_the_context_usable(hsk, trk, synth_frames):
    lib, L = hsk._lib.load(), hsk._lib
    c = NC.count_cases()[-1]
    xyz = c["xyz"]
    view = np.array([[0.0, 0.0, 0.0]], f32)
    good = device(trk, c)
    state = kit.state_of(trk, True)

    def rc(xyz_p=xyz.ctypes.data, n=len(xyz), view_p=view.ctypes.data, nv=1, normals=True):
        p = hsk.default_normal_params(trk, **as_kwargs(c["params"]))
        outs = [np.full((len(xyz), 3), 9, f32), np.full(len(xyz), 9, f32), np.full(len(xyz), 9, np.uint32), np.full(len(xyz), 9, np.uint8)]
        st = L.HskNormalStats(n_cells=77)
        r = lib.hsk_estimate_normals(trk.h, xyz_p, n, view_p, nv, C.byref(p), outs[0].ctypes.data if normals else None, outs[1].ctypes.data,
                                     outs[2].ctypes.data, outs[3].ctypes.data, C.byref(st))
        if r != 0:
            assert lib.hsk_last_error(trk.h) and all((o == 9).all() for o in outs) and st.n_cells == 77, "an error must leave a message and the outputs untouched"
        return r

    def rc_fields(**fields):
        # (default_normal_params refuses flags and pad as keywords: they are set on the structure)
        plain = {k: v for k, v in fields.items() if k not in ("flags", "pad")}
        p = hsk.default_normal_params(trk, **dict(as_kwargs(c["params"]), **plain))
        for k in ("flags", "pad"):
            if k in fields:
                setattr(p, k, fields[k])
        outs = [np.full((len(xyz), 3), 9, f32), np.full(len(xyz), 9, f32)]
        r = lib.hsk_estimate_normals(trk.h, xyz.ctypes.data, len(xyz), None, 0, C.byref(p), outs[0].ctypes.data, outs[1].ctypes.data, None, None, None)
        if r != 0:
            assert all((o == 9).all() for o in outs)
        return r

    assert rc() == 0
    nan, inf = float("nan"), float("inf")
    bad_fields = (dict(radius_m=0.0009), dict(radius_m=0.2501), dict(radius_m=nan), dict(radius_m=inf), dict(radius_m=-0.05), dict(min_neighbours=2),
                  dict(min_neighbours=9, max_neighbours=8), dict(max_neighbours=(1 << 20) + 1), dict(line_rel=-0.1), dict(line_rel=1.5), dict(line_rel=nan),
                  dict(line_rel=inf), dict(flags=1))
    for bad in bad_fields:
        assert rc_fields(**bad) == -1 and b"parameter" in lib.hsk_last_error(trk.h), bad
    assert rc_fields(radius_m=0.25, max_neighbours=1 << 20, line_rel=1.0) == 0
    assert rc(xyz_p=None) == -1 and b"null" in lib.hsk_last_error(trk.h)
    assert rc(normals=False) == -1 and b"null" in lib.hsk_last_error(trk.h)
    assert rc(view_p=None) == -1 and b"null" in lib.hsk_last_error(trk.h)
    assert rc(n=(1 << 24) + 1) == -1 and b"2^24" in lib.hsk_last_error(trk.h)
    many = np.zeros((257, 3), f32)
    assert rc(view_p=many.ctypes.data, nv=257) == -1 and b"256" in lib.hsk_last_error(trk.h)
    assert rc(view_p=many.ctypes.data, nv=256) == 0
    for v in (nan, inf, -inf):
        odd = np.array([[0, 0, 0], [0, v, 0]], f32)
        assert rc(view_p=odd.ctypes.data, nv=2) == -1 and b"finite" in lib.hsk_last_error(trk.h)
    assert lib.hsk_estimate_normals(None, xyz.ctypes.data, len(xyz), None, 0, None, good[0].ctypes.data, None, None, None, None) == -1
    # no points: HSK_OK and zero stats, whatever the pointers
    st = L.HskNormalStats(n_cells=77, n_pairs=5)
    out = np.full(3, 9, f32)
    assert lib.hsk_estimate_normals(trk.h, None, 0, None, 0, None, out.ctypes.data, None, None, None, C.byref(st)) == 0
    assert {k: getattr(st, k) for k in NT.STATS} == dict.fromkeys(NT.STATS, 0) and (out == 9).all()
    empty = trk.estimate_normals(np.zeros((0, 3), f32))
    assert empty[0].shape == (0, 3) and empty[4] == dict.fromkeys(NT.STATS, 0)
    with pytest.raises(hsk.KinfuError, match="parameter"):
        trk.estimate_normals(xyz, radius_m=0.5)
    with pytest.raises(TypeError, match="no field"):
        trk.estimate_normals(xyz, flags=1)
    kit.assert_state(trk, state, "an error must leave the context untouched")
    assert_equal(device(trk, c), good, "after the errors")
    # a frame in flight
    t = hsk.KinfuTracker(n=64)
    try:
        t.process_frame(synth_frames(0)[1])
        t.submit_frame(synth_frames(1)[1])
        with pytest.raises(hsk.KinfuError, match="in flight"):
            t.estimate_normals(xyz)
        _, ok = t.wait_frame()
        assert ok and t.estimate_normals(xyz, **as_kwargs(c["params"]))[4] == good[4]
    finally:
        t.close()
    # a context that stores part of its volume, and the slabs of a group
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        with pytest.raises(hsk.KinfuError, match="slab"):
            part.estimate_normals(xyz)
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(synth_frames(0)[1])
        for i in range(g.n_slabs()):
            with pytest.raises(hsk.KinfuError, match="slab"):
                g.slab(i).estimate_normals(xyz)
    finally:
        g.close()


def test_a_thin_walls_faces_stay_apart_in_the_oriented_detection(hsk, trk):
    pts, face = NC.thin_wall()
    nrm, _, _, cls, st = trk.estimate_normals(pts, NC.WALL_VIEWPOINTS, radius_m=0.02, min_neighbours=5)
    assert st["n_ok"] == 882
    recs, labels, bad = trk.detect_planes_cloud(pts.astype(f32), nrm)
    assert bad == 0 and len(recs) == 2 and [int(r["n_inliers"]) for r in recs] == [441, 441]
    a, b = recs[0]["abcd"][:3].astype(f64), recs[1]["abcd"][:3].astype(f64)
    assert a @ b < -0.999 and np.bincount(labels[face == 0], minlength=2).max() == 441


def test_an_oblique_plane_without_normals_imports_as_surfels(hsk):
    """estimate_normals -> splat_cloud(SURFEL) within 1.0 mm of the analytic depth (the bound tests/test_splat_host.py holds the true
    normals to); DISC on the same cloud errs by more than 10 mm (its derived error at this tilt and spacing is 23.1 mm)"""
    case = SC.oblique_cases()[0]
    cam = SC.CAMS[case["cam"]]
    t = kit.volume_ctx(hsk, (32, 32, 32), SIZE, width=cam["width"], height=cam["height"], fx=float(cam["fx"]), fy=float(cam["fy"]),
                       cx=float(cam["cx"]), cy=float(cam["cy"]))
    try:
        nrm, _, _, _, st = t.estimate_normals(case["xyz"], [[0.0, 0.0, 0.0]], radius_m=3.0 * SC.OBLIQUE_S)
        assert st["n_ok"] == len(case["xyz"])
        ref = SC.oblique_depth(case["cam"]) * 1000.0
        kw = {k: (int(v) if k == "mode" else float(v)) for k, v in case["params"].items()}
        img, sst = t.splat_cloud(case["xyz"], case["pose"], nrm, **kw)
        err = np.abs(img.astype(f64) - ref).max()
        disc, _ = t.splat_cloud(case["xyz"], case["pose"], None, **dict(kw, mode=ST.DISC))
        err_disc = np.abs(disc.astype(f64) - ref).max()
        print(f"largest depth error: surfel with estimated normals {err:.3f} mm, disc {err_disc:.3f} mm")
        assert sst["n_pixels"] == img.size and sst["n_backfacing"] == 0 and err <= 1.0 and err_disc > 10.0
    finally:
        t.close()
