"""Pose scoring and relocalisation without a GPU: the kernel's work on one point (housescan_amd/csrc/hsk_reloc_point.h, compiled
for the host) against the numpy twin (tests/reloc_twin.py), bit for bit; hsk_rank_scores and hsk_pose_lattice against the
twin; the property DESIGN.md 8g claims for the rule, shown on the twins; the C layout of the new structs and their Python
mirror; the argument errors that need no device."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import kit
import reloc_twin as RT
from align_cases import TAU
from kit import blocked, same_bits
from reloc_cases import HALF_CELL_M, ROOM_SIZE, ROOM_TAU, displaced_pair, room_volume, score_cases, thick_wall_volume

f32 = np.float32

CAM_L2 = (80, 60, 262.5 / 4, 262.5 / 4, 159.5 / 4, 119.5 / 4)     # level 2 of the 320 x 240 camera of the GPU tests


# ---- 1. the kernel's work on one point, compiled for the host ----------------------------------------------------------
def test_the_kernels_point_function_equals_the_twin_on_the_host(tmp_path):
    """the text every lane of k_reloc_score runs, built for the host with the address and undefined-behaviour sanitizers (their
    runtime linked into the program): six counts and sum_abs per pose against the twin, zero differences; NaN, infinite and
    far-away points gather inside the volume like any other"""
    exe = kit.build_harness("reloc_point", tmp_path)
    vol = thick_wall_volume()
    ps, cases = score_cases()
    poses = np.stack(list(cases.values()))
    ref = RT.score(vol, AT.DST_SIZE, ps, poses)
    for name, r in zip(cases, ref):
        print(f"{name}: {r}")
    assert int(ref["n_skipped"][0]) == 2 and (ref["n_skipped"] == 2).all()
    for c in RT.CLASSES:
        assert (ref[c] > 0).any(), f"no case has a point in {c}"
    assert (np.array([int(sum(r[c] for c in RT.CLASSES)) for r in ref]) == len(ps)).all()           # exactly one class per point
    assert ref["n_near"][0] > 0.9 * len(ps) and ref["n_outside"][2] == len(ps) - 2 and ref["n_free"][3] > 100 and ref["n_behind"][4] > 100
    path = tmp_path / "in.bin"
    with open(path, "wb") as f:
        for part in (np.array(AT.DST_DIMS, np.int32), np.array(AT.DST_SIZE, f32), np.uint32(len(poses)), np.uint32(len(ps)), poses, blocked(vol),
                     np.ascontiguousarray(ps.T, f32)):
            f.write(np.ascontiguousarray(part).tobytes())
    out = kit.run_harness(exe, path, text=True)
    got = np.array([[int(v) for v in line.split()] for line in out.strip().splitlines()], np.int64)
    want = np.array([[int(r[c]) for c in RT.CLASSES] + [int(r["sum_abs"])] for r in ref], np.int64)
    assert np.array_equal(got, want), (got, want)


# ---- 2. hsk_rank_scores ------------------------------------------------------------------------------------------------------
def test_rank_scores_equals_the_twin_ties_included(hsk):
    rng = np.random.default_rng(5)
    s = np.zeros(200, RT.SCORE_DTYPE)
    for c in RT.CLASSES:
        s[c] = rng.integers(0, 40, len(s))
    s["sum_abs"] = rng.integers(0, 5, len(s))                  # few values: equal keys with equal and with different sums
    s[17], s[91] = s[3], s[3]                                  # fully equal scores: the lower index first
    s["n_near"][150], s["n_free"][150], s["n_behind"][150] = 0, 4000000000, 4000000000      # a key below -2^32
    ref = RT.rank(s)
    got = hsk.rank_scores(s)
    assert got.dtype == np.uint32 and np.array_equal(got, ref)
    key = s["n_near"].astype(np.int64) - s["n_free"].astype(np.int64) - s["n_behind"].astype(np.int64)
    k, a = key[got], s["sum_abs"][got].astype(np.int64)
    assert (np.diff(k) <= 0).all() and got[-1] == 150
    same_key = np.diff(k) == 0
    assert same_key.sum() > 20 and (np.diff(a)[same_key] >= 0).all()
    same_all = same_key & (np.diff(a) == 0)
    assert same_all.sum() > 5 and (np.diff(got.astype(np.int64))[same_all] > 0).all()
    where = {int(i): n for n, i in enumerate(got)}
    assert where[3] + 1 == where[17] and where[17] + 1 == where[91]
    assert len(hsk.rank_scores(s[:0])) == 0
    assert hsk._lib.load().hsk_rank_scores(None, 3, None) == -1


# ---- 3. hsk_pose_lattice -------------------------------------------------------------------------------------------------------
def test_pose_lattice(hsk):
    lib = hsk._lib.load()
    last, _ = displaced_pair(0)
    step_rad = float(np.radians(20.0))
    L = hsk.pose_lattice(last, 0.2, 3, step_rad, 2)
    assert L.shape == (8575, 4, 4) and L.dtype == f32
    ref = RT.lattice(last, 0.2, 3, step_rad, 2)
    assert np.abs(L.astype(np.float64) - ref.astype(np.float64)).max() <= 1e-6
    assert same_bits(L[8575 // 2], last)                                          # all offsets 0: the centre, bit for bit
    inv = np.empty(16, f32)
    fp = C.POINTER(C.c_float)
    for m in L:
        assert lib.hsk_invert_rigid(np.ascontiguousarray(m).ctypes.data_as(fp), inv.ctypes.data_as(fp)) == 0
    # the order: b fastest, then a, k, j, and i slowest -- each step of an index moves what it should, in the camera's frame
    rel = np.linalg.inv(last.astype(np.float64)) @ L[1].astype(np.float64)       # i = j = k = -3, a = -2, b = -1
    assert np.allclose(rel, RT.shift(-0.6, -0.6, -0.6) @ RT.rot_y(-2 * step_rad) @ RT.rot_x(-1 * step_rad), atol=1e-6)
    rel = np.linalg.inv(last.astype(np.float64)) @ L[5 * 5 * 7 * 7 * 4 + 5 * 5 * 7 * 3 + 5 * 5 * 6 + 5 * 2 + 4].astype(np.float64)
    assert np.allclose(rel, RT.shift(0.2, 0.0, 0.6) @ RT.rot_x(2 * step_rad), atol=1e-6)  # i = +1, j = 0, k = +3, a = 0, b = +2
    one = hsk.pose_lattice(last, 0.2, 0, step_rad, 0)
    assert one.shape == (1, 4, 4) and same_bits(one[0], last)
    # the two-call protocol, the capacity and the cap of 65536 poses
    n = C.c_size_t(0)
    c = np.ascontiguousarray(last).reshape(16)
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, 1, step_rad, 1, None, 0, C.byref(n)) == 0 and n.value == 27 * 9
    buf = np.zeros((27 * 9, 16), f32)
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, 1, step_rad, 1, buf.ctypes.data, 27 * 9 - 1, C.byref(n)) == -1 and not buf.any()
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, 1, step_rad, 1, buf.ctypes.data, 27 * 9, C.byref(n)) == 0 and n.value == 27 * 9
    assert same_bits(buf.reshape(-1, 4, 4), hsk.pose_lattice(last, 0.2, 1, step_rad, 1))
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, 3, step_rad, 6, None, 0, C.byref(n)) == 0 and n.value == 343 * 169    # 57967
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, 3, step_rad, 7, None, 0, C.byref(n)) == -1                             # 77175
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, 1000, step_rad, 1000, None, 0, C.byref(n)) == -1
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, -1, step_rad, 0, None, 0, C.byref(n)) == -1
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), float("nan"), 1, step_rad, 0, None, 0, C.byref(n)) == -1
    assert lib.hsk_pose_lattice(None, 0.2, 1, step_rad, 0, None, 0, C.byref(n)) == -1
    assert lib.hsk_pose_lattice(c.ctypes.data_as(fp), 0.2, 1, step_rad, 0, None, 0, None) == -1
    with pytest.raises(hsk.KinfuError, match="65536"):
        hsk.pose_lattice(last, 0.2, 3, step_rad, 7)


# ---- 4. the rule's property, on the twins ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_a_displaced_camera_is_found_by_the_candidates_not_by_the_alignment_alone(case):
    """the camera 0.61 m / 35 degrees (0.62 m / 38 degrees) from the last pose, an 80 x 60 frame traced analytically: the
    alignment from the last pose alone does not end converged within half a cell; the twin's relocalisation over a lattice
    around the last pose ends FOUND within it.  The lattice is +-0.4 m in steps of 0.4 m times yaw and pitch +-40 degrees in
    steps of 20: 675 poses (the issue's 8575-pose lattice, 0.2 m, ends 0.54 / 0.18 mm from the truth as well but takes 25 s
    here; 0.3 m with 20 degrees to either side, 1125 poses, does NOT find the first camera: its yaw of 33 degrees is 13 from
    the nearest candidate)"""
    vol = room_volume()
    last, truth = displaced_pair(case)
    ps, ns = RT.trace(truth, *CAM_L2)
    assert not np.isnan(ps).any() and np.allclose(np.linalg.norm(ns.astype(np.float64), axis=1), 1.0, atol=1e-6)
    alone, st = AT.align(vol, ROOM_SIZE, ROOM_TAU, ps, ns, last)
    err_alone = AT.point_error(alone, truth, ps)
    print(f"case {case}: from the last pose alone: {AT.STATUS[st['status']]}, {err_alone * 1e3:.1f} mm from the truth "
          f"(the start: {AT.point_error(last, truth, ps) * 1e3:.0f} mm)")
    assert not (st["status"] == AT.CONVERGED and err_alone <= HALF_CELL_M)
    L = RT.lattice(last, 0.4, 1, np.radians(20.0), 2)
    assert len(L) == 675
    M, rs = RT.relocalize(vol, ROOM_SIZE, ROOM_TAU, ps, ns, L)
    err = AT.point_error(M, truth, ps)
    for r, (_, a) in enumerate(rs["refined"]):
        print(f"case {case}: rank {r}: candidate {rs['candidate'][r]} score {rs['scores'][rs['candidate'][r]]} -> {AT.STATUS[a['status']]} after "
              f"{a['iterations']}, n_used {a['n_used'][-1]} of {rs['n_valid']}, rms {float(a['rms_m'][-1]) * 1e3:.2f} mm")
    print(f"case {case}: {RT.STATUS[rs['status']]}, {err * 1e3:.3f} mm from the truth")
    assert rs["status"] == RT.FOUND and rs["n_valid"] == 4800 and len(rs["refined"]) == 4
    assert err <= HALF_CELL_M


def test_relocalize_twin_statuses():
    vol = room_volume()
    last, truth = displaced_pair(0)
    ps, ns = RT.trace(truth, *CAM_L2)
    M, rs = RT.relocalize(vol, ROOM_SIZE, ROOM_TAU, ps, ns, np.zeros((0, 4, 4), f32))
    assert rs["status"] == RT.EMPTY and rs["best"] == -1 and same_bits(M, np.eye(4, dtype=f32))
    M, rs = RT.relocalize(vol, ROOM_SIZE, ROOM_TAU, np.full_like(ps, np.nan), ns, last[None])
    assert rs["status"] == RT.EMPTY and rs["n_valid"] == 0
    M, rs = RT.relocalize(vol, ROOM_SIZE, ROOM_TAU, ps, ns, last[None])          # the only candidate is 0.6 m off: not accepted
    assert rs["status"] == RT.NONE and rs["best"] == 0 and same_bits(M, last)
    M, rs = RT.relocalize(vol, ROOM_SIZE, ROOM_TAU, ps, ns, np.stack([last, truth.astype(f32)]), n_refine=1)
    assert rs["status"] == RT.FOUND and rs["best"] == 1 and rs["candidate"] == [1] and AT.point_error(M, truth, ps) <= HALF_CELL_M


# ---- 5. header, C layout, Python mirror -----------------------------------------------------------------------------------------
def test_reloc_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    S, P, R = _lib.HskPoseScore, _lib.HskRelocParams, _lib.HskRelocStats
    assert C.sizeof(S) == 32 and hsk.kinfu.SCORE_DTYPE.itemsize == 32 and RT.SCORE_DTYPE == hsk.kinfu.SCORE_DTYPE
    assert [n for n, _ in S._fields_] == list(RT.CLASSES) + ["sum_abs"]
    assert (_lib.HSK_RELOC_FOUND, _lib.HSK_RELOC_NONE, _lib.HSK_RELOC_EMPTY) == (RT.FOUND, RT.NONE, RT.EMPTY)


def test_default_reloc_params_without_a_context(hsk):
    from housescan_amd import _lib
    p = _lib.HskRelocParams()
    _lib.load().hsk_default_reloc_params(None, C.byref(p))
    assert (p.level, p.n_refine, p.accept_fraction, p.accept_rms_m) == (2, 4, 0.5, 0.0)     # (the rms bar comes from a context's tau)
    assert (p.align.max_iters, p.align.probes, p.align.max_points) == (30, 3, 262144)
    _lib.load().hsk_default_reloc_params(None, None)


# ---- 6. the argument errors that need no device ---------------------------------------------------------------------------------
def test_null_contexts_are_refused(hsk):
    lib = hsk._lib.load()
    assert lib.hsk_set_loss_policy(None, 1) == -1 and lib.hsk_get_loss_policy(None) == -1
    one = np.zeros(1, RT.SCORE_DTYPE)
    eye = np.eye(4, dtype=f32)
    assert lib.hsk_score_cloud(None, np.zeros(3, f32).ctypes.data, 1, eye.ctypes.data, 1, one.ctypes.data_as(C.POINTER(hsk._lib.HskPoseScore))) == -1
    out = np.zeros(16, f32)
    assert lib.hsk_relocalize(None, np.zeros((480, 640), np.uint16).ctypes.data, 640, 480, eye.ctypes.data, 1, None,
                              out.ctypes.data_as(C.POINTER(C.c_float)), None) == -1
    for name in ("set_loss_policy", "get_loss_policy", "score_cloud", "relocalize", "default_reloc_params"):
        assert callable(getattr(hsk.KinfuTracker, name))
    assert callable(hsk.pose_lattice) and callable(hsk.rank_scores)
    with pytest.raises(ValueError, match="poses"):
        hsk.KinfuTracker._poses(np.zeros(15, f32))
