"""Oriented plane detection without a GPU: the kernels' work on one point (housescan_amd/csrc/hsk_plane_point.h, compiled for the
host) against the numpy twin (tests/planes_twin.py), bit for bit; the host refit hsk_plane_refit against the twin, bit for bit;
the C layout of the new structs and their Python mirror; the argument errors that need no device; the two properties DESIGN.md
8h claims for the rule, shown on the twin -- the analytic scene's six faces, and the two faces of a thin wall that the unoriented
host detector mixes; write_room_dir with planes found elsewhere."""
import ctypes as C
import os

import numpy as np
import pytest

import align_twin as AT
import kit
import planes_twin as PT
from kit import same_bits
from planes_cases import COS_MIN, DIST_M, assert_scene_bar, odd_cloud, scene_cloud, score_planes_for_tests, twin_scene, twin_wall

f32 = np.float32


# ---- 1. the kernels' point function, compiled for the host ----------------------------------------------------------------
def test_the_kernels_point_function_equals_the_twin_on_the_host(tmp_path):
    """the text every lane of the plane kernels runs, built for the host with the address and undefined-behaviour sanitizers
    (their runtime linked into the program): per plane the inlier count, sum_abs and the ten moments against the twin, zero
    differences; NaN, infinite, far-away points and |x| either side of 64"""
    exe = kit.build_harness("plane_point", tmp_path)
    ps, ns = odd_cloud()
    n = len(ps)
    planes = score_planes_for_tests(40)
    labels = np.full(n, -1, np.int32)
    labels[::7] = 2                                 # a seventh of the cloud is taken
    ok = PT.valid(ps, ns)
    assert (~ok).sum() == 11 and ok[25] and not ok[27] and ok[29] and not ok[31] and ok[33] and ok[35] and ok[23] and ok[37] and ok[39]
    open_ = ok & (labels < 0)
    inl, a_s = PT.inliers(planes, ps, ns, open_, DIST_M, COS_MIN)
    want = [[int(ok.sum())]]
    for j in range(len(planes)):
        want.append([int(inl[j].sum()), int(PT.abs_q(a_s[j][inl[j]]).sum())] + PT.moments(ps[inl[j]])[1:])
    assert want[1][0] > 2000 and sum(w[0] == 0 for w in want[1:]) >= 2 and sum(w[0] > 100 for w in want[1:]) >= 10
    with np.errstate(all="ignore"):
        seeds = np.concatenate([ns[:8], -PT.dot3(*(ns[:8, i] for i in range(3)), *(ps[:8, i] for i in range(3)))[:, None]], axis=1).astype(f32)
    path = tmp_path / "in.bin"
    with open(path, "wb") as f:
        for part in (np.uint32(n), np.uint32(len(planes)), f32(DIST_M), f32(COS_MIN), planes, np.ascontiguousarray(ps.T), np.ascontiguousarray(ns.T), labels):
            f.write(np.ascontiguousarray(part).tobytes())
    out = kit.run_harness(exe, path, text=True)
    lines = [[int(v) for v in line.split()] for line in out.strip().splitlines()]
    got, got_seeds = lines[:1 + len(planes)], np.array(lines[1 + len(planes):], np.uint32)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:3]
    assert np.array_equal(got_seeds, seeds.view(np.uint32))


# ---- 2. hsk_plane_refit ----------------------------------------------------------------------------------------------------
def refit_cases():
    _, ps, ns = scene_cloud()
    ok = PT.valid(ps, ns)
    cases = []
    for r in twin_scene()[0][:3]:                   # real moments: a face's inliers, refitted from a plane 2 degrees off
        inl = PT.inliers(r["abcd"][None], ps, ns, ok, DIST_M, COS_MIN)[0][0]
        tilted = (r["abcd"].astype(np.float64) + [0.02, -0.03, 0.025, 0.004]).astype(f32)
        cases.append((PT.moments(ps[inl]), r["abcd"]))
        cases.append((PT.moments(ps[inl]), tilted))
        cases.append((PT.moments(ps[inl]), -r["abcd"]))                              # the sign flip: the previous normal decides
    rng = np.random.default_rng(4)
    big = rng.uniform(-64, 64, (3000, 3)).astype(f32)
    big[:, 1] = (0.3 * big[:, 0] - 0.2 * big[:, 2] + rng.normal(0, 0.01, len(big))).astype(f32)
    m = PT.moments(big)
    scale = (2 ** 24) // m[0]                       # the same distribution 2^24 points strong: second moments near 2^60
    huge = [v * scale for v in m]
    assert max(abs(v) for v in huge) > 2 ** 58 and huge[0] <= 2 ** 24
    cases.append((huge, (0.0, 1.0, 0.0, 0.0)))
    cases.append((huge, (0.0, -1.0, 0.0, 0.0)))
    cases.append(([2 ** 24] + [2 ** 42 - 1] * 3 + [2 ** 60 - 1, 2 ** 59, -2 ** 59, 2 ** 60 - 3, 2 ** 58 + 1, 2 ** 60 - 5], (0.6, 0.0, 0.8, 1.0)))
    line = np.outer(np.arange(50), [0.01, 0.02, -0.015]).astype(f32) + f32(0.5)      # a collinear set: two eigenvalues ~ 0
    cases.append((PT.moments(line), (1.0, 0.0, 0.0, -0.5)))
    cases.append((PT.moments(np.tile(f32([0.25, 0.5, 0.75]), (10, 1))), (0.0, 0.0, 1.0, -0.75)))          # one point ten times: C = 0
    cases.append((PT.moments(line[:2]), (1.0, 0.0, 0.0, -0.5)))                      # fewer than three
    cases.append(([0] * 10, (1.0, 0.0, 0.0, -0.5)))
    return cases


def test_plane_refit_equals_the_twin_bit_for_bit(hsk):
    flips = fits = 0
    for sums, prev in refit_cases():
        ref, ref_ok = PT.refit(sums, prev)
        got, ok = hsk.plane_refit(sums, prev)
        assert ok == ref_ok and same_bits(got, ref), (sums, prev, got, ref)
        if ok:
            fits += 1
            n = got[:3].astype(np.float64)
            assert abs(np.linalg.norm(n) - 1.0) < 1e-6 and n @ np.asarray(prev, np.float64)[:3] >= 0.0
            other, _ = hsk.plane_refit(sums, -np.asarray(prev, f32))
            flips += same_bits(other, -got) or same_bits(other[:3], -got[:3])
        else:
            assert same_bits(got, np.asarray(prev, f32))
    assert fits >= 12 and flips >= 10
    # a face's own moments give the face back: within a tenth of a millimetre and a hundredth of a degree of the twin's plane
    (sums, prev), r = refit_cases()[1], twin_scene()[0][0]
    got, ok = hsk.plane_refit(sums, prev)
    assert ok and np.degrees(np.arccos(min(1.0, float(got[:3].astype(np.float64) @ r["abcd"][:3].astype(np.float64))))) < 0.05
    assert abs(float(got[3]) - float(r["abcd"][3])) < 1e-3
    lib = hsk._lib.load()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    s, a, o, okc = np.zeros(10, np.int64), np.zeros(4, f32), np.zeros(4, f32), C.c_int()
    assert lib.hsk_plane_refit(None, a.ctypes.data_as(fp), o.ctypes.data_as(fp), C.byref(okc)) == -1
    assert lib.hsk_plane_refit(s.ctypes.data_as(ip), None, o.ctypes.data_as(fp), C.byref(okc)) == -1
    assert lib.hsk_plane_refit(s.ctypes.data_as(ip), a.ctypes.data_as(fp), None, C.byref(okc)) == -1
    assert lib.hsk_plane_refit(s.ctypes.data_as(ip), a.ctypes.data_as(fp), o.ctypes.data_as(fp), None) == -1
    for bad in ([-1] + [0] * 9, [2 ** 24 + 1] + [0] * 9, [5, 2 ** 62 + 1] + [0] * 8, [5, 0, 0, 0, -2 ** 62 - 1] + [0] * 5):
        with pytest.raises(hsk.KinfuError):
            hsk.plane_refit(bad, (1.0, 0.0, 0.0, 0.0))


# ---- 3. header, C layout, Python mirror, the errors that need no device -------------------------------------------------------
def test_plane_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, R = _lib.HskPlaneParams, _lib.HskPlaneRecord
    assert C.sizeof(P) == 32 and C.sizeof(R) == 32 and hsk.kinfu.PLANE_DTYPE.itemsize == 32 and PT.RECORD_DTYPE == hsk.kinfu.PLANE_DTYPE


def test_default_plane_params(hsk):
    from housescan_amd import _lib, products
    import inspect
    p = _lib.HskPlaneParams()
    _lib.load().hsk_default_plane_params(C.byref(p))
    host = inspect.signature(products.detect_planes).parameters
    assert p.dist_m == f32(host["dist_thresh"].default) and p.min_fraction == f32(host["min_fraction"].default)
    assert (p.max_planes, p.n_hypotheses, p.refits, p.seed) == (12, 512, 2, 0x9E3779B97F4A7C15)
    assert p.cos_min == f32(np.cos(np.radians(30.0)))
    for name, val in PT.DEFAULTS.items():
        assert getattr(p, name) == (f32(val) if isinstance(val, float) else val), name
    _lib.load().hsk_default_plane_params(None)


def test_null_contexts_are_refused(hsk):
    lib = hsk._lib.load()
    rec = (hsk._lib.HskPlaneRecord * 64)()
    n = C.c_size_t()
    pts = np.zeros((4, 3), f32)
    cnt = np.zeros(1, np.uint32)
    assert lib.hsk_detect_planes_oriented(None, pts.ctypes.data, pts.ctypes.data, 4, None, rec, 64, C.byref(n), None, None) == -1
    assert lib.hsk_detect_planes_volume(None, None, rec, 64, C.byref(n), None, 0, C.byref(n)) == -1
    assert lib.hsk_score_planes(None, pts.ctypes.data, pts.ctypes.data, None, 4, np.zeros(4, f32).ctypes.data, 1, 0.02, 0.5, cnt.ctypes.data) == -1
    for name in ("detect_planes", "detect_planes_cloud", "score_planes"):
        assert callable(getattr(hsk.KinfuTracker, name))
    with pytest.raises(TypeError, match="unknown plane parameter"):
        hsk.KinfuTracker._plane_params({"iterations": 3})
    assert hsk.KinfuTracker._plane_params({"refits": 0, "seed": 7}).refits == 0


# ---- 4. the rule's properties, on the twin -----------------------------------------------------------------------------------
def test_the_twin_finds_the_rooms_six_faces_with_inward_normals():
    """(a): align_twin's scene at 80 x 64 x 48 over 3 m through np_twin.extract_cloud and mesh_twin.normal_at"""
    _, ps, ns = scene_cloud()
    assert len(ps) == 14912
    rec, labels, bad = twin_scene()
    assert bad == 0 and labels.max() == 5
    assert_scene_bar(rec, "twin")
    lo, hi = np.array(AT.ROOM)
    centre = 0.5 * (lo + hi)
    for r in rec:                                   # inward: the room's centre lies on the positive side of every plane
        assert float(r["abcd"][:3].astype(np.float64) @ centre + r["abcd"][3]) > 0.5
    assert [int((labels == k).sum()) for k in range(6)] == [int(r["n_inliers"]) for r in rec]
    assert (np.diff(rec["n_inliers"].astype(np.int64)) <= 0).all()


def test_the_twin_splits_a_thin_wall_into_its_faces_and_the_host_detector_does_not(hsk):
    """(b): two 150 x 150 faces 3 cm apart with opposite normals, plus a floor.  The oriented rule returns each face as a plane
    holding exactly its points; the unoriented host detector (hsk_detect_planes) on the same cloud puts points of both faces
    into one plane"""
    from housescan_amd import products
    ps, ns, face, rec, labels, bad = twin_wall()
    assert bad == 0 and len(rec) == 3 and (rec["n_inliers"] == 22500).all()
    of_face = {}
    for k in range(3):
        faces_in = np.unique(face[labels == k])
        assert len(faces_in) == 1
        of_face[int(faces_in[0])] = k
        assert np.array_equal(labels == k, face == faces_in[0])                      # exactly the face's points
    left, right = rec[of_face[0]]["abcd"], rec[of_face[1]]["abcd"]
    assert np.allclose(left, (-1.0, 0.0, 0.0, 1.0), atol=1e-4) and np.allclose(right, (1.0, 0.0, 0.0, -1.03), atol=1e-4)
    planes, host_labels = products.detect_planes(ps)
    mixed = [k for k in range(len(planes)) if (face[host_labels == k] == 0).any() and (face[host_labels == k] == 1).any()]
    for k in range(len(planes)):
        print(f"host plane {k}: {planes[k]} holds {np.bincount(face[host_labels == k], minlength=3)} points of the faces (left, right, floor)")
    assert mixed, "the host detector kept the wall's faces apart"


# ---- 5. write_room_dir with planes found elsewhere ---------------------------------------------------------------------------
def test_write_room_dir_takes_precomputed_planes_and_is_unchanged_without_them(tmp_path, hsk):
    from housescan_amd import products
    _, ps, ns = scene_cloud()
    rec, labels, _ = twin_scene()
    a, b, c = (str(tmp_path / d) for d in "abc")
    planes_a, n_a = products.write_room_dir(a, ps)
    planes_b, n_b = products.write_room_dir(b, ps, planes=None)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and n_a == n_b and same_bits(planes_a, planes_b)
    for name in os.listdir(a):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    planes_c, n_c = products.write_room_dir(c, ps, planes=(rec["abcd"], labels, ps))
    assert n_c == n_a and same_bits(planes_c, rec["abcd"])
    want = ["cloud_bin.pcd", "cloud_downsampled.pcd", "planes.txt"] + [f"cloud_plane_hull{k}.pcd" for k in range(6)]
    assert sorted(os.listdir(c)) == sorted(want)
    for name in ("cloud_bin.pcd", "cloud_downsampled.pcd"):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(c, name), "rb").read()
    txt = np.array([[float(v) for v in line.split()] for line in open(os.path.join(c, "planes.txt")).read().splitlines()], f32)
    assert same_bits(txt, np.ascontiguousarray(rec["abcd"]))
    for k, r in enumerate(rec):
        hull = products.plane_hull(ps, labels, k, r["abcd"])
        assert len(hull) >= 4
        raw = open(os.path.join(c, f"cloud_plane_hull{k}.pcd"), "rb").read()
        assert raw.endswith(hull.tobytes())
        assert np.abs(hull.astype(np.float64) @ r["abcd"][:3].astype(np.float64) + float(r["abcd"][3])).max() < 1e-5
    with pytest.raises(ValueError, match="nothing to act on"):
        products.write_room_dir(c, ps, planes=(rec["abcd"], labels, ps), max_planes=3)
    with pytest.raises(ValueError, match="labels"):
        products.write_room_dir(c, ps, planes=(rec["abcd"], labels[:-1], ps))
