"""Oriented plane detection on the GPU, BIT FOR BIT against the numpy restatement of the rule (tests/planes_twin.py):
hsk_score_planes at the sizes where the score kernel takes another path; hsk_detect_planes_oriented, every field and every label,
on the analytic scene and on the thin wall; hsk_detect_planes_volume against the cloud form on the context's own cloud, what it
leaves untouched, and the rule's bar on the scene; the errors."""
import ctypes as C

import numpy as np
import pytest

import planes_twin as PT
from kit import same_bits, state_of, volume_ctx
from level_cases import jittered
from planes_cases import COS_MIN, DIST_M, assert_scene_bar, odd_cloud, scene_cloud, score_planes_for_tests, twin_scene, twin_wall

pytestmark = pytest.mark.gpu
f32 = np.float32


def ctx(hsk, **over):
    return volume_ctx(hsk, PT.SCENE_DIMS, PT.SCENE_SIZE, **over)


@pytest.fixture(scope="module")
def trk(hsk):
    """the scene's volume on the device; the cloud calls do not read it"""
    t = ctx(hsk)
    t.upload_tsdf(scene_cloud()[0])
    yield t
    t.close()


def assert_same_result(got, ref, what):
    (rec, labels), (ref_rec, ref_labels) = got, ref
    assert rec.dtype == ref_rec.dtype and len(rec) == len(ref_rec), (what, rec, ref_rec)
    for name in ("n_inliers", "pad", "sum_abs"):
        assert np.array_equal(rec[name], ref_rec[name]), (what, name, rec[name], ref_rec[name])
    assert same_bits(np.ascontiguousarray(rec["abcd"]), np.ascontiguousarray(ref_rec["abcd"])), (what, rec["abcd"], ref_rec["abcd"])
    assert labels.dtype == np.int32 and np.array_equal(labels, ref_labels), (what, int((labels != ref_labels).sum()))


# ---- 6. hsk_score_planes against the twin ---------------------------------------------------------------------------------
def test_score_planes_matches_the_twin(hsk, trk):
    """n in {0, 1, 63, 64, 65, 257, the whole cloud} x 1, 3 and 513 planes, with and without a label mask: a wave's tail, one
    point more than a wave, more than a block's row of 256, several tiles; one lane's hypothesis, a part of a wave's 64, more
    than eight rounds of 64 with a tail of one; NaN and infinite planes; the odd points among the first 64"""
    ps, ns = odd_cloud()
    n_all = len(ps)
    assert n_all > 4 * 1024 and n_all % 1024 != 0 and n_all % 256 != 0           # several tiles, the last one partial in its rows
    planes = score_planes_for_tests(513)
    mask = np.full(n_all, -1, np.int32)
    mask[::7], mask[3::50] = 2, 0
    ok = PT.valid(ps, ns)
    inl = np.concatenate([PT.inliers(planes[j:j + 64], ps, ns, ok, DIST_M, COS_MIN)[0] for j in range(0, len(planes), 64)])
    assert inl.shape == (513, n_all) and (inl.sum(axis=1) > 1000).sum() >= 6 and (inl.sum(axis=1) == 0).sum() >= 2
    assert np.array_equal(inl.sum(axis=1).astype(np.uint32), PT.score(ps, ns, planes, DIST_M, COS_MIN))
    before = state_of(trk, True)
    for n in (0, 1, 63, 64, 65, 257, n_all):
        for m in (1, 3, 513):
            pl = planes[:m] if m > 1 else planes[4:5]
            rows = inl[:m] if m > 1 else inl[4:5]
            got = trk.score_planes(ps[:n], ns[:n], pl, DIST_M, COS_MIN)
            ref = rows[:, :n].sum(axis=1).astype(np.uint32)
            assert got.dtype == np.uint32 and np.array_equal(got, ref), f"n = {n}, planes = {m}: {got[got != ref][:3]} != {ref[got != ref][:3]}"
            got = trk.score_planes(ps[:n], ns[:n], pl, DIST_M, COS_MIN, labels=mask[:n])
            ref = (rows[:, :n] & (mask[None, :n] < 0)).sum(axis=1).astype(np.uint32)
            assert np.array_equal(got, ref), f"n = {n}, planes = {m}, masked: {got[got != ref][:3]} != {ref[got != ref][:3]}"
    assert len(trk.score_planes(ps, ns, planes[:0])) == 0
    # other thresholds: everything that faces the plane's way within a metre; nothing
    for dist_m, cos_min in ((1.0, -1.0), (0.001, 1.0)):
        assert np.array_equal(trk.score_planes(ps, ns, planes[:9], dist_m, cos_min), PT.score(ps, ns, planes[:9], dist_m, cos_min))
    for a, b in zip(before, state_of(trk, True)):
        assert same_bits(a, b), "hsk_score_planes moved something"


# ---- 7. hsk_detect_planes_oriented against the twin --------------------------------------------------------------------------
def test_detect_planes_cloud_matches_the_twin_on_the_scene(hsk, trk):
    """(a), every field and every label; then the parameters' corners: one hypothesis per round, one plane, no refit"""
    _, ps, ns = scene_cloud()
    ref_rec, ref_labels, ref_bad = twin_scene()
    before = state_of(trk, True)
    rec, labels, bad = trk.detect_planes_cloud(ps, ns)
    assert bad == ref_bad == 0
    assert_same_result((rec, labels), (ref_rec, ref_labels), "the scene")
    assert_scene_bar(rec, "device, cloud form")
    for over in (dict(n_hypotheses=1), dict(max_planes=1), dict(refits=0), dict(n_hypotheses=65, refits=1, seed=12345, min_fraction=0.1),
                 dict(dist_m=0.05, cos_min=0.5, max_planes=3, refits=8)):
        ref = PT.detect(ps, ns, **over)
        got = trk.detect_planes_cloud(ps, ns, **over)
        print(f"{over}: {len(got[0])} planes, {got[0]['n_inliers']}")
        assert_same_result(got[:2], ref[:2], over)
    assert len(trk.detect_planes_cloud(ps, ns, max_planes=1)[0]) == 1
    for a, b in zip(before, state_of(trk, True)):
        assert same_bits(a, b), "hsk_detect_planes_oriented moved something"


def test_detect_planes_cloud_with_odd_points_and_small_clouds(hsk, trk):
    ps, ns = odd_cloud()
    ref = PT.detect(ps, ns)
    got = trk.detect_planes_cloud(ps, ns)
    assert got[2] == ref[2] == 11 and len(got[0]) == 6
    assert_same_result(got[:2], ref[:2], "the odd cloud")
    assert (got[1][~PT.valid(ps, ns)] == -1).all()                 # an invalid point keeps label -1
    # only NaN normals: no valid point, no plane
    rec, labels, bad = trk.detect_planes_cloud(ps, np.full_like(ns, np.nan))
    assert len(rec) == 0 and bad == len(ps) and (labels == -1).all()
    # n < 3: the least count is 3
    _, good_ps, good_ns = scene_cloud()
    for n in (0, 1, 2):
        rec, labels, bad = trk.detect_planes_cloud(good_ps[:n], good_ns[:n], min_fraction=0.0)
        assert len(rec) == 0 and bad == 0 and len(labels) == n and (labels == -1).all()
        assert len(PT.detect(good_ps[:n], good_ns[:n], min_fraction=0.0)[0]) == 0
    # three points of one face, min_fraction 0: spread over the face they are one plane of three; three neighbours in a voxel row
    # are collinear, the refit turns the plane about them, the support is lost and the labels are taken back
    face0 = np.flatnonzero(twin_scene()[1] == 0)
    for pick, n_planes in ((face0[[0, len(face0) // 2, -1]], 1), (face0[:3], 0)):
        ref = PT.detect(good_ps[pick], good_ns[pick], min_fraction=0.0)
        got = trk.detect_planes_cloud(good_ps[pick], good_ns[pick], min_fraction=0.0)
        assert len(ref[0]) == n_planes and (n_planes == 0 or ref[0]["n_inliers"][0] == 3) and (ref[1] == n_planes - 1).all()
        assert_same_result(got[:2], ref[:2], "three points")
    assert len(PT.detect(good_ps[face0[:3]], good_ns[face0[:3]], min_fraction=0.0, refits=0)[0]) == 1      # (it is the refit that loses it)


def test_detect_planes_cloud_splits_the_thin_wall(hsk, trk):
    """(b), every field and every label: 67 500 points, the two faces of the wall as two planes of 22 500 points each"""
    ps, ns, face, ref_rec, ref_labels, _ = twin_wall()
    rec, labels, bad = trk.detect_planes_cloud(ps, ns)
    assert bad == 0
    assert_same_result((rec, labels), (ref_rec, ref_labels), "the thin wall")
    for k in range(3):
        assert len(np.unique(face[labels == k])) == 1 and (labels == k).sum() == 22500


def test_detect_planes_cloud_on_a_sweeps_second_trip(hsk, trk):
    """1024 x 256 + 65 points: the moments' and the labels' sweeps run the grid's cap of 1024 blocks, and block 0 takes a second
    trip of one partial wave; the score kernel's 257th tile is partial in its first row; every field and every label"""
    ps, ns = jittered(262209)
    over = dict(n_hypotheses=8, max_planes=2, refits=1)
    ref = PT.detect(ps, ns, **over)
    assert len(ref[0]) == 2 and ref[2] > 0, (ref[0], ref[2])          # (the case cannot go empty silently)
    got = trk.detect_planes_cloud(ps, ns, **over)
    assert got[2] == ref[2]
    assert_same_result(got[:2], ref[:2], "262209 points")


# ---- 8. hsk_detect_planes_volume ----------------------------------------------------------------------------------------------
def test_detect_planes_volume_is_the_cloud_form_on_the_contexts_own_cloud(hsk):
    """the uploaded 80 x 64 x 48 scene volume (non-cubic, three different cells): the labels are in extract_cloud_attrs' order; the
    result equals the cloud form's on that cloud and the twin's; it meets (a)'s bar; pose, TSDF and model maps stay; extract_cloud
    before and after returns the same bits"""
    vol, twin_ps, twin_ns = scene_cloud()
    t = ctx(hsk)
    try:
        t.upload_tsdf(vol)
        cloud_before, total_before = t.extract_cloud()
        before = state_of(t, True)
        rec, labels = t.detect_planes()
        for a, b in zip(before, state_of(t, True)):
            assert same_bits(a, b), "hsk_detect_planes_volume moved something"
        cloud_after, total_after = t.extract_cloud()
        assert total_after == total_before == len(labels) and same_bits(cloud_after, cloud_before)
        xyz, nrm, _, total, _ = t.extract_cloud_attrs(rgb=False)
        assert total == len(xyz) == len(labels) == 14912 and same_bits(xyz, cloud_before)
        again = t.detect_planes()                                                  # behind other products: the same
        assert_same_result(again, (rec, labels), "a second call")
        assert_same_result((rec, labels), t.detect_planes_cloud(xyz, nrm)[:2], "volume form against cloud form")
        assert same_bits(xyz, twin_ps)
        assert_same_result((rec, labels), twin_scene()[:2], "volume form against the twin")
        assert_scene_bar(rec, "device, volume form")
        # other parameters go through
        got = t.detect_planes(max_planes=2, refits=0, n_hypotheses=100)
        assert_same_result(got, t.detect_planes_cloud(xyz, nrm, max_planes=2, refits=0, n_hypotheses=100)[:2], "two planes, no refit")
        # the two-call protocol
        lib = hsk._lib.load()
        n, k = C.c_size_t(), C.c_size_t()
        recs = (hsk._lib.HskPlaneRecord * 64)()
        lab = np.full(total, 9, np.int32)
        assert lib.hsk_detect_planes_volume(t.h, None, None, 0, None, None, 0, C.byref(n)) == 0 and n.value == total
        assert lib.hsk_detect_planes_volume(t.h, None, recs, 64, C.byref(k), lab.ctypes.data, total - 1, C.byref(n)) == -1 and n.value == total
        assert (lab == 9).all()
        assert lib.hsk_detect_planes_volume(t.h, None, recs, 11, C.byref(k), None, 0, C.byref(n)) == -1           # cap below max_planes (12)
        assert lib.hsk_detect_planes_volume(t.h, None, recs, 12, C.byref(k), None, 0, C.byref(n)) == 0 and k.value == 6       # no labels wanted
        assert lib.hsk_detect_planes_volume(t.h, None, recs, 64, None, None, 0, C.byref(n)) == -1
        assert lib.hsk_detect_planes_volume(t.h, None, recs, 64, C.byref(k), None, 0, None) == -1
        # an empty volume: no points, no planes
        t.reset()
        rec0, lab0 = t.detect_planes()
        assert len(rec0) == 0 and len(lab0) == 0
    finally:
        t.close()


# ---- 9. the errors ----------------------------------------------------------------------------------------------------------------
def test_argument_and_state_errors(hsk, trk):
    lib = hsk._lib.load()
    _, ps, ns = scene_cloud()
    ps, ns = np.ascontiguousarray(ps[:256]), np.ascontiguousarray(ns[:256])
    recs = (hsk._lib.HskPlaneRecord * 64)()
    k, n = C.c_size_t(), C.c_size_t()
    cnt = np.full(2, 0xFFFFFFFF, np.uint32)
    eq = np.array([[0, 0, 1, -0.4], [1, 0, 0, -0.3]], f32)

    def detect(h=trk.h, p=ps.ctypes.data, q=ns.ctypes.data, m=256, params=None, r=recs, cap=64, out=C.byref(k)):
        return lib.hsk_detect_planes_oriented(h, p, q, m, params, r, cap, out, None, None)

    def score(h=trk.h, p=ps.ctypes.data, q=ns.ctypes.data, m=256, e=eq.ctypes.data, ne=2, dist=0.02, cos=0.5, out=cnt.ctypes.data):
        return lib.hsk_score_planes(h, p, q, None, m, e, ne, dist, cos, out)

    assert detect() == 0 and score() == 0
    assert detect(p=None) == -1 and detect(q=None) == -1 and detect(r=None) == -1 and detect(out=None) == -1
    assert detect(m=(1 << 24) + 1) == -1 and "2^24" in lib.hsk_last_error(trk.h).decode()
    assert detect(cap=11) == -1 and detect(cap=12) == 0
    for name, bad in (("dist_m", 0.0), ("dist_m", 1.5), ("dist_m", float("nan")), ("cos_min", 1.5), ("cos_min", -1.5), ("cos_min", float("nan")),
                      ("min_fraction", float("nan")), ("min_fraction", -0.1), ("min_fraction", float("inf")), ("max_planes", 0), ("max_planes", 65),
                      ("n_hypotheses", 0), ("n_hypotheses", 4097), ("refits", -1), ("refits", 9)):
        p = hsk.KinfuTracker._plane_params({name: bad})
        assert detect(params=C.byref(p)) == -1 and "range" in lib.hsk_last_error(trk.h).decode(), (name, bad)
        assert lib.hsk_detect_planes_volume(trk.h, C.byref(p), recs, 64, C.byref(k), None, 0, C.byref(n)) == -1, (name, bad)
    p = hsk.KinfuTracker._plane_params(dict(dist_m=1.0, cos_min=-1.0, min_fraction=2.0, max_planes=64, n_hypotheses=4096, refits=8))
    assert detect(params=C.byref(p)) == 0 and k.value == 0               # the least count is above the cloud's size
    assert score(p=None) == -1 and score(q=None) == -1 and score(e=None) == -1 and score(out=None) == -1
    assert score(ne=4097) == -1 and score(m=(1 << 24) + 1) == -1
    assert score(dist=0.0) == -1 and score(dist=1.5) == -1 and score(cos=2.0) == -1 and score(dist=float("nan")) == -1
    assert (cnt != 0xFFFFFFFF).all() and cnt[0] > 0                 # (the refused calls wrote nothing; the first one did)
    cnt[:] = 0xFFFFFFFF
    assert score(m=0, p=None, q=None) == 0 and (cnt == 0).all() and score(ne=0, e=None, out=None) == 0
    assert detect(m=0, p=None, q=None) == 0 and k.value == 0
    with pytest.raises(hsk.KinfuError):
        trk.detect_planes_cloud(ps, ns, max_planes=65)
    with pytest.raises(ValueError, match="normals"):
        trk.detect_planes_cloud(ps, ns[:-1])
    # HSK_ERR_STATE: a frame in flight
    busy = hsk.KinfuTracker(n=64)
    try:
        busy.submit_frame(hsk.synth_depth(hsk.synth_pose(0)))
        assert detect(h=busy.h) == -3 and "in flight" in lib.hsk_last_error(busy.h).decode()
        assert score(h=busy.h) == -3
        assert lib.hsk_detect_planes_volume(busy.h, None, recs, 64, C.byref(k), None, 0, C.byref(n)) == -3
        busy.wait_frame()
        assert detect(h=busy.h) == 0 and score(h=busy.h) == 0
        assert lib.hsk_detect_planes_volume(busy.h, None, recs, 64, C.byref(k), None, 0, C.byref(n)) == 0 and n.value > 1000
    finally:
        busy.close()
    # ... the volume form on a context that stores part of its volume, and on the slabs of a group; the cloud forms read no volume
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        assert lib.hsk_detect_planes_volume(part.h, None, recs, 64, C.byref(k), None, 0, C.byref(n)) == -3 and "slab" in lib.hsk_last_error(part.h).decode()
        assert lib.hsk_detect_planes_volume(part.h, None, None, 0, None, None, 0, C.byref(n)) == -3
        assert detect(h=part.h) == 0 and score(h=part.h) == 0
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        for i in range(g.n_slabs()):
            assert lib.hsk_detect_planes_volume(g.slab(i).h, None, recs, 64, C.byref(k), None, 0, C.byref(n)) == -3
        assert g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))[1]
    finally:
        g.close()
