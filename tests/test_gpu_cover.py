"""Scan coverage on the GPU: hsk_score_views, hsk_render_coverage and hsk_coverage_census against the numpy restatement of the rule
(tests/cover_twin.py), every count and every pixel EQUAL; a volume with deferred free-space weights; nothing else of the context
moves; the three calls in the middle of a pipelined scan; the errors; and the loop they are for -- the best-ranked view of a
half-scanned room, integrated, observes every voxel that decided one of its FRONTIER rays.  The volume of the twin comparisons is
test_cover_host's: align_twin's scene at 80 x 64 x 48 over 3 m (three different cells) with a never-observed patch in one wall."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import cover_twin as CT
import reloc_twin as RT
from align_cases import TAU
from cover_cases import AWAY, EYE, TOWARDS, carved_volume, probe_40x30
from kit import same_bits, state_of, volume_ctx

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZE64 = (3.0, 3.0, 3.0)


def ctx(hsk, dims, size=AT.DST_SIZE, **over):
    return volume_ctx(hsk, dims, size, **over)


@pytest.fixture(scope="module")
def carved(hsk):
    trk = ctx(hsk, AT.DST_DIMS)
    trk.upload_tsdf(carved_volume())
    yield trk
    trk.close()


def view_poses(n):
    """the views of the rule's classes and eye states (test_cover_host), then rigid neighbours of the view towards the patch up to
    25 degrees and 0.4 m away"""
    poses = [TOWARDS, AWAY, RT.look_at((-0.5, 1.5, 1.5), (1.5, 1.5, 1.5)), RT.look_at((40.0, 1.5, 1.5), (1.5, 1.5, 1.5)),
             RT.look_at((0.1, 1.5, 1.5), (1.5, 1.5, 1.5)), RT.look_at((0.26, 1.5, 1.5), (1.5, 1.5, 1.5))]
    rng = np.random.default_rng(17)
    while len(poses) < n:
        poses.append(AT.rigid(rng.uniform(-25, 25), rng.uniform(-400, 400, 3), axis=rng.normal(size=3), centre=EYE) @ TOWARDS)
    return np.stack(poses[:n]).astype(f32)


def as_kwargs(pr):
    return {k: (int(v) if k in ("width", "height") else float(v)) for k, v in pr.items()}


def probe_of(p):
    """an HskProbe as the twin's dict"""
    return CT.probe(p.width, p.height, p.fx, p.fy, p.cx, p.cy, p.near_m, p.far_m, p.step_m)


# ---- 1. hsk_score_views against the twin ---------------------------------------------------------------------------------------
def test_score_views_matches_the_twin(hsk, carved):
    """40 x 30 (a ragged last tile row) under 0, 1, 5 and 257 poses; 1 x 1, 7 x 5 and 8 x 8 under 5; 1, 2 and 4096 samples (the
    cap) through 7 x 5; the context's default probe; the class counts of every pose sum to width * height"""
    vol = carved_volume()
    poses = view_poses(257)
    pr = probe_40x30()
    ref = CT.score(vol, AT.DST_SIZE, pr, poses)
    for c in CT.CLASSES:
        assert (ref[c] > 0).any() or c == "n_open", c            # (every ray reaches a wall within far_m: OPEN comes with the short rays below)
    assert set(ref["eye_state"].tolist()) == {0, 1, 2, 3}
    for m in (0, 1, 5, 257):
        got = carved.score_views(poses[:m], **as_kwargs(pr))
        assert got.dtype == ref.dtype and np.array_equal(got, ref[:m]), f"n_poses = {m}: {got[got != ref[:m]][:3]} != {ref[:m][got != ref[:m]][:3]}"
        assert (sum(got[c].astype(np.int64) for c in CT.CLASSES) == 1200).all()
    print(f"towards the patch: {got[0]}")
    assert np.array_equal(hsk.rank_views(got), CT.rank(ref))
    for w, h in ((1, 1), (7, 5), (8, 8)):
        pr = probe_40x30(w=w, h=h)
        got, ref = carved.score_views(poses[:5], **as_kwargs(pr)), CT.score(vol, AT.DST_SIZE, pr, poses[:5])
        assert np.array_equal(got, ref), f"{w} x {h}: {got} != {ref}"
        assert (sum(got[c].astype(np.int64) for c in CT.CLASSES) == w * h).all()
    step = f32(0.5) * f32(TAU)
    for what, near, far, st, n in (("one sample", 0.5, 0.5, step, 1), ("two samples", 0.5, f32(0.5) + f32(1.5) * step, step, 2),
                                   ("the cap", 0.1, 3.5, f32(0.0004), 4096)):
        pr = CT.probe(7, 5, 33.0, 33.0, 3.0, 2.0, near, far, st)
        assert CT.n_samples(pr) == n, what
        got, ref = carved.score_views(poses[:5], **as_kwargs(pr)), CT.score(vol, AT.DST_SIZE, pr, poses[:5])
        assert np.array_equal(got, ref), f"{what}: {got} != {ref}"
        assert ref["n_open"].any() or n == 4096
    default = carved.score_views(poses[:5])
    pr = probe_of(hsk.default_probe(carved))
    assert (pr["width"], pr["height"]) == (160, 120) and pr["step_m"] == step
    assert np.array_equal(default, CT.score(vol, AT.DST_SIZE, pr, poses[:5]))


def test_score_views_at_the_limit_of_65536_poses(hsk, carved):
    """the launch holds at most 65535 poses in its second dimension and 2^22 workgroups in all; beyond either a workgroup takes
    several poses.  65536 poses -- 257 different ones, repeated -- through a 1 x 1 probe (the last pose is the one workgroup's
    second) against the twin, eye_state included; and through 168 x 104 (273 tiles, 69 workgroups a pose: 60787 poses a launch
    row, 4749 workgroup rows take two) the first five against the twin and every record equal to that of the pose it repeats"""
    vol = carved_volume()
    base = view_poses(257)
    poses = np.concatenate([base] * 256)[:65536]
    assert len(poses) == 65536
    pr = probe_40x30(w=1, h=1)
    got = carved.score_views(poses, **as_kwargs(pr))
    ref = CT.score(vol, AT.DST_SIZE, pr, poses, batch=8192)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} records differ, the first at {int(np.argmax(got != ref))}"
    assert set(got["eye_state"].tolist()) == {0, 1, 2, 3} and (sum(got[c].astype(np.int64) for c in CT.CLASSES) == 1).all()
    pr = probe_40x30(w=168, h=104)
    got = carved.score_views(poses, **as_kwargs(pr))
    assert np.array_equal(got[:5], CT.score(vol, AT.DST_SIZE, pr, poses[:5]))
    assert np.array_equal(got, got[np.arange(65536) % 257]) and (sum(got[c].astype(np.int64) for c in CT.CLASSES) == 168 * 104).all()
    assert len(np.unique(got[:257])) > 200


# ---- 2. hsk_render_coverage per pixel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(40, 30), (7, 5), (1, 1)])
def test_render_coverage_matches_the_twin_pixel_for_pixel(hsk, carved, size):
    vol = carved_volume()
    pr = probe_40x30(w=size[0], h=size[1])
    seen = set()
    for pose in view_poses(8):
        got = carved.render_coverage(pose, **as_kwargs(pr))
        ref = CT.ray_walk(vol, AT.DST_SIZE, pr, pose)
        assert got["cls"].dtype == np.uint8 and got["depth"].dtype == np.uint16 and got["gain"].dtype == np.uint16
        assert np.array_equal(got["cls"], ref["cls"]) and np.array_equal(got["depth"], ref["depth_mm"]) and np.array_equal(got["gain"], ref["gain"])
        assert got["score"] == carved.score_views(pose[None], **as_kwargs(pr))[0] == CT.score(vol, AT.DST_SIZE, pr, pose[None])[0]
        seen |= set(np.unique(got["cls"]).tolist())
        only = carved.render_coverage(pose, cls=False, depth=True, gain=False, **as_kwargs(pr))      # one image alone
        assert set(only) == {"depth", "score"} and np.array_equal(only["depth"], got["depth"]) and only["score"] == got["score"]
    if size == (40, 30):
        assert seen >= {CT.HIT, CT.FRONTIER, CT.BLIND, CT.OUTSIDE}
        assert CT.OPEN in set(np.unique(carved.render_coverage(TOWARDS, **as_kwargs(probe_40x30(far_m=0.6)))["cls"]).tolist())


# ---- 3. hsk_coverage_census against the twin ---------------------------------------------------------------------------------
def boxes(nz):
    return {"the whole volume": None, "bounds that are multiples of neither 4 nor 8": ((3, 5, 7), (61, 50, 33)), "one voxel": ((62, 30, 20), (63, 31, 21)),
            "the grid's low z face": ((0, 0, 0), (80, 64, 1)), "the grid's high corner": ((77, 61, nz - 3), (80, 64, nz)), "the grid's low x face": ((0, 0, 0), (1, 64, nz)),
            "the last plane": ((0, 0, nz - 1), (80, 64, nz)), "empty": ((10, 10, 10), (10, 40, 40))}


def speckled(vol, seed):
    """the volume with a fifth of its voxels set to a random state: neighbours of every kind on every axis, the grid's faces too"""
    rng = np.random.default_rng(seed)
    out = vol.copy()
    pick = rng.random(vol.shape[:3]) < 0.2
    n = int(pick.sum())
    out[pick, 0] = rng.choice(np.array([32767, 1200, 0, -1, -32767], np.int16), n)
    out[pick, 1] = rng.choice(np.array([0, 0, 1, 7], np.int16), n)
    return out


@pytest.mark.parametrize("nz", [48, 46, 41])
def test_census_matches_the_twin(hsk, nz):
    """48 planes; 46 and 41: vol_z is no multiple of 4 (nor of 8), the last plane group holds padding planes, which are no voxels"""
    vol = speckled(carved_volume(), nz)[:nz]
    dims = (80, 64, nz)
    trk = ctx(hsk, dims, size=(3.0, 3.0, 3.0 * nz / 48))
    try:
        trk.upload_tsdf(vol)
        for name, box in boxes(nz).items():
            got, ref = trk.coverage(box), CT.census(vol, box)
            print(f"{nz} planes, {name}: {got}")
            for key in ("n_unseen", "n_free", "n_solid", "n_frontier"):
                assert got[key] == ref[key], (nz, name, key, got, ref)
            assert np.array_equal(got["faces"], ref["faces"]), (nz, name, got, ref)
            lo, hi = ((0, 0, 0), dims) if box is None else box
            assert got["n_unseen"] + got["n_free"] + got["n_solid"] == np.prod([h - l for l, h in zip(lo, hi)])
            assert int(got["faces"].sum()) >= got["n_frontier"]
        whole = trk.coverage()
        assert whole["n_frontier"] > 1000 and (whole["faces"] > 0).all()
    finally:
        trk.close()


# ---- 4. deferred weights ------------------------------------------------------------------------------------------------------
def test_census_and_scores_on_a_volume_with_deferred_weights(hsk):
    """four frames of a room integrated at 64^3 leave free-space weights in the summaries (test_gpu_reloc's construction); census
    and scores are taken BEFORE any download and equal the twin fed by the download of a second, identically grown context;
    afterwards the first context's download equals the second's"""
    poses = [hsk.synth_room_pose(0, k, 720) for k in (0, 12, 24, 36)]
    depths = [hsk.synth_room_depth(0, p) for p in poses]

    def grown():
        trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
        for d, p in zip(depths, poses):
            trk.integrate(d, p)
        return trk

    a, b = grown(), grown()
    try:
        cen = b.coverage()
        part = b.coverage(((5, 9, 2), (59, 41, 63)))
        # (the frames' own poses, one of them turned 25 degrees towards what no frame saw, and one turned away from all of it)
        views = np.stack(poses + [RT.displaced(poses[0], (0.0, 0.0, 0.0), 25.0, 0.0).astype(f32), RT.displaced(poses[0], (0.1, -0.05, 0.1), 150.0, 20.0).astype(f32)])
        sc = b.score_views(views)
        img = b.render_coverage(views[4])
        vol = a.download_tsdf()
        assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
        pr = probe_of(hsk.default_probe(b))
        ref_c, ref_p, ref_s = CT.census(vol), CT.census(vol, ((5, 9, 2), (59, 41, 63))), CT.score(vol, SIZE64, pr, views)
        print(f"deferred weights: census {cen}, scores {sc}")
        for got, ref in ((cen, ref_c), (part, ref_p)):
            assert {k: got[k] for k in got if k != "faces"} == {k: ref[k] for k in ref if k != "faces"} and np.array_equal(got["faces"], ref["faces"])
        assert np.array_equal(sc, ref_s) and (sc["n_frontier"][:5] > 0).all() and (sc["n_hit"][:5] > 0).all()
        ref_i = CT.ray_walk(vol, SIZE64, pr, views[4])
        assert np.array_equal(img["cls"], ref_i["cls"]) and np.array_equal(img["depth"], ref_i["depth_mm"]) and np.array_equal(img["gain"], ref_i["gain"])
        assert cen["n_free"] > 10000 and cen["n_solid"] > 1000 and cen["n_unseen"] > 10000
        assert np.array_equal(b.download_tsdf(), vol)
    finally:
        a.close()
        b.close()


# ---- 5. nothing else moved -----------------------------------------------------------------------------------------------------
def test_the_three_calls_move_nothing_of_the_context(hsk):
    trk = hsk.KinfuTracker(n=64)
    try:
        for k in range(3):
            trk.process_frame(hsk.synth_depth(hsk.synth_pose(k)))
        before = state_of(trk, True)
        trk.coverage()
        trk.coverage(((1, 2, 3), (60, 61, 62)))
        trk.score_views(np.stack([trk.get_pose(), hsk.synth_pose(10)]))
        trk.render_coverage(trk.get_pose())
        for a, b in zip(before, state_of(trk, True)):
            assert same_bits(a, b)
        pose, ok = trk.process_frame(hsk.synth_depth(hsk.synth_pose(3)))        # ... and the scan goes on
        assert ok
    finally:
        trk.close()


# ---- 6. mid-pipeline -------------------------------------------------------------------------------------------------------------
def test_the_three_calls_between_submit_and_wait_change_nothing(hsk, synth_frames):
    """a pipelined scan at 64^3 with a census, a scoring and a coverage image between submit and wait of every frame: the same
    poses, verdicts and volume as the scan without them; what the calls return in the middle of the scan is what the volume held
    once the frame before them was fused"""
    frames = [synth_frames(k)[1] for k in range(8)]

    def run(with_calls):
        trk = hsk.KinfuTracker(n=64)
        out, mid = [], []
        for i, d in enumerate(frames):
            trk.submit_frame(d)
            if with_calls:
                views = np.stack([synth_frames(i)[0], synth_frames(i + 5)[0]]).astype(f32)
                mid.append((trk.coverage(), trk.score_views(views), trk.render_coverage(views[1])))
            out.append(trk.wait_frame())
        return trk, out, mid

    a, ra, mid = run(True)
    b, rb, _ = run(False)
    try:
        assert all(ok for _, ok in ra[1:])
        for (pa, oa), (pb, ob) in zip(ra, rb):
            assert oa == ob and same_bits(pa, pb)
        assert same_bits(a.download_tsdf(), b.download_tsdf())
        cen, sc, img = mid[-1]
        views = np.stack([synth_frames(7)[0], synth_frames(12)[0]]).astype(f32)
        after = (a.coverage(), a.score_views(views), a.render_coverage(views[1]))
        assert {k: v for k, v in cen.items() if k != "faces"} == {k: v for k, v in after[0].items() if k != "faces"}
        assert np.array_equal(cen["faces"], after[0]["faces"]) and np.array_equal(sc, after[1]) and np.array_equal(img["cls"], after[2]["cls"])
        assert cen["n_free"] > mid[0][0]["n_free"] > 0
    finally:
        a.close()
        b.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched_and_the_context_usable(hsk, carved):
    lib, L = hsk._lib.load(), hsk._lib
    eye = np.ascontiguousarray(TOWARDS, f32)
    fp = C.POINTER(C.c_float)
    good = carved.score_views(eye[None], **as_kwargs(probe_40x30()))

    def score_rc(poses=eye[None], n=None, probe=None, **fields):
        p = hsk.default_probe(carved, **dict(as_kwargs(probe_40x30()), **fields)) if probe is None else probe
        poses = np.ascontiguousarray(poses, f32)
        out = np.full(max(len(poses), 1), 7, CT.VIEW_SCORE_DTYPE)
        rc = lib.hsk_score_views(carved.h, C.byref(p), poses.ctypes.data, len(poses) if n is None else n, out.ctypes.data_as(C.POINTER(L.HskViewScore)))
        if rc != 0:
            assert lib.hsk_last_error(carved.h) and (out == np.full(1, 7, CT.VIEW_SCORE_DTYPE)[0]).all(), "an error must leave a message and `out` untouched"
        return rc

    assert score_rc() == 0
    for bad in (dict(width=0), dict(height=0), dict(width=4097), dict(height=4097), dict(fx=0.0), dict(fy=-1.0), dict(fx=float("nan")),
                dict(fy=float("inf")), dict(step_m=0.0), dict(step_m=-0.1), dict(step_m=float("nan")), dict(step_m=float("inf")), dict(near_m=-0.1),
                dict(near_m=float("nan")), dict(far_m=0.05), dict(far_m=float("inf")), dict(far_m=float("nan"))):
        assert score_rc(**bad) == -1, bad
        cls = np.full((30, 40), 9, np.uint8)
        p = hsk.default_probe(carved, **dict(as_kwargs(probe_40x30()), **bad))
        assert lib.hsk_render_coverage(carved.h, C.byref(p), eye.ctypes.data_as(fp), cls.ctypes.data, None, None, None) == -1 and (cls == 9).all(), bad
    assert score_rc(n=65537) == -1 and b"65536" in lib.hsk_last_error(carved.h)
    skew = np.stack([eye, eye, eye])
    skew[2, 0, 0] += 0.01
    assert score_rc(poses=skew) == -1 and b"pose 2" in lib.hsk_last_error(carved.h)
    assert lib.hsk_score_views(carved.h, None, None, 1, None) == -1
    assert lib.hsk_score_views(carved.h, None, None, 0, None) == 0                       # no poses: nothing to do
    assert len(carved.score_views(np.zeros((0, 4, 4), f32))) == 0
    assert lib.hsk_render_coverage(carved.h, None, None, None, None, None, None) == -1
    assert lib.hsk_render_coverage(carved.h, None, skew[2].ctypes.data_as(fp), None, None, None, None) == -1 and b"pose 0" in lib.hsk_last_error(carved.h)
    cov = L.HskCoverage(n_unseen=77)
    for lo, hi in (((-1, 0, 0), (80, 64, 48)), ((0, 0, 0), (81, 64, 48)), ((0, 0, 0), (80, 64, 49)), ((0, 9, 0), (80, 8, 48))):
        box = L.HskVoxelBox()
        box.lo[:], box.hi[:] = lo, hi
        assert lib.hsk_coverage_census(carved.h, C.byref(box), C.byref(cov)) == -1 and cov.n_unseen == 77 and lib.hsk_last_error(carved.h)
    assert lib.hsk_coverage_census(carved.h, None, None) == -1
    with pytest.raises(hsk.KinfuError, match="width and height"):
        carved.score_views(eye[None], width=5000)
    with pytest.raises(hsk.KinfuError, match="box"):
        carved.coverage(((0, 0, 0), (80, 64, 49)))
    assert np.array_equal(carved.score_views(eye[None], **as_kwargs(probe_40x30())), good)
    # a context that stores part of its volume, and the slabs of a group
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        for call in (lambda t: t.coverage(), lambda t: t.score_views(np.eye(4, dtype=f32)[None]), lambda t: t.render_coverage(np.eye(4, dtype=f32))):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call(part)
        assert lib.hsk_coverage_census(part.h, None, C.byref(cov)) == -3 and cov.n_unseen == 77
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        for i in range(g.n_slabs()):
            for call in (lambda t: t.coverage(), lambda t: t.score_views(np.eye(4, dtype=f32)[None]), lambda t: t.render_coverage(np.eye(4, dtype=f32))):
                with pytest.raises(hsk.KinfuError, match="slab"):
                    call(g.slab(i))
        _, ok = g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))
        assert ok
    finally:
        g.close()


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------
def room_box(hsk, n=64, size=3.0):
    e = hsk.synth_room_extents(0).astype(np.float64)
    lo = [max(0, int(np.floor(e[2 * i] / (size / n)))) for i in range(3)]
    hi = [min(n, int(np.ceil(e[2 * i + 1] / (size / n)))) for i in range(3)]
    return tuple(lo), tuple(hi)


def test_the_best_ranked_view_observes_what_decided_its_frontier_rays(hsk):
    """room 0 scanned at 64^3 through the first of its three turns (the level one: floor and ceiling stay open); a lattice of
    positions, yaw and pitch around the last pose is scored and ranked; the frame the sensor takes at the best view is integrated: every voxel
    that decided one of that view's FRONTIER rays is UNSEEN no longer, and n_unseen in the room's box has gone down by at least
    their number.  The probe is the default one cropped by 64 sensor pixels on every side: a voxel is integrated when its CENTRE
    projects into the frame, and the centre lies up to half a cell's diagonal (41 mm; 54 pixels at near_m = 0.4) from the sample."""
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 240, 12)]
    trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
    try:
        for p in poses:
            trk.integrate(hsk.synth_room_depth(0, p), p)
        box = room_box(hsk)
        before = trk.coverage(box)
        print(f"half scanned: {before}")
        assert before["faces"][2] + before["faces"][3] > 100, "the level turn leaves floor or ceiling open"
        full = hsk.default_probe(trk)
        pr = dict(width=full.width - 32, height=full.height - 32, cx=full.cx - 16, cy=full.cy - 16)
        L = hsk.pose_lattice(poses[-1], 0.4, 1, float(np.radians(35.0)), 1)             # 243 views, 0.4 m and 35 degrees to every side
        sc = trk.score_views(L, **pr)
        order = hsk.rank_views(sc)
        best = L[order[0]]
        print(f"best view {order[0]}: {sc[order[0]]}")
        assert sc["eye_state"][order[0]] == 0 and sc["gain"][order[0]] > 0 and sc["n_frontier"][order[0]] > 100
        vol = trk.download_tsdf()
        walk = CT.ray_walk(vol, SIZE64, probe_of(hsk.default_probe(trk, **pr)), best)
        img = trk.render_coverage(best, **pr)
        assert np.array_equal(img["cls"], walk["cls"]) and np.array_equal(img["gain"], walk["gain"])
        decided = np.unique(walk["voxel"][walk["cls"] == CT.FRONTIER], axis=0)
        in_box = np.all((decided >= box[0]) & (decided < box[1]), axis=1)
        assert (CT.states(vol)[decided[:, 2], decided[:, 1], decided[:, 0]] == CT.UNSEEN).all() and in_box.sum() > 50
        trk.integrate(hsk.synth_room_depth(0, best), best)
        after = trk.coverage(box)
        now = CT.states(trk.download_tsdf())[decided[:, 2], decided[:, 1], decided[:, 0]]
        print(f"after the suggested view: {after}; {int((now == CT.UNSEEN).sum())} of {len(decided)} deciding voxels still unseen")
        assert (now != CT.UNSEEN).all()
        assert before["n_unseen"] - after["n_unseen"] >= int(in_box.sum())
    finally:
        trk.close()
