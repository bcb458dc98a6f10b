"""hsk_bake_texture on the GPU: rgb, normal_rgb, mask, uv, charts and info byte for byte against the numpy restatement of the rule
(tests/texture_twin.py) on the cases of tests/texture_cases.py -- the coloured box simplified on the device, a hand-made mesh with
every block size, an odd bucket, skipped faces and a face outside the volume -- and on a scanned room without a flush; the analytic
wall and the projections that fail; the call protocol, the refusals, and that a bake writes nothing anyone else reads.  The shapes
are the smallest at which the kernel can go wrong: X = 72 crosses a 64-voxel segment and no dimension is a multiple of 16, the
atlases have unowned tiles, blocks of several sizes and, at W = 64, many rows of super-tiles."""
import ctypes as C

import numpy as np
import pytest

import simplify_twin as ST
import texture_cases as TC
import texture_twin as TT
from kit import same_bits
from simplify_cases import twin_of
from texture_cases import check_failed, check_wall, differing, loaded

pytestmark = pytest.mark.gpu
f32 = np.float32


def bake(trk, v, f, **params):
    """every output of one call, in the twin's names"""
    got = trk.bake_texture(v, f, rgb=True, normal_rgb=True, mask=True, **params)
    got["info"] = {n: got[n] for n in TT.INFO_FIELDS}
    return got


@pytest.fixture(scope="module")
def box(hsk):
    vol, col, size = TC.box_case()
    trk = loaded(hsk, vol, col, size)
    yield trk
    trk.close()


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [4, 8])
def test_the_box_simplified_on_the_device_matches_the_twin(box, oracle, c):
    vol, col, size = TC.box_case()
    v, f, _, _, _ = box.extract_mesh_simplified(cluster_voxels=c, normals=False)
    tw_mesh = twin_of(oracle, "box with colour", c, ST.QUADRIC)
    assert same_bits(v, tw_mesh["vertices"]) and np.array_equal(f, tw_mesh["faces"])      # (so the host tests' twin results are these meshes')
    for W in (64, 256):
        got = bake(box, v, f, atlas_width=W)
        tw = TC.twin_bake(("box", c, W), vol, col, size, v, f, atlas_width=W)
        assert differing(got, tw) == 0, (c, W, got["info"], tw["info"])
        print(c, W, got["info"])
    assert tw["info"]["n_owned"] > 50000 and 0 < tw["info"]["n_colored"] < tw["info"]["n_owned"]


def test_a_hand_made_mesh_matches_the_twin(box):
    vol, col, size = TC.box_case()
    hv, hf = TC.hand_mesh()
    for key, params in ((("hand", 0, 64), dict(atlas_width=64)),
                        (("hand, long projection", 0, 64), dict(atlas_width=64, n_iter=16, f_tol=0.0, max_offset_m=0.02, texels_per_metre=40.0)),
                        (("hand, no steps", 0, 128), dict(atlas_width=128, n_iter=0))):
        got = bake(box, hv, hf, **params)
        tw = TC.twin_bake(key, vol, col, size, hv, hf, **params)
        assert differing(got, tw) == 0, (key, got["info"], tw["info"])
    tw = TC.twin_bake(("hand", 0, 64), vol, col, size, hv, hf, atlas_width=64)
    assert all(n > 0 for n in tw["info"]["n_blocks"]) and tw["info"]["n_faces_skipped"] == 5 and tw["info"]["n_blocks"][2] == 1
    assert 0 < tw["info"]["n_projected"] < tw["info"]["n_owned"]
    # an empty mesh: an atlas of height 0, nothing to write
    got = box.bake_texture(np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), atlas_width=64, normal_rgb=True)
    assert (got["width"], got["height"], got["n_owned"]) == (64, 0, 0) and got["rgb"].shape == (0, 64, 3) and got["mask"].shape == (0, 64)


def test_the_analytic_wall_and_failed_projections_on_the_device(hsk):
    col = TC.wall_colour()
    trk = loaded(hsk, TC.wall_volume(), col, TC.WALL_SIZE)
    try:
        v, f = TC.wall_mesh(0.3)
        got = bake(trk, v, f, atlas_width=128)
        tw = TC.twin_bake("wall", TC.wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)
        assert differing(got, tw) == 0
        got["points"] = tw["points"]          # (the device hands no points out: the images are the twin's byte for byte, so are they)
        check_wall(got)
        v, f = TC.wall_mesh(10.0)
        got = bake(trk, v, f, atlas_width=128)
        tw = TC.twin_bake("wall, 10 off", TC.wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)
        assert differing(got, tw) == 0
        got["points"] = tw["points"]
        check_failed(got, v, colored=True)
        trk.upload_tsdf(TC.unseen_wall_volume())
        got = bake(trk, v, f, atlas_width=128)
        tw = TC.twin_bake("wall, unseen", TC.unseen_wall_volume(), col, TC.WALL_SIZE, v, f, atlas_width=128)
        assert differing(got, tw) == 0
        got["points"] = tw["points"]
        check_failed(got, v, colored=True)
    finally:
        trk.close()


def rgbd_frame(hsk, k):
    pose = hsk.synth_pose(k)
    return hsk.synth_depth(pose), hsk.synth_rgb(pose)


def test_a_scanned_room_matches_the_twin_and_a_bake_disturbs_nothing(hsk):
    """64^3, four RGB-D frames: the bake runs on the volume with its deferred weights (no flush), the twin on the downloads; a bake
    between submit and wait leaves the frame's result what it is; the volume, the colour and the pose stay bit for bit"""
    trk, ref = hsk.KinfuTracker(n=64), hsk.KinfuTracker(n=64)
    try:
        for t in (trk, ref):
            t.enable_color()
        for k in range(3):
            d, c = rgbd_frame(hsk, k)
            trk.process_frame_rgbd(d, c)
            ref.process_frame_rgbd(d, c)
        v, f, _, _, _ = trk.extract_mesh_simplified(cluster_voxels=4, normals=False)
        assert len(f) > 300
        d, c = rgbd_frame(hsk, 3)
        trk.submit_frame_rgbd(d, c)
        got = bake(trk, v, f, atlas_width=256)          # behind the frame in flight: it sees the fourth frame's volume
        res = trk.wait_frame()
        ref.submit_frame_rgbd(d, c)
        want = ref.wait_frame()
        assert np.array_equal(np.asarray(res[0]).view(np.uint32), np.asarray(want[0]).view(np.uint32)) and res[1] == want[1]
        pose = trk.get_pose()
        again = bake(trk, v, f, atlas_width=256)
        assert differing(again, got) == 0
        vol, col = trk.download_tsdf(), trk.download_color()
        assert np.array_equal(vol, ref.download_tsdf()) and np.array_equal(col, ref.download_color())
        assert np.array_equal(np.asarray(trk.get_pose()).view(np.uint32), np.asarray(pose).view(np.uint32))
        tw = TT.bake(vol, col, (3.0, 3.0, 3.0), v, f, atlas_width=256)
        assert differing(got, tw) == 0, (got["info"], tw["info"])
        assert tw["info"]["n_projected"] > 0.5 * tw["info"]["n_inside"] and tw["info"]["n_colored"] > 0
        print(tw["info"])
    finally:
        trk.close()
        ref.close()


# ---- 2. the call ------------------------------------------------------------------------------------------------------------------
def test_call_protocol(box, hsk):
    lib, L, h = box.lib, hsk._lib, box.h
    vol, col, size = TC.box_case()
    hv, hf = TC.hand_mesh()
    p = L.HskTextureParams(0.0, 64, 4, 0.01, 0.0)
    args = (h, hv.ctypes.data, len(hv), hf.ctypes.data, len(hf), C.byref(p))
    info = L.HskTextureInfo()
    # all NULL: the info only
    assert lib.hsk_bake_texture(*args, None, None, None, 0, None, None, C.byref(info)) == 0
    W, H = int(info.width), int(info.height)
    assert (W, H) == (64, 128) and info.n_owned == 0 and info.n_faces_charted == 10
    n = W * H
    full = bake(box, hv, hf, atlas_width=64)
    cap0 = box.product_capacity()
    # the outputs one at a time give the bytes of all together
    for name, size_b in (("rgb", 3 * n), ("normal_rgb", 3 * n), ("mask", n)):
        buf = np.full(size_b, 0xAB, np.uint8)
        ptrs = [buf.ctypes.data if name == q else None for q in ("rgb", "normal_rgb", "mask")]
        one = L.HskTextureInfo()
        assert lib.hsk_bake_texture(*args, *ptrs, n, None, None, C.byref(one)) == 0
        assert np.array_equal(buf, full[name].reshape(-1)), name
        assert [one.n_owned, one.n_inside, one.n_projected, one.n_colored, one.n_normal] == [full[k] for k in TT.INFO_FIELDS[5:]]
    uv, charts = np.zeros((len(hf), 3, 2), f32), np.zeros(len(hf), TT.CHART_DTYPE)
    assert lib.hsk_bake_texture(*args, None, None, None, 0, uv.ctypes.data, charts.ctypes.data, None) == 0
    assert np.array_equal(uv.view(np.uint32), full["uv"].view(np.uint32)) and np.array_equal(charts, full["charts"])
    # a second call of the same size allocates nothing
    bake(box, hv, hf, atlas_width=64)
    assert box.product_capacity() == cap0 > 0
    # a cap one short: HSK_ERR_ARG with the info, nothing written
    bufs = [np.full(3 * n, 0xAB, np.uint8), np.full(3 * n, 0xAB, np.uint8), np.full(n, 0xAB, np.uint8)]
    uv[:], info = 7.0, L.HskTextureInfo()
    assert lib.hsk_bake_texture(*args, *(b.ctypes.data for b in bufs), n - 1, uv.ctypes.data, None, C.byref(info)) == -1
    assert all((b == 0xAB).all() for b in bufs) and (uv == 7.0).all() and (info.width, info.height) == (W, H)
    assert b"cap_texels" in lib.hsk_last_error(h)
    # the argument errors on a live context
    for bad in (L.HskTextureParams(-1.0, 64, 4, 0.01, 0.0), L.HskTextureParams(float("nan"), 64, 4, 0.01, 0.0), L.HskTextureParams(0.0, 96, 4, 0.01, 0.0),
                L.HskTextureParams(0.0, 64, -1, 0.01, 0.0), L.HskTextureParams(0.0, 64, 17, 0.01, 0.0), L.HskTextureParams(0.0, 64, 4, -0.01, 0.0),
                L.HskTextureParams(0.0, 64, 4, 0.01, float("inf"))):
        assert lib.hsk_bake_texture(h, hv.ctypes.data, len(hv), hf.ctypes.data, len(hf), C.byref(bad), None, None, None, 0, None, None, None) == -1
    assert lib.hsk_bake_texture(h, None, len(hv), hf.ctypes.data, len(hf), None, None, None, None, 0, None, None, None) == -1
    # an atlas that would be too high: refused with the needed height
    f = np.tile(np.array([[0, 1, 2]], np.int32), (4200, 1))
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    info = L.HskTextureInfo()
    assert lib.hsk_bake_texture(h, v.ctypes.data, 3, f.ctypes.data, 4200, C.byref(L.HskTextureParams(100.0, 64, 4, 0.01, 0.0)), None, None, None, 0,
                                None, None, C.byref(info)) == -1 and info.height == 64 * 2100
    # NULL params: the defaults (W = 1024)
    assert lib.hsk_bake_texture(h, hv.ctypes.data, len(hv), hf.ctypes.data, len(hf), None, None, None, None, 0, None, None, C.byref(info)) == 0
    assert (info.width, info.height) == (1024, 64)
    # the volume and the colour are what they were
    assert np.array_equal(box.download_tsdf(), vol) and np.array_equal(box.download_color(), col)


def test_refusals(hsk, synth_frames):
    vol, col, size = TC.box_case()
    hv, hf = TC.hand_mesh()
    trk = loaded(hsk, vol, None, size)
    try:
        with pytest.raises(hsk.KinfuError, match="colour"):
            trk.bake_texture(hv, hf, atlas_width=64)
        got = trk.bake_texture(hv, hf, atlas_width=64, rgb=False, normal_rgb=True)     # normal_rgb and mask need no colour
        tw = TC.twin_bake(("hand, without colour", 0, 64), vol, None, size, hv, hf, atlas_width=64)
        got["info"], got["rgb"] = {n: got[n] for n in TT.INFO_FIELDS}, tw["rgb"]
        assert differing(got, tw) == 0 and got["n_colored"] == 0
    finally:
        trk.close()
    grp = hsk.KinfuGroup(hsk.default_config(64), device_ids=[0, 0])
    try:
        grp.process_frame(synth_frames(0)[1])
        for i in range(grp.n_slabs()):
            with pytest.raises(hsk.KinfuError, match="slab"):
                grp.slab(i).bake_texture(hv, hf, rgb=False)
    finally:
        grp.close()
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        with pytest.raises(hsk.KinfuError, match="slab"):
            part.bake_texture(hv, hf, rgb=False)
    finally:
        part.close()
