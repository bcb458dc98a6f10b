"""hsk_bake_texture_keyframes on the GPU: rgb, mask, source, normal_rgb, uv, charts and both infos byte for byte against the numpy
restatement of the rule (tests/keytex_twin.py) on every case of tests/keytex_cases.py, in both modes; what it shares with
hsk_bake_texture; a context without colour; a scan with keyframes added while a frame is in flight; the store; the call protocol
and the refusals.  The shapes are the smallest at which the kernel can go wrong: keyframes of 50 x 38 and 16 x 12 pixels (no
multiple of 4), 70 of them (more than a wave has lanes), atlases with unowned tiles and waves whose texels disagree about a keyframe
(the image border and the occluder's edge cross tiles)."""
import ctypes as C

import numpy as np
import pytest

import keytex_cases as KC
import keytex_twin as KT
import texture_cases as TC
import texture_twin as TT
from keytex_cases import differing
from texture_cases import loaded

pytestmark = pytest.mark.gpu
f32 = np.float32
MODES = (KT.BEST, KT.BLEND)
WALL_CASES = ("frontal", "edited depth", "edited depth, fallback", "competing", "ring of 70", "empty store")
BOX_CASES = ("box", "box, no colour, loose")


def store(trk, kfs, cap=None, size=(KC.KW, KC.KH)):
    """a fresh store holding the keyframes"""
    trk.release_keyframes()
    h, w = kfs[0]["depth"].shape if kfs else (size[1], size[0])
    trk.enable_keyframes(cap or max(1, len(kfs)), w, h)
    for i, kf in enumerate(kfs):
        assert trk.add_keyframe(kf["depth"], kf["rgb"], kf["pose"], kf["intr"]) == i


def bake(trk, v, f, keytex, tex):
    """every output of one call, in the twin's names"""
    got = trk.bake_texture_keyframes(v, f, rgb=True, normal_rgb=True, mask=True, source=True, **tex, **keytex)
    got["info"] = {n: got[n] for n in TT.INFO_FIELDS}
    got["kinfo"] = {n: got[n] for n in KT.KINFO_FIELDS}
    return got


def check_case(hsk, key, case):
    vol, col, size, v, f, kfs, keytex, tex = case
    trk = loaded(hsk, vol, col, size)
    try:
        store(trk, kfs)
        for mode in MODES:
            tw = KC.twin_bake(key, mode, *case)
            got = bake(trk, v, f, dict(keytex, mode=mode), tex)
            assert differing(got, tw) == 0, (key, mode, got["kinfo"], tw["kinfo"], got["info"], tw["info"])
            print(key, mode, got["kinfo"])
    finally:
        trk.close()


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WALL_CASES)
def test_the_wall_matches_the_twin(hsk, key):
    check_case(hsk, key, KC.wall_cases()[key])


@pytest.mark.parametrize("key", BOX_CASES)
def test_the_box_matches_the_twin(hsk, oracle, key):
    check_case(hsk, key, KC.box_cases(oracle)[key])


# ---- 2. what the two bakes share, and what they do not ---------------------------------------------------------------------------
def test_shared_outputs_equal_bake_texture_and_colour_is_not_needed(hsk, oracle):
    vol, col, size, v, f, kfs, keytex, tex = KC.box_cases(oracle)["box"]
    trk = loaded(hsk, vol, col, size)
    try:
        store(trk, kfs)
        base = trk.bake_texture(v, f, rgb=True, normal_rgb=True, mask=True, **tex)
        for mode in MODES:
            got = bake(trk, v, f, dict(keytex, mode=mode), tex)
            assert np.array_equal(got["normal_rgb"], base["normal_rgb"]) and np.array_equal(got["uv"].view(np.uint32), base["uv"].view(np.uint32))
            assert np.array_equal(got["charts"], base["charts"])
            shared = TT.OWNED | TT.INSIDE | TT.PROJECTED | TT.NORMAL
            keyed = (got["mask"] & KT.KEYFRAME) != 0
            assert np.array_equal(got["mask"] & shared, base["mask"] & shared) and keyed.sum() > 1000
            # COLORED keeps its meaning: set only where the colour volume coloured the texel, which it did where no keyframe passed
            assert ((got["mask"][keyed] & TT.COLORED) == 0).all() and np.array_equal(got["mask"][~keyed], base["mask"][~keyed])
            assert np.array_equal(got["rgb"][~keyed], base["rgb"][~keyed])
            assert [got[n] for n in TT.INFO_FIELDS if n != "n_colored"] == [base[n] for n in TT.INFO_FIELDS if n != "n_colored"]
        # an empty store with the fallback: hsk_bake_texture's images, all five low bits and its info
        trk.clear_keyframes()
        got = bake(trk, v, f, {}, tex)
        for name in ("rgb", "normal_rgb", "mask"):
            assert np.array_equal(got[name], base[name]), name
        assert (got["source"] == KT.NONE).all() and got["info"] == {n: base[n] for n in TT.INFO_FIELDS} and got["n_fallback"] == base["n_colored"]
    finally:
        trk.close()
    # without a colour volume hsk_bake_texture refuses rgb, the keyframe bake does not
    trk = loaded(hsk, vol, None, size)
    try:
        store(trk, kfs)
        with pytest.raises(hsk.KinfuError, match="colour"):
            trk.bake_texture(v, f, **tex)
        got = bake(trk, v, f, keytex, tex)
        assert got["n_keyed"] > 1000 and got["n_fallback"] == 0 and got["n_colored"] == 0 and got["rgb"][(got["mask"] & KT.KEYFRAME) != 0].any()
        base = trk.bake_texture(v, f, rgb=False, normal_rgb=True, mask=True, **tex)
        assert np.array_equal(got["mask"] & 31, base["mask"]) and np.array_equal(got["normal_rgb"], base["normal_rgb"])
        assert got["info"] == {n: base[n] for n in TT.INFO_FIELDS}
    finally:
        trk.close()


def test_keyframes_added_while_a_frame_is_in_flight_disturb_nothing(hsk):
    """64^3, four depth-only frames, no colour volume: keyframes are added between submit and wait, and a bake runs there; the
    frame's result, the volume and the pose are bit-equal to a context that kept no keyframes; the bake matches the twin on the
    downloaded volume and a second bake repeats it"""
    trk, ref = hsk.KinfuTracker(n=64), hsk.KinfuTracker(n=64)
    try:
        trk.enable_keyframes(4)
        assert trk.keyframe_count() == dict(n=0, cap=4, w=640, h=480, bytes=4 * ((64 + 6 * 640 * 480 + 255) & ~255))
        kfs = []
        for k in range(3):
            pose = hsk.synth_pose(k)
            d, c = hsk.synth_depth(pose), hsk.synth_rgb(pose)
            trk.submit_frame(d)
            trk.add_keyframe(d, c, pose)                      # behind the frame in flight, intr = the context's camera
            res = trk.wait_frame()
            ref.submit_frame(d)
            want = ref.wait_frame()
            assert np.array_equal(np.asarray(res[0]).view(np.uint32), np.asarray(want[0]).view(np.uint32)) and res[1] == want[1]
            kfs.append(KT.keyframe(d, c, pose, [525.0, 525.0, 319.5, 239.5]))
        v, f, _, _, _ = trk.extract_mesh_simplified(cluster_voxels=4, normals=False)
        assert len(f) > 300
        pose = hsk.synth_pose(3)
        d, c = hsk.synth_depth(pose), hsk.synth_rgb(pose)
        trk.submit_frame(d)
        trk.add_keyframe(d, c, pose)
        kfs.append(KT.keyframe(d, c, pose, [525.0, 525.0, 319.5, 239.5]))
        got = bake(trk, v, f, {}, dict(atlas_width=256))      # behind the frame in flight: it sees the fourth frame's volume
        res = trk.wait_frame()
        ref.submit_frame(d)
        want = ref.wait_frame()
        assert np.array_equal(np.asarray(res[0]).view(np.uint32), np.asarray(want[0]).view(np.uint32)) and res[1] == want[1]
        again = bake(trk, v, f, {}, dict(atlas_width=256))
        assert differing(again, got) == 0
        vol = trk.download_tsdf()
        assert np.array_equal(vol, ref.download_tsdf())
        assert np.array_equal(np.asarray(trk.get_pose()).view(np.uint32), np.asarray(ref.get_pose()).view(np.uint32))
        tw = KT.bake(vol, None, (3.0, 3.0, 3.0), v, f, kfs, {}, atlas_width=256)
        assert differing(got, tw) == 0, (got["kinfo"], tw["kinfo"])
        assert tw["kinfo"]["n_pairs_seen"] > tw["kinfo"]["n_keyed"] > 0 and len(np.unique(tw["source"])) >= 3    # (several keyframes see a texel)
        print(tw["kinfo"])
        # the store outlives a reset
        trk.reset()
        assert trk.keyframe_count()["n"] == 4
    finally:
        trk.close()
        ref.close()


# ---- 3. the store ---------------------------------------------------------------------------------------------------------------------
def test_the_store(hsk):
    vol, col, size, v, f, kfs, keytex, tex = KC.wall_cases()["competing"]
    trk = loaded(hsk, vol, None, size)
    lib, L, h = trk.lib, hsk._lib, trk.h
    try:
        with pytest.raises(hsk.KinfuError, match="no keyframe store"):
            trk.bake_texture_keyframes(v, f, **tex)
        with pytest.raises(hsk.KinfuError, match="no keyframe store"):
            trk.add_keyframe(kfs[0]["depth"], kfs[0]["rgb"], kfs[0]["pose"], kfs[0]["intr"])
        assert trk.keyframe_count() == dict(n=0, cap=0, w=0, h=0, bytes=0)
        for bad in ((0, 50, 38), (256, 50, 38), (4, 1, 38), (4, 50, 4097)):
            assert lib.hsk_enable_keyframes(h, *bad) == -1
        store(trk, kfs, cap=len(kfs))
        assert trk.keyframe_count() == dict(n=6, cap=6, w=KC.KW, h=KC.KH, bytes=6 * ((64 + 6 * KC.KW * KC.KH + 255) & ~255))
        # what went in comes back
        for i, kf in enumerate(kfs):
            pose, intr, d, c = trk.get_keyframe(i)
            want = kf["pose"].copy()
            want[3] = (0, 0, 0, 1)
            assert np.array_equal(pose.view(np.uint32), want.view(np.uint32)) and np.array_equal(intr, kf["intr"])
            assert np.array_equal(d, kf["depth"]) and np.array_equal(c, kf["rgb"])
        assert lib.hsk_get_keyframe(h, 6, None, None, None, None) == -1 and lib.hsk_get_keyframe(h, -1, None, None, None, None) == -1
        # a full store is refused with nothing written
        before = bake(trk, v, f, keytex, tex)
        assert lib.hsk_add_keyframe(h, kfs[1]["depth"].ctypes.data, kfs[1]["rgb"].ctypes.data, KC.KW, KC.KH, kfs[1]["pose"].ctypes.data, None, None) == -3
        assert b"full" in lib.hsk_last_error(h) and trk.keyframe_count()["n"] == 6 and differing(bake(trk, v, f, keytex, tex), before) == 0
        # the same three numbers keep the store and its contents, others are refused until it is released
        trk.enable_keyframes(6, KC.KW, KC.KH)
        assert trk.keyframe_count()["n"] == 6
        assert lib.hsk_enable_keyframes(h, 7, KC.KW, KC.KH) == -3 and lib.hsk_enable_keyframes(h, 6, KC.KW + 1, KC.KH) == -3
        # the argument errors of an add
        trk.clear_keyframes()
        assert trk.keyframe_count()["n"] == 0 and trk.keyframe_count()["cap"] == 6
        d, c, pose, intr = (np.ascontiguousarray(kfs[0][n]) for n in ("depth", "rgb", "pose", "intr"))
        ok = [d.ctypes.data, c.ctypes.data, KC.KW, KC.KH, pose.ctypes.data, intr.ctypes.data, None]
        nan_pose = pose.copy()
        nan_pose[1, 2] = np.nan
        for at, val in ((0, None), (1, None), (2, KC.KW + 1), (3, KC.KH - 1), (4, None), (4, nan_pose.ctypes.data),
                        (5, np.array([0.0, 40.0, 1.0, 1.0], f32).ctypes.data), (5, np.array([40.0, -1.0, 1.0, 1.0], f32).ctypes.data),
                        (5, np.array([np.inf, 40.0, 1.0, 1.0], f32).ctypes.data), (5, np.array([40.0, 40.0, np.nan, 1.0], f32).ctypes.data)):
            args = list(ok)
            args[at] = val
            assert lib.hsk_add_keyframe(h, *args) == -1, (at, val)
        assert trk.keyframe_count()["n"] == 0
        index = C.c_int(-1)
        assert lib.hsk_add_keyframe(h, *ok[:6], C.byref(index)) == 0 and index.value == 0
        # intr NULL: the context's camera
        assert trk.add_keyframe(d, c, pose) == 1
        cfg = trk.cfg
        assert np.array_equal(trk.get_keyframe(1, images=False)[1], np.array([cfg.fx, cfg.fy, cfg.cx, cfg.cy], f32))
        trk.release_keyframes()
        assert trk.keyframe_count() == dict(n=0, cap=0, w=0, h=0, bytes=0)
        trk.enable_keyframes(2, 16, 12)
    finally:
        trk.close()


# ---- 4. the call ------------------------------------------------------------------------------------------------------------------
def test_call_protocol(hsk):
    vol, col, size, v, f, kfs, keytex, tex = KC.wall_cases()["competing"]
    trk = loaded(hsk, vol, col, size)
    lib, L, h = trk.lib, hsk._lib, trk.h
    try:
        store(trk, kfs)
        p = L.HskTextureParams(0.0, 128, 4, 0.01, 0.0)
        kp = trk.default_keytex_params()
        kp.fallback_volume = 0
        args = (h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(p), C.byref(kp))
        info, kinfo = L.HskTextureInfo(), L.HskKeytexInfo()
        # all NULL: the infos only
        assert lib.hsk_bake_texture_keyframes(*args, None, None, None, None, 0, None, None, C.byref(info), C.byref(kinfo)) == 0
        W, H = int(info.width), int(info.height)
        assert (W, H) == (128, 64) and info.n_owned == 0 and kinfo.n_keyframes == 6 and kinfo.n_keyed == 0
        n = W * H
        full = bake(trk, v, f, keytex, tex)
        cap0 = trk.product_capacity()
        # the outputs one at a time give the bytes of all together
        names = ("rgb", "normal_rgb", "mask", "source")
        for name, size_b in (("rgb", 3 * n), ("normal_rgb", 3 * n), ("mask", n), ("source", n)):
            buf = np.full(size_b, 0xAB, np.uint8)
            ptrs = [buf.ctypes.data if name == q else None for q in names]
            one, kone = L.HskTextureInfo(), L.HskKeytexInfo()
            assert lib.hsk_bake_texture_keyframes(*args, *ptrs, n, None, None, C.byref(one), C.byref(kone)) == 0
            assert np.array_equal(buf, full[name].reshape(-1)), name
            assert [one.n_owned, one.n_inside, one.n_projected, one.n_colored, one.n_normal] == [full[k] for k in TT.INFO_FIELDS[5:]]
            assert [getattr(kone, k) for k in KT.KINFO_FIELDS] == [full[k] for k in KT.KINFO_FIELDS]
        uv, charts = np.zeros((len(f), 3, 2), f32), np.zeros(len(f), TT.CHART_DTYPE)
        assert lib.hsk_bake_texture_keyframes(*args, None, None, None, None, 0, uv.ctypes.data, charts.ctypes.data, None, None) == 0
        assert np.array_equal(uv.view(np.uint32), full["uv"].view(np.uint32)) and np.array_equal(charts, full["charts"])
        # a second call of the same size allocates nothing
        bake(trk, v, f, keytex, tex)
        assert trk.product_capacity() == cap0 > 0
        # a cap one short: HSK_ERR_ARG with the info, nothing written
        bufs = [np.full(3 * n, 0xAB, np.uint8), np.full(3 * n, 0xAB, np.uint8), np.full(n, 0xAB, np.uint8), np.full(n, 0xAB, np.uint8)]
        uv[:], info = 7.0, L.HskTextureInfo()
        assert lib.hsk_bake_texture_keyframes(*args, *(b.ctypes.data for b in bufs), n - 1, uv.ctypes.data, None, C.byref(info), None) == -1
        assert all((b == 0xAB).all() for b in bufs) and (uv == 7.0).all() and (info.width, info.height) == (W, H)
        assert b"cap_texels" in lib.hsk_last_error(h)
        # the argument errors
        K = L.HskKeytexParams
        d = [getattr(kp, name) for name, _ in kp._fields_]
        for at, val in ((0, 2), (0, -1), (1, -0.1), (1, float("nan")), (2, float("inf")), (1, 5.0), (3, 1.5), (3, -0.1), (4, -1.0), (5, -0.1),
                        (5, float("nan")), (6, 1.1), (6, -0.1)):
            bad = list(d)
            bad[at] = val
            assert lib.hsk_bake_texture_keyframes(h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(p), C.byref(K(*bad)), None, None, None, None, 0,
                                                  None, None, None, None) == -1, (at, val)
        bad_tex = L.HskTextureParams(0.0, 96, 4, 0.01, 0.0)
        assert lib.hsk_bake_texture_keyframes(h, v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(bad_tex), None, None, None, None, None, 0, None, None,
                                              None, None) == -1
        assert lib.hsk_bake_texture_keyframes(h, None, len(v), f.ctypes.data, len(f), None, None, None, None, None, None, 0, None, None, None, None) == -1
        # NULL params: the defaults of both (W = 1024; the fallback on)
        assert lib.hsk_bake_texture_keyframes(h, v.ctypes.data, len(v), f.ctypes.data, len(f), None, None, None, None, None, None, 0, None, None,
                                              C.byref(info), None) == 0 and (info.width, info.height) == (1024, 64)
        # the volume and the colour are what they were
        assert np.array_equal(trk.download_tsdf(), vol) and np.array_equal(trk.download_color(), col)
    finally:
        trk.close()


def test_refusals(hsk, synth_frames):
    v, f = TC.wall_mesh(0.3)
    kf = KC.frontal()
    grp = hsk.KinfuGroup(hsk.default_config(64), device_ids=[0, 0])
    try:
        grp.process_frame(synth_frames(0)[1])
        for i in range(grp.n_slabs()):
            s = grp.slab(i)
            with pytest.raises(hsk.KinfuError, match="slab"):
                s.enable_keyframes(4, KC.KW, KC.KH)
            with pytest.raises(hsk.KinfuError, match="slab"):
                s.add_keyframe(kf["depth"], kf["rgb"], kf["pose"], kf["intr"])
            with pytest.raises(hsk.KinfuError, match="slab"):
                s.bake_texture_keyframes(v, f)
            assert s.keyframe_count()["cap"] == 0
    finally:
        grp.close()
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        with pytest.raises(hsk.KinfuError, match="slab"):
            part.enable_keyframes(4, KC.KW, KC.KH)
        with pytest.raises(hsk.KinfuError, match="slab"):
            part.bake_texture_keyframes(v, f)
    finally:
        part.close()
