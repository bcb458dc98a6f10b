"""Sparse volume images on the GPU against the numpy twin (tests/pack_twin.py), BIT FOR BIT: hsk_pack_volume's bytes are the
twin's image of download_tsdf() / download_color() and the context's header fields; hsk_unpack_volume makes a whole, consistent
context; files; and hsk_resume_scan, which lets a fresh context that loaded a saved volume go on tracking exactly as the
context that grew it would have."""
import ctypes as C
import os

import numpy as np
import pytest

import pack_twin as PT
import view_twin as VT
from fuse_cases import HOUSE_DIMS, HOUSE_SIZE, N, SIZE, _close_scans, make_ctx, room_scan  # noqa: F401  (the fixture closes the scans)
from kit import same_bits_nan
from pack_cases import assert_same_image, ctx_fields
from section_cases import SCAN_FRAMES, room_frames

pytestmark = pytest.mark.gpu
f32 = np.float32


def with_color(trk, max_weight=64):
    trk.enable_color(max_weight)
    trk.color_params = (max_weight,)
    return trk


def twin_image(hsk, trk):
    return PT.pack(trk.download_tsdf(), trk.download_color() if getattr(trk, "color_params", None) else None, ctx_fields(hsk, trk))


def scanned_twin_is_nontrivial(img, color=True):
    f = PT.info(img)
    t = f["tsdf_bricks"]
    assert t[PT.ZERO] > 0 and t[PT.SPLIT] > 0 and t[PT.RAW] > 0, f"the twin's image lacks a class: {t}"
    if color:
        assert f["color_bricks"][1] > 0 and f["color_bricks"][0] > 0, f["color_bricks"]
    return f


# ---- 1. pack ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
def test_an_empty_context_packs_to_header_and_tables(hsk, color):
    trk = make_ctx(hsk, (64, 64, 64), color=False)
    try:
        if color:
            with_color(trk)
        img, info = trk.pack_volume(with_info=True)
        assert_same_image(img, twin_image(hsk, trk), "empty")
        assert info["tsdf_bricks"].tolist() == [512, 0, 0, 0] and len(img) == 256 + 512 * (2 if color else 1)
        assert hsk.volume_image_info(img)["total_bytes"] == len(img)
    finally:
        trk.close()


CRAFTED = [((64, 64, 64), True), ((64, 32, 20), True), ((128, 64, 40), False), ((64, 64, 22), True)]


@pytest.mark.parametrize("dims,color", CRAFTED)
def test_crafted_volumes_pack_to_the_twins_bytes(hsk, dims, color):
    tsdf, col = PT.crafted_volume(dims, seed=7 + dims[2], color=color)
    assert (tsdf[..., 1] == 256).any() and ((tsdf[..., 1] == 0) & (tsdf[..., 0] != 0)).any()
    trk = make_ctx(hsk, dims, (3.0, 1.5, 2.0), color=False)
    try:
        if color:
            with_color(trk, 200)
            trk.upload_color(col)
        trk.upload_tsdf(tsdf)
        want = PT.pack(tsdf, col, ctx_fields(hsk, trk))
        f = PT.info(want)
        assert all(n > 0 for n in f["tsdf_bricks"]), f["tsdf_bricks"]
        img, info = trk.pack_volume(with_info=True)
        assert_same_image(img, want, f"crafted {dims}")
        assert info["tsdf_bricks"].tolist() == list(f["tsdf_bricks"]) and info["color_bricks"].tolist() == list(f["color_bricks"])
        assert np.array_equal(trk.download_tsdf(), tsdf), "packing changed the volume"
        # ... and back, into a context that holds something else
        other = make_ctx(hsk, dims, (3.0, 1.5, 2.0), color=False)
        try:
            if color:
                with_color(other, 200)
                other.upload_color(np.full_like(col, 3))
            junk = np.empty_like(tsdf)
            junk[...] = (11, 2)
            other.upload_tsdf(junk)
            other.unpack_volume(img)
            assert np.array_equal(other.download_tsdf(), tsdf)
            if color:
                assert np.array_equal(other.download_color(), col)
            assert_same_image(other.pack_volume(), PT.pack(tsdf, col, ctx_fields(hsk, other)), f"crafted {dims}, packed again")
        finally:
            other.close()
    finally:
        trk.close()


def test_room_scan_packs_to_the_twins_bytes(hsk):
    trk, tsdf, col = room_scan(hsk, 0)
    trk.color_params = (64,)
    want = PT.pack(tsdf, col, ctx_fields(hsk, trk))
    f = scanned_twin_is_nontrivial(want)
    img, info = trk.pack_volume(with_info=True)
    print(f"room 0 at {N}^3: bricks {f['tsdf_bricks']}, colour {f['color_bricks']}, {len(img)} bytes = "
          f"{len(img) / (tsdf.nbytes + col.nbytes):.3f} of the raw volume")
    assert_same_image(img, want, "room 0")
    assert info["total_bytes"] == len(img)


def test_house_volume_packs_to_the_twins_bytes(hsk):
    """a 256 x 128 x 128 volume over 6 x 3 x 3 m that two rooms were fused into"""
    import fuse_twin as FT
    CELL = 3.0 / N
    src0, _, _ = room_scan(hsk, 0)
    src1, _, _ = room_scan(hsk, 1)
    house = with_color(make_ctx(hsk, HOUSE_DIMS, HOUSE_SIZE, color=False))
    try:
        assert house.fuse_from(src0, FT.rot_about("y", 20.0, (1.5, 1.5, 1.5), (0.7 + 0.4 * CELL, 0.3 * CELL, -0.2 * CELL)))["n_fused"] > 0
        assert house.fuse_from(src1, FT.rot_about("y", -10.0, (1.5, 1.5, 1.5), (2.6, 0.1 * CELL, 0.2 * CELL)))["n_fused"] > 0
        want = twin_image(hsk, house)
        scanned_twin_is_nontrivial(want)
        assert_same_image(house.pack_volume(), want, "house")
    finally:
        house.close()


# ---- 2. deferred weights ------------------------------------------------------------------------------------------
def tracked_room(hsk, n_frames=30, wait=True):
    frames = room_frames(hsk, 1, 0, n_frames)
    trk = with_color(hsk.KinfuTracker(n=N, init_pose=hsk.synth_room_pose(1, 0, SCAN_FRAMES)))
    out = []
    for i, (d, c) in enumerate(frames):
        trk.submit_frame_rgbd(d, c)
        if i >= 2:
            out.append(trk.wait_frame())
    while len(out) < len(frames):
        out.append(trk.wait_frame())
    assert all(ok for _, ok in out[1:])
    return trk


def test_pack_writes_the_deferred_weights_back_first(hsk):
    a, b = tracked_room(hsk), tracked_room(hsk)
    try:
        img_a = a.pack_volume()                      # straight behind the pipelined frames: no explicit flush
        tsdf = b.download_tsdf()                     # (the download writes b's weights back)
        assert (tsdf[..., 1] > 1).any()
        img_b = b.pack_volume()
        assert_same_image(img_a, img_b, "deferred weights")
        assert_same_image(img_b, twin_image(hsk, b), "after the download")
        scanned_twin_is_nontrivial(img_b)
    finally:
        a.close()
        b.close()


# ---- 3. round trip: the destination is a whole, consistent context -------------------------------------------------
def assert_same_context(hsk, a, b, tsdf):
    for x, y in zip(a.extract_cloud_attrs(), b.extract_cloud_attrs()):
        assert same_bits_nan(np.asarray(x), np.asarray(y)), "cloud"
    assert a.extract_cloud(cap=0)[1] > 1000
    for x, y in zip(a.extract_mesh_indexed(), b.extract_mesh_indexed()):
        assert same_bits_nan(np.asarray(x), np.asarray(y)), "indexed mesh"
    pose = hsk.synth_room_pose(0, 40, SCAN_FRAMES)
    va = a.render_view(pose=pose, mode=VT.COLOR_LIT, vmap=True, nmap=True)
    vb = b.render_view(pose=pose, mode=VT.COLOR_LIT, vmap=True, nmap=True)
    assert va["n_hit"] > 1000
    for key in va:
        assert same_bits_nan(np.asarray(va[key]), np.asarray(vb[key])), f"view: {key}"
    for x, y in zip(a.raycast(pose, want_keys=True), b.raycast(pose, want_keys=True)):
        assert same_bits_nan(x, y), "raycast"
    depth, rgb = hsk.synth_room_depth(0, pose), hsk.synth_rgb(pose, 0)
    for t in (a, b):
        t.integrate(depth, pose)
        t.integrate_color(depth, rgb, pose)
    assert a.integrate_coarse_counts() == b.integrate_coarse_counts()
    ta, tb = a.download_tsdf(), b.download_tsdf()
    assert np.array_equal(ta, tb) and not np.array_equal(ta, tsdf)
    assert np.array_equal(a.download_color(), b.download_color())


@pytest.mark.parametrize("over_another_scan", [False, True])
def test_unpack_makes_a_whole_consistent_context(hsk, over_another_scan):
    src, tsdf, col = room_scan(hsk, 0)
    img = src.pack_volume()
    info = hsk.volume_image_info(img)
    if over_another_scan:
        dst = tracked_room(hsk, 12)                     # holds room 1, with deferred weights and a tracker state of its own
    else:
        dst = with_color(hsk.KinfuTracker(hsk.config_from_volume(info)))
    # The reference is NOT the original context but a copy of it, made by hsk_upload_tsdf / hsk_upload_color from the original's
    # downloaded arrays: the checks below integrate one more frame into both contexts, and the original (the module's shared
    # scan) must stay as it is for the other tests.  The copy owes nothing to the code under test.
    ref = with_color(hsk.KinfuTracker(hsk.config_from_volume(info)))
    try:
        ref.upload_tsdf(tsdf)
        ref.upload_color(col)
        pose_before = dst.get_pose()
        dst.unpack_volume(img)
        assert np.array_equal(dst.get_pose(), pose_before), "unpack must not touch the tracker pose"
        assert np.array_equal(dst.download_tsdf(), tsdf) and np.array_equal(dst.download_color(), col)
        assert_same_context(hsk, dst, ref, tsdf)
    finally:
        dst.close()
        ref.close()


# ---- 4. the colour rules ---------------------------------------------------------------------------------------------
def test_colour_rules(hsk):
    src, tsdf, col = room_scan(hsk, 0)
    img_c = src.pack_volume()
    plain = hsk.KinfuTracker(n=N)
    try:
        plain.upload_tsdf(tsdf)
        img_p = plain.pack_volume()
        assert PT.info(img_p)["flags"] == 0 and PT.info(img_c)["flags"] == 1
        # image with colour, context without: the colour section is skipped
        plain.reset()
        plain.unpack_volume(img_c)
        assert np.array_equal(plain.download_tsdf(), tsdf)
        with pytest.raises(hsk.KinfuError, match="colour is not enabled"):
            plain.download_color()
    finally:
        plain.close()
    both = with_color(hsk.KinfuTracker(n=N))
    try:
        both.unpack_volume(img_c)                        # both have colour: taken
        assert np.array_equal(both.download_color(), col) and (col[..., 3] > 0).any()
        both.unpack_volume(img_p)                        # image without colour: the colour volume is zeroed
        assert np.array_equal(both.download_tsdf(), tsdf) and not both.download_color().any()
    finally:
        both.close()


# ---- 5. the protocol -------------------------------------------------------------------------------------------------
def test_two_call_protocol_and_the_cached_pass(hsk):
    lib = hsk._lib.load()
    src, tsdf, col = room_scan(hsk, 0)
    trk = with_color(hsk.KinfuTracker(n=N))
    try:
        trk.upload_tsdf(tsdf)
        trk.upload_color(col)
        n, info = C.c_size_t(), hsk._lib.HskVolumeInfo()
        assert lib.hsk_pack_volume(trk.h, None, 0, C.byref(n), C.byref(info)) == 0        # counts only
        total = n.value
        assert total == info.total_bytes > 256 and info.pass_reused == 0
        buf = np.full(total + 16, 0xAB, np.uint8)
        n.value = 0
        assert lib.hsk_pack_volume(trk.h, buf.ctypes.data, total - 1, C.byref(n), C.byref(info)) == -1   # one byte short
        assert n.value == total and (buf == 0xAB).all() and info.pass_reused == 1
        assert "smaller" in lib.hsk_last_error(trk.h).decode()
        assert lib.hsk_pack_volume(trk.h, buf.ctypes.data, total, C.byref(n), C.byref(info)) == 0
        assert info.pass_reused == 1 and (buf[total:] == 0xAB).all()
        first = buf[:total].tobytes()
        assert_same_image(first, twin_image(hsk, trk), "protocol")
        assert lib.hsk_pack_volume(trk.h, None, 0, C.byref(n), None) == 0 and n.value == total       # info may be NULL
        # every kind of volume change voids the pass, and the new image is the new volume's
        pose = hsk.synth_room_pose(0, 40, SCAN_FRAMES)
        depth, rgb = hsk.synth_room_depth(0, pose), hsk.synth_rgb(pose, 0)
        changes = {
            "fuse": lambda: trk.fuse_from(src, np.eye(4, dtype=f32)),
            "integrate": lambda: trk.integrate(depth, pose),
            "integrate_color": lambda: trk.integrate_color(depth, rgb, pose),
            "upload_color": lambda: trk.upload_color(np.roll(col, 8, axis=2)),
            "upload_tsdf": lambda: trk.upload_tsdf(np.roll(tsdf, 8, axis=1)),
            "unpack": lambda: trk.unpack_volume(first),
            "a frame": lambda: trk.process_frame_rgbd(depth, rgb),
            "reset": trk.reset,
        }
        last = first
        for what, change in changes.items():
            change()
            img, inf = trk.pack_volume(with_info=True)          # (its size query runs the pass, its fill reuses it)
            assert trk.pack_volume_info()["pass_reused"] == 1, what
            assert_same_image(img, twin_image(hsk, trk), what)
            assert img != last, f"{what} did not change the image"
            last = img
        assert PT.info(last)["tsdf_bricks"][PT.ZERO] == PT.info(last)["n_bricks"]      # (behind the reset)
    finally:
        trk.close()


def test_enabling_colour_voids_the_cached_pass(hsk):
    """the pass is held for the volume AND the colour flag: colour enabled behind a pass, with no volume change, runs it again,
    and the image then carries the colour section"""
    trk = make_ctx(hsk, (64, 32, 20), color=False)
    try:
        assert trk.pack_volume_info()["pass_reused"] == 0 and trk.pack_volume_info()["pass_reused"] == 1
        plain = trk.pack_volume()
        with_color(trk)
        assert trk.pack_volume_info()["pass_reused"] == 0 and trk.pack_volume_info()["pass_reused"] == 1
        img = trk.pack_volume()
        assert_same_image(img, twin_image(hsk, trk), "colour enabled behind a pass")
        assert PT.info(plain)["flags"] == 0 and PT.info(img)["flags"] == 1 and len(img) > len(plain)
    finally:
        trk.close()


# ---- 6. files --------------------------------------------------------------------------------------------------------
def test_files(hsk, tmp_path):
    src, tsdf, col = room_scan(hsk, 0)
    path = tmp_path / "volume.hskv"
    info = src.save_volume(path)
    img = src.pack_volume()
    assert path.read_bytes() == img and info["total_bytes"] == len(img) and not os.path.exists(str(path) + ".tmp")
    assert hsk.volume_file_info(path)["tsdf_bricks"].tolist() == info["tsdf_bricks"].tolist()
    dst = with_color(hsk.KinfuTracker(n=N))
    try:
        dst.load_volume(path)
        assert np.array_equal(dst.download_tsdf(), tsdf) and np.array_equal(dst.download_color(), col)
        # a corrupted file leaves the volume as it was
        dst.integrate(hsk.synth_depth(hsk.synth_pose(0)), hsk.synth_pose(0))
        before_t, before_c = dst.download_tsdf(), dst.download_color()
        f = PT.info(img)
        bad = bytearray(img)
        bad[f["at"][0] + 5] = 7
        for what, data in (("class byte", bytes(bad)), ("truncated", img[:-1]), ("header only", img[:256])):
            p = tmp_path / "bad.hskv"
            p.write_bytes(data)
            with pytest.raises(hsk.KinfuError, match="hskinfu error -1"):
                dst.load_volume(p)
            assert np.array_equal(dst.download_tsdf(), before_t) and np.array_equal(dst.download_color(), before_c), what
        with pytest.raises(hsk.KinfuError, match="hskinfu error -3"):
            dst.load_volume(tmp_path / "missing.hskv")
    finally:
        dst.close()
    made = hsk.KinfuTracker.from_volume_file(path)
    try:
        assert np.array_equal(made.download_tsdf(), tsdf) and np.array_equal(made.download_color(), col)
        assert np.array_equal(made.get_pose(), info["pose"])
        made.color_params = (64,)
        assert_same_image(made.pack_volume(), PT.pack(tsdf, col, ctx_fields(hsk, made)), "from_volume_file")
    finally:
        made.close()


# ---- 7. resume -------------------------------------------------------------------------------------------------------
K = 10   # frames 0..K, the save, frames K+1..2K of the scripted stream; 128^3 tracks all of them


def stream_frames(hsk):
    poses = [hsk.synth_pose(k) for k in range(2 * K + 1)]
    return [(hsk.synth_depth(p), hsk.synth_rgb(p)) for p in poses]


def feed(trk, frames, mode):
    out = []
    if mode == "sync":
        for d, c in frames:
            out.append(trk.process_frame_rgbd(d, c))
    else:
        for i, (d, c) in enumerate(frames):
            trk.submit_frame_rgbd(d, c)
            if i >= 2:
                out.append(trk.wait_frame())
        while len(out) < len(frames):
            out.append(trk.wait_frame())
    return out


@pytest.mark.parametrize("mode,use_graph", [("sync", 0), ("async", 0), ("sync", 1), ("async", 2)])
def test_resume_reproduces_the_uninterrupted_scan(hsk, tmp_path, mode, use_graph):
    frames = stream_frames(hsk)
    whole = with_color(hsk.KinfuTracker(n=N, use_graph=use_graph))
    try:
        want = feed(whole, frames, mode)
        assert all(ok for _, ok in want[1:]), [ok for _, ok in want]
        want_t, want_c = whole.download_tsdf(), whole.download_color()
    finally:
        whole.close()
    path = tmp_path / "half.hskv"
    first = with_color(hsk.KinfuTracker(n=N, use_graph=use_graph))
    try:
        got = feed(first, frames[:K + 1], mode)
        first.save_volume(path)
    finally:
        first.close()
    info = hsk.volume_file_info(path)
    assert np.array_equal(info["pose"], got[-1][0]) and info["frame"] == K + 1

    def second_half(resume):
        trk = with_color(hsk.KinfuTracker(n=N, use_graph=use_graph))
        try:
            trk.load_volume(path)
            if resume:
                trk.resume_scan(info["pose"])
            else:
                trk.raycast(info["pose"])
            res = feed(trk, frames[K + 1:], mode)
            return res, trk.download_tsdf(), trk.download_color()
        finally:
            trk.close()

    res, t, c = second_half(True)
    got = got + res
    for k, ((p, ok), (p0, ok0)) in enumerate(zip(got, want)):
        assert ok == ok0, f"frame {k}: tracked {ok} != {ok0}"
        assert np.array_equal(p.view(np.uint32), p0.view(np.uint32)), f"frame {k}: pose\n{p}\n{p0}"
    assert np.array_equal(t, want_t) and np.array_equal(c, want_c)
    # the gap this call closes: behind hsk_raycast the next frame is a FIRST frame (no ICP; it integrates at the given pose)
    res_n, _, _ = second_half(False)
    assert res_n[0][1] is False
    same = all(np.array_equal(p.view(np.uint32), p0.view(np.uint32)) for (p, _), (p0, _) in zip(res_n, want[K + 1:]))
    assert not same, "hsk_raycast alone reproduced the poses: the negative control does not bite"


# ---- 8. errors -------------------------------------------------------------------------------------------------------
def test_errors(hsk, tmp_path):
    lib = hsk._lib.load()
    trk = make_ctx(hsk, (64, 64, 64), color=False)
    depth = hsk.synth_depth(hsk.synth_pose(0))
    eye = np.eye(4, dtype=f32).reshape(16)
    fp = eye.ctypes.data_as(C.POINTER(C.c_float))
    n = C.c_size_t()
    try:
        trk.integrate(depth, hsk.synth_pose(0))
        img = trk.pack_volume()
        a = np.frombuffer(img, np.uint8)
        # NULLs
        assert lib.hsk_pack_volume(None, None, 0, C.byref(n), None) == -1 and lib.hsk_pack_volume(trk.h, None, 0, None, None) == -1
        assert lib.hsk_unpack_volume(None, a.ctypes.data, a.size) == -1 and lib.hsk_unpack_volume(trk.h, None, a.size) == -1
        assert lib.hsk_save_volume(None, b"x", None) == -1 and lib.hsk_save_volume(trk.h, None, None) == -1
        assert lib.hsk_load_volume(None, b"x") == -1 and lib.hsk_load_volume(trk.h, None) == -1
        assert lib.hsk_resume_scan(None, fp) == -1 and lib.hsk_resume_scan(trk.h, None) == -1
        # a frame in flight
        trk.submit_frame(depth)
        for call in (trk.pack_volume, lambda: trk.unpack_volume(img), lambda: trk.save_volume(tmp_path / "v.hskv"),
                     lambda: trk.load_volume(tmp_path / "v.hskv"), lambda: trk.resume_scan(eye)):
            with pytest.raises(hsk.KinfuError, match="in flight"):
                call()
        trk.wait_frame()
        # an unwritable path
        with pytest.raises(hsk.KinfuError, match="hskinfu error -3"):
            trk.save_volume(tmp_path / "no_such_dir" / "v.hskv")
        # mismatched dims, size, truncation distance
        for what, other in (("dims", make_ctx(hsk, (64, 64, 32), color=False)),
                            ("size_m", make_ctx(hsk, (64, 64, 64), (3.0, 3.0, 2.5), color=False)),
                            ("truncation", make_ctx(hsk, (64, 64, 64), color=False, trunc_dist_m=0.25))):
            try:
                before = other.download_tsdf()
                with pytest.raises(hsk.KinfuError, match=what):
                    other.unpack_volume(img)
                assert np.array_equal(other.download_tsdf(), before)
            finally:
                other.close()
    finally:
        trk.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(depth)
        for i in range(g.n_slabs()):
            s = g.slab(i)
            for call in (s.pack_volume, lambda: s.unpack_volume(img), lambda: s.resume_scan(eye)):
                with pytest.raises(hsk.KinfuError, match="hskinfu error -3"):
                    call()
        assert g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))[1]
    finally:
        g.close()
