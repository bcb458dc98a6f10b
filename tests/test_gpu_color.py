"""RGB-D colour and the cloud with normals and colour, on the GPU: the colour update bit-exact against a numpy restatement
built on the integrate's projection (tests/np_twin.py), through every frame path; the read-out bit-exact against the
downloaded volumes; and what a scanned room looks like."""
import os

import numpy as np
import pytest

from color_cases import frame_of, run_tracker
from color_twin import band_of, integrate_color, np_attrs
from np_twin import _Grid, scale_depth, tau_of

pytestmark = pytest.mark.gpu
f32 = np.float32
FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5
SIZE3 = (3.0, 3.0, 3.0)


def cube_band(n, band_m):
    return band_of((n, n, n), SIZE3, band_m, 0.03)


def cube_color(col, scaled, rgb, pose, band, max_w):
    """one frame's colour update of a cubic volume over 3 m, from the default camera (tests/color_twin.py)"""
    return integrate_color(col, SIZE3, scaled, rgb, FX, FY, CX, CY, pose, band, max_w)


def random_color(rng, n, max_w):
    col = rng.integers(0, 256, size=(n, n, n, 4), dtype=np.uint8)
    col[..., 3] = rng.integers(0, max_w + 1, size=(n, n, n))
    col[..., 3][rng.random((n, n, n)) < 0.1] = max_w  # some already capped
    return col


@pytest.mark.parametrize("n,src,band_m,max_w", [(64, "synth", 0.0, 64), (64, "room", 0.01, 1), (128, "synth", 0.02, 255),
                                                (128, "room", 0.0, 1), (256, "synth", 0.0, 64)])
def test_integrate_color_stage_bitexact(hsk, n, src, band_m, max_w):
    rng = np.random.default_rng(n + max_w)
    trk = hsk.KinfuTracker(n=n)
    trk.enable_color(max_w, band_m)
    col = random_color(rng, n, max_w)
    trk.upload_color(col)
    assert np.array_equal(trk.download_color(), col)
    tsdf0 = trk.download_tsdf()
    band = cube_band(n, band_m)
    for k in (3, 9):
        pose, depth, rgb = frame_of(hsk, src, k)
        trk.integrate_color(depth, rgb, pose)
        scaled = trk.download_scaled_depth()
        assert np.array_equal(scaled.view(np.uint32), scale_depth(depth, FX, FY, CX, CY).view(np.uint32))
        cube_color(col, scaled, rgb, pose, band, max_w)
        got = trk.download_color()
        bad = np.argwhere((got != col).any(axis=3))
        assert len(bad) == 0, f"{len(bad)} voxels differ, first {bad[:5].tolist()}"
    assert np.array_equal(trk.download_tsdf(), tsdf0), "integrate_color must leave the TSDF alone"
    trk.close()


def replay(n, frames, results, max_w=64):
    col = np.zeros((n, n, n, 4), np.uint8)
    for k, ((_, depth, rgb), (pose, ok)) in enumerate(zip(frames, results)):
        if ok or k == 0:  # frame 0 integrates at the initial pose; every tracked frame integrates (no gate)
            cube_color(col, scale_depth(depth, FX, FY, CX, CY), rgb, pose, cube_band(n, 0.0), max_w)
    return col


@pytest.mark.parametrize("n", [128, 256])
def test_tracker_color_bitexact(hsk, n):
    frames = [frame_of(hsk, "synth", k) for k in range(30)]
    trk, res = run_tracker(hsk, n, frames)
    ref, res0 = run_tracker(hsk, n, frames, color=False)
    assert all(ok for _, ok in res[1:])
    for (p, ok), (p0, ok0) in zip(res, res0):
        assert ok == ok0 and np.array_equal(p.view(np.uint32), p0.view(np.uint32))
    assert np.array_equal(trk.download_tsdf(), ref.download_tsdf()), "colour must not change the TSDF"
    got = trk.download_color()
    want = replay(n, frames, res)
    bad = np.argwhere((got != want).any(axis=3))
    assert len(bad) == 0, f"{len(bad)} voxels differ, first {bad[:5].tolist()}"
    assert (got[..., 3] > 0).sum() > 10000
    trk.close()
    ref.close()


def test_paths_agree(hsk):
    n = 128
    frames = [frame_of(hsk, "synth", k) for k in range(12)]
    base, res = run_tracker(hsk, n, frames)
    want = base.download_color()
    assert np.array_equal(want, replay(n, frames, res))
    tsdf = base.download_tsdf()
    for use_graph, mode, prof in [(1, "sync", False), (2, "sync", False), (0, "async", False), (2, "async", False), (0, "sync", True)]:
        trk, r = run_tracker(hsk, n, frames, use_graph=use_graph, mode=mode, profile=prof)
        assert [ok for _, ok in r] == [ok for _, ok in res]
        assert np.array_equal(trk.download_color(), want), (use_graph, mode, prof)
        assert np.array_equal(trk.download_tsdf(), tsdf), (use_graph, mode, prof)
        trk.close()
    base.close()


@pytest.mark.parametrize("use_graph", [0, 1, 2])
def test_depth_only_frames_leave_color(hsk, use_graph):
    n = 64
    frames = [frame_of(hsk, "synth", k) for k in range(10)]
    trk = hsk.KinfuTracker(n=n, use_graph=use_graph)
    trk.enable_color()
    results = []
    for k, (pose, depth, rgb) in enumerate(frames):
        if k % 3 == 2:
            before = trk.download_color()
            results.append((trk.process_frame(depth), False))
            assert np.array_equal(trk.download_color(), before), f"depth-only frame {k} changed the colour"
        else:
            results.append((trk.process_frame_rgbd(depth, rgb), True))
    # pipelined depth-only frames, then a coloured one
    before = trk.download_color()
    trk.submit_frame(frames[-1][1])
    trk.submit_frame(frames[-1][1])
    assert trk.wait_frame()[1] and trk.wait_frame()[1]
    assert np.array_equal(trk.download_color(), before)
    # the whole run against the rule applied to the coloured frames only
    col = np.zeros((n, n, n, 4), np.uint8)
    for k, (((_, depth, rgb)), ((pose, ok), colored)) in enumerate(zip(frames, results)):
        if colored and (ok or k == 0):
            cube_color(col, scale_depth(depth, FX, FY, CX, CY), rgb, pose, cube_band(n, 0.0), 64)
    assert np.array_equal(before, col)
    trk.close()


def test_loss_zeroes_color(hsk):
    n = 64
    trk = hsk.KinfuTracker(n=n)
    trk.enable_color()
    f = [frame_of(hsk, "synth", k) for k in range(4)]
    trk.process_frame_rgbd(f[0][1], f[0][2])
    trk.process_frame_rgbd(f[1][1], f[1][2])
    assert trk.download_color().any()
    blank = np.zeros_like(f[0][1])
    _, tracked = trk.process_frame_rgbd(blank, f[2][2])
    assert not tracked
    assert not trk.download_tsdf().any() and not trk.download_color().any()
    # pipelined: a lost frame, and one dropped in flight behind it.  Both have run on the device before the host collects them
    # (and resets): the volumes, read in between, show that neither coloured nor integrated -- the kernels' own `lost` test
    trk.submit_frame_rgbd(f[0][1], f[0][2])
    trk.submit_frame_rgbd(f[1][1], f[1][2])
    assert trk.wait_frame()[1] is False and trk.wait_frame()[1] is True
    col1, tsdf1 = trk.download_color(), trk.download_tsdf()
    assert col1.any()
    trk.submit_frame_rgbd(blank, f[2][2])
    trk.submit_frame_rgbd(f[2][1], f[2][2])
    trk.synchronize()
    assert np.array_equal(trk.download_color(), col1), "a lost frame, or one dropped behind it, coloured"
    assert np.array_equal(trk.download_tsdf(), tsdf1)
    p1, t1 = trk.wait_frame()
    p2, t2 = trk.wait_frame()
    assert not t1 and not t2
    assert not trk.download_tsdf().any() and not trk.download_color().any()
    # the restarted scan colours as a fresh one
    r = [trk.process_frame_rgbd(d, c) for _, d, c in f[:3]]
    assert np.array_equal(trk.download_color(), replay(n, f[:3], r))
    # hsk_reset zeroes it as well
    trk.reset()
    assert not trk.download_color().any()
    trk.close()


def test_extract_cloud_attrs_bitexact(hsk, tmp_path):
    n = 128
    frames = [frame_of(hsk, "synth", k) for k in range(15)]
    trk, _ = run_tracker(hsk, n, frames)
    xyz0, total0 = trk.extract_cloud()
    xyz, nrm, rgb, total, unc = trk.extract_cloud_attrs()
    assert total == total0 and total > 1000
    assert np.array_equal(xyz.view(np.uint32), xyz0.view(np.uint32))
    tsdf, col = trk.download_tsdf(), trk.download_color()
    want_n, want_rgb, want_unc = np_attrs(tsdf, col, xyz)
    assert np.array_equal(np.isnan(nrm), np.isnan(want_n))
    assert np.array_equal(nrm[~np.isnan(nrm)].view(np.uint32), want_n[~np.isnan(want_n)].view(np.uint32))
    assert (~np.isnan(nrm[:, 0])).sum() > 0.9 * total
    assert np.array_equal(rgb, want_rgb) and unc == want_unc
    # NULL attribute pointers; a capped read; normals without colour on a context without it
    x2, n2, r2, _, _ = trk.extract_cloud_attrs(normals=False, rgb=False)
    assert n2 is None and r2 is None and np.array_equal(x2.view(np.uint32), xyz.view(np.uint32))
    x3, n3, r3, _, _ = trk.extract_cloud_attrs(cap=100)
    assert np.array_equal(x3, xyz[:100]) and np.array_equal(r3, rgb[:100]) and np.array_equal(n3[~np.isnan(n3)], nrm[:100][~np.isnan(nrm[:100])])
    plain, _ = run_tracker(hsk, n, frames, color=False)
    with pytest.raises(hsk.KinfuError):
        plain.extract_cloud_attrs()
    xp, npl, _, _, _ = plain.extract_cloud_attrs(rgb=False)
    assert np.array_equal(xp.view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(np.isnan(npl), np.isnan(nrm)) and np.array_equal(npl[~np.isnan(npl)], nrm[~np.isnan(nrm)])
    for call in (lambda: plain.process_frame_rgbd(frames[0][1], frames[0][2]), lambda: plain.submit_frame_rgbd(frames[0][1], frames[0][2]),
                 lambda: plain.integrate_color(frames[0][1], frames[0][2], frames[0][0]), plain.download_color):
        with pytest.raises(hsk.KinfuError):
            call()
    # the room directory: cloud_bin.pcd parses back to the extracted arrays
    from housescan_amd import products
    from color_cases import read_pcd_xyzrgbnormal
    d = str(tmp_path / "room")
    products.write_room_dir(d, xyz, cloud_rgb=rgb, cloud_normals=nrm)
    _, xb, bits, nb, _ = read_pcd_xyzrgbnormal(os.path.join(d, "cloud_bin.pcd"))
    assert np.array_equal(xb.view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(bits, (rgb[:, 0].astype(np.uint32) << 16) | (rgb[:, 1].astype(np.uint32) << 8) | rgb[:, 2])
    assert np.array_equal(nb.view(np.uint32), nrm.view(np.uint32))
    trk.close()
    plain.close()


def test_extract_cloud_attrs_normals_with_three_different_cells(hsk):
    """the alignment tests' scene, 80 x 64 x 48 over 3 m -- a cell per axis, a row pitch that is not the plane pitch: the normals
    against mesh_twin.normal_at bit for bit, with samples whose lower tap is the last voxel of a 64-B block in x and in z"""
    import align_twin as AT
    import fuse_twin as FT
    import mesh_twin as MT
    X, Y, Z = AT.DST_DIMS
    vol = AT.scene_volume(AT.DST_DIMS, AT.DST_SIZE, tau_of(AT.DST_SIZE, AT.DST_DIMS, 0.03))
    trk = hsk.KinfuTracker(hsk.default_config(Z, vol_x=X, vol_y=Y, vol_z=Z, vol_size_m=AT.DST_SIZE, own_z1=Z))
    trk.upload_tsdf(vol)
    xyz, nrm, _, total, _ = trk.extract_cloud_attrs(rgb=False)
    trk.close()
    G = _Grid(vol, AT.DST_SIZE, Z, 0)
    with np.errstate(all="ignore"):
        want = MT.normal_at(G, xyz, AT.DST_DIMS)
    deep = ~np.isnan(want[:, 0])
    assert total == len(xyz) > 5000 and deep.sum() > 0.8 * total
    assert MT.same_normals(nrm, want)
    # the lower taps of the samples one cell either side in x and in z, by the fusion twin's arithmetic
    for axis in (0, 2):
        p = [xyz[deep, i].copy() for i in range(3)]
        p[axis] = (p[axis] + G.cell[axis]).astype(f32)
        vox = FT.sample(vol, AT.DST_SIZE, p)[3][axis]
        low = vox - (p[axis] < ((vox.astype(f32) + f32(0.5)) * G.cell[axis]).astype(f32))
        assert ((low & 3) == 3).sum() > 200, axis


def test_room_scan_physical(hsk):
    """room 0 as a sensor sees it (holes, noise), synthetic colour, 256^3: the colours of the cloud against the colour of the
    scene at the point, the normals against the walls'.  Wall points near another wall (within 3 cells: corners and edges,
    where the TSDF's gradient mixes two planes) are left out.  Measured on the first run (150 frames): every coloured point
    within 16 levels (median 2); of the points within 5 mm of a wall, 90.6 / 96.7 / 97.4 / 97.5 % have their normal within
    10 deg (median 1.7 .. 2.3 deg).  The rest is geometry, not noise: the same scan without sensor noise leaves 8.7 % of wall
    0/0's points beyond 10 deg (median 0.5 deg) -- furniture standing against the wall puts points of its own faces, and of
    the junction the TSDF rounds off, within 5 mm of the wall's plane.  So the wall test asks for 88 % within 10 deg and a
    median under 3 deg, not for every point (DESIGN.md "Colour")."""
    n, scan, count = 256, 720, 150
    poses, frames = hsk.synth_sensor_frames(count, room=0, scan=scan)
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    trk.enable_color()
    tracked = []
    trk.submit_frame_rgbd(frames[0], hsk.synth_rgb(poses[0], 0))
    for k in range(1, count):
        trk.submit_frame_rgbd(frames[k], hsk.synth_rgb(poses[k], 0))
        tracked.append(trk.wait_frame()[1])
    tracked.append(trk.wait_frame()[1])
    assert all(tracked[1:]), "the room scan must stay tracked"
    xyz, nrm, rgb, total, unc = trk.extract_cloud_attrs()
    colored = (rgb != 0).any(axis=1)
    assert colored.sum() > 0.9 * total, (colored.sum(), total, unc)
    want = np.rint(128.0 + 100.0 * np.sin(2.0 * np.pi * xyz.astype(np.float64) / 1.2))
    err = np.abs(rgb.astype(np.float64) - want).max(axis=1)[colored]
    share = (err <= 16).mean()
    assert share >= 0.98, f"only {share:.4f} of the coloured points within 16 levels (median error {np.median(err)})"
    e = hsk.synth_room_extents(0)
    cell = 3.0 / n
    checked = 0
    for ax in range(3):
        for side, into in ((0, 1.0), (1, -1.0)):
            plane = e[2 * ax + side]
            near = np.abs(xyz[:, ax] - plane) < 0.005
            for other in range(3):
                if other != ax:
                    near &= (np.abs(xyz[:, other] - e[2 * other]) > 3 * cell) & (np.abs(xyz[:, other] - e[2 * other + 1]) > 3 * cell)
            near &= ~np.isnan(nrm[:, 0])
            if near.sum() < 50:
                continue
            ang = np.degrees(np.arccos(np.clip(nrm[near, ax] * into, -1.0, 1.0)))
            good = (ang <= 10.0).mean()
            assert good >= 0.88, f"wall {ax}/{side}: {good:.4f} of {near.sum()} normals within 10 deg"
            assert np.median(ang) < 3.0, f"wall {ax}/{side}: median angle {np.median(ang):.2f} deg"
            checked += 1
    assert checked >= 3
    trk.close()


@pytest.mark.parametrize("devices", [(0, 0), (0,)])
def test_slab_refuses_color(hsk, devices):
    """a slab of a group refuses colour -- also the one slab of a one-slab group, which owns the whole volume"""
    g = hsk.KinfuGroup(n=64, device_ids=devices)
    for i in range(g.n_slabs()):
        with pytest.raises(hsk.KinfuError):
            g.slab(i).enable_color()
    g.close()


def test_gated_frames_color_when_they_integrate(hsk):
    """integrate_move_thresh > 0: the host's gate decides per frame, and colour follows the integrate.  Repeated frames barely
    move, so the gate skips them; which frames integrated is read off the TSDF (it changes exactly when one does)"""
    n = 64
    seq = [0, 1, 2, 2, 2, 3, 4, 4, 5, 6, 6, 6, 7]
    frames = [frame_of(hsk, "synth", k) for k in seq]
    trk = hsk.KinfuTracker(n=n, integrate_move_thresh=0.002)
    trk.enable_color()
    col = np.zeros((n, n, n, 4), np.uint8)
    prev = trk.download_tsdf()
    integrated = []
    for k, (_, depth, rgb) in enumerate(frames):
        pose, ok = trk.process_frame_rgbd(depth, rgb)
        assert ok or k == 0
        cur = trk.download_tsdf()
        did = not np.array_equal(cur, prev)
        integrated.append(did)
        prev = cur
        if did:
            cube_color(col, scale_depth(depth, FX, FY, CX, CY), rgb, pose, cube_band(n, 0.0), 64)
        assert np.array_equal(trk.download_color(), col), f"frame {k} (integrated: {did})"
    assert integrated[0] and any(integrated[1:]) and not all(integrated), integrated
    trk.close()


@pytest.mark.parametrize("use_graph,mode", [(1, "sync"), (2, "async"), (2, "sync")])
def test_enable_after_graph_capture(hsk, use_graph, mode):
    """colour enabled after the frame chain was captured without it: the graphs are captured again, with the colour launch"""
    n = 64
    frames = [frame_of(hsk, "synth", k) for k in range(10)]
    trk = hsk.KinfuTracker(n=n, use_graph=use_graph)
    for _, depth, _ in frames[:4]:
        if mode == "sync":
            assert trk.process_frame(depth)[1] or depth is frames[0][1]
        else:
            trk.submit_frame(depth)
            trk.wait_frame()
    trk.enable_color()
    assert not trk.download_color().any()
    res = []
    rest = frames[4:]
    if mode == "sync":
        res = [trk.process_frame_rgbd(d, c) for _, d, c in rest]
    else:
        for i, (_, d, c) in enumerate(rest):
            trk.submit_frame_rgbd(d, c)
            if i >= 1:
                res.append(trk.wait_frame())
        res.append(trk.wait_frame())
    assert all(ok for _, ok in res)
    col = np.zeros((n, n, n, 4), np.uint8)
    for (_, d, c), (pose, _) in zip(rest, res):
        cube_color(col, scale_depth(d, FX, FY, CX, CY), c, pose, cube_band(n, 0.0), 64)
    assert np.array_equal(trk.download_color(), col)
    trk.close()
