"""The colour path where a cube and the default camera hide a mistake: k_color_integrate (housescan_amd/csrc/color.hip) and the
colour picks of the two read-outs (extract.hip) against tests/color_twin.py on ragged and flat volumes with a cell per axis,
a second camera with fx != fy whose 16-px tile table has a clipped last column and row, adversarial frames, crafted poses at
the chunk skip's edges, and the frame path with every parameter off its default.  Integer against integer: zero differing
voxels or points, no tolerance."""
import numpy as np
import pytest

import color_cases as CC
import color_twin as CT
from kit import same_bits
from np_twin import scale_depth, tau_of

pytestmark = pytest.mark.gpu
f32 = np.float32


def same_color(got, want, what):
    bad = np.argwhere((got != want).any(axis=3))
    assert len(bad) == 0, f"{what}: {len(bad)} voxels differ, first (z, y, x) {bad[:5].tolist()}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def random_tsdf(rng, dims):
    vol = rng.integers(-32767, 32768, size=(dims[2], dims[1], dims[0], 2)).astype(np.int16)
    vol[..., 1] = rng.integers(0, 129, size=vol.shape[:3])
    return vol


class Stage:
    """a context and the twin's volume side by side: every frame goes through hsk_integrate_color and the twin, the twin fed
    the scaled depth the device made (itself compared with the numpy restatement's, bit for bit)"""

    def __init__(self, hsk, rng, dims, size, cam, max_w):
        self.dims, self.size, self.cam = dims, size, cam
        self.trk = hsk.KinfuTracker(CC.tracker_config(hsk, dims, size, cam))
        self.trk.enable_color(max_w, 0.0)
        self.col = CC.random_color(rng, dims, max_w)
        self.trk.upload_color(self.col)
        assert np.array_equal(self.trk.download_color(), self.col)
        self.tsdf = random_tsdf(rng, dims)
        self.trk.upload_tsdf(self.tsdf)

    def frame(self, pose, depth, rgb, max_w, band_m, what):
        self.trk.enable_color(max_w, band_m)
        self.trk.integrate_color(depth, rgb, pose)
        scaled = self.trk.download_scaled_depth()
        assert np.array_equal(scaled.view(np.uint32), scale_depth(depth, *self.cam[2:]).view(np.uint32)), what
        n = CT.integrate_color(self.col, self.size, scaled, rgb, *self.cam[2:], pose, CT.band_of(self.dims, self.size, band_m, CC.TRUNC), max_w)
        same_color(self.trk.download_color(), self.col, what)
        return n

    def close(self):
        assert np.array_equal(self.trk.download_tsdf(), self.tsdf), "integrate_color must leave the TSDF alone"
        self.trk.close()


@pytest.mark.parametrize("seed", CC.SEEDS)
@pytest.mark.parametrize("camera", list(CC.CAMERAS))
@pytest.mark.parametrize("volume", list(CC.VOLUMES))
def test_integrate_color_fuzz(hsk, volume, camera, seed):
    """blocky depth with 1 mm and 65535 mm pixels, colour of independent random bytes, poses inside, outside, upside down and
    looking away, onto a random colour volume with weights 0, in between and capped; the band and the weight cap change with
    every frame.  The seeds (tests/color_cases.py) are chosen so that the twin alone meets the conditions below"""
    rng, dims, size, cam, max_w0, frames = CC.fuzz_case(volume, camera, seed)
    st = Stage(hsk, rng, dims, size, cam, max_w0)
    ns = [st.frame(pose, depth, rgb, max_w, band_m, f"{volume} {camera} seed {seed} frame {k}")
          for k, (pose, depth, rgb, max_w, band_m) in enumerate(frames)]
    st.close()
    ins = [CC.inside(f[0], size) for f in frames]
    print(f"{volume} {camera} seed {seed}: coloured per frame {ns}, camera inside {ins}")
    assert sum(ns) >= 5000 and sum(n > 0 for n in ns) >= 4, ns
    assert any(ins) and not all(ins), ins


def _pose(R, t):
    P = np.eye(4, dtype=f32)
    P[:3, :3] = np.asarray(R, f32)
    P[:3, 3] = np.asarray(t, f32)
    return P


def _turn(axis):
    """a quarter turn about an axis, its entries exactly 0 and +-1"""
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3, dtype=f32)
    R[i, i], R[i, j], R[j, i], R[j, j] = 0, -1, 1, 0
    return R


def _generic_rotation():
    a, b = np.radians(33.0), np.radians(-21.0)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    return Ry @ Rx


@pytest.mark.parametrize("camera", list(CC.CAMERAS))
def test_integrate_color_crafted_poses(hsk, camera):
    """the ragged volume from poses at the edges of the chunk skip: camera-space depth exactly 0 on a whole plane of voxels that
    holds chunk corners (the `front` test; 1 / 0 in the corners' projection); a chunk that straddles z = 0; a chunk face 0.04 m
    and 0.06 m ahead, either side of the gate at 0.05 m; a camera looking away; one 1 000 m off; a frame without depth"""
    dims, size = CC.VOLUMES["ragged"]
    cam = CC.CAMERAS[camera]
    W, H = cam[:2]
    rng = np.random.default_rng(77)
    st = Stage(hsk, rng, dims, size, cam, 64)
    cell = [f32(size[i]) / f32(dims[i]) for i in range(3)]
    # the centre of voxel (32, 16, 16), the first of a chunk on every axis, by the kernel's own expression: g is exactly 0 there
    on_centre = [(f32(v) + f32(0.5)) * cell[i] for i, v in enumerate((32, 16, 16))]
    xy = [f32(1.31), f32(0.87)]
    face = (f32(16) + f32(0.5)) * cell[2]   # the first plane of voxel centres of the chunks from z = 16 on
    inside = [f32(40.3) * cell[0], f32(24.7) * cell[1], f32(20.4) * cell[2]]
    default, thin, capped = CC.COLOR_PARAMS
    poses = [("identity on a voxel centre", _pose(np.eye(3), on_centre), default),
             ("quarter turn about x on a voxel centre", _pose(_turn(0), on_centre), default),
             ("quarter turn about y on a voxel centre", _pose(_turn(1), on_centre), default),
             ("quarter turn about z on a voxel centre", _pose(_turn(2), on_centre), default),
             ("inside a chunk", _pose(_generic_rotation(), inside), default),
             ("inside a chunk, thin band", _pose(_generic_rotation().T, inside), thin),
             ("0.04 m before a chunk face", _pose(np.eye(3), xy + [face - f32(0.04)]), default),
             ("0.06 m before a chunk face", _pose(np.eye(3), xy + [face - f32(0.06)]), default),
             ("far away", _pose(np.eye(3), [f32(size[0] / 2), f32(size[1] / 2), f32(-1000.0)]), capped)]
    ns = {}
    for name, pose, (max_w, band_m) in poses:
        ns[name] = st.frame(pose, CC.random_depth(rng, H, W), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8), max_w, band_m, name)
    print(f"{camera}: coloured {ns}")
    assert all(ns[p[0]] > 0 for p in poses[:5]), ns
    assert ns["0.04 m before a chunk face"] > 0 and ns["0.06 m before a chunk face"] > 0, ns
    # a whole plane of voxels really is at camera-space depth 0 in the first four
    g = [np.arange(dims[i], dtype=f32) + f32(0.5) for i in range(3)]
    for i in range(3):
        assert ((g[i] * cell[i] - on_centre[i]) == 0).sum() == 1
    before = st.col.copy()
    away = _pose(np.diag([1.0, -1.0, -1.0]), [f32(size[0] / 2), f32(size[1] / 2), f32(-0.5)])   # in front of z = 0, looking along -z
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    assert st.frame(away, CC.random_depth(rng, H, W), rgb, 64, 0.0, "looking away") == 0
    assert st.frame(poses[4][1], np.zeros((H, W), np.uint16), rgb, 64, 0.0, "no depth") == 0
    assert np.array_equal(st.trk.download_color(), before)
    st.close()


@pytest.mark.parametrize("camera", list(CC.CAMERAS))
def test_band_is_open_at_both_ends(hsk, camera):
    """band_m set to the very sdf of a voxel, once from in front of the surface and once from behind it: sdf == band and
    sdf == -band are outside the band, and the voxel keeps its colour (a `<=` would take it)"""
    from np_twin import _project
    dims, size = CC.VOLUMES["ragged"]
    cam = CC.CAMERAS[camera]
    W, H = cam[:2]
    rng = np.random.default_rng(78)
    st = Stage(hsk, rng, dims, size, cam, 64)
    pose = _pose(_generic_rotation(), [f32(1.1), f32(0.8), f32(0.3)])
    depth = CC.random_depth(rng, H, W)
    rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    ok, _, _, Ds, sdf, _, _, _ = _project(dims, size, scale_depth(depth, *cam[2:]), *cam[2:], pose, 0)
    seen = ok & (Ds != 0)
    for sign in (1.0, -1.0):
        at = np.argwhere(seen & (sdf * f32(sign) > f32(0.02)) & (sdf * f32(sign) < f32(0.06)))
        assert len(at) > 20
        z, y, x = at[len(at) // 2]
        band_m = float(sdf[z, y, x] * f32(sign))
        before = st.col[z, y, x].copy()
        assert st.frame(pose, depth, rgb, 64, band_m, f"band = {sign:+.0f} sdf of voxel {(x, y, z)}") > 20
        assert np.array_equal(st.col[z, y, x], before)
    st.close()


def test_tracker_color_with_every_parameter_off_its_default(hsk):
    """test_gpu_configs.py's configuration with every field off its default (160 x 96 x 200 voxels over 3.0 x 2.4 x 3.2 m,
    320 x 240, fx != fy, an off-centre principal point, its own start pose), colour enabled, ten RGB-D frames: synchronously,
    pipelined, and pipelined from captured graphs.  The colour volume is the twin's, replayed with the poses and verdicts the
    device returned; TSDF and poses are those of a depth-only run"""
    W, H = 320, 240
    fx, fy, cx, cy = 262.5 * 1.04, 262.5 * 0.97, W / 2 - 0.5 + 3.25, H / 2 - 0.5 - 2.5
    dims, size, trunc = (160, 96, 200), (3.0, 2.4, 3.2), 0.07
    start = hsk.synth_pose(0).copy()
    start[:3, 3] += np.array([0.02, -0.03, 0.01], np.float32)
    kw = dict(trunc_dist_m=trunc, icp_iters=(6, 3, 2), icp_dist_thresh_m=0.07, icp_angle_thresh_sin=float(np.sin(np.radians(15.0))),
              init_pose=start)
    frames = [(hsk.synth_depth(hsk.synth_pose(2 * k), W, H, fx, fy, cx, cy), hsk.synth_rgb(hsk.synth_pose(2 * k), -1, W, H, fx, fy, cx, cy))
              for k in range(10)]

    def make(use_graph, color):
        trk = hsk.KinfuTracker(CC.tracker_config(hsk, dims, size, (W, H, fx, fy, cx, cy), use_graph=use_graph, **kw))
        if color:
            trk.enable_color()
        return trk

    plain = make(0, False)
    want = [plain.process_frame(d) for d, _ in frames]
    tsdf = plain.download_tsdf()
    plain.close()
    assert sum(ok for _, ok in want) >= 8
    col = np.zeros((dims[2], dims[1], dims[0], 4), np.uint8)
    band = CT.band_of(dims, size, 0.0, trunc)
    assert band == f32(2.0) * (f32(size[1]) / f32(dims[1])) < tau_of(size, dims, trunc)
    for k, ((depth, rgb), (pose, ok)) in enumerate(zip(frames, want)):
        if ok or k == 0:  # frame 0 integrates at the start pose; every tracked frame integrates (no gate)
            CT.integrate_color(col, size, scale_depth(depth, fx, fy, cx, cy), rgb, fx, fy, cx, cy, pose, band, 64)
    assert (col[..., 3] > 0).sum() > 10000
    for use_graph, mode in [(0, "sync"), (0, "async"), (2, "async")]:
        trk = make(use_graph, True)
        got = []
        if mode == "sync":
            got = [trk.process_frame_rgbd(d, c) for d, c in frames]
        else:
            for i, (d, c) in enumerate(frames):
                trk.submit_frame_rgbd(d, c)
                if i >= 1:
                    got.append(trk.wait_frame())
            got.append(trk.wait_frame())
        for k, ((p, ok), (p0, ok0)) in enumerate(zip(got, want)):
            assert ok == ok0 and np.array_equal(p.view(np.uint32), p0.view(np.uint32)), (use_graph, mode, k)
        assert np.array_equal(trk.download_tsdf(), tsdf), (use_graph, mode, "colour must not change the TSDF")
        same_color(trk.download_color(), col, f"use_graph {use_graph} {mode}")
        trk.close()


def test_readouts_pick_color_in_a_volume_with_a_cell_per_axis(hsk, oracle):
    """the alignment tests' scene at 80 x 64 x 48 (a cell per axis; the colour volume's row pitch is not its plane pitch) under a
    random colour volume with 45 % of the weights and one whole z slab of them 0: the cloud's and the indexed mesh's colours,
    normals and uncoloured counts against the twins, with many picks that fall through to the edge's other end and many
    edges with no colour at all"""
    import align_twin as AT
    import mesh_twin as MT
    X, Y, Z = AT.DST_DIMS
    rng = np.random.default_rng(5)
    vol = AT.scene_volume(AT.DST_DIMS, AT.DST_SIZE, tau_of(AT.DST_SIZE, AT.DST_DIMS, 0.03))
    col = rng.integers(0, 256, size=(Z, Y, X, 4), dtype=np.uint8)
    col[..., 3] = rng.integers(1, 256, size=(Z, Y, X))
    col[..., 3][rng.random((Z, Y, X)) < 0.45] = 0
    col[20, :, :, 3] = 0
    trk = hsk.KinfuTracker(CC.tracker_config(hsk, AT.DST_DIMS, AT.DST_SIZE, CC.CAMERAS["vga"]))
    trk.enable_color()
    trk.upload_tsdf(vol)
    trk.upload_color(col)
    t = vol[..., 0].astype(np.int32)

    def census(a, b):
        first, other, pick = CT.pick_color(t, col, a, b)
        return int(((first[:, 3] == 0) & (other[:, 3] != 0)).sum()), int((pick[:, 3] == 0).sum())

    # the cloud
    xyz, nrm, rgb, total, unc = trk.extract_cloud_attrs()
    want_n, want_rgb, want_unc = CT.np_attrs(vol, col, xyz, AT.DST_SIZE)
    assert total == len(xyz) > 5000
    assert MT.same_normals(nrm, want_n) and (~np.isnan(want_n[:, 0])).sum() > 0.8 * total
    bad = np.argwhere((rgb != want_rgb).any(axis=1))
    assert len(bad) == 0, f"cloud: {len(bad)} of {total} colours differ, first points {bad[:5, 0].tolist()}"
    assert unc == want_unc
    z, y, x, _, bz, by, bx = CT.cut_edges(vol)
    second, none = census((z, y, x), (bz, by, bx))
    print(f"cloud: {total} points, {second} picks from the second end, {none} uncoloured")
    assert second >= 500 and none >= 500 and none == want_unc
    # the indexed mesh
    v, f, mn, mrgb, munc = trk.extract_mesh_indexed()
    ntri, codes = oracle.mc_table()
    with np.errstate(all="ignore"):
        tw = MT.mesh_indexed(vol, ntri, codes, size=AT.DST_SIZE, col=col)
    assert same_bits(v, tw["vertices"]) and np.array_equal(f, tw["faces"]) and len(f) > 5000
    assert MT.same_normals(mn, tw["normals"])
    bad = np.argwhere((mrgb != tw["rgb"]).any(axis=1))
    assert len(bad) == 0, f"mesh: {len(bad)} of {len(v)} colours differ, first vertices {bad[:5, 0].tolist()}"
    assert munc == tw["n_uncolored"]
    e = tw["edges"]
    a = (e[:, 0], e[:, 1], e[:, 2])
    b = (e[:, 0] + (e[:, 3] == 2), e[:, 1] + (e[:, 3] == 1), e[:, 2] + (e[:, 3] == 0))
    second, none = census(a, b)
    print(f"mesh: {len(v)} vertices, {second} picks from the second end, {none} uncoloured")
    assert second >= 500 and none >= 500 and none == tw["n_uncolored"]
    trk.close()
