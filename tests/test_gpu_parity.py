"""GPU parity tests proper: HIP kernels (through the C ABI) vs the CPU oracle on the same seeded inputs.

Bar: bit-exact for the int16 TSDF, the uint16 depth pyramid, the float maps (compared as bit patterns, NaN
included), the 27 ICP sums (exact by the 2^-26 snapping) and the float poses.
"""
import os

import numpy as np
import pytest

from kit import ROOT, assert_same_bits
from parity_cases import _lookat_pose, _random_depth, _random_pose

pytestmark = pytest.mark.gpu
# The fuzz tests hold two assertions about what the suite's OWN seeds happen to produce (so many updates, so many lost
# frames): they show that the seeds exercise what they are meant to, and say nothing about parity.  tools/fuzz_campaign.py,
# which runs the same tests over hundreds of other seeds, switches them off -- so that every parity comparison behind them
# still runs for every seed (a seed that tripped the expectation used to leave its volume and its pipelined run unchecked).
SEED_EXPECTATIONS = True


@pytest.mark.parametrize("n", [64, 128, 256, 512])   # 512: the headline size, every voxel compared
def test_integrate_bit_exact(hsk, oracle, synth_frames, n):
    cfg_o = oracle.default_config(n)
    trk = hsk.KinfuTracker(n=n)
    vol = np.zeros((n, n, n, 2), np.int16)
    for k in (0, 7, 14, 21):
        pose, depth = synth_frames(k)
        scaled = oracle.scale_depth(cfg_o, depth)
        n_upd = oracle.integrate(cfg_o, vol, scaled, pose)
        assert trk.count_updates(depth, pose) == n_upd
        trk.integrate(depth, pose)
        assert_same_bits(trk.download_scaled_depth(), scaled, "scaled depth")
        assert_same_bits(trk.download_tsdf(), vol, f"tsdf after frame {k}")
    assert (vol[..., 1] > 0).sum() > 0.1 * n ** 3
    trk.close()


def test_integrate_ragged_and_empty(hsk, oracle, synth_frames):
    """edge cases: all-zero depth (nothing updated), non-cubic volume, camera inside the volume looking away"""
    n = 64
    cfg_o = oracle.default_config(n, vol=(64, 32, 96), size=(3.0, 1.5, 4.5))
    trk = hsk.KinfuTracker(hsk.default_config(n, vol_y=32, vol_z=96, vol_size_m=(3.0, 1.5, 4.5), own_z1=96))
    vol = np.zeros((96, 32, 64, 2), np.int16)
    pose, depth = synth_frames(3)
    zero = np.zeros_like(depth)
    assert trk.count_updates(zero, pose) == 0
    trk.integrate(zero, pose)
    assert not trk.download_tsdf().any()
    for p in (pose, np.array([[-1, 0, 0, 1.5], [0, 1, 0, 0.7], [0, 0, -1, 1.0], [0, 0, 0, 1]], np.float32)):
        n_upd = oracle.integrate(cfg_o, vol, oracle.scale_depth(cfg_o, depth), p)
        assert trk.count_updates(depth, p) == n_upd
        trk.integrate(depth, p)
        assert_same_bits(trk.download_tsdf(), vol, "tsdf (ragged volume)")
    trk.close()


@pytest.mark.parametrize("seed", range(9))
def test_integrate_and_raycast_fuzz(hsk, oracle, seed):
    """random blocky depth images and arbitrary camera poses (inside / outside the volume, looking anywhere) into a cubic
    and a non-cubic volume: TSDF, update counts and the raycast of the result bit-exact against the oracle"""
    rng = np.random.default_rng(1000 + seed)
    if seed % 3 == 0:
        n, shape, kw_o, kw_h = 128, (128, 128, 128), {}, {}
    elif seed % 3 == 1:
        n, shape = 64, (96, 160, 64)     # (z, y, x)
        kw_o = dict(vol=(64, 160, 96), size=(1.5, 3.75, 2.25))
        kw_h = dict(vol_y=160, vol_z=96, vol_size_m=(1.5, 3.75, 2.25), own_z1=96)
    else:
        # x not a multiple of a wave's 64 voxels, y not of a workgroup's 16 rows, z of neither 4 nor 8 planes: partial
        # footprints, partial lane-blocks at the top of the volume
        n, shape = 72, (50, 40, 72)
        kw_o = dict(vol=(72, 40, 50), size=(2.7, 1.5, 1.875))
        kw_h = dict(vol_y=40, vol_z=50, vol_size_m=(2.7, 1.5, 1.875), own_z1=50)
    cfg_o = oracle.default_config(n, **kw_o)
    trk = hsk.KinfuTracker(hsk.default_config(n, **kw_h)) if kw_h else hsk.KinfuTracker(n=n)
    size = np.array(kw_o.get("size", (3.0, 3.0, 3.0)))
    vol = np.zeros(shape + (2,), np.int16)
    total = 0
    for k in range(8):
        pose = (_lookat_pose if k % 2 else _random_pose)(rng, size / 2, size * (0.9 if k % 4 >= 2 else 0.4))
        depth = _random_depth(rng)
        n_upd = oracle.integrate(cfg_o, vol, oracle.scale_depth(cfg_o, depth), pose)
        assert trk.count_updates(depth, pose) == n_upd
        trk.integrate(depth, pose)
        assert_same_bits(trk.download_tsdf(), vol, f"tsdf, seed {seed} frame {k}")
        total += n_upd
    if SEED_EXPECTATIONS:
        assert total > 30000
    for k in range(3):
        pose = (_lookat_pose if k else _random_pose)(rng, size / 2, size * 0.5)
        vm, nm, keys = trk.raycast(pose, want_keys=True)
        ovm, onm, okeys, _ = oracle.raycast(cfg_o, vol, pose)
        assert np.array_equal(keys, okeys)
        assert_same_bits(vm, ovm, "raycast vmap (fuzz)")
        assert_same_bits(nm, onm, "raycast nmap (fuzz)")
    trk.close()


def test_weight_saturates_at_128(hsk, oracle, synth_frames):
    n = 32
    cfg_o = oracle.default_config(n)
    trk = hsk.KinfuTracker(n=n)
    vol = np.zeros((n, n, n, 2), np.int16)
    pose, depth = synth_frames(0)
    scaled = oracle.scale_depth(cfg_o, depth)
    for _ in range(130):
        oracle.integrate(cfg_o, vol, scaled, pose)
        trk.integrate(depth, pose)
    out = trk.download_tsdf()
    assert out[..., 1].max() == 128
    assert_same_bits(out, vol, "tsdf after 130 integrations")
    trk.close()


def test_free_space_weights_long_run(hsk, oracle, synth_frames):
    """the weights of deep free space are kept outside the volume until something reads them (lane-block summaries):
    blocks the frustum's rim has cut hold differing weights and count their pending observations in a byte -- run one
    pose long enough to overflow that count (126) and to saturate every weight (128), with NO download in between, then
    move on; the volume read back is the oracle's, and so is every later one"""
    n = 64
    cfg_o = oracle.default_config(n)
    trk = hsk.KinfuTracker(n=n)
    vol = np.zeros((n, n, n, 2), np.int16)
    frames = [synth_frames(k) for k in (0, 30, 60)]
    scaled = [oracle.scale_depth(cfg_o, d) for _, d in frames]
    plan = [0, 0, 1, 1, 1, 0, 2] + [1] * 140 + [2, 0, 1]
    for i, f in enumerate(plan):
        oracle.integrate(cfg_o, vol, scaled[f], frames[f][0])
        trk.integrate(frames[f][1], frames[f][0])
        if i in (3, len(plan) - 4):   # one early read-back, then none until the long run is over
            assert_same_bits(trk.download_tsdf(), vol, f"tsdf after step {i}")
    assert_same_bits(trk.download_tsdf(), vol, "tsdf after the long run")
    w = vol[..., 1]
    assert w.max() == 128 and ((w > 0) & (w < 128)).sum() > 1000   # saturated and partly observed regions both exist
    # the raycast reads TSDF values only, and must not care where the weights live
    vm, nm, keys = trk.raycast(frames[1][0], want_keys=True)
    ovm, onm, okeys, _ = oracle.raycast(cfg_o, vol, frames[1][0])
    assert np.array_equal(keys, okeys)
    assert_same_bits(vm, ovm, "raycast vmap after the long run")
    trk.close()


def test_chunk_level_counts_long_run(hsk, oracle, synth_frames):
    """round 5's coarse level: a wave-chunk (16 x 16 voxels x 8 planes) that is wholly free space records an observation as
    ONE count in its chunk byte.  Run one pose long enough that the byte reaches its ceiling (254 pending observations: the
    next free frame must push the count down into the lane-block bytes, where a rim block's own count overflows in turn and
    its words are rewritten), with other poses in between (their frustums cut chunks that hold pending counts: the counts are
    pushed down under blocks the frame does not touch) and a cloud taken while everything is pending -- no download until the
    end, where the volume must be the oracle's.  256^3: small enough for the oracle, fine enough for chunks to be free."""
    n = 256
    cfg_o = oracle.default_config(n)
    trk = hsk.KinfuTracker(n=n)
    vol = np.zeros((n, n, n, 2), np.int16)
    frames = [synth_frames(k) for k in (0, 40, 75)]
    scaled = [oracle.scale_depth(cfg_o, d) for _, d in frames]
    plan = [0] * 130 + [1] + [0] * 60 + [2, 1] + [0] * 75 + [1, 0, 0]
    seen_quiet = seen_bumped = 0
    for i, f in enumerate(plan):
        oracle.integrate(cfg_o, vol, scaled[f], frames[f][0], omp=True)
        trk.integrate(frames[f][1], frames[f][0])
        if i in (5, 120, 200, len(plan) - 1):
            mixed, settled, free_worked, quiet = trk.integrate_coarse_counts()
            seen_quiet = max(seen_quiet, quiet)
            seen_bumped = max(seen_bumped, settled)
        if i == 150:   # a product in the middle: no flush, nothing may change
            pts, total = trk.extract_cloud()
            opts, ototal = oracle.extract_cloud(cfg_o, vol)
            assert total == ototal and np.array_equal(pts.view(np.uint32), opts.view(np.uint32))
    assert seen_quiet > 500, seen_quiet            # the chunk bytes were really in use
    assert_same_bits(trk.download_tsdf(), vol, "tsdf after 270 integrations without a read-back")
    w = vol[..., 1]
    assert w.max() == 128 and ((w > 0) & (w < 128)).sum() > 10000
    trk.close()


def test_upload_then_integrate_more(hsk, oracle, synth_frames):
    """a volume uploaded into a fresh context (its free-space summaries rebuilt from the words) takes further frames exactly
    as the context it came from: both equal the oracle's volume, with and without a read-back in between"""
    n = 64
    cfg_o = oracle.default_config(n)
    a = hsk.KinfuTracker(n=n)
    vol = np.zeros((n, n, n, 2), np.int16)
    for k in (0, 4, 8, 12):
        pose, depth = synth_frames(k)
        oracle.integrate(cfg_o, vol, oracle.scale_depth(cfg_o, depth), pose)
        a.integrate(depth, pose)
    b = hsk.KinfuTracker(n=n)
    b.upload_tsdf(a.download_tsdf())
    for k in (16, 20, 24, 12, 12):
        pose, depth = synth_frames(k)
        oracle.integrate(cfg_o, vol, oracle.scale_depth(cfg_o, depth), pose)
        a.integrate(depth, pose)
        b.integrate(depth, pose)
    assert_same_bits(b.download_tsdf(), vol, "uploaded context after five more frames")
    assert_same_bits(a.download_tsdf(), vol, "original context after five more frames")
    ca, cb = a.extract_cloud(), b.extract_cloud()
    assert_same_bits(np.asarray(cb[0] if isinstance(cb, tuple) else cb), np.asarray(ca[0] if isinstance(ca, tuple) else ca), "clouds of the two contexts")
    a.close()
    b.close()


def test_preprocess_bit_exact(hsk, oracle, synth_frames):
    cfg_o = oracle.default_config(64)
    trk = hsk.KinfuTracker(n=64)
    rng = np.random.default_rng(7)
    for k in (0, 30):
        pose, depth = synth_frames(k)
        d = depth.copy()
        # holes + mm noise so that the bilateral range weights and the pyrDown gate do real work
        d = (d.astype(np.int32) + rng.integers(-8, 9, d.shape)).clip(0, 65535).astype(np.uint16)
        d[rng.random(d.shape) < 0.02] = 0
        d[100:140, 200:260] = 0
        trk.preprocess(d)
        lv = [oracle.bilateral(cfg_o, d)]
        lv.append(oracle.pyrdown(lv[0]))
        lv.append(oracle.pyrdown(lv[1]))
        assert_same_bits(trk.download_scaled_depth(), oracle.scale_depth(cfg_o, d), "scaled depth")
        for l in range(3):
            assert_same_bits(trk.download_depth_level(l), lv[l], f"depth level {l}")
            vm = oracle.vmap(cfg_o, lv[l], l)
            assert_same_bits(trk.download_map(0, l), vm, f"vmap level {l}")
            assert_same_bits(trk.download_map(1, l), oracle.nmap(vm), f"nmap level {l}")
    trk.close()


def test_bilateral_extreme_range_weights_bit_exact(hsk, oracle):
    """Range weights at the far end of the table: differences of 380 - 511 mm (weights in and below binary32's subnormal
    range), the cut-off at 512, 16-bit extremes, and windows without a weighty tap (the image's last column and row are in
    no window, their own included) -- the kernel's tile of 4 x depth and its +0 terms for outside taps must not show."""
    cfg_o = oracle.default_config(64)
    trk = hsk.KinfuTracker(n=64)
    rng = np.random.default_rng(11)
    H, W = 480, 640
    imgs = []
    base = np.full((H, W), 2000, np.int64)
    imgs.append(base + rng.integers(380, 516, (H, W)) * rng.integers(0, 2, (H, W)))        # every other tap far down the table
    imgs.append(base + (np.arange(W)[None, :] % 2) * rng.integers(395, 440, (H, W)))       # columns alternate: subnormal weights only, but for the own column
    imgs.append(rng.integers(0, 65536, (H, W)))                                             # anything 16 bits hold
    imgs.append(np.where(rng.random((H, W)) < 0.5, 65535, 65535 - rng.integers(0, 600, (H, W))))
    for img in imgs:
        d = img.clip(0, 65535).astype(np.uint16)
        trk.preprocess(d)
        assert_same_bits(trk.download_depth_level(0), oracle.bilateral(cfg_o, d), "bilateral")
    trk.close()


def test_bilateral_tables_match_oracle(hsk, oracle):
    import ctypes as C
    ws, wc = hsk.bilateral_tables()
    # the oracle's tables are private; reproduce them through its public filter on an impulse instead:
    # a flat image must pass through unchanged and the tables must be monotone / normalised at 0
    assert ws[84] == 1.0 and wc[0] == 1.0 and (np.diff(wc) <= 0).all()
    flat = np.full((64, 64), 1234, np.uint16)
    assert (oracle.bilateral(oracle.default_config(64, W=64, H=64), flat) == 1234).all()


def _fused_volume(hsk, oracle, synth_frames, n, frames):
    cfg_o = oracle.default_config(n)
    vol = np.zeros((n, n, n, 2), np.int16)
    for k in frames:
        pose, depth = synth_frames(k)
        oracle.integrate(cfg_o, vol, oracle.scale_depth(cfg_o, depth), pose)
    return cfg_o, vol


@pytest.mark.parametrize("n", [64, 128, 256, 512])   # 256 / 512: long wave-wide crossings of clear super-bricks, step keys included
def test_raycast_bit_exact(hsk, oracle, synth_frames, n):
    cfg_o, vol = _fused_volume(hsk, oracle, synth_frames, n, (0, 5, 10))
    trk = hsk.KinfuTracker(n=n)
    trk.upload_tsdf(vol)
    inside = np.array([[0.94, 0, 0.34, 1.2], [0, 1, 0, 1.4], [-0.34, 0, 0.94, 0.6], [0, 0, 0, 1]], np.float32)
    for pose in (synth_frames(10)[0], synth_frames(40)[0], inside):
        vm, nm, keys = trk.raycast(pose, want_keys=True)
        ovm, onm, okeys, _ = oracle.raycast(cfg_o, vol, pose)
        assert np.array_equal(keys, okeys)
        assert_same_bits(vm, ovm, "raycast vmap")
        assert_same_bits(nm, onm, "raycast nmap")
        assert (~np.isnan(vm[0])).mean() > 0.3
    trk.close()


def _sparse_volume(rng, shape, size, tau, n_blobs):
    """mostly free space (+1, weight 1) with a few solid balls: the TSDF of the union, truncated at tau"""
    Z, Y, X = shape
    cell = np.array(size, np.float64) / np.array([X, Y, Z])
    zz, yy, xx = np.meshgrid((np.arange(Z) + 0.5) * cell[2], (np.arange(Y) + 0.5) * cell[1], (np.arange(X) + 0.5) * cell[0], indexing="ij")
    sd = np.full(shape, 1e9)
    for _ in range(n_blobs):
        c = rng.uniform(0.15, 0.85, 3) * np.array(size)
        r = rng.uniform(0.06, 0.22)
        sd = np.minimum(sd, np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) - r)
    vol = np.zeros(shape + (2,), np.int16)
    vol[..., 0] = np.rint(np.clip(sd / tau, -1.0, 1.0) * 32767.0).astype(np.int16)
    vol[..., 1] = 1
    return vol


@pytest.mark.parametrize("case", ["cubic256", "flat", "tall"])
def test_raycast_crossings_in_sparse_volumes(hsk, oracle, case):
    """The wave-wide crossings of clear super-bricks run on through further clear ones along the ray (a DDA over the faces
    that stops near edges and corners): volumes that are almost all air, seen along the axes, along the 45-degree
    diagonals, from cameras that sit exactly on super-brick faces, edges and corners, and from random poses -- keys and
    maps bit-exact against the oracle's step-by-step march."""
    rng = np.random.default_rng({"cubic256": 7, "flat": 8, "tall": 9}[case])
    if case == "cubic256":
        n, shape, size, kw_o, kw_h = 256, (256, 256, 256), (3.0, 3.0, 3.0), {}, {}
    elif case == "flat":
        n, shape, size = 256, (64, 192, 256), (3.0, 2.25, 0.75)      # (z, y, x); size (x, y, z)
        kw_o = dict(vol=(256, 192, 64), size=size)
        kw_h = dict(vol_y=192, vol_z=64, vol_size_m=size, own_z1=64)
    else:
        n, shape, size = 80, (320, 112, 80), (1.0, 1.4, 4.0)
        kw_o = dict(vol=(80, 112, 320), size=size)
        kw_h = dict(vol_y=112, vol_z=320, vol_size_m=size, own_z1=320)
    cfg_o = oracle.default_config(n, omp=True, **kw_o)
    trk = hsk.KinfuTracker(hsk.default_config(n, **kw_h)) if kw_h else hsk.KinfuTracker(n=n)
    vol = _sparse_volume(rng, shape, size, oracle.tau(cfg_o), 5)
    trk.upload_tsdf(vol)
    size = np.array(size)

    def pose_of(R, t):
        P = np.eye(4, dtype=np.float32)
        P[:3, :3] = np.asarray(R, np.float32)
        P[:3, 3] = np.asarray(t, np.float32)
        return P

    c45, I = np.float32(np.sqrt(0.5)), np.eye(3)
    Ry45 = [[c45, 0, c45], [0, 1, 0], [-c45, 0, c45]]
    Rx45 = [[1, 0, 0], [0, c45, -c45], [0, c45, c45]]
    Rback = [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]
    edge = size / np.array(shape[::-1]) * (64 if case != "tall" else 32)   # a super-brick edge (4 bricks of 16 / 8 voxels)
    poses = [pose_of(I, size * [0.5, 0.5, -0.1]),                 # along +z from outside
             pose_of(I, [edge[0], edge[1], 0.0]),                   # on a corner line of the super-brick grid, on the volume's face
             pose_of(Ry45, [edge[0], edge[1] * 1.5, edge[2] * 0.5]),  # diagonal in x / z, starting on a face
             pose_of(Rx45, [edge[0] * 1.5, edge[1], edge[2]]),      # diagonal in y / z, starting on an edge
             pose_of(Rback, size * [0.5, 0.5, 1.05]),               # along -z from behind
             pose_of(np.asarray(Ry45) @ np.asarray(Rx45), edge * 1.0)]  # from a corner of the grid, oblique
    for k in range(4):
        poses.append((_lookat_pose if k % 2 else _random_pose)(rng, size / 2, size * (0.45 if k < 2 else 0.9)))
    hits = 0
    for i, pose in enumerate(poses):
        vm, nm, keys = trk.raycast(pose, want_keys=True)
        ovm, onm, okeys, _ = oracle.raycast(cfg_o, vol, pose, omp=True)
        assert np.array_equal(keys, okeys), f"{case} pose {i}: keys differ at {int((keys != okeys).sum())} pixels"
        assert_same_bits(vm, ovm, f"{case} pose {i}: vmap")
        assert_same_bits(nm, onm, f"{case} pose {i}: nmap")
        hits += int((~np.isnan(vm[0])).sum())
    assert hits > 20000, hits
    trk.close()


def test_raycast_empty_volume(hsk, oracle, synth_frames):
    trk = hsk.KinfuTracker(n=64)
    vm, nm, keys = trk.raycast(synth_frames(0)[0], want_keys=True)
    assert np.isnan(vm).all() and np.isnan(nm).all() and (keys == 0x7FFFFFFF).all()
    trk.close()


def test_icp_sums_and_solve_bit_exact(hsk, oracle, synth_frames):
    n = 128
    cfg_o = oracle.default_config(n)
    ot = oracle.Tracker(cfg_o)
    trk = hsk.KinfuTracker(n=n, use_graph=0)
    for k in range(3):
        pose, depth = synth_frames(k)
        po, _ = ot.process(depth)
        ph, _ = trk.process_frame(depth)
        assert_same_bits(ph, po, f"pose frame {k}")
    # next frame: compare the 27 sums at the coarsest and the finest level for a perturbed estimate
    pose, depth = synth_frames(3)
    trk.preprocess(depth)
    prev = trk.get_pose()
    est = prev.copy()
    est[:3, 3] += np.array([0.004, -0.003, 0.002], np.float32)
    lv = [oracle.bilateral(cfg_o, depth)]
    lv.append(oracle.pyrdown(lv[0]))
    lv.append(oracle.pyrdown(lv[1]))
    for level in (2, 1, 0):
        vm = oracle.vmap(cfg_o, lv[level], level)
        nm = oracle.nmap(vm)
        osum, nvalid = oracle.icp_accumulate(cfg_o, level, vm, nm, ot.model_map(2, level), ot.model_map(3, level), est, prev)
        assert nvalid > 1000
        hsum = trk.icp_accumulate(level, est)
        assert_same_bits(hsum, osum, f"ICP sums level {level}")
        # row-sharded accumulation (multi-GPU all-reduce mode) adds up to the same bits
        H = cfg_o.H >> level
        parts = [trk.icp_accumulate(level, est, r0, r1) for r0, r1 in ((0, H // 3), (H // 3, H // 2), (H // 2, H))]
        assert_same_bits(parts[0] + parts[1] + parts[2], osum, "row-sharded ICP sums")
        xo, oko = oracle.icp_solve(osum)
        xh, okh = trk.icp_solve(hsum)
        assert oko and okh
        assert_same_bits(xh, xo, "6x6 solve")
    # singular system => not ok
    assert not trk.icp_solve(np.zeros(27))[1] and not oracle.icp_solve(np.zeros(27))[1]
    trk.close()


def test_icp_sums_extremes_bit_exact(hsk, oracle):
    """the exact accumulation's edge cases through the C ABI: scaled products that are exact ties, products of 2^45, sums close
    to 2^27 -- whole image and row-sharded"""
    from icp_extremes import extreme_maps
    n = 64
    cfg_o = oracle.default_config(n)
    trk = hsk.KinfuTracker(n=n)
    eye = np.eye(4, dtype=np.float32)
    for level in (0, 1, 2):
        W, H = cfg_o.W >> level, cfg_o.H >> level
        s = float(1 << level)
        vcur, ncur, vmod, nmod = extreme_maps(W, H, cfg_o.fx / s, cfg_o.fy / s, cfg_o.cx / s, cfg_o.cy / s, seed=5 + level)
        for kind, arr in enumerate((vcur, ncur, vmod, nmod)):
            trk.upload_map(kind, level, arr)
        trk.set_pose(eye)
        osum, nvalid = oracle.icp_accumulate(cfg_o, level, vcur, ncur, vmod, nmod, eye, eye)
        assert nvalid > 1000
        assert_same_bits(trk.icp_accumulate(level, eye), osum, f"extreme ICP sums level {level}")
        parts = [trk.icp_accumulate(level, eye, r0, r1) for r0, r1 in ((0, H // 3), (H // 3, H // 2), (H // 2, H))]
        assert_same_bits(parts[0] + parts[1] + parts[2], osum, "row-sharded extreme ICP sums")
    trk.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_tracker_bit_exact_and_accurate(hsk, oracle, synth_frames, graph):
    """whole pipeline, 12 frames: poses and TSDF identical to the oracle; trajectory within 3 mm / 0.1 deg of truth"""
    n = 128
    cfg_o = oracle.default_config(n)
    ot = oracle.Tracker(cfg_o, omp=True)
    trk = hsk.KinfuTracker(n=n, use_graph=graph)
    for k in range(12):
        gt, depth = synth_frames(k)
        po, oko = ot.process(depth)
        ph, okh = trk.process_frame(depth)
        assert oko == okh == (k > 0)
        assert_same_bits(ph, po, f"pose frame {k}")
        dt = np.linalg.norm(ph[:3, 3] - gt[:3, 3]) * 1000.0
        ang = np.degrees(np.arccos(np.clip((np.trace(ph[:3, :3].astype(np.float64).T @ gt[:3, :3]) - 1) / 2, -1, 1)))
        assert dt < 3.0 and ang < 0.1, (k, dt, ang)
    assert_same_bits(trk.download_tsdf(), ot.volume(), "tsdf after 12 tracked frames")
    for level in range(3):
        assert_same_bits(trk.download_map(2, level), ot.model_map(2, level), f"model vmap {level}")
        assert_same_bits(trk.download_map(3, level), ot.model_map(3, level), f"model nmap {level}")
    trk.close()


def test_tracker_long_stream_vs_oracle(hsk, oracle):
    """260 tracked frames, pipelined (submit / wait, one frame in flight ahead) -- past the saturation of the weights at
    128 and through every state of the free-space summaries: every pose and the final TSDF are the oracle tracker's"""
    import torch
    n, total = 96, 260
    cfg_o = oracle.default_config(n)
    ot = oracle.Tracker(cfg_o, omp=True)
    frames = [hsk.synth_depth(hsk.synth_pose(k)) for k in range(total)]
    want = [ot.process(d) for d in frames]
    dev = torch.from_numpy(np.stack(frames).view(np.int16)).cuda()
    trk = hsk.KinfuTracker(n=n)
    got = []
    trk.submit_frame_dev(dev[0].data_ptr())
    for k in range(1, total):
        trk.submit_frame_dev(dev[k].data_ptr())
        got.append(trk.wait_frame())
    got.append(trk.wait_frame())
    for k, ((po, oko), (pp, okp)) in enumerate(zip(want, got)):
        assert oko == okp, f"frame {k}"
        assert_same_bits(pp, po, f"pose of frame {k}")
    assert all(ok for _, ok in want[1:])
    vol = ot.volume()
    assert vol[..., 1].max() == 128
    assert_same_bits(trk.download_tsdf(), vol, "tsdf after 260 frames")
    trk.close()


@pytest.mark.parametrize("w,h", [(320, 240), (336, 252), (160, 120), (1280, 960)])   # (1280 x 960: four times the pixels; 960 blocks at the ICP's fine level)
def test_tracker_other_image_sizes(hsk, oracle, w, h):
    """image sizes other than 640x480 take other kernel shapes (ICP pixels per lane by level width, the raycast's fused
    pyramid only when both dimensions are multiples of 8, partial tiles otherwise): still bit-exact against the oracle,
    synchronous and pipelined"""
    import torch
    n = 96
    s = w / 640.0
    intr = dict(fx=525.0 * s, fy=525.0 * s, cx=w / 2 - 0.5, cy=h / 2 - 0.5)
    cfg_o = oracle.default_config(n, W=w, H=h, **intr)
    ot = oracle.Tracker(cfg_o, omp=True)
    trk = hsk.KinfuTracker(n=n, width=w, height=h, **intr)
    pipe = hsk.KinfuTracker(n=n, width=w, height=h, **intr)
    frames = [hsk.synth_depth(hsk.synth_pose(k), w, h, intr["fx"], intr["fy"], intr["cx"], intr["cy"]) for k in range(8)]
    dev = [torch.from_numpy(f.view(np.int16)).cuda() for f in frames]
    want = []
    for k, depth in enumerate(frames):
        po, oko = ot.process(depth)
        ph, okh = trk.process_frame(depth)
        assert oko == okh == (k > 0)
        assert_same_bits(ph, po, f"{w}x{h} pose frame {k}")
        want.append((po, oko))
    assert_same_bits(trk.download_tsdf(), ot.volume(), f"{w}x{h} tsdf")
    for level in range(3):
        assert_same_bits(trk.download_map(2, level), ot.model_map(2, level), f"{w}x{h} model vmap {level}")
        assert_same_bits(trk.download_map(3, level), ot.model_map(3, level), f"{w}x{h} model nmap {level}")
    got = []
    pipe.submit_frame_dev(dev[0].data_ptr())
    for k in range(1, 8):
        pipe.submit_frame_dev(dev[k].data_ptr())
        got.append(pipe.wait_frame())
    got.append(pipe.wait_frame())
    for k, ((po, oko), (pp, okp)) in enumerate(zip(want, got)):
        assert oko == okp
        assert_same_bits(pp, po, f"{w}x{h} pipelined pose frame {k}")
    assert_same_bits(pipe.download_tsdf(), ot.volume(), f"{w}x{h} pipelined tsdf")
    trk.close()
    pipe.close()


def test_tracking_lost_resets(hsk, synth_frames):
    trk = hsk.KinfuTracker(n=64)
    _, d0 = synth_frames(0)
    trk.process_frame(d0)
    pose, tracked = trk.process_frame(np.zeros_like(d0))  # no valid pixel => singular system => lost
    assert not tracked
    assert np.allclose(pose[:3, 3], [1.5, 1.5, -0.3])
    assert not trk.download_tsdf().any()
    # and it recovers: next frame is a "first" frame again
    _, t2 = trk.process_frame(d0)
    assert not t2
    _, t3 = trk.process_frame(synth_frames(1)[1])
    assert t3
    trk.close()


@pytest.mark.parametrize("seed", range(4))
def test_tracker_fuzz_vs_oracle(hsk, oracle, synth_frames, seed):
    """a stream that mixes good frames with garbage (random blocky depth: ICP correspondences everywhere and nowhere,
    degenerate or wild solves), empty frames and frames repeated after a loss: every pose, every tracked / lost verdict and
    the final TSDF and model maps identical to the oracle tracker -- synchronous and pipelined"""
    import torch
    rng = np.random.default_rng(2000 + seed)
    n = 96
    cfg_o = oracle.default_config(n)
    ot = oracle.Tracker(cfg_o, omp=True)
    trk = hsk.KinfuTracker(n=n)
    pipe = hsk.KinfuTracker(n=n)
    frames = []
    k = 0
    for i in range(14):
        r = rng.random()
        if i >= 2 and r < 0.2:
            frames.append(_random_depth(rng))
        elif i >= 2 and r < 0.3:
            frames.append(np.zeros((480, 640), np.uint16))
        elif i >= 2 and r < 0.4:
            k += int(rng.integers(5, 30))     # a jump along the trajectory: ICP starts far from the answer
            frames.append(synth_frames(k)[1])
        else:
            frames.append(synth_frames(k)[1])
            k += 1
    want = []
    for i, depth in enumerate(frames):
        po, oko = ot.process(depth)
        ph, okh = trk.process_frame(depth)
        assert oko == okh, f"seed {seed} frame {i}: tracked verdicts differ"
        assert_same_bits(ph, po, f"seed {seed} pose frame {i}")
        want.append((po, oko))
    # (seeds 0 and 3 track through their garbage frames; the others lose 2-4 frames)
    if SEED_EXPECTATIONS:
        assert seed in (0, 3) or sum(not ok for _, ok in want[1:]) >= 2
    assert_same_bits(trk.download_tsdf(), ot.volume(), "tsdf (tracker fuzz)")
    for level in range(3):
        assert_same_bits(trk.download_map(2, level), ot.model_map(2, level), f"model vmap {level} (tracker fuzz)")
    dev = [torch.from_numpy(f.view(np.int16)).cuda() for f in frames]
    # pipelined: a loss drops the frame submitted behind it (the caller resubmits), exactly as the synchronous order
    i, got = 0, []
    while i < len(frames):
        pipe.submit_frame_dev(dev[i].data_ptr())
        got.append(pipe.wait_frame())
        i += 1
    for i, ((po, oko), (pp, okp)) in enumerate(zip(want, got)):
        assert oko == okp
        assert_same_bits(pp, po, f"seed {seed} submit/wait pose frame {i}")
    assert_same_bits(pipe.download_tsdf(), ot.volume(), "tsdf (tracker fuzz, submit/wait)")
    trk.close()
    pipe.close()


def test_errors_are_values(hsk, synth_frames):
    trk = hsk.KinfuTracker(n=32)
    with pytest.raises(hsk.KinfuError, match="size"):
        trk.process_frame(np.zeros((240, 320), np.uint16))
    with pytest.raises(hsk.KinfuError):
        hsk.KinfuTracker(hsk.default_config(32, vol_x=30))
    trk.close()


def test_extract_cloud_matches_oracle(hsk, oracle, synth_frames):
    n = 64
    cfg_o, vol = _fused_volume(hsk, oracle, synth_frames, n, (0, 5, 10, 15))
    trk = hsk.KinfuTracker(n=n)
    trk.upload_tsdf(vol)
    pts, total = trk.extract_cloud()
    opts, ototal = oracle.extract_cloud(cfg_o, vol)
    assert total == ototal and total > 1000
    assert_same_bits(pts, opts, "extracted cloud")
    # surface points lie on the synthetic scene: back wall z = 2.8 within one cell
    back = pts[np.abs(pts[:, 2] - 2.8) < 0.05]
    assert len(back) > 100
    trk.close()


def test_full_size_properties(hsk, synth_frames):
    """512^3 (BASELINE.json size): size-independent properties instead of an oracle sweep."""
    n = 512
    trk = hsk.KinfuTracker(n=n)
    pose, depth = synth_frames(0)
    n_upd = trk.count_updates(depth, pose)
    trk.integrate(depth, pose)
    vol = trk.download_tsdf()
    w = vol[..., 1]
    assert int((w > 0).sum()) == n_upd                      # exactly the counted voxels were rewritten
    assert set(np.unique(w).tolist()) <= {0, 1}
    trk.integrate(depth, pose)                              # idempotence of the running mean on identical input
    vol2 = trk.download_tsdf()
    assert np.array_equal(vol2[..., 0], vol[..., 0]) and vol2[..., 1].max() == 2
    # raycast of the fused frame reproduces the input depth: z of the model vertex in camera frame ~ depth
    vm, nm = trk.raycast(pose)
    z_cam = vm[2] - pose[2, 3]
    valid = ~np.isnan(z_cam) & (depth > 0)
    assert valid.mean() > 0.5
    err = np.abs(z_cam[valid] * 1000.0 - depth[valid])
    assert np.median(err) < 4.0                             # < one 5.86 mm cell
    nn = np.linalg.norm(nm[:, ~np.isnan(nm[0])], axis=0)
    assert np.abs(nn - 1).max() < 1e-5
    trk.close()


def test_golden_vectors_gpu(hsk):
    """HIP path vs the committed golden vectors (tests/golden/make_golden.py), no oracle involved"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kinfu_golden.npz"))
    W, H, FX, CX, CY = 160, 120, 131.25, 79.75, 59.75
    n = int(g["n"])
    trk = hsk.KinfuTracker(hsk.default_config(n, width=W, height=H, fx=FX, fy=FX, cx=CX, cy=CY))
    poses = []
    for k in g["frames"]:
        poses.append(trk.process_frame(hsk.synth_depth(hsk.synth_pose(int(k)), W, H, FX, FX, CX, CY))[0])
    assert_same_bits(np.stack(poses), g["poses"], "golden poses")
    assert_same_bits(trk.download_tsdf()[8:24, 8:24, 8:24], g["tsdf_crop"], "golden tsdf crop")
    assert_same_bits(trk.download_map(2, 0)[:, 40:70, 60:100], g["vmap_crop"], "golden vmap crop")
    assert_same_bits(trk.download_map(3, 0)[:, 40:70, 60:100], g["nmap_crop"], "golden nmap crop")
    trk.preprocess(hsk.synth_depth(hsk.synth_pose(4), W, H, FX, FX, CX, CY))
    assert_same_bits(trk.icp_accumulate(0, poses[-1]), g["icp27"], "golden ICP sums")
    # vectors added in round 2 (generated by the numpy twin)
    x6, ok = trk.icp_solve(g["icp27"])
    assert ok
    assert_same_bits(x6, g["solve6"], "golden 6x6 solve (host mirror of the device solve)")
    pts, total = trk.extract_cloud()
    assert total == int(g["cloud_count"])
    assert_same_bits(pts[:256], g["cloud_head"], "golden cloud head")
    trk.close()
    # a second tracker stops exactly where the golden run stopped: model maps of the coarsest level and the step keys
    trk = hsk.KinfuTracker(hsk.default_config(n, width=W, height=H, fx=FX, fy=FX, cx=CX, cy=CY))
    for k in g["frames"]:
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(int(k)), W, H, FX, FX, CX, CY))
    assert_same_bits(trk.download_map(2, 2), g["vmap2"], "golden model vmap level 2")
    assert_same_bits(trk.download_map(3, 2), g["nmap2"], "golden model nmap level 2")
    _, _, keys = trk.raycast(poses[-1], want_keys=True)
    assert np.array_equal(keys[40:70, 60:100], g["keys_crop"])
    trk.preprocess(hsk.synth_depth(hsk.synth_pose(int(g["frames"][1])), W, H, FX, FX, CX, CY))
    assert np.array_equal(trk.download_depth_level(0), g["bilateral1"])
    trk.close()


def test_slab_contexts_compose_to_single_volume(hsk, oracle, synth_frames):
    """two z-slab contexts on one GPU driven through the hsk_mgpu_* building blocks, composited on the host the
    way the collectives do (MIN of keys, SUM of bit patterns): bit-identical to the single-volume context"""
    import ctypes as C
    import torch
    from housescan_amd.sharded import HipSlabEngine, slab_halo, slab_range
    n, world = 64, 2
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)   # a capturable stream: the torch ops below and both engines order on it
    ref = hsk.KinfuTracker(n=n, use_graph=0)
    engines = []
    for r in range(world):
        cfg = hsk.default_config(n, use_graph=1)   # graphs: hsk_mgpu_frame_front captures its frame front per buffer set
        cfg.own_z0, cfg.own_z1 = slab_range(r, world, n)
        cfg.halo = slab_halo(max(0.03, 2.1 * 3.0 / n), 3.0 / n)
        engines.append(HipSlabEngine(hsk.KinfuTracker(cfg), torch, dev, side))
    held = {}
    pending = []
    nframes = 9
    torch.cuda.synchronize()
    ctx = torch.cuda.stream(side)
    ctx.__enter__()
    for k in range(nframes):
        _, depth = synth_frames(k)
        pref, okref = ref.process_frame(depth)
        d_dev = held.pop(k, None)
        if d_dev is None:
            d_dev = torch.from_numpy(depth.view(np.int16)).to(dev)
        first = engines[0].frame_index() == 0
        fused = k >= 3   # frames 3..8: the one-call, graph-replayed frame front (capture on 3 and 4, replay afterwards)
        if fused:
            keys = [e.frame_front(d_dev).clone() for e in engines]
        else:
            for e in engines:
                e.frame_begin(d_dev)
        if k + 1 < nframes and k % 2 == 0:   # every other frame: the next frame is copied + filtered ahead, on the second stream
            nxt = torch.from_numpy(synth_frames(k + 1)[1].view(np.int16)).to(dev)
            held[k + 1] = nxt          # the prefetched pointer must be the one passed to the next frame_begin / frame_front
            for e in engines:
                e.prefetch(nxt)
        if first:
            outs = [e.frame_end(None, None) for e in engines]
        elif fused:
            kmin = torch.minimum(keys[0], keys[1])
            bits = [e.raycast_resolve(kmin).clone() for e in engines]
            bsum = bits[0] + bits[1]
            if k >= 5:
                # pipelined end: the pose read-back is queued, the next frame is enqueued before it is collected
                for e in engines:
                    assert not e.restart_pending()
                    e.frame_end_async(kmin, bsum)
                pending.append((k, pref, okref))
                if len(pending) < 2 and k + 1 < nframes:
                    continue
                kk, pp, oo = pending.pop(0)
                outs = [e.wait_frame() for e in engines]
                for p_, ok_ in outs:
                    assert ok_ == oo
                    assert_same_bits(p_, pp, f"slab pose frame {kk} (pipelined)")
                continue
            outs = [e.frame_end(kmin, bsum) for e in engines]
        else:
            if k % 2 == 1:
                for e in engines:   # "replicated" mode: every slab context runs the fused 19-iteration ICP itself
                    e.icp_replicated()
            else:
                for level in (2, 1, 0):
                    for _ in range([10, 5, 4][level]):
                        # "allreduce" mode: each engine sums half of the rows, the sums are added exactly
                        h = 480 >> level
                        parts = [e.icp_accumulate(level, r * h // 2, (r + 1) * h // 2).clone() for r, e in enumerate(engines)]
                        tot = parts[0] + parts[1]
                        for e in engines:
                            e.icp_update(tot)
            for e in engines:
                e.integrate()
            keys = [e.raycast_local().clone() for e in engines]
            kmin = torch.minimum(keys[0], keys[1])
            bits = [e.raycast_resolve(kmin).clone() for e in engines]
            bsum = bits[0] + bits[1]
            outs = [e.frame_end(kmin, bsum) for e in engines]
        for p, ok in outs:
            assert ok == okref
            assert_same_bits(p, pref, f"slab pose frame {k}")
    while pending:   # the frames still in flight
        kk, pp, oo = pending.pop(0)
        for e in engines:
            p_, ok_ = e.wait_frame()
            assert ok_ == oo
            assert_same_bits(p_, pp, f"slab pose frame {kk} (pipelined, drained)")
    ctx.__exit__(None, None, None)
    torch.cuda.synchronize()
    full = ref.download_tsdf()
    for r, e in enumerate(engines):
        z0, z1 = slab_range(r, world, n)
        got = e.t.download_tsdf()
        assert_same_bits(got[z0 - e.t.stored_z0:z1 - e.t.stored_z0], full[z0:z1], f"slab {r} owned planes")
        for level in range(3):
            assert_same_bits(e.t.download_map(2, level), ref.download_map(2, level), f"slab {r} model vmap {level}")
            assert_same_bits(e.t.download_map(3, level), ref.download_map(3, level), f"slab {r} model nmap {level}")
        e.t.close()
    ref.close()


def _pose_err(p, gt):
    dt = np.linalg.norm(p[:3, 3] - gt[:3, 3]) * 1000.0
    ang = np.degrees(np.arccos(np.clip((np.trace(p[:3, :3].astype(np.float64).T @ gt[:3, :3]) - 1) / 2, -1, 1)))
    return dt, ang


def test_config2_256_tracker_vs_oracle_and_truth(hsk, oracle, synth_frames):
    """BASELINE configs[1]: 640x480 into 256^3, integrate + ICP + raycast; poses bit-identical to the oracle and
    within the stated tolerance of the scripted ground truth: 3 mm / 0.1 deg"""
    n = 256
    ot = oracle.Tracker(oracle.default_config(n), omp=True)
    trk = hsk.KinfuTracker(n=n)
    for k in range(8):
        gt, depth = synth_frames(k)
        po, _ = ot.process(depth)
        ph, ok = trk.process_frame(depth)
        assert ok == (k > 0)
        assert_same_bits(ph, po, f"pose frame {k}")
        dt, ang = _pose_err(ph, gt)
        assert dt < 3.0 and ang < 0.1, (k, dt, ang)
    assert_same_bits(trk.download_tsdf(), ot.volume(), "256^3 tsdf after 8 frames")
    trk.close()


def test_headline_512_tracker_vs_oracle(hsk, oracle, synth_frames):
    """BASELINE's metric configuration itself: 640x480 into 512^3 through the pipelined pair the benchmark times
    (submit ahead, wait behind); every pose, the whole TSDF and the model maps bit-identical to the oracle"""
    n = 512
    ot = oracle.Tracker(oracle.default_config(n), omp=True)
    trk = hsk.KinfuTracker(n=n)
    frames = [synth_frames(k) for k in range(40)]   # (the oracle tracks 512^3 at ~7 frames/s on the box's 16 cores)
    want = [ot.process(d) for _, d in frames]
    trk.process_frame(frames[0][1])
    trk.submit_frame(frames[1][1])
    got = []
    for _, d in frames[2:]:
        trk.submit_frame(d)
        got.append(trk.wait_frame())
    got.append(trk.wait_frame())
    for k, ((ph, ok), (po, oko)) in enumerate(zip(got, want[1:]), start=1):
        assert ok and oko
        assert_same_bits(ph, po, f"512^3 pose frame {k}")
    assert_same_bits(trk.download_tsdf(), ot.volume(), "512^3 tsdf after 40 frames")
    for level in range(3):
        assert_same_bits(trk.download_map(2, level), ot.model_map(2, level), f"512^3 model vmap {level}")
        assert_same_bits(trk.download_map(3, level), ot.model_map(3, level), f"512^3 model nmap {level}")
    trk.close()
    ot.close()


def test_noisy_stream_trajectory(hsk):
    """SURVEY.md 8(d) noise run: sigma = 1.2 mm * (z / 1 m)^2 (seed 1234) + 2 % dropout (seed 5678); not a parity
    test -- the tracker must stay locked: < 10 mm / 0.5 deg from ground truth over 40 frames at 256^3"""
    trk = hsk.KinfuTracker(n=256)
    gts, frames = hsk.synth_noisy_frames(40)
    worst = (0.0, 0.0)
    for k, (gt, d) in enumerate(zip(gts, frames)):
        pose, ok = trk.process_frame(d)
        assert ok == (k > 0), f"tracking lost at frame {k}"
        dt, ang = _pose_err(pose, gt)
        worst = (max(worst[0], dt), max(worst[1], ang))
    assert worst[0] < 10.0 and worst[1] < 0.5, worst
    trk.close()


def test_noisy_stream_512_vs_oracle(hsk, oracle):
    """The noise run ON THE MEASURED PATH: the sigma = 1.2 mm z^2 / 2 % dropout stream at the headline
    size, 40 pipelined frames -- every pose, the TSDF and the model maps bit-equal to the oracle's.  Sensor noise widens
    exactly what the integrate's fast paths depend on being narrow (uncertain lane-blocks, non-uniform summaries, chunks
    that are not wholly free), and every pixel of the bilateral filter and the ICP gates sees data that is not a render."""
    n, frames_n = 512, 40
    gts, frames = hsk.synth_noisy_frames(frames_n)
    ot = oracle.Tracker(oracle.default_config(n), omp=True)
    want = [ot.process(d) for d in frames]
    trk = hsk.KinfuTracker(n=n)
    got = []
    trk.submit_frame(frames[0])
    for d in frames[1:]:
        trk.submit_frame(d)
        got.append(trk.wait_frame())
    got.append(trk.wait_frame())
    for k, ((ph, okh), (po, oko)) in enumerate(zip(got, want)):
        assert okh == oko, (k, okh, oko)
        assert_same_bits(ph, po, f"noisy 512^3 pose frame {k}")
    assert sum(1 for _, ok in got[1:] if not ok) == 0, "the noisy stream must stay tracked"
    dt, ang = _pose_err(got[-1][0], gts[-1])
    assert dt < 10.0 and ang < 0.5, (dt, ang)
    assert_same_bits(trk.download_tsdf(), ot.volume(), "noisy 512^3 tsdf after 40 frames")
    for level in range(3):
        assert_same_bits(trk.download_map(2, level), ot.model_map(2, level), f"noisy 512^3 model vmap {level}")
        assert_same_bits(trk.download_map(3, level), ot.model_map(3, level), f"noisy 512^3 model nmap {level}")
    trk.close()
    ot.close()


def test_pipelined_frames_from_a_graph_match_eager(hsk, synth_frames):
    """use_graph = 2 (round 6): the main-stream chain of a pipelined frame -- 19 ICP launches, 3 integrate, the raycast -- replayed
    from one hipGraph per image-buffer set.  Every pose, the verdicts (a garbage frame in the stream loses tracking and restarts
    the scan), the TSDF and the model maps equal the eager form's; hsk_submit_host_us counts the submissions of both."""
    n = 128
    frames = [synth_frames(k)[1] for k in range(14)]
    frames[8] = np.zeros_like(frames[8])              # no valid pixel: a singular system, tracking lost, the scan restarts
    res = []
    for g in (0, 2):
        trk = hsk.KinfuTracker(n=n, use_graph=g)
        out = []
        trk.submit_frame(frames[0])
        for d in frames[1:]:
            trk.submit_frame(d)
            out.append(trk.wait_frame())
        out.append(trk.wait_frame())
        us, cnt = trk.submit_host_us()
        assert cnt >= 8 and all(u >= 0.0 for u in us) and us[3] > 0.0
        res.append((out, trk.download_tsdf(), [trk.download_map(2, l) for l in range(3)], us, cnt))
        trk.close()
    (a, va, ma, _, ca), (b, vb, mb, _, cb) = res
    assert ca == cb
    assert any(not ok for _, ok in a[1:]), "the garbage frame must lose tracking"
    for k, ((pa, oa), (pb, ob)) in enumerate(zip(a, b)):
        assert oa == ob, k
        assert_same_bits(pa, pb, f"graph vs eager pose {k}")
    assert_same_bits(va, vb, "graph vs eager tsdf")
    for l in range(3):
        assert_same_bits(ma[l], mb[l], f"graph vs eager model vmap {l}")


def test_prepare_readout_then_products(hsk, oracle, synth_frames):
    """hsk_prepare_readout (round 6): everything a read-out allocates on first use made up front; the products that follow are
    the oracle's, the call is idempotent, and the light class counts nothing on a render without holes"""
    n = 128
    trk = hsk.KinfuTracker(n=n)
    trk.prepare_readout()
    trk.prepare_readout(1 << 20)
    ot = oracle.Tracker(oracle.default_config(n))
    for k in range(5):
        d = synth_frames(k)[1]
        trk.process_frame(d)
        ot.process(d)
    assert trk.integrate_light_entries() == 0 and trk.integrate_queue_entries() > 0
    cloud, total = trk.extract_cloud()
    want, wtotal = oracle.extract_cloud(oracle.default_config(n), ot.volume())
    assert total == wtotal
    assert_same_bits(cloud, want, "cloud after prepare_readout")
    tri, nt = trk.extract_mesh(cubes=True)
    assert nt > 0 and len(tri) == nt
    trk.close()
    ot.close()


def test_sensor_holes_stream_512_vs_oracle(hsk, oracle):
    """HOLES AS A SENSOR MAKES THEM on the measured path: hsk_synth_render_sensor -- no return from grazing
    rays, shadow bands behind depth discontinuities, the range cut, an absorbing block, sigma = 1.2 mm z^2 -- i.e. CONTIGUOUS
    invalid regions (5-18 % of the pixels; housescan/HoniHelper.hs:20-36), 40 pipelined frames at 512^3: every pose, the TSDF and
    the model maps bit-equal to the oracle's.  Contiguous holes are what pass A's light path and the coarse level's
    whole-column rule are for: blocks and chunks whose pixels are ALL holes or all far."""
    n, frames_n = 512, 40
    gts, frames = hsk.synth_sensor_frames(frames_n, absorbing=True)
    frac = float(np.mean([(f == 0).mean() for f in frames]))
    assert 0.04 < frac < 0.30, frac
    ot = oracle.Tracker(oracle.default_config(n), omp=True)
    want = [ot.process(d) for d in frames]
    trk = hsk.KinfuTracker(n=n)
    got = []
    trk.submit_frame(frames[0])
    for d in frames[1:]:
        trk.submit_frame(d)
        got.append(trk.wait_frame())
    got.append(trk.wait_frame())
    for k, ((ph, okh), (po, oko)) in enumerate(zip(got, want)):
        assert okh == oko, (k, okh, oko)
        assert_same_bits(ph, po, f"sensor-holes 512^3 pose frame {k}")
    assert sum(1 for _, ok in got[1:] if not ok) == 0, "the sensor-holes stream must stay tracked"
    dt, ang = _pose_err(got[-1][0], gts[-1])
    assert dt < 10.0 and ang < 0.5, (dt, ang)
    assert_same_bits(trk.download_tsdf(), ot.volume(), "sensor-holes 512^3 tsdf after 40 frames")
    for level in range(3):
        assert_same_bits(trk.download_map(2, level), ot.model_map(2, level), f"sensor-holes 512^3 model vmap {level}")
        assert_same_bits(trk.download_map(3, level), ot.model_map(3, level), f"sensor-holes 512^3 model nmap {level}")
    trk.close()
    ot.close()


@pytest.mark.parametrize("variant,first,count", [(0, 0, 64), (1, 225, 45), (0, 470, 40)])
def test_room_scan_512_vs_oracle(hsk, oracle, variant, first, count):
    """THE ROOM SCAN ON THE MEASURED PATH: the camera stands INSIDE the volume (hsk_synth_room_*: a closed
    room with furniture, the three-turn turntable scan of 720 frames HouseScan's rooms are made with, README.md:12,
    Main.hs:1738-1762), 512^3, pipelined host frames -- every pose, the TSDF and the model maps bit-equal to the oracle's
    tracker started from the same init_pose.  Three windows: 64 frames of the level turn (room 0); the end of the level turn
    and 30 frames of the turn that swings UP to 38 deg (room 1: the ceiling with its beams comes into view); 40 frames
    round the start of the turn that swings DOWN (room 0).  Every headline figure before round 6 was a camera OUTSIDE the
    volume looking in: here the frustum starts inside it (near plane, rim and apex within the grid), rays leave through
    five walls, and the free space in front of the camera is the room itself."""
    n, scan = 512, 720
    gts = [hsk.synth_room_pose(variant, first + k, scan) for k in range(count)]
    frames = [hsk.synth_room_depth(variant, p) for p in gts]
    ot = oracle.Tracker(oracle.default_config(n, omp=True, init_R=gts[0][:3, :3], init_t=gts[0][:3, 3]), omp=True)
    want = [ot.process(d) for d in frames]
    trk = hsk.KinfuTracker(n=n, init_pose=gts[0])
    got = []
    trk.submit_frame(frames[0])
    for d in frames[1:]:
        trk.submit_frame(d)
        got.append(trk.wait_frame())
    got.append(trk.wait_frame())
    for k, ((ph, okh), (po, oko)) in enumerate(zip(got, want)):
        assert okh == oko, (k, okh, oko)
        assert_same_bits(ph, po, f"room {variant} 512^3 pose frame {first + k}")
    assert sum(1 for _, ok in got[1:] if not ok) == 0, "the room scan must stay tracked"
    dt, ang = _pose_err(got[-1][0], gts[-1])
    assert dt < 10.0 and ang < 0.3, (dt, ang)
    assert_same_bits(trk.download_tsdf(), ot.volume(), f"room {variant} 512^3 tsdf after frames {first}..{first + count - 1}")
    for level in range(3):
        assert_same_bits(trk.download_map(2, level), ot.model_map(2, level), f"room 512^3 model vmap {level}")
        assert_same_bits(trk.download_map(3, level), ot.model_map(3, level), f"room 512^3 model nmap {level}")
    trk.close()
    ot.close()


def test_1024_properties(hsk, synth_frames):
    """BASELINE configs[3] volume (1024^3, 4 GiB) on one GPU: size-independent properties, nothing downloaded"""
    trk = hsk.KinfuTracker(n=1024)
    poses = []
    for k in range(4):
        gt, depth = synth_frames(k)
        p, ok = trk.process_frame(depth)
        assert ok == (k > 0)
        dt, ang = _pose_err(p, gt)
        assert dt < 3.0 and ang < 0.1, (k, dt, ang)
        poses.append(p)
    gt, depth = synth_frames(3)
    n_upd = trk.count_updates(depth, poses[-1])
    assert 0.1 * 1024 ** 3 < n_upd < 0.6 * 1024 ** 3
    vm, nm = trk.raycast(poses[-1])
    R, t = poses[-1][:3, :3], poses[-1][:3, 3]
    z_cam = np.einsum("i,ihw->hw", R[:, 2], vm - t[:, None, None])       # camera-frame z of the model vertex
    valid = ~np.isnan(z_cam) & (depth > 0)
    assert valid.mean() > 0.6
    assert np.median(np.abs(z_cam[valid] * 1000.0 - depth[valid])) < 3.0   # one 2.93 mm cell
    pts, total = trk.extract_cloud(cap=100000)
    assert total > 500000 and np.isfinite(pts).all()
    trk.close()


def test_room_products_from_fused_scan(tmp_path, hsk):
    """scan -> TSDF -> cloud -> room directory for HouseScan's loadRoom: the detected planes are the scene's walls"""
    from housescan_amd import products as P
    trk = hsk.KinfuTracker(n=256)
    for k in range(0, 120, 2):
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(k)))
    cloud, total = trk.extract_cloud()
    assert total == len(cloud) > 100000
    planes, n_down = P.write_room_dir(str(tmp_path / "room"), cloud, leaf=0.03, dist_thresh=0.025, min_fraction=0.02)
    walls = [(0, 0.2), (0, 2.8), (1, 0.3), (1, 2.7), (2, 2.8)]
    for axis, coord in walls:
        assert any(abs(p[axis]) > 0.99 and abs(-p[3] / p[axis] - coord) < 0.03 for p in planes), (axis, coord, planes)
    assert os.path.exists(tmp_path / "room" / "cloud_plane_hull0.pcd") and n_down > 5000
    trk.close()


def test_async_submit_wait_matches_sync(hsk, synth_frames):
    """hsk_submit_frame_dev / hsk_wait_frame with frames in flight gives the same poses and TSDF as the
    synchronous call, in order"""
    import torch
    n = 128
    a = hsk.KinfuTracker(n=n)
    b = hsk.KinfuTracker(n=n)
    frames = [synth_frames(k)[1] for k in range(10)]
    dev = [torch.from_numpy(f.view(np.int16)).cuda() for f in frames]
    sync = [a.process_frame(f) for f in frames]
    got = []
    b.submit_frame_dev(dev[0].data_ptr())
    b.submit_frame_dev(dev[1].data_ptr())
    for i in range(2, 10):
        b.submit_frame_dev(dev[i].data_ptr())
        got.append(b.wait_frame())
    got.append(b.wait_frame())
    got.append(b.wait_frame())
    with pytest.raises(hsk.KinfuError, match="no frame in flight"):
        b.wait_frame()
    for k, ((ps, oks), (pa, oka)) in enumerate(zip(sync, got)):
        assert oks == oka, k
        assert_same_bits(pa, ps, f"async pose {k}")
    assert_same_bits(b.download_tsdf(), a.download_tsdf(), "async tsdf")
    # the same with frames in host memory: copied at submission, so the caller may reuse its buffer at once
    c = hsk.KinfuTracker(n=n)
    scratch = np.empty_like(frames[0])
    got = []
    for i, f in enumerate(frames):
        scratch[:] = f
        c.submit_frame(scratch)
        scratch[:] = 0                      # the library must not be reading this any more
        if i >= 2:
            got.append(c.wait_frame())
    got += [c.wait_frame(), c.wait_frame()]
    for k, ((ps, oks), (pc, okc)) in enumerate(zip(sync, got)):
        assert oks == okc, k
        assert_same_bits(pc, ps, f"host-frame async pose {k}")
    assert_same_bits(c.download_tsdf(), a.download_tsdf(), "host-frame async tsdf")
    a.close()
    b.close()
    c.close()


def test_async_tracking_loss_drops_in_flight_frames(hsk, synth_frames):
    import torch
    trk = hsk.KinfuTracker(n=64)
    good = [torch.from_numpy(synth_frames(k)[1].view(np.int16)).cuda() for k in range(4)]
    blank = torch.zeros(480 * 640, dtype=torch.int16, device="cuda")
    trk.submit_frame_dev(good[0].data_ptr())
    trk.submit_frame_dev(good[1].data_ptr())
    assert trk.wait_frame()[1] is False and trk.wait_frame()[1] is True
    trk.submit_frame_dev(blank.data_ptr())          # singular system => lost
    trk.submit_frame_dev(good[2].data_ptr())        # in flight behind the lost frame => dropped
    p1, t1 = trk.wait_frame()
    p2, t2 = trk.wait_frame()
    assert not t1 and not t2 and np.allclose(p1[:3, 3], [1.5, 1.5, -0.3])
    assert not trk.download_tsdf().any()            # reset happened once the ring drained
    trk.submit_frame_dev(good[0].data_ptr())        # restarts as a first frame
    trk.submit_frame_dev(good[1].data_ptr())
    assert trk.wait_frame()[1] is False and trk.wait_frame()[1] is True
    trk.close()


def test_reset_and_destroy_with_frames_in_flight(hsk, synth_frames):
    """hsk_reset waits for the pipelined frames (they report through the pinned ring, not through events) before it
    clears the volume; their results are still collected, as dropped; closing a context with frames in flight is safe"""
    import torch
    trk = hsk.KinfuTracker(n=128)
    dev = [torch.from_numpy(synth_frames(k)[1].view(np.int16)).cuda() for k in range(6)]
    for k in range(3):
        trk.process_frame_dev(dev[k].data_ptr())
    trk.submit_frame_dev(dev[3].data_ptr())
    trk.submit_frame_dev(dev[4].data_ptr())
    trk.reset()                                      # both frames are in flight
    assert not trk.download_tsdf().any()
    for _ in range(2):
        pose, ok = trk.wait_frame()
        assert not ok and np.allclose(pose[:3, 3], [1.5, 1.5, -0.3])
    # the scan restarts and matches a fresh context bit for bit
    ref = hsk.KinfuTracker(n=128)
    for k in range(3):
        pa, oa = trk.process_frame_dev(dev[k].data_ptr())
        pb, ob = ref.process_frame_dev(dev[k].data_ptr())
        assert oa == ob
        assert_same_bits(pa, pb, f"pose after reset {k}")
    assert_same_bits(trk.download_tsdf(), ref.download_tsdf(), "tsdf after reset")
    trk.submit_frame_dev(dev[3].data_ptr())
    trk.submit_frame_dev(dev[4].data_ptr())
    trk.close()                                      # frames in flight: destroy synchronises first
    ref.close()


def test_scan_two_rooms_and_stitch(tmp_path, hsk):
    """BASELINE configs[0] end to end: two closed rooms scanned by the core (three turns each) -> room directories ->
    loadRoom / orient / corner suggestions / cuboid fit / wall connections / least-squares placement -> .xf and a
    stitched .ply (tools/stitch_rooms_demo.py is the same flow as a script)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import stitch_rooms_demo as demo
    from housescan_amd import house as H
    from housescan_amd import products as P
    dirs, truth = [], []
    for v in (0, 1):
        cloud, worst, lost, _ = demo.scan_room(hsk, v, 256, 720)
        print("room %d: worst trajectory error %.4f m" % (v, worst))
        assert lost == 0 and worst < 0.05, (v, lost, worst)
        d = str(tmp_path / f"room{v}" / "walls")
        planes, n_down = P.write_room_dir(d, cloud, leaf=0.04, dist_thresh=0.025, min_fraction=0.03)
        assert len(planes) >= 6 and n_down > 8000
        dirs.append(d)
        e = hsk.synth_room_extents(v)
        truth.append(sorted([e[1] - e[0], e[3] - e[2], e[5] - e[4]]))
    hs, rooms, rm = demo.stitch(hsk, dirs, [0, 1], log=lambda *_: None)
    assert np.all(rm < 1e-5)
    merged = []
    for rid, d, dims in zip(rooms, dirs, truth):
        ids, corners = hs.room_corners(rid)
        ext = corners.max(axis=0) - corners.min(axis=0)
        assert np.allclose(sorted(ext), dims, atol=0.03), (ext, dims)          # the fitted cuboid is the room
        M = hs.room_projection(rid)
        assert abs(np.linalg.det(M[:3, :3].astype(np.float64)) - 1) < 1e-5
        merged.append(P.transform_cloud(H.read_pcd_xyz(os.path.join(d, "cloud_bin.pcd")), M))
    a, b = (hs.room_corners(r)[1] for r in rooms)
    lo = lambda c, ax: np.sort(c[:, ax])[:4].mean()       # noqa: E731  (mean of a fitted cuboid's low / high face)
    hi = lambda c, ax: np.sort(c[:, ax])[4:].mean()       # noqa: E731
    assert abs((lo(b, 0) - hi(a, 0)) - 0.1) < 1e-4                             # 10 cm wall between the rooms
    assert abs(lo(b, 1) - lo(a, 1)) < 1e-4 and abs(lo(b, 2) - lo(a, 2)) < 1e-4  # floors level, low-z walls flush
    # ... and the full-resolution clouds, moved by the exported matrices, show the same gap: no scan point of either
    # room lies inside the shared wall
    gap_lo, gap_hi = hi(a, 0), lo(b, 0)
    for cloud in merged:
        inside = (cloud[:, 0] > gap_lo + 0.03) & (cloud[:, 0] < gap_hi - 0.03)
        assert inside.mean() < 1e-3
    assert np.percentile(merged[0][:, 0], 99.5) < gap_lo + 0.03 and np.percentile(merged[1][:, 0], 0.5) > gap_hi - 0.03
    H.write_ply_points(str(tmp_path / "house.ply"), np.concatenate(merged))
    assert len(H.read_ply_points(str(tmp_path / "house.ply"))) == sum(len(m) for m in merged)
    hs.close()


def test_bench_two_ranks_match_one(tmp_path):
    """bench.py's N > 1 flow end to end on the one GPU of the box: two ranks (torch.distributed.run) share device 0
    and exchange over gloo -- the z-slab split, the key / bit-pattern collectives, the pipelined slab frames and the
    max-over-ranks timing all run; the final pose must be bit-identical to the single-process run's"""
    import json
    import socket
    import subprocess
    import sys
    common = ["--steps", "24", "--warmup", "6", "--volume", "256", "--quick"]

    def last_json(cmd):
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    one = last_json([sys.executable, "bench.py", "--full"] + common)
    assert one["tracking"]["lost_frames"] == 0 and one["roofline"]["traffic"] is None and "frame_ms" in one
    for icp in ("replicated", "allreduce"):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        two = last_json([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                         "--master-port", str(port), "bench.py", "--gpus", "2", "--engine", "torch", "--backend", "gloo", "--share-gpu",
                         "--icp", icp] + common)
        assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["tracking"]["lost_frames"] == 0
        assert two["tracking"]["final_pose_f32_hex"] == one["tracking"]["final_pose_f32_hex"], icp
    # ... and the default engine (hsk_group_* in the rank form): `python bench.py --gpus 2` BARE -- the launcher starts two
    # fresh worker processes per form, a slab each, all on device 0 here.  RCCL refuses two ranks on one device
    # ("Duplicate GPU"), so its two forms must be recorded as failed and the run must still end with the direct form's
    # checked result: peer buffers through hipIpc handles, flags on a shared page -- what runs on an N-GPU node
    for launch in ("bare", "torchrun"):
        if launch == "bare":
            cmd = [sys.executable, "bench.py"]
        else:
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                   "--master-port", str(port), "bench.py"]
        two = last_json(cmd + ["--gpus", "2", "--share-gpu", "--steps", "6", "--warmup", "2", "--volume", "256", "--no-1024"])
        assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["headline_form"] == "direct", (launch, two)
        assert two["config"]["exchange"].startswith("one-hop") and two["tracking"]["lost_frames"] == 0
        assert two["matches_single_gpu"] is True and two["ranks_seen"] == 2
        assert two["forms"]["direct"]["matches_detail"]["planes_compared"] >= 256
        assert two["stage_us"]["exchange_us"] > 0 and two["stage_us"]["slab_work_us"] > 0
        assert "failed" in two["forms"]["rccl"] and "rccl@256" in two["launcher"]["failed_forms"], two["forms"]["rccl"]
        assert two["rooms_weak"]["rooms"] == 2 and two["rooms_weak"]["lost_frames"] == 0 and two["rooms_weak"]["matches_single_gpu"] is True
        assert two["single_gpu_same_frames"]["lost_frames"] == 0
        assert two["predicted_us"] is None   # (DESIGN section 6 prices 512^3 and 1024^3 only)
    one6 = last_json([sys.executable, "bench.py", "--steps", "6", "--warmup", "2", "--volume", "256", "--quick"])
    assert two["tracking"]["final_pose_f32_hex"] == one6["tracking"]["final_pose_f32_hex"] == two["single_gpu_same_frames"]["final_pose_f32_hex"]


def test_bench_eight_ranks_share_the_gpu(tmp_path):
    """`python bench.py --gpus 8 --share-gpu` BARE: the first 8-GPU run will exercise an 8-way hipIpc
    handle exchange, an 8 x 8 flag page and the launcher's 8-worker watchdog -- here with all eight ranks on device 0 (RCCL
    refuses that, so its forms are recorded as failed; the direct form and the rooms must come out checked).  No scaling
    claim follows from it: eight slabs share one GPU."""
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "8", "--share-gpu", "--volume", "256", "--steps", "6", "--warmup", "2", "--no-1024"],
                       cwd=ROOT, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 8 and line["headline_form"] == "direct" and line["scaling"] == "strong", line
    assert line["matches_single_gpu"] is True and line["ranks_seen"] == 8 and line["tracking"]["lost_frames"] == 0
    assert line["forms"]["direct"]["matches_detail"]["planes_compared"] >= 256
    assert "failed" in line["forms"]["rccl"]
    assert line["rooms_weak"]["rooms"] == 8 and line["rooms_weak"]["lost_frames"] == 0 and line["rooms_weak"]["matches_single_gpu"] is True
    out = os.environ.get("HSK_KEEP_BENCH_LINE")
    if out:
        open(out, "w").write(json.dumps(line) + "\n")


def test_bench_group_engine_world_of_one(tmp_path):
    """the default N > 1 engine of bench.py (hsk_group_* with a communicator made from a broadcast unique id) on a world of
    ONE rank launched through torch.distributed.run: the id hand-over, the RCCL communicator, the pipelined group calls and
    the JSON line; the pose equals the single-GPU run's"""
    import json
    import socket
    import subprocess
    import sys
    common = ["--steps", "12", "--warmup", "3", "--volume", "128", "--quick"]

    def last_json(cmd, env=None):
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    one = last_json([sys.executable, "bench.py"] + common)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSK_BENCH_FORCE_MULTI="1")
    grp = last_json([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                     "--master-port", str(port), "bench.py", "--gpus", "1"] + common[:-1], env=env)
    assert grp["config"]["parallelism"].startswith("slab1") and grp["tracking"]["lost_frames"] == 0
    assert grp["scaling"] == "strong" and grp["rooms_weak"]["scaling"] == "weak" and grp["rooms_weak"]["lost_frames"] == 0
    assert grp["tracking"]["final_pose_f32_hex"] == one["tracking"]["final_pose_f32_hex"]
    # every form ran (a world of one rank: ncclCommInitRank with world 1, the all-reduced ICP, the direct form) and every
    # one of them equals the single context pose for pose and plane for plane
    assert grp["launcher"]["failed_forms"] == {} and grp["ranks_seen"] == 1
    for f in ("rccl", "rccl_icp_allreduce", "direct"):
        assert grp["forms"][f]["matches_single_gpu"] is True and grp["forms"][f]["lost_frames"] == 0, f
    # ... and the launcher's single-context worker is the same measurement as run_single's (within the noise of 12 frames)
    assert 0.5 < grp["single_gpu_same_frames"]["value"] / one["value"] < 2.0
