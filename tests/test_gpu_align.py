"""hsk_align_cloud / hsk_align_volume on the GPU against the numpy restatement of the rule (tests/align_twin.py), BIT FOR BIT: the
refined matrix, the status, the iteration count, every iteration's n_used and rms, the last step and the last 28 sums.  The
scene is test_align_host's: a room seen from inside with a box on its floor as an 80 x 64 x 48 destination over 3 m (three
different cells), and a 64^3 source holding the same scene moved by a known matrix, whose cloud and normals come from the
library's own extract_cloud_attrs.  Then: a destination grown by the tracker with deferred weights pending, hsk_align_volume
against the two calls it stands for, nothing else of either context moved, align-then-fuse, and the errors."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import fuse_twin as FT
import np_twin as T
from align_cases import HALF_CELL_M, M_TRUE, TAU
from kit import same_bits, volume_ctx

pytestmark = pytest.mark.gpu
f32 = np.float32
M_TRUE32 = M_TRUE.astype(f32)
PERTURBED = (AT.rigid(2.0, (150.0, -100.0, 120.0)) @ M_TRUE).astype(f32)
ROOM_FRAMES = 720

_S = {}


def dst_ctx(hsk, dims=AT.DST_DIMS, size=AT.DST_SIZE, **over):
    return volume_ctx(hsk, dims, size, **over)


@pytest.fixture(scope="module")
def scene(hsk):
    """the destination and the source contexts with their host volumes, and the source's cloud with normals; made once.  The
    source is given the destination's truncation distance, so that it can also be fused (test 8)"""
    dst = dst_ctx(hsk)
    src = hsk.KinfuTracker(n=64, trunc_dist_m=float(TAU))
    d_vol = AT.scene_volume(AT.DST_DIMS, AT.DST_SIZE, TAU)
    s_vol = AT.scene_volume(AT.SRC_DIMS, AT.SRC_SIZE, TAU, M=M_TRUE)
    dst.upload_tsdf(d_vol)
    src.upload_tsdf(s_vol)
    xyz, nrm, _, total, _ = src.extract_cloud_attrs(rgb=False)
    assert total == len(xyz) and 3000 <= total <= 40000, total
    assert len(xyz) % 64 != 0 and len(xyz) % 256 != 0, "pick another scene: the cloud's size hides the tail of the last wave"
    _S.update(dst=dst, src=src, d_vol=d_vol, s_vol=s_vol, xyz=xyz, nrm=nrm)
    yield _S
    dst.close()
    src.close()
    _S.clear()


def twin(s, M0, xyz=None, nrm=None, **kw):
    return AT.align(s["d_vol"], AT.DST_SIZE, TAU, s["xyz"] if xyz is None else xyz, s["nrm"] if nrm is None else nrm, M0, **kw)


def assert_same(got, ref, what):
    """a device result (matrix, dict) against a twin result, zero differences"""
    (m, st), (rm, rs) = got, ref
    print(f"{what}: {st['status']} after {st['iterations']}, n_points {st['n_points']} stride {st['stride']}, n_used {st['n_used']}, "
          f"rms {[float(v) for v in st['rms_m']]}")
    assert st["status"] == AT.STATUS[rs["status"]], f"{what}: status {st['status']} != {AT.STATUS[rs['status']]}"
    assert st["iterations"] == rs["iterations"], f"{what}: iterations {st['iterations']} != {rs['iterations']}"
    assert (st["n_points"], st["stride"]) == (rs["n_points"], rs["stride"]), what
    assert st["n_used"] == rs["n_used"], f"{what}: n_used {st['n_used']} != {rs['n_used']}"
    assert same_bits(st["sums_last"], rs["sums_last"]), f"{what}: sums {st['sums_last']} != {rs['sums_last']}"
    assert same_bits(st["rms_m"], rs["rms_m"]), f"{what}: rms {st['rms_m']} != {rs['rms_m']}"
    assert same_bits(st["x_last"], rs["x_last"]), f"{what}: x_last {st['x_last']} != {rs['x_last']}"
    assert same_bits(m, rm), f"{what}: matrix {m} != {rm}"


# ---- 4. against the twin ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["probes3", "direct", "stride3"])
def test_align_cloud_matches_the_twin(hsk, scene, case):
    s = scene
    n = len(s["xyz"])
    kw = {"probes3": dict(J=3), "direct": dict(J=0), "stride3": dict(J=3, max_points=(n + 2) // 3)}[case]
    ref = twin(s, PERTURBED, **kw)
    dev_kw = {k: v for k, v in kw.items() if k != "J"}
    got = s["dst"].align_cloud(s["xyz"], s["nrm"], PERTURBED, probes=kw["J"], **dev_kw)
    assert_same(got, ref, case)
    if case == "stride3":
        assert ref[1]["stride"] == 3 and ref[1]["n_points"] == (n + 2) // 3
    if case != "direct":
        assert ref[1]["status"] == AT.CONVERGED and ref[1]["n_used"][-1] > 0.8 * ref[1]["n_points"]
        err = AT.point_error(got[0], M_TRUE, s["xyz"][ref[1]["index"]][ref[1]["used"]])
        print(f"{case}: {err * 1e3:.3f} mm from the truth")
        assert err <= HALF_CELL_M


@pytest.mark.parametrize("count", [0, 63, 1000])
def test_point_counts_and_the_first_iterations_sums(hsk, scene, count):
    """no point, fewer than a wave, and a count that is a multiple neither of 64 nor of the block's 256; one iteration, so that
    sums_last is the first iteration's"""
    s = scene
    xyz, nrm = s["xyz"][2000:2000 + count], s["nrm"][2000:2000 + count]
    ref = twin(s, PERTURBED, xyz, nrm, max_iters=1, min_points=1)
    got = s["dst"].align_cloud(xyz, nrm, PERTURBED, max_iters=1, min_points=1)
    assert_same(got, ref, f"{count} points")
    if count == 0:
        assert got[1]["status"] == "few" and same_bits(got[0], PERTURBED) and got[1]["n_used"] == [0]
    else:
        assert got[1]["status"] in ("max_iters", "degenerate") and 0 < got[1]["n_used"][0] <= count and np.abs(got[1]["sums_last"]).max() > 0


def test_the_whole_cloud_in_one_iteration(hsk, scene):
    s = scene
    ref = twin(s, PERTURBED, max_iters=1)
    assert_same(s["dst"].align_cloud(s["xyz"], s["nrm"], PERTURBED, max_iters=1), ref, "one iteration")
    assert ref[1]["status"] == AT.MAX_ITERS and ref[1]["n_used"][0] > 2000
    # NaN normals (the cloud's rim has them; here every other point): such points never contribute
    bad = s["nrm"].copy()
    bad[::2] = np.nan
    ref = twin(s, PERTURBED, nrm=bad, max_iters=2)
    assert_same(s["dst"].align_cloud(s["xyz"], bad, PERTURBED, max_iters=2), ref, "NaN normals")
    assert not ref[1]["used"][::2].any() and ref[1]["used"].any()


# ---- 5. a destination grown by the tracker -------------------------------------------------------------------------
def test_a_destination_with_deferred_weights(hsk):
    """four frames of a room integrated at 64^3 leave free-space weights in the summaries; the twin is fed by the download of a
    second, identically grown context (the download writes them back), the device call writes them back itself.  (Every
    deferred state keeps its weights >= 1 in the volume, DESIGN.md 2.2, so the rule's Ws > 0 alone would not tell; the volume
    downloaded behind the call must be the twin's input.)"""
    poses = [hsk.synth_room_pose(0, k, ROOM_FRAMES) for k in (0, 12, 24, 36)]
    depths = [hsk.synth_room_depth(0, p) for p in poses]

    def grown():
        trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
        for d, p in zip(depths, poses):
            trk.integrate(d, p)
        return trk

    a, b = grown(), grown()
    try:
        vol = a.download_tsdf()
        assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
        xyz, nrm, _, total, _ = a.extract_cloud_attrs(rgb=False)
        assert total == len(xyz) > 2000
        tau = T.tau_of((3.0,) * 3, (64,) * 3, 0.03)
        M0 = AT.rigid(0.5, (20.0, -15.0, 10.0)).astype(f32)
        ref = AT.align(vol, (3.0,) * 3, tau, xyz, nrm, M0)
        assert ref[1]["n_used"][0] > 1000
        assert_same(b.align_cloud(xyz, nrm, M0), ref, "deferred weights")
        assert np.array_equal(b.download_tsdf(), vol)
    finally:
        a.close()
        b.close()


# ---- 6. hsk_align_volume ---------------------------------------------------------------------------------------------
def test_align_volume_is_the_two_calls(hsk, scene):
    s = scene
    m_v, st_v = s["dst"].align_from(s["src"], PERTURBED)
    m_c, st_c = s["dst"].align_cloud(s["xyz"], s["nrm"], PERTURBED)
    assert same_bits(m_v, m_c)
    for key in st_c:
        assert same_bits(np.asarray(st_v[key]), np.asarray(st_c[key])), key
    ref = twin(s, PERTURBED)
    assert_same((m_v, st_v), ref, "align_from")
    assert st_v["status"] == "converged"
    err = AT.point_error(m_v, M_TRUE, s["xyz"][ref[1]["used"]])
    print(f"align_from: {err * 1e3:.3f} mm from the truth")
    assert err <= HALF_CELL_M


# ---- 7. nothing else moved ---------------------------------------------------------------------------------------------
def test_nothing_else_moved(hsk, scene):
    s = scene
    dst, src = s["dst"], s["src"]
    pose = dst.get_pose()
    cloud, total = dst.extract_cloud()
    src_cloud = src.extract_cloud_attrs(rgb=False)
    dst.align_from(src, PERTURBED)
    dst.align_cloud(s["xyz"], s["nrm"], PERTURBED, probes=0)
    assert np.array_equal(dst.download_tsdf(), s["d_vol"]) and same_bits(dst.get_pose(), pose)
    again, total2 = dst.extract_cloud()
    assert total2 == total and same_bits(again, cloud)
    assert np.array_equal(src.download_tsdf(), s["s_vol"])
    for a, b in zip(src_cloud, src.extract_cloud_attrs(rgb=False)):
        assert (a is None and b is None) or same_bits(np.asarray(a), np.asarray(b))


# ---- 8. align, then fuse ------------------------------------------------------------------------------------------------
def test_align_then_fuse(hsk, scene):
    """the source fused into an empty volume of the destination's shape by the refined matrix takes as many samples as by the
    true one, to within what the twin's own two fuses differ by (measured here on the CPU: 13 of 142 028 voxels, 0.009 %)"""
    s = scene
    m_out, st = s["dst"].align_cloud(s["xyz"], s["nrm"], PERTURBED)
    assert st["status"] == "converged"
    empty = np.zeros_like(s["d_vol"])
    n_out = FT.fuse(empty, AT.DST_SIZE, s["s_vol"], AT.SRC_SIZE, m_out)[2]["n_fused"]
    n_true = FT.fuse(empty, AT.DST_SIZE, s["s_vol"], AT.SRC_SIZE, M_TRUE32)[2]["n_fused"]
    share = abs(n_out - n_true) / n_true
    print(f"the twin's fuses: {n_out} by the refined matrix, {n_true} by the true one, share {share:.5%}")
    assert n_true > 20000 and share < 0.01
    got = []
    for m in (m_out, M_TRUE32):
        house = dst_ctx(hsk, trunc_dist_m=float(TAU))
        try:
            got.append(house.fuse_from(s["src"], m)["n_fused"])
        finally:
            house.close()
    print(f"the device's fuses: {got}")
    assert abs(got[0] - got[1]) <= abs(n_out - n_true)     # (in voxels: share * n_true in binary64 falls short of the integer)


# ---- 9. errors ---------------------------------------------------------------------------------------------------------
def test_errors(hsk, scene):
    s = scene
    lib = hsk._lib.load()
    dst, src = s["dst"], s["src"]
    xyz, nrm = np.ascontiguousarray(s["xyz"][:512]), np.ascontiguousarray(s["nrm"][:512])
    fp = C.POINTER(C.c_float)
    sentinel = np.full(16, 7.0, f32)
    out = sentinel.copy()
    eye = np.eye(4, dtype=f32)

    def cloud(d=dst.h, p=xyz, q=nrm, n=512, m=eye, o=out, params=None):
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        mp = None if m is None else np.ascontiguousarray(m, f32).reshape(16).ctypes.data_as(fp)
        rc = lib.hsk_align_cloud(d, ptr(p), ptr(q), n, mp, None if params is None else C.byref(params), None if o is None else o.ctypes.data_as(fp), None)
        assert same_bits(out, sentinel), "a refused call wrote the matrix"
        return rc

    def volume(d=dst.h, sc=src.h, m=eye, o=out):
        mp = None if m is None else np.ascontiguousarray(m, f32).reshape(16).ctypes.data_as(fp)
        rc = lib.hsk_align_volume(d, sc, mp, None, None if o is None else o.ctypes.data_as(fp), None)
        assert same_bits(out, sentinel), "a refused call wrote the matrix"
        return rc

    def params(**kw):
        p = hsk._lib.HskAlignParams()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    # HSK_ERR_ARG: null arguments
    assert cloud(d=None) == -1 and cloud(p=None) == -1 and cloud(q=None) == -1 and cloud(m=None) == -1 and cloud(o=None) == -1
    assert volume(d=None) == -1 and volume(sc=None) == -1 and volume(m=None) == -1 and volume(o=None) == -1
    assert volume(sc=dst.h) == -1 and "same context" in lib.hsk_last_error(dst.h).decode()
    # ... a matrix that is not rigid
    scaled = eye.copy()
    scaled[:3, :3] *= f32(1.05)
    row = eye.copy()
    row[3, 3] = 0.5
    for m in (scaled, row):
        assert cloud(m=m) == -1 and "rigid" in lib.hsk_last_error(dst.h).decode()
        assert volume(m=m) == -1
    # ... a parameter out of range
    for bad in (params(max_iters=65), params(max_iters=-1), params(probes=9), params(probes=-2), params(cos_gate=1.5), params(cos_gate=-0.5),
                params(cos_gate=float("nan")), params(max_points=(1 << 20) + 1), params(eps_rot=-1.0), params(eps_trans_m=float("nan")),
                params(max_rot=-0.1), params(max_shift_m=float("inf"))):
        assert cloud(params=bad) == -1 and "parameter" in lib.hsk_last_error(dst.h).decode()
    # ... the exactness conditions: half the diagonal of a 10 m box is 8.66 m; 9 probes of 0.9 m reach 8.1 m
    big = hsk.KinfuTracker(n=64, vol_size_m=(10.0, 10.0, 10.0))
    coarse = hsk.KinfuTracker(n=64, trunc_dist_m=0.9)
    try:
        assert cloud(d=big.h) == -1 and "diagonal" in lib.hsk_last_error(big.h).decode()
        assert cloud(d=coarse.h, params=params(probes=8)) == -1 and "truncation" in lib.hsk_last_error(coarse.h).decode()
        assert cloud(d=coarse.h, params=params(probes=7), o=np.zeros(16, f32)) == 0
    finally:
        big.close()
        coarse.close()
    # no point at all is not an error
    ok_out = np.zeros(16, f32)
    assert cloud(p=None, q=None, n=0, o=ok_out) == 0 and same_bits(ok_out, eye.reshape(16))
    # HSK_ERR_STATE: a frame in flight, in either context
    depth = hsk.synth_depth(hsk.synth_pose(0))
    busy = hsk.KinfuTracker(n=64)
    try:
        busy.submit_frame(depth)
        assert cloud(d=busy.h) == -3 and "in flight" in lib.hsk_last_error(busy.h).decode()
        assert volume(d=busy.h) == -3 and volume(sc=busy.h) == -3 and "in flight" in lib.hsk_last_error(dst.h).decode()
        busy.wait_frame()
        assert cloud(d=busy.h, o=np.zeros(16, f32)) == 0
    finally:
        busy.close()
    # ... a context that stores part of its volume, and the slabs of a group
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        assert cloud(d=part.h) == -3 and "slab" in lib.hsk_last_error(part.h).decode()
        assert volume(d=part.h) == -3 and volume(sc=part.h) == -3
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(depth)
        for i in range(g.n_slabs()):
            assert cloud(d=g.slab(i).h) == -3 and volume(d=g.slab(i).h) == -3 and volume(sc=g.slab(i).h) == -3
        assert g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))[1]
    finally:
        g.close()
    # the Python mirror raises
    with pytest.raises(hsk.KinfuError, match="rigid"):
        dst.align_cloud(xyz, nrm, scaled)
    with pytest.raises(hsk.KinfuError, match="same context"):
        dst.align_from(dst, eye)
    with pytest.raises(ValueError, match="normals"):
        dst.align_cloud(xyz, nrm[:10], eye)
