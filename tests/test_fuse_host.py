"""Volume fusion without a GPU: the two host-only entry points (hsk_invert_rigid, hsk_fuse_footprint) against the numpy twin
(tests/fuse_twin.py), and the twin's own properties -- the ones DESIGN.md 8d claims for the rule: the requantisation round trip,
the identity fuse, the fuse repeated, and a plane that stays a plane to two raw units under a rotation."""
import ctypes as C

import numpy as np
import pytest

import fuse_twin as FT
from fuse_cases import PLANE_TAU, general, plane_case

f32 = np.float32
SIZE = (3.0, 3.0, 3.0)


def observed_volume(n, seed=5, hole=True):
    """a volume observed everywhere (weights 1..9) with a smooth TSDF of both signs; with `hole`, a block nobody observed"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    F = np.sin(x * 0.31 + 0.2) * np.cos(y * 0.23) * np.sin(z * 0.17 + 1.0)
    vol = np.empty((n, n, n, 2), np.int16)
    vol[..., 0] = np.rint(F * 32767).astype(np.int16)
    vol[..., 1] = rng.integers(1, 10, (n, n, n))
    if hole:
        vol[n // 4:n // 2, n // 3:n // 2, 2:n // 3] = 0
    return vol


# ---- hsk_invert_rigid -------------------------------------------------------------------------------------
def test_invert_rigid_is_the_binary64_inverse_rounded_once(hsk):
    from housescan_amd import products
    rng = np.random.default_rng(3)
    for k in range(50):
        m = (FT.rot_about("xyz"[k % 3], rng.uniform(-180, 180), rng.uniform(0, 3, 3), rng.uniform(-5, 5, 3)).astype(np.float64)
             @ FT.rot_about("xyz"[(k + 1) % 3], rng.uniform(-180, 180), rng.uniform(0, 3, 3)).astype(np.float64)).astype(f32)
        inv = products.invert_rigid(m)
        # the binary64 inverse of a rigid matrix, from the binary32 entries: R^T and -R^T t, one rounding
        R, t = m[:3, :3].astype(np.float64), m[:3, 3].astype(np.float64)
        ref = np.eye(4)
        ref[:3, :3] = R.T
        ref[:3, 3] = [-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)]
        assert np.array_equal(inv.view(np.uint32), ref.astype(f32).view(np.uint32))
        assert np.array_equal(inv.view(np.uint32), FT.invert_rigid(m).view(np.uint32))
        assert np.abs(m.astype(np.float64) @ inv.astype(np.float64) - np.eye(4)).max() < 1e-6
        assert np.abs(inv.astype(np.float64) - np.linalg.inv(m.astype(np.float64))).max() < 1e-5


def test_invert_rigid_refuses_what_section_in_room_refuses(hsk):
    lib = hsk._lib.load()
    fp = C.POINTER(C.c_float)
    out = np.zeros(16, f32)

    def rc(m):
        a = np.ascontiguousarray(m, f32).reshape(16)
        return lib.hsk_invert_rigid(a.ctypes.data_as(fp), out.ctypes.data_as(fp))

    good = general()
    assert rc(good) == 0
    bad_row = good.copy()
    bad_row[3, 3] = 2.0
    assert rc(bad_row) == -1
    bad_row = good.copy()
    bad_row[3, 0] = 1e-3
    assert rc(bad_row) == -1
    scaled = good.copy()
    scaled[:3, :3] *= f32(1.01)
    assert rc(scaled) == -1
    sheared = good.copy()
    sheared[0, 1] += f32(0.01)
    assert rc(sheared) == -1
    nan = good.copy()
    nan[1, 1] = np.nan
    assert rc(nan) == -1
    assert lib.hsk_invert_rigid(None, out.ctypes.data_as(fp)) == -1
    assert lib.hsk_invert_rigid(good.reshape(16).ctypes.data_as(fp), None) == -1
    # in place
    a = good.reshape(16).copy()
    assert lib.hsk_invert_rigid(a.ctypes.data_as(fp), a.ctypes.data_as(fp)) == 0
    assert np.array_equal(a.reshape(4, 4).view(np.uint32), FT.invert_rigid(good).view(np.uint32))


# ---- hsk_fuse_footprint -----------------------------------------------------------------------------------
def footprint_cases(n):
    cell = 3.0 / n
    return {
        "identity": (np.eye(4, dtype=f32), (n,) * 3, SIZE),
        "offset": (FT.translation(((5 + 0.5) * cell, -(3 + 0.5) * cell, (2 + 0.5) * cell)), (n,) * 3, SIZE),
        "rotation": (general(n=n), (n,) * 3, SIZE),
        "rotation, far corner": (FT.rot_about("y", 40.0, (1.5, 1.5, 1.5), (2.2, -1.9, 1.8)), (n,) * 3, SIZE),
        "outside": (FT.translation((7.5, 0.0, 0.0)), (n,) * 3, SIZE),
        "outside after a turn": (FT.rot_about("z", 90.0, (0, 0, 0), (-0.5, 0.0, 0.0)), (n,) * 3, SIZE),
        "larger source": (FT.translation((-1.0, -0.5, -1.2)), (n // 2, n // 2, n // 2), (1.5, 1.5, 1.5)),
        "house": (FT.translation((2.9, 0.0, 0.0)), (2 * n, n, n), (6.0, 3.0, 3.0)),
    }


@pytest.mark.parametrize("name", list(footprint_cases(32)))
def test_footprint_matches_the_twin_and_holds_every_fused_voxel(hsk, name):
    from housescan_amd import products
    n = 40 if name in ("rotation", "offset") else 32
    m, ddims, dsize = footprint_cases(n)[name]
    box = products.fuse_footprint((n,) * 3, SIZE, ddims, dsize, m)
    assert box == FT.footprint((n,) * 3, SIZE, ddims, dsize, m), name
    src = observed_volume(n, hole=False)
    dst = np.zeros((ddims[2], ddims[1], ddims[0], 2), np.int16)
    _, _, st = FT.fuse(dst, dsize, src, SIZE, m)
    if name.startswith("outside"):
        assert box == (0,) * 6 and st["n_fused"] == 0
        return
    assert st["n_fused"] > 0, name
    assert FT.box_contains(box, st["box"]), f"{name}: footprint {box} does not hold the fused voxels' box {st['box']}"
    for i in range(3):
        assert 0 <= box[2 * i] < box[2 * i + 1] <= ddims[i]
    if name == "identity":
        assert box == (0, n, 0, n, 0, n)
    if name == "larger source":       # the source covers the destination: clipped to all of it
        assert box == (0, n // 2) * 3
    if name in ("offset", "rotation, far corner", "house"):   # ... and it is a footprint, not the whole destination
        assert (box[1] - box[0]) * (box[3] - box[2]) * (box[5] - box[4]) < ddims[0] * ddims[1] * ddims[2]


def test_footprint_refusals(hsk):
    lib = hsk._lib.load()
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    d = np.array([32, 32, 32], np.int32)
    s = np.array(SIZE, f32)
    box = np.zeros(6, np.int32)
    bp = box.ctypes.data_as(C.POINTER(C.c_int32))
    m = general().reshape(16)
    args = lambda **kw: [kw.get("sd", d).ctypes.data_as(ip), kw.get("ss", s).ctypes.data_as(fp), d.ctypes.data_as(ip),  # noqa: E731
                         s.ctypes.data_as(fp), kw.get("m", m).ctypes.data_as(fp), bp]
    assert lib.hsk_fuse_footprint(*args()) == 0
    assert lib.hsk_fuse_footprint(*args(sd=np.array([32, 0, 32], np.int32))) == -1
    assert lib.hsk_fuse_footprint(*args(ss=np.array([3.0, -1.0, 3.0], f32))) == -1
    scaled = general()
    scaled[:3, :3] *= f32(1.1)
    assert lib.hsk_fuse_footprint(*args(m=scaled.reshape(16))) == -1
    a = args()
    a[5] = None
    assert lib.hsk_fuse_footprint(*a) == -1


# ---- the rule's own properties ---------------------------------------------------------------
def test_requantisation_round_trip_is_exact():
    raw = np.arange(-32768, 32768).astype(np.int32)
    F = (raw.astype(f32) / f32(32767)).astype(f32)
    assert np.array_equal(np.rint((F * f32(32767)).astype(f32)).astype(np.int32), raw)


def test_identity_fuse_reproduces_the_source_and_a_second_fuse_doubles_the_weight():
    n = 64
    src = observed_volume(n, hole=False)
    src[..., 1] = 1
    out, _, st = FT.fuse(np.zeros_like(src), SIZE, src, SIZE, np.eye(4, dtype=f32))
    assert st["n_fused"] == (n - 2) ** 3 == 238328
    inner = (slice(1, n - 1),) * 3
    assert st["fused"][inner].all() and st["box"] == (1, n - 1) * 3
    assert np.array_equal(out[inner][..., 0], src[inner][..., 0])
    assert (out[inner][..., 1] == 1).all()
    shell = ~st["fused"]
    assert (out[shell] == 0).all()
    twice, _, st2 = FT.fuse(out, SIZE, src, SIZE, np.eye(4, dtype=f32))
    assert st2["n_fused"] == (n - 2) ** 3
    assert np.array_equal(twice[..., 0], out[..., 0])
    assert np.array_equal(twice[inner][..., 1], 2 * out[inner][..., 1]) and (twice[shell] == 0).all()


def test_unobserved_taps_and_weights():
    """a voxel takes a sample only when all eight taps are observed; the weight it takes is their minimum; the weight saturates"""
    n = 32
    src = observed_volume(n)
    m = general(n=n)
    dst = observed_volume(n, seed=9, hole=False)
    dst[..., 1] = 125
    out, _, st = FT.fuse(dst, SIZE, src, SIZE, m)
    assert 0 < st["n_fused"] < n ** 3
    assert np.array_equal(out[~st["fused"]], dst[~st["fused"]])
    w = out[st["fused"]][:, 1]
    assert w.min() >= 126 and w.max() == FT.MAX_WEIGHT and (w == FT.MAX_WEIGHT).any() and (w < FT.MAX_WEIGHT).any()
    # no voxel whose source point lies in or next to the hole took a sample from it: fusing the hole alone fuses nothing
    only_hole = np.zeros_like(src)
    _, _, st0 = FT.fuse(dst, SIZE, only_hole, SIZE, m)
    assert st0["n_fused"] == 0


def test_colour_is_merged_by_its_weights():
    n = 32
    rng = np.random.default_rng(1)
    src, dst = observed_volume(n), observed_volume(n, seed=2, hole=False)
    sc = rng.integers(0, 256, (n, n, n, 4)).astype(np.uint8)
    sc[..., 3] = rng.integers(0, 3, (n, n, n)) * 40
    dc = rng.integers(0, 256, (n, n, n, 4)).astype(np.uint8)
    dc[..., 3] = rng.integers(0, 64, (n, n, n))
    m = general(n=n)
    out, oc, st = FT.fuse(dst, SIZE, src, SIZE, m, dc, sc, max_w=64)
    assert 0 < st["n_colored"] < st["n_fused"]
    assert np.array_equal(oc[~st["fused"]], dc[~st["fused"]])
    assert oc[..., 3].max() == 64
    # without a colour volume on one side the TSDF result is the same and the colour is not touched
    out2, oc2, st2 = FT.fuse(dst, SIZE, src, SIZE, m, dc, None)
    assert np.array_equal(out2, out) and np.array_equal(oc2, dc) and st2["n_colored"] == 0


# ---- a plane stays a plane ---------------------------------------------------------------------------------


def test_a_rotated_plane_stays_within_two_raw_units():
    """trilinear interpolation reproduces a linear field exactly, so what is left of the crossing's error is two quantisations
    of half a raw unit each: 2 tau / 32767 = 18 um is the bar (the twin: 4.4 um worst over 2 852 crossings, 207 700 voxels
    fused; a prototype of the rule that counted crossings its own way: 4.6 um over 5 146)"""
    src, m, nrm, d = plane_case()
    out, _, st = FT.fuse(np.zeros_like(src), SIZE, src, SIZE, m)
    assert st["n_fused"] > 100000
    pts = FT.crossings(out, SIZE)
    assert len(pts) > 1000
    err = np.abs(pts @ nrm - d)
    print(f"fused {st['n_fused']}, {len(pts)} crossings, worst {err.max() * 1e6:.2f} um")
    assert err.max() <= 2 * PLANE_TAU / 32767
