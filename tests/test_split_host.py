"""The scene split without a GPU: the kernels' shared text (housescan_amd/csrc/hsk_split_point.h, compiled for the host) against the
numpy twin (tests/split_twin.py) on the volumes the GPU tests use; the twin's own pins -- hand-computed voxels, the analytic room
with a box on the floor, against the wall and lifted off it, and the room after their removal; the default
parameters; the C layout of the new structs and their Python mirror; the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import diff_twin as DT
import kit
import split_cases as SC
import split_twin as ST
from diff_cases import words_of
from kit import blocked
from split_cases import records_as_dicts


# ---- 1. the twin's own pins ---------------------------------------------------------------------------------------------------------
def test_the_twin_on_hand_computed_voxels():
    """a 1 x 1 x 8 line, cell 1/16 m (every product below is exact), the plane x = 0.25 m with its normal along +x: s_k = (x + 0.5) /
    16 - 0.25 metres; front 0.05, back 0.15"""
    vol = np.array([(-100, 1), (-300, 1), (-600, 1), (-1000, 1), (500, 1), (0, 0), (-32768, 1), (-7, 1)], np.int16).reshape(1, 1, 8, 2)
    size, dims = (0.5, 0.0625, 0.0625), (8, 1, 1)
    r = ST.quantise([[1, 0, 0, -0.25]], [ST.WALL], size, dims, 0.1, 0.05, 0.15, 0.5)
    assert (r["Q"][0].tolist(), int(r["Qd"][0]), r["N"][0].tolist(), r["w"].tolist()) == ([2 ** 25, 0, 0], -2 ** 28, [4096, 0, 0], [4096] * 3)
    assert [int(ST.distance(r, 0, (1, 1, 8))[0, 0, x]) for x in (0, 3, 4)] == [2 ** 25 - 2 ** 28, 7 * 2 ** 25 - 2 ** 28, 9 * 2 ** 25 - 2 ** 28]
    # one-sided at x = 0 (2 (r(1) - r(0))), central at 1..3 and at 5 (itself unobserved, r = 0 does not enter), one-sided at 4, at 6
    # (only x = 7 is observed; -32768 counts as -32767) and at 7
    assert ST.gradient(vol)[0][0, 0].tolist() == [-400, -500, -700, 1100, 3000, -32767 - 500, 2 * (-7 + 32767), 2 * (-7 + 32767)]
    cls, plane, n_edge, n_flat = ST.classify(vol, r)
    # x = 0 lies 0.219 m behind the plane: not NEAR; 1..3 are NEAR (s = -0.156 is not: back = 0.15 -> x = 1 is OBJECT too), but their
    # gradients point away from the normal at 1 and 2; 3 is ALIGNED; 4 and 5 are not INSIDE; 6 and 7 lie in front of the front
    assert cls[0, 0].tolist() == [ST.OBJECT, ST.OBJECT, ST.OBJECT, ST.WALL, ST.NONE_CLS, ST.NONE_CLS, ST.OBJECT, ST.OBJECT]
    assert plane[0, 0].tolist() == [255, 255, 255, 0, 255, 255, 255, 255] and (n_edge, n_flat) == (0, 0)
    out, label, recs, n_minor = ST.objects(cls, plane, r, 3)
    assert out[0, 0].tolist() == [ST.OBJECT] * 3 + [ST.WALL, 0, 0, ST.MINOR, ST.MINOR] and n_minor == 1 and label[0, 0].tolist() == [0, 0, 0] + [ST.NONE] * 5
    assert recs == [{"root": (0, 0, 0), "n_voxels": 3, "sum": (3, 0, 0), "lo": (0, 0, 0), "hi": (3, 1, 1), "contact": (0, 0, 1, 0), "plane_mask": 1,
                     "height_lo": 0, "height_hi": 0}]
    # the edge rule, the tie and G = 0: an isolated voxel is ALIGNED with every plane; NEAR two planes at equal |s| the lower index
    # wins; a gradient along -x NEAR two planes along +x and +y agrees with neither and takes the nearer
    one = np.zeros((3, 3, 3, 2), np.int16)
    one[1, 1, 1] = (-5, 1)
    two = ST.quantise([[1, 0, 0, -0.09375], [1, 0, 0, -0.09375], [0, 1, 0, -0.0625]], [ST.OTHER, ST.FLOOR, ST.WALL], (0.1875,) * 3, (3, 3, 3), 0.1, 0.05, 0.15, 0.5)
    cls, plane, n_edge, n_flat = ST.classify(one, two)
    assert (cls[1, 1, 1], plane[1, 1, 1], n_edge, n_flat) == (ST.OTHER, 0, 0, 1)
    one[1, 1, 2], one[1, 1, 0] = (-900, 1), (-1, 1)
    cls, plane, n_edge, n_flat = ST.classify(one, two)
    assert (cls[1, 1, 1], plane[1, 1, 1], n_edge) == (ST.OTHER, 0, 2)                 # s = 0 for planes 0 and 1, 0.03125 for plane 2; (0, 1, 1) likewise
    assert ST.plane_kinds([[0, 0, 1, 0]], (0, 0, 1)).tolist() == [ST.FLOOR]


def test_the_plane_word_on_hand_computed_distances():
    r = ST.quantise([[0, 0, 1, -0.25]], [ST.FLOOR], (0.0625, 0.0625, 0.5), (1, 1, 8), 0.125, 0.05, 0.15, 0.5)
    vol = np.zeros((8, 1, 1, 2), np.int16)
    rec = {"root": (0, 0, 0), "n_voxels": 1, "lo": (0, 0, 0), "hi": (1, 1, 8), "plane_mask": 1}
    label = np.full((8, 1, 1), ST.NONE, np.uint32)
    label[0] = 0
    out, _, st = ST.remove(vol, label, [rec], r, None, ST.RESTORE, 0, 7)
    # s = (z + 0.5) / 16 - 0.25 = -7/32 .. 7/32 in steps of 1/16; tau = 1/8: below -tau word 0; raw = floor((65534 s / tau + 1) / 2)
    want = [(0, 0), (0, 0)] + [(int(np.floor((65534 * min(s, 4) / 4 + 1) / 2)), 7) for s in (-3, -1, 1, 3, 5, 7)]
    assert out[:, 0, 0].tolist() == [list(w) for w in want] and want[2] == (-24575, 7) and want[-1] == (32767, 7)
    assert st == {"n_objects": 1, "n_targets": 1, "n_written": 8, "n_restored": 6, "n_colored": 0}


def test_the_analytic_room_on_the_twin():
    """DESIGN.md 8r's figures: 64 x 48 x 40, cell 0.05, floor z = 6.3, wall x = 50.4, dist 0.5 cell, back tau + 0.5 cell"""
    cls, _, _, recs, st = SC.twin_of(("room", "the empty room"))
    assert st["n_class"][ST.OBJECT] == st["n_class"][ST.MINOR] == 0 and not recs and st["n_edge"] > 0       # the edge rule covers the floor-wall edge
    lo, hi = DT.ROOM_BOX
    cls, _, label, recs, st = SC.twin_of(("room", "a box on the floor"))
    assert st["n_objects"] == 1 and recs[0]["contact"][ST.FLOOR - 1] > 0 and recs[0]["plane_mask"] == 1
    z, y, x = np.nonzero(label != ST.NONE)
    assert (x + 0.5 > lo[0]).all() and (x + 0.5 < hi[0]).all() and (y + 0.5 > lo[1]).all() and (y + 0.5 < hi[1]).all() and (z + 0.5 > lo[2]).all() and (z + 0.5 < hi[2]).all()
    assert SC.twin_of(("room", "a box against the wall"))[3][0]["plane_mask"] == 3 and len(SC.twin_of(("room", "a box against the wall"))[3]) == 1
    lifted = SC.twin_of(("room", "a box lifted off the floor"))[3]
    assert len(lifted) == 1 and lifted[0]["plane_mask"] == 0 and lifted[0]["contact"] == (0, 0, 0, 0)
    masks = sorted(c["plane_mask"] for c in SC.twin_of(("room", "two boxes"))[3])
    assert masks == [1, 3]


@pytest.mark.parametrize("name", ["a box on the floor", "a box against the wall", "a box lifted off the floor", "two boxes"])
def test_a_removal_gives_the_empty_room_on_the_twin(name):
    """after remove_objects(RESTORE, halo 3) the volume equals room(None) within 1 raw unit wherever both are observed (one unit is
    what the 2^-30 m quantisation can flip at a rounding boundary) and its crossing counts are the empty room's"""
    out, _, st = SC.remove_twin(("room", name), SC.ALL, ST.RESTORE, 3 if name != "two boxes" else 4, 1)
    empty = DT.room(None)
    both = (out[..., 1] != 0) & (empty[..., 1] != 0)
    worst = int(np.abs(out[..., 0].astype(np.int64) - empty[..., 0])[both].max())
    counts = [int(c.sum()) for c in DT.crossings(out)]
    print(f"{name}: {st}, worst difference {worst}, crossings z, y, x {counts}")
    assert worst <= 1 and counts == [2400, 0, 1632] and counts == [int(c.sum()) for c in DT.crossings(empty)]
    assert (st["n_restored"] == 0) == (name == "a box lifted off the floor")


def test_the_cases_reach_what_they_are_for():
    """the conditions of the shared volumes, on the twin"""
    for dims in SC.RANDOM_DIMS:
        for n in SC.RANDOM_PLANES:
            cls, plane, label, recs, st = SC.twin_of(("random", dims, n))
            assert st["n_objects"] >= 1 and st["n_minor_objects"] >= 1, (dims, n)
            assert (n == 0) == (sum(st["n_class"][1:5]) == 0), (dims, n)
        st = SC.twin_of(("random", dims, 64))[4]
        assert st["n_edge"] > 0 and all(v > 0 for v in st["n_class"]), dims
        assert any(c["lo"][0] < 16 < c["hi"][0] and c["lo"][1] < 16 < c["hi"][1] and c["lo"][2] < 8 < c["hi"][2] for c in SC.twin_of(("random", dims, 7))[3]), dims
    assert SC.rule_of(SC.case_of(("random", SC.ANISO_DIMS, 7, SC.ANISO_SIZE)))["w"].tolist() == [4096, 3072, 3840]
    cls, plane, label, recs, st = SC.twin_of(("shape", "objects in the small room"))
    assert [c["n_voxels"] for c in recs] == [125, 27, 27, 12] and st["n_minor_objects"] == 2 and st["n_class"][ST.MINOR] == 12 and st["n_no_normal"] >= 2
    assert recs[0]["lo"] == (14, 14, 6) and recs[0]["hi"] == (19, 19, 11) and recs[1]["root"] == (20, 8, 10) and recs[2]["lo"] == (0, 0, 17)
    assert (cls[12, 5, 10], cls[4, 20, 8], plane[4, 20, 8]) == (ST.MINOR, ST.FLOOR, 0)
    cls, plane, label, recs, st = SC.twin_of(("shape", "a plane inside each grid face"))
    assert all(v > 0 for v in st["n_class"][1:6]) and sorted(np.unique(plane).tolist()) == [0, 1, 2, 3, 4, 5, 255] and bin(recs[0]["plane_mask"]) == "0b111111"
    cls, plane, label, recs, st = SC.twin_of(("shape", "twice the planes and a block at the edge"))
    assert st["n_class"][ST.OTHER] == st["n_class"][ST.CEILING] == 0 and st["n_edge"] > 0 and set(np.unique(plane).tolist()) <= {0, 1, 255}
    c = SC.case_of(("shape", "twice the planes and a block at the edge"))
    plain = ST.classify(SC.small_room(), SC.rule_of(c))
    assert (plane[4, 9:15, 26] != 255).all() and st["n_edge"] > plain[2]             # the block's voxels at the edge: y-gradients, classed all the same
    cls, plane, label, recs, st = SC.twin_of(("shape", "no planes"))
    assert st["n_class"][ST.OBJECT] + st["n_class"][ST.MINOR] == int(ST.inside(SC.case_of(("shape", "no planes"))["vol"]).sum()) and recs[0]["plane_mask"] == 0


# ---- 2. the kernels' shared text on the host -------------------------------------------------------------------------------------
OBJECT_DTYPE = np.dtype([("root", "<i4", (3,)), ("pad", "<i4"), ("n_voxels", "<u8"), ("sum", "<u8", (3,)), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                         ("contact", "<u4", (4,)), ("plane_mask", "<u8"), ("height_lo", "<i4"), ("height_hi", "<i4")])


def run_harness(exe, tmp_path, c, rule, roots, mode, halo, fill_weight, color, voxels, radius):
    Z, Y, X = c["vol"].shape[:3]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([X, Y, Z, len(rule["Q"]), c["params"]["min_voxels"], mode, halo, fill_weight, color is not None, radius, len(voxels),
                          -1 if roots is None else len(roots)], np.int32).tobytes())
        f.write(np.array([rule["front"], rule["back"], rule["tauq"], *rule["w"], rule["floor"]], np.int64).tobytes())
        f.write(np.array([rule["cos2"]], np.float64).tobytes())
        for k in range(len(rule["Q"])):
            f.write(np.array([*rule["Q"][k], rule["Qd"][k], *rule["N"][k], rule["kind"][k]], np.int64).tobytes())
        f.write(blocked(c["vol"]).tobytes())
        if color is not None:
            f.write(np.ascontiguousarray(color).tobytes())
        f.write(np.asarray(voxels, np.int32).tobytes())
        f.write(np.asarray([] if roots is None else roots, np.uint32).tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    n, m = X * Y * Z, len(voxels)
    cls = np.frombuffer(raw, np.uint8, n).reshape(Z, Y, X)
    plane = np.frombuffer(raw, np.uint8, n, n).reshape(Z, Y, X)
    label = np.frombuffer(raw[2 * n:6 * n], np.uint32).reshape(Z, Y, X)
    n_kept, n_minor, n_edge, n_flat = map(int, np.frombuffer(raw[6 * n:6 * n + 32], np.uint64))
    off = 6 * n + 32
    recs = np.frombuffer(raw[off:off + 104 * n_kept], OBJECT_DTYPE)
    off += 104 * n_kept
    at = (np.frombuffer(raw, np.uint8, m, off), np.frombuffer(raw, np.uint8, m, off + m), np.frombuffer(raw[off + 2 * m:off + 6 * m], np.uint32))
    off += 6 * m
    out = words_of(raw[off:off + 4 * n], n, 0).reshape(Z, Y, X, 2)
    off += 4 * n
    col = None
    if color is not None:
        col = np.frombuffer(raw, np.uint8, 4 * n, off).reshape(Z, Y, X, 4)
        off += 4 * n
    st = dict(zip(("n_objects", "n_targets", "n_written", "n_restored", "n_colored"), map(int, np.frombuffer(raw[off:off + 40], np.uint64))))
    return cls, plane, label, recs, (n_minor, n_edge, n_flat), at, out, col, st


def test_the_kernels_rule_equals_the_twin_on_the_host(tmp_path):
    """hsk_split_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program), splitting and removing sequentially: classes, planes, labels, records in order, the stats, the point query and the
    volume and colour after each removal against the twin, zero differences"""
    exe = kit.build_harness("split_point", tmp_path)
    keys = [k for k in SC.all_keys() if k[0] != "random" or k[1] in ((72, 56, 40), (80, 64, 41))]
    rng = np.random.default_rng(11)
    for i, key in enumerate(keys):
        c = SC.case_of(key)
        t_cls, t_plane, t_label, t_recs, t_st = SC.twin_of(key)
        X, Y, Z = c["dims"]
        for j, (which, mode, halo, fw) in enumerate(c["removes"] or [(SC.ALL, ST.RESTORE, 2, 1)]):
            voxels, radius = rng.integers(0, (X, Y, Z), (150, 3)), (0, 2, 4)[(i + j) % 3]
            roots = SC.roots_of(key, which)
            cls, plane, label, recs, (n_minor, n_edge, n_flat), at, out, col, st = run_harness(exe, tmp_path, c, SC.rule_of(c), roots, mode, halo, fw, SC.color_of(key),
                                                                                               voxels, radius)
            print(f"{key} remove {which} mode {mode} halo {halo}: {t_st}, {st}")
            assert int((cls != t_cls).sum()) == 0 and int((plane != t_plane).sum()) == 0 and int((label != t_label).sum()) == 0, key
            assert records_as_dicts(recs) == t_recs and (n_minor, n_edge, n_flat) == (t_st["n_minor_objects"], t_st["n_edge"], t_st["n_no_normal"]), key
            size = (float(X), float(Y), float(Z))
            for got, want in zip(at, ST.split_at(t_cls, t_plane, t_label, size, voxels + 0.5, radius)):
                assert np.array_equal(got, want), key
            t_out, t_col, t_rst = SC.remove_twin(key, which, mode, halo, fw)
            assert int((out != t_out).sum()) == 0 and st == t_rst, key
            assert (col is None) == (t_col is None) and (col is None or np.array_equal(col, t_col)), key


# ---- 3. the default parameters, header, C layout, Python mirror, errors without a device ------------------------------------------
def test_default_split_params_without_a_context(hsk):
    p, t = hsk.default_split_params(), ST.default_params((3.0, 3.0, 3.0), (256, 256, 256), 0.03)
    assert (p.dist_m, p.back_m, p.cos_min, p.min_voxels) == (float(t["dist_m"]), float(t["back_m"]), float(t["cos_min"]), t["min_voxels"])
    assert p.min_voxels == hsk.default_prune_params().min_voxels and p.cos_min == float(np.float32(np.cos(np.radians(30.0))))
    q = hsk.default_split_params(dist_m=0.5, back_m=1.5, cos_min=0.25, min_voxels=77)
    assert (q.dist_m, q.back_m, q.cos_min, q.min_voxels) == (0.5, 1.5, 0.25, 77)
    r = hsk.default_remove_params()
    assert (r.mode, r.halo, r.fill_weight) == (hsk.REMOVE_RESTORE, ST.default_halo((3.0, 3.0, 3.0), (256, 256, 256), 0.03), 1) and r.halo == 4
    assert hsk.default_remove_params(mode=hsk.REMOVE_ERASE, halo=0, fill_weight=9).halo == 0
    for call in (lambda: hsk.default_split_params(halo=3), lambda: hsk.default_remove_params(dist_m=1)):
        with pytest.raises(TypeError, match="no field"):
            call()
    hsk._lib.load().hsk_default_split_params(None, None)
    hsk._lib.load().hsk_default_remove_params(None, None)


def test_split_plane_kinds_on_tilted_normals(hsk):
    """a normal tilted from up by 14.9 and 15.1 degrees is a floor and is not; from the horizon by 14.9 and 15.1 degrees a wall and
    not; the same about -up; equal to the twin's binary64 on random normals"""
    def tilted(deg, about_up=True):
        a = np.radians(deg)
        return [np.sin(a), -np.cos(a), 0.0, 0.3] if about_up else [np.cos(a), -np.sin(a), 0.0, 0.3]
    up = (0.0, -1.0, 0.0)
    abcd = np.array([tilted(14.9), tilted(15.1), tilted(180 - 14.9), tilted(180 - 15.1), tilted(14.9, False), tilted(15.1, False), tilted(-14.9, False),
                     tilted(-15.1, False), tilted(45.0)], np.float32)
    got = hsk.split_plane_kinds(abcd, up)
    assert got["kind"].tolist() == [hsk.KIND_FLOOR, hsk.KIND_OTHER, hsk.KIND_CEILING, hsk.KIND_OTHER, hsk.KIND_WALL, hsk.KIND_OTHER, hsk.KIND_WALL,
                                    hsk.KIND_OTHER, hsk.KIND_OTHER]
    assert np.array_equal(got["abcd"], abcd) and got.dtype == hsk.kinfu.SPLIT_PLANE_DTYPE
    rng = np.random.default_rng(2)
    many, tilt = rng.normal(size=(500, 4)).astype(np.float32), rng.normal(size=3).astype(np.float32)
    for lc, ws in ((np.cos(np.radians(15.0)), np.sin(np.radians(15.0))), (0.5, 0.5), (1.0, 0.0), (0.0, 1.0)):
        assert np.array_equal(hsk.split_plane_kinds(many, tilt, lc, ws)["kind"], ST.plane_kinds(many, tilt, lc, ws)), (lc, ws)
    assert len(set(hsk.split_plane_kinds(many, tilt)["kind"].tolist())) == 4
    lib, L = hsk._lib.load(), hsk._lib
    pl = (L.HskSplitPlane * 1)()
    pl[0].abcd[:] = [0, 0, 1, 0]
    u = (C.c_float * 3)(0, 0, 1)
    assert lib.hsk_split_plane_kinds(pl, 1, u, 0.9, 0.1) == 0 and pl[0].kind == L.HSK_KIND_FLOOR
    assert lib.hsk_split_plane_kinds(None, 1, u, 0.9, 0.1) == -1 and lib.hsk_split_plane_kinds(pl, 1, None, 0.9, 0.1) == -1
    assert lib.hsk_split_plane_kinds(pl, 1, u, 1.5, 0.1) == -1 and lib.hsk_split_plane_kinds(pl, 1, u, 0.9, -0.1) == -1 and lib.hsk_split_plane_kinds(pl, 1, u, float("nan"), 0.1) == -1
    assert lib.hsk_split_plane_kinds(pl, 1, (C.c_float * 3)(0, 0, 0), 0.9, 0.1) == -1 and b"up" in lib.hsk_last_error(None)
    pl[0].abcd[:] = [0, 0, 0, 0]
    assert lib.hsk_split_plane_kinds(pl, 1, u, 0.9, 0.1) == -1 and lib.hsk_split_plane_kinds(pl, 0, u, 0.9, 0.1) == 0


def test_split_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, S, O, T, R, Q = _lib.HskSplitPlane, _lib.HskSplitParams, _lib.HskObject, _lib.HskSplitStats, _lib.HskRemoveParams, _lib.HskRemoveStats
    assert (C.sizeof(P), C.sizeof(S), C.sizeof(O), C.sizeof(T), C.sizeof(R), C.sizeof(Q)) == (24, 24, 104, 104, 12, 40)
    K = hsk.kinfu
    assert K.OBJECT_DTYPE == OBJECT_DTYPE and K.OBJECT_DTYPE.itemsize == 104 and [K.OBJECT_DTYPE.fields[n][1] for n, _ in O._fields_] == [getattr(O, n).offset for n, _ in O._fields_]
    assert K.SPLIT_PLANE_DTYPE.itemsize == 24 and [K.SPLIT_PLANE_DTYPE.fields[n][1] for n, _ in P._fields_] == [getattr(P, n).offset for n, _ in P._fields_]
    assert (ST.NONE_CLS, ST.FLOOR, ST.CEILING, ST.WALL, ST.OTHER, ST.OBJECT, ST.MINOR) == (
        hsk.SPLIT_NONE, hsk.SPLIT_FLOOR, hsk.SPLIT_CEILING, hsk.SPLIT_WALL, hsk.SPLIT_OTHER, hsk.SPLIT_OBJECT, hsk.SPLIT_MINOR)
    assert (ST.FLOOR, ST.CEILING, ST.WALL, ST.OTHER, ST.ERASE, ST.RESTORE, ST.NONE) == (
        hsk.KIND_FLOOR, hsk.KIND_CEILING, hsk.KIND_WALL, hsk.KIND_OTHER, hsk.REMOVE_ERASE, hsk.REMOVE_RESTORE, _lib.HSK_COMPONENT_NONE)
    assert tuple(n for n, _ in S._fields_ if n != "pad") == K.SPLIT_FIELDS and tuple(n for n, _ in R._fields_) == K.REMOVE_FIELDS


def test_null_contexts_are_refused(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    n, st = C.c_size_t(77), L.HskSplitStats(n_objects=77)
    assert lib.hsk_split_scene(None, None, 0, None, None, 0, C.byref(n), C.byref(st)) == -1 and n.value == 77 and st.n_objects == 77
    cls = np.full(4, 9, np.uint8)
    assert lib.hsk_download_split(None, None, cls.ctypes.data, None, None) == -1 and (cls == 9).all()
    assert lib.hsk_split_at(None, None, 0, 0, None, None, None) == -1
    rst = L.HskRemoveStats(n_written=77)
    assert lib.hsk_remove_objects(None, None, 0, None, C.byref(rst)) == -1 and rst.n_written == 77
    assert lib.hsk_release_split(None) == -1
    for name in ("split_scene", "download_split", "split_at", "remove_objects", "release_split", "default_split_params", "default_remove_params"):
        assert callable(getattr(hsk.KinfuTracker, name))
    for name in ("split_plane_kinds", "split_planes", "default_split_params", "default_remove_params"):
        assert callable(getattr(hsk, name))
