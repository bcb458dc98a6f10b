"""Volume differencing without a GPU: the kernels' shared text (housescan_amd/csrc/hsk_diff_point.h, compiled for the host) against
the numpy twin (tests/diff_twin.py) on the volume pairs the GPU tests use; the twin's own pins -- hand-computed classes, the
analytic room and the shifted wall; the default parameters; the C layout of the new structs and their Python
mirror; the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import diff_cases as DC
import diff_twin as DT
import kit
from diff_cases import records_as_dicts, words_of
from kit import blocked


def line(values):
    """a 1 x 1 x n volume: (raw, weight) per voxel along x"""
    return np.array(values, np.int16).reshape(1, 1, -1, 2)


# ---- 1. the twin's own pins ---------------------------------------------------------------------------------------------------------
def test_the_twin_on_hand_computed_classes():
    ref = line([(0, 0), (5, 1), (0, 0), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (-32768, 1), (32766, 1)])
    cur = line([(9, 0), (5, 0), (7, 1), (16383, 1), (16384, 1), (-16383, 1), (-16384, 1), (0, 1), (32766, 1), (-32768, 1)])
    assert DT.classify(ref, cur)[0, 0].tolist() == [DT.UNSEEN, DT.ONLY_REF, DT.ONLY_CUR, DT.SAME, DT.VANISHED, DT.SAME, DT.APPEARED, DT.SAME, DT.VANISHED, DT.APPEARED]
    # a raw of -32768 counts as -32767: |d| = 65533 is below a thresh of 65534
    assert DT.classify(ref, cur, thresh=65534)[0, 0, 8:].tolist() == [DT.SAME, DT.SAME]
    # min_weight: observed iff W >= min_weight
    assert DT.classify(line([(0, 2), (0, 3), (0, 3)]), line([(0, 3), (0, 2), (0, 3)]), min_weight=3)[0, 0].tolist() == [DT.ONLY_CUR, DT.ONLY_REF, DT.SAME]
    # regions on a 1 x 3 x 6 grid: A A . V / . . . V / diagonal contact does not connect
    cls = np.array([[[4, 4, 3, 5, 3, 3], [3, 3, 4, 5, 3, 3], [3, 3, 3, 3, 4, 3]]], np.uint8)
    out, region, recs, n_minor = DT.regions(cls, 2)
    assert region[0].tolist() == [[0, 0, DT.NONE, 3, DT.NONE, DT.NONE], [DT.NONE, DT.NONE, 3, 3, DT.NONE, DT.NONE], [DT.NONE] * 6]
    assert out[0, 2, 4] == DT.MINOR and n_minor == 1 and out[0, 1, 2] == DT.APPEARED
    # three voxels before two; the mixed region has both counts
    assert [(c["root"], c["n_voxels"], c["n_appeared"], c["n_vanished"], c["lo"], c["hi"]) for c in recs] == [
        ((3, 0, 0), 3, 1, 2, (2, 0, 0), (4, 2, 1)), ((0, 0, 0), 2, 2, 0, (0, 0, 0), (2, 1, 1))]
    # ties go to the smaller root
    cls = np.array([[[4, 3, 5, 3, 4]]], np.uint8)
    assert [c["root"][0] for c in DT.regions(cls, 1)[2]] == [0, 2, 4]


def test_the_twin_point_query_and_adopt_on_a_line():
    cls = np.array([[[3, 3, 4, 3, 3, 3, 5, 3]]], np.uint8)
    _, region, _, _ = DT.regions(cls, 1)
    size = (8.0, 1.0, 1.0)
    pts = [(x + 0.5, 0.5, 0.5) for x in range(8)] + [(-0.5, 0.5, 0.5), (4.0, 0.5, 0.5), (8.0, 0.5, 0.5)]
    c0, r0 = DT.diff_at(cls, region, size, pts, 0)
    assert c0.tolist() == [3, 3, 4, 3, 3, 3, 5, 3, 0, 3, 0] and r0[2] == 2 and r0[6] == 6 and (np.delete(r0, [2, 6]) == DT.NONE).all()
    # voxel 4 lies two from both: the smaller lin wins; a point on a cell face belongs to the upper cell
    c2, r2 = DT.diff_at(cls, region, size, pts, 2)
    assert c2.tolist() == [4, 4, 4, 4, 4, 5, 5, 5, 0, 4, 0] and r2.tolist()[:8] == [2, 2, 2, 2, 2, 6, 6, 6]
    ref, cur = line([(0, 1)] * 8), line([(1, 2), (2, 2), (3, 0), (4, 2), (5, 2), (6, 0), (7, 2), (8, 2)])
    out, _, st = DT.adopt(ref, cur, cls, DT.ADOPT_VANISHED, 1)
    assert out[0, 0].tolist() == [[0, 1]] * 5 + [[0, 1], [7, 2], [8, 2]] and st == {"n_targets": 1, "n_adopted": 2, "n_colored": 0}
    m = np.zeros((5, 5, 5), bool)
    m[2, 2, 2] = True
    assert DT.dilate(m, 1).sum() == 27 and DT.dilate(m, 2).all() and DT.dilate(m, 0).sum() == 1


def test_the_analytic_room_on_the_twin():
    """DESIGN.md 8q's figures: 64 x 48 x 40, tau = 2.1 cells, floor z = 6.3, wall x = 50.4, the box (20.3, 14.2, 6.3) ..
    (33.7, 30.6, 19.4)"""
    _, _, recs, st = DC.shape_twin("the box appears")
    assert st["n_regions"] == 1 and (recs[0]["n_voxels"], recs[0]["n_appeared"], recs[0]["lo"], recs[0]["hi"]) == (2758, 2758, (19, 13, 7), (35, 32, 20))
    _, _, recs, st = DC.shape_twin("the box vanishes")
    assert st["n_regions"] == 1 and (recs[0]["n_voxels"], recs[0]["n_vanished"], recs[0]["lo"], recs[0]["hi"]) == (2758, 2758, (19, 13, 7), (35, 32, 20))
    _, _, recs, st = DC.shape_twin("the box moves")
    assert st["n_regions"] == 2 and [(c["n_voxels"], c["n_appeared"], c["n_vanished"]) for c in recs] == [(1221, 0, 1221), (1221, 1221, 0)]
    # the known property: a wall shifted along its normal stays SAME up to half the truncation distance
    empty = DC.shapes()["the box appears"]["ref"]
    for shift, flooded in ((0.5, False), (1.0, False), (1.04, False), (1.1, True)):
        n = DT.diff(empty, DT.room(wall_x=50.4 + shift))[3]["n_class"]
        assert (n[DT.APPEARED] + n[DT.VANISHED] + n[DT.MINOR] > 4000) == flooded and (flooded or n[DT.APPEARED] + n[DT.VANISHED] + n[DT.MINOR] == 0), shift


@pytest.mark.parametrize("halo", [1, 2])
def test_adopt_makes_ref_equal_cur_where_it_matters_on_the_twin(halo):
    c = DC.shapes()["the box appears"]
    ref, cur = c["ref"], c["cur"]
    out, _, st = DC.adopt_twin(("shape", "the box appears"), ref, cur, DC.shape_twin("the box appears")[0], DC.BOTH, halo)
    again = DT.diff(out, cur)[3]["n_class"]
    assert again[DT.APPEARED] + again[DT.VANISHED] + again[DT.MINOR] == 0
    assert all(np.array_equal(a, b) for a, b in zip(DT.crossings(out), DT.crossings(cur)))
    both = (out[..., 1] != 0) & (cur[..., 1] != 0)
    assert np.array_equal(out[both], cur[both]) and st["n_adopted"] > st["n_targets"] == 2758


def test_with_halo_0_the_surfaces_are_not_curs_on_the_twin():
    """at halo 0 a second diff is empty too (every CHANGED voxel was replaced, the others were below thresh), but
    ref's crossings are not cur's and ref differs from cur beside the region -- why the default halo is 2"""
    c = DC.shapes()["the box appears"]
    ref, cur = c["ref"], c["cur"]
    out, _, st = DC.adopt_twin(("shape", "the box appears"), ref, cur, DC.shape_twin("the box appears")[0], DC.BOTH, 0)
    again = DT.diff(out, cur)[3]["n_class"]
    assert st["n_adopted"] == st["n_targets"] == 2758 and again[DT.APPEARED] + again[DT.VANISHED] + again[DT.MINOR] == 0
    assert not all(np.array_equal(a, b) for a, b in zip(DT.crossings(out), DT.crossings(cur)))
    both = (out[..., 1] != 0) & (cur[..., 1] != 0)
    assert not np.array_equal(out[both], cur[both])


def test_the_cases_reach_what_they_are_for():
    """the conditions of the shared pairs, on the twin"""
    for dims in DC.RANDOM_DIMS:
        cls, region, recs, st = DC.random_twin(dims)
        assert all(n > 0 for n in st["n_class"]), dims
        assert st["n_regions"] >= 3 and st["n_minor_regions"] >= 1, dims
        assert any(c["lo"][0] < 16 < c["hi"][0] and c["lo"][1] < 16 < c["hi"][1] and c["lo"][2] < 8 < c["hi"][2] for c in recs), dims
    T = {name: DC.shape_twin(name) for name in DC.shapes()}
    for name in ("the wall shifted by 0.5", "the wall shifted by 1.0", "identical volumes"):
        assert T[name][3]["n_regions"] == 0 and not (T[name][0] >= DT.APPEARED).any(), name
    for t in (16384, 1, 65534):
        cls = T[f"d at thresh {t}"][0]
        assert (cls[3, 5, 6], cls[3, 5, 9], cls[9, 13, 17], cls[9, 13, 20]) == (DT.VANISHED, DT.SAME, DT.APPEARED, DT.SAME), t
    cls = T["W at min_weight 3"][0]
    assert (cls[5, 8, 12], cls[5, 14, 12], cls[5, 8, 18], cls[5, 14, 18]) == (DT.VANISHED, DT.ONLY_REF, DT.ONLY_CUR, DT.UNSEEN)
    cls = T["min_weight 128"][0]
    assert (cls[0, 0, 0], cls[0, 0, 8], cls[0, 12, 0], cls[0, 12, 8], cls[19, 3, 30]) == (DT.ONLY_CUR, DT.APPEARED, DT.UNSEEN, DT.ONLY_REF, DT.APPEARED)
    cls = T["raw -32768 on either side"][0]
    assert (cls[4, 4, 5], cls[6, 4, 5], cls[8, 4, 5], cls[10, 4, 5]) == (DT.SAME, DT.SAME, DT.VANISHED, DT.APPEARED)
    one = T["a face joins APPEARED and VANISHED"][2]
    assert len(one) == 1 and (one[0]["n_voxels"], one[0]["n_appeared"], one[0]["n_vanished"]) == (128, 64, 64)
    assert [(c["n_appeared"], c["n_vanished"]) for c in T["an edge does not join"][2]] == [(64, 0), (0, 64)]
    mv = T["min_voxels and one less"]
    assert [c["n_voxels"] for c in mv[2]] == [18, 18, 12] and mv[3]["n_minor_regions"] == 1 and mv[3]["n_class"][DT.MINOR] == 11
    assert mv[2][0]["root"] == (9, 15, 6) and mv[2][1]["root"] == (20, 3, 12)                     # equal sizes: the smaller root first
    six = T["a region on each grid face"][1] != DT.NONE
    assert six[:, :, 0].any() and six[:, :, -1].any() and six[:, 0].any() and six[:, -1].any() and six[0].any() and six[-1].any()
    assert T["a region on each grid face"][3]["n_regions"] == 6
    allc = T["everything changed"]
    assert allc[3]["n_regions"] == 1 and allc[2][0]["n_voxels"] == 9 * 24 * 24 and allc[2][0]["hi"] == (24, 24, 9)
    c = DC.shapes()["cur unobserved inside the halo"]
    _, _, st = DC.adopt_twin(("shape", "cur unobserved inside the halo"), c["ref"], c["cur"], T["cur unobserved inside the halo"][0], DC.BOTH, 2)
    halo_voxels = int(DT.dilate(T["cur unobserved inside the halo"][0] == DT.APPEARED, 2).sum())
    assert 0 < st["n_adopted"] < halo_voxels == 8 * 8 * 8
    # a halo that runs off the grid, and one class only
    c = DC.shapes()["a region on each grid face"]
    assert DC.adopt_twin(("shape", "a region on each grid face"), c["ref"], c["cur"], T["a region on each grid face"][0], DC.BOTH, 8)[2]["n_adopted"] > 8000
    c = DC.shapes()["the box moves"]
    a = DC.adopt_twin(("shape", "the box moves"), c["ref"], c["cur"], T["the box moves"][0], DT.ADOPT_APPEARED, 2)[2]
    b = DC.adopt_twin(("shape", "the box moves"), c["ref"], c["cur"], T["the box moves"][0], DC.BOTH, 2)[2]
    assert a["n_targets"] == 1221 and b["n_targets"] == 2442 and a["n_adopted"] < b["n_adopted"]


# ---- 2. the kernels' shared text on the host -------------------------------------------------------------------------------------


def run_harness(exe, tmp_path, ref, cur, params, which, halo, ref_color, cur_color, voxels, radius):
    Z, Y, X = ref.shape[:3]
    p = dict(thresh=DT.DEFAULT_THRESH, min_weight=1, min_voxels=1)
    p.update(params)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([X, Y, Z, p["thresh"], p["min_weight"], p["min_voxels"], which, halo, ref_color is not None, cur_color is not None, radius, len(voxels)],
                         np.int32).tobytes())
        f.write(blocked(ref).tobytes())
        f.write(blocked(cur).tobytes())
        for col in (ref_color, cur_color):
            if col is not None:
                f.write(np.ascontiguousarray(col).tobytes())
        f.write(np.asarray(voxels, np.int32).tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    n, m = X * Y * Z, len(voxels)
    cls = np.frombuffer(raw, np.uint8, n).reshape(Z, Y, X)
    region = np.frombuffer(raw, np.uint32, n, n).reshape(Z, Y, X)
    n_kept, n_minor = map(int, np.frombuffer(raw, np.uint64, 2, 5 * n))
    off = 5 * n + 16
    recs = np.frombuffer(raw, np.dtype([("root", "<i4", (3,)), ("pad", "<i4"), ("n_voxels", "<u8"), ("n_appeared", "<u8"), ("n_vanished", "<u8"),
                                        ("lo", "<i4", (3,)), ("hi", "<i4", (3,))]), n_kept, off)
    off += 64 * n_kept
    at_cls = np.frombuffer(raw, np.uint8, m, off)
    at_region = np.frombuffer(raw[off + m:off + 5 * m], np.uint32)
    off += 5 * m
    out = words_of(raw[off:off + 4 * n], n, 0).reshape(Z, Y, X, 2)
    off += 4 * n
    col = None
    if ref_color is not None:
        col = np.frombuffer(raw, np.uint8, 4 * n, off).reshape(Z, Y, X, 4)
        off += 4 * n
    st = dict(zip(("n_targets", "n_adopted", "n_colored"), map(int, np.frombuffer(raw[off:off + 24], np.uint64))))
    return cls, region, recs, n_minor, at_cls, at_region, out, col, st


def test_the_kernels_rule_equals_the_twin_on_the_host(tmp_path):
    """hsk_diff_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program), diffing and adopting sequentially: classes, labels, records in order, the point query and the adopted volume and
    colour against the twin, zero differences"""
    exe = kit.build_harness("diff_point", tmp_path)
    cases = []
    for name, c in DC.shapes().items():
        ca, cb = DC.colors_of(name)
        for which, halo in (c["adopts"] or [(DC.BOTH, 2)]):
            cases.append((name, ("shape", name), c["ref"], c["cur"], c["params"], which, halo, ca, cb, DC.shape_twin(name)))
    for dims in ((72, 56, 40), (80, 64, 41)):
        ref, cur = DC.random_pair(dims)
        ca, cb = DC.random_colors(dims)
        cases.append((f"random {dims}", ("random", dims), ref, cur, dict(min_voxels=DC.RANDOM_MIN_VOXELS), DC.BOTH, 2, ca, cb, DC.random_twin(dims)))
    rng = np.random.default_rng(11)
    for i, (name, key, ref, cur, params, which, halo, ca, cb, (t_cls, t_region, t_recs, t_st)) in enumerate(cases):
        Z, Y, X = ref.shape[:3]
        voxels, radius = rng.integers(0, (X, Y, Z), (200, 3)), (0, 2, 4)[i % 3]
        size = (float(X), float(Y), float(Z))
        cls, region, recs, n_minor, at_cls, at_region, out, col, st = run_harness(exe, tmp_path, ref, cur, params, which, halo, ca, cb, voxels, radius)
        print(f"{name} which {which} halo {halo}: {t_st}, {st}")
        assert int((cls != t_cls).sum()) == 0 and int((region != t_region).sum()) == 0, name
        assert records_as_dicts(recs) == t_recs and n_minor == t_st["n_minor_regions"], name
        r_cls, r_region = DT.diff_at(t_cls, t_region, size, voxels + 0.5, radius)
        assert np.array_equal(at_cls, r_cls) and np.array_equal(at_region, r_region), name
        t_out, t_col, t_ast = DC.adopt_twin(key, ref, cur, t_cls, which, halo, ca, cb)
        assert int((out != t_out).sum()) == 0 and st == t_ast, name
        assert (col is None) == (t_col is None) and (col is None or np.array_equal(col, t_col)), name


# ---- 3. the default parameters, header, C layout, Python mirror, errors without a device ------------------------------------------
def test_default_diff_params_without_a_context(hsk):
    p = hsk.default_diff_params()
    assert (p.thresh, p.min_weight, p.min_voxels) == (16384, 1, hsk.default_prune_params().min_voxels)
    assert p.min_voxels == DT.default_min_voxels((3.0, 3.0, 3.0), (256, 256, 256), 0.03)
    q = hsk.default_diff_params(thresh=9, min_weight=4, min_voxels=77)
    assert (q.thresh, q.min_weight, q.min_voxels) == (9, 4, 77)
    with pytest.raises(TypeError, match="no field"):
        hsk.default_diff_params(halo=3)
    hsk._lib.load().hsk_default_diff_params(None, None)


def test_diff_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, R, S, A, T = _lib.HskDiffParams, _lib.HskDiffRegion, _lib.HskDiffStats, _lib.HskAdoptParams, _lib.HskAdoptStats
    assert (C.sizeof(P), C.sizeof(R), C.sizeof(S), C.sizeof(A), C.sizeof(T)) == (16, 64, 80, 8, 24)
    assert hsk.kinfu.DIFF_REGION_DTYPE.itemsize == 64 and [hsk.kinfu.DIFF_REGION_DTYPE.fields[n][1] for n, _ in R._fields_] == [getattr(R, n).offset for n, _ in R._fields_]
    assert (DT.UNSEEN, DT.ONLY_REF, DT.ONLY_CUR, DT.SAME, DT.APPEARED, DT.VANISHED, DT.MINOR) == (
        hsk.DIFF_UNSEEN, hsk.DIFF_ONLY_REF, hsk.DIFF_ONLY_CUR, hsk.DIFF_SAME, hsk.DIFF_APPEARED, hsk.DIFF_VANISHED, hsk.DIFF_MINOR)
    assert (DT.ADOPT_APPEARED, DT.ADOPT_VANISHED, DT.NONE) == (hsk.ADOPT_APPEARED, hsk.ADOPT_VANISHED, _lib.HSK_COMPONENT_NONE)
    assert tuple(n for n, _ in P._fields_) == hsk.kinfu.DIFF_FIELDS and tuple(n for n, _ in A._fields_) == hsk.kinfu.ADOPT_FIELDS


def test_null_contexts_are_refused(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    n, st = C.c_size_t(77), L.HskDiffStats(n_regions=77)
    assert lib.hsk_diff_volume(None, None, None, None, 0, C.byref(n), C.byref(st)) == -1 and n.value == 77 and st.n_regions == 77
    cls = np.full(4, 9, np.uint8)
    assert lib.hsk_download_diff(None, None, cls.ctypes.data, None) == -1 and (cls == 9).all()
    assert lib.hsk_diff_at(None, None, 0, 0, None, None) == -1
    ast = L.HskAdoptStats(n_adopted=77)
    assert lib.hsk_adopt_diff(None, None, None, C.byref(ast)) == -1 and ast.n_adopted == 77
    assert lib.hsk_release_diff(None) == -1
    for name in ("diff_volume", "download_diff", "diff_at", "adopt_diff", "release_diff", "resampled_like", "default_diff_params"):
        assert callable(getattr(hsk.KinfuTracker, name))
