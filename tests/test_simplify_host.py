"""The simplified mesh without a GPU: the numpy twin (tests/simplify_twin.py) pinned by hand; the kernels' shared text
(housescan_amd/csrc/hsk_simplify_point.h) compiled for the host with the sanitizers into a program of its own, simplifying every
small volume of the GPU list sequentially, against the twin -- every sum, vertex, normal, colour, face and statistic, zero
differences; hsk_cluster_vertex on sums of triangles that lie exactly on integer planes; the boundary identity of a closed surface;
the C layout of the new structs; the argument errors that need no device; the overflow static_assert.  The volumes built here are
the GPU tests' too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kit
import simplify_twin as ST
from kit import ROOT, same_bits
from mesh_twin import same_normals
from simplify_cases import (CLUSTERS, MODES, SMALL_DIMS, SMALL_SIZE, directed_edge_balance, grid, mesh_of, signed_volume, small_cases, sphere_volume, stats_list, twin_of)

f32 = np.float32


# ---- 1. the twin pinned by hand -------------------------------------------------------------------------------------------------
def test_the_twin_on_a_plane_between_grid_planes(oracle):
    """z = 5.3, not a multiple of 1/256 voxel: stored values -900 at z = 5 and 2100 at z = 6, q = (512 * 900 + 3000) // 6000 = 77"""
    x, y, z = grid(SMALL_DIMS)
    t = ((z - 5.3) * 3000.0).round().astype(np.int16)
    vol = np.stack([t, np.full(t.shape, 1, np.int16)], axis=-1)
    assert (vol[5, :, :, 0] == -900).all() and (vol[6, :, :, 0] == 2100).all()
    for mode in MODES:
        tw = ST.simplify(vol, *oracle.mc_table(), c=4, mode=mode, size=SMALL_SIZE)
        n = len(tw["vertices"])
        assert n == 8 * 6 and (tw["pos_q"][:, 2] == 256 * 5 + 77).all()          # one vertex per cluster of the plane's layer
        assert (tw["rank"] == (1 if mode == ST.QUADRIC else 0)).all()
        f = tw["faces"]
        assert len(f) and (f[:, 0] != f[:, 1]).all() and (f[:, 0] != f[:, 2]).all() and (f[:, 1] != f[:, 2]).all()
        assert tw["stats"]["n_rank"] == ([0, n, 0, 0] if mode == ST.QUADRIC else [n, 0, 0, 0]) and tw["stats"]["n_clamped"] == 0
        assert np.isfinite(tw["normals"]).all() and (tw["normals"][:, 2] == 1.0).all()   # towards free space, +z


def test_the_twin_on_a_blob_inside_one_cluster_and_on_the_empty_volume(oracle):
    for c in CLUSTERS:
        tw = twin_of(oracle, "blob", c, ST.QUADRIC)
        st = tw["stats"]
        assert len(tw["vertices"]) == 0 and len(tw["faces"]) == 0 and tw["faces"].shape == (0, 3)
        assert st["n_in_vertices"] == 6 and st["n_in_faces"] == 8 == st["n_faces_collapsed"] and st["n_clusters"] == 1
        e = twin_of(oracle, "empty", c, ST.MEAN)
        assert len(e["vertices"]) == 0 and len(e["faces"]) == 0
        assert all(v == 0 or v == [0, 0, 0, 0] for v in e["stats"].values())


def test_quantised_position_arithmetic():
    assert ST.quantised_vertices(np.array([[[[-4000, 1], [0, 1]]]], np.int16), np.array([[0, 0, 0, 0]]))[0].tolist() == [[256, 0, 0]]   # ratio exactly 1
    assert ST.quantised_vertices(np.array([[[[0, 1], [-4000, 1]]]], np.int16), np.array([[0, 0, 0, 0]]))[0].tolist() == [[0, 0, 0]]
    assert ST.quantised_vertices(np.array([[[[3, 1], [-3, 1]]]], np.int16), np.array([[0, 0, 0, 0]]))[0].tolist() == [[128, 0, 0]]
    assert ST.quantised_vertices(np.array([[[[32767, 1], [-32767, 1]]]], np.int16), np.array([[0, 0, 0, 0]]))[0].tolist() == [[128, 0, 0]]


# ---- 2. the kernels' shared text on the host, under the sanitizers ---------------------------------------------------------------
def run_harness(exe, tmp_path, oracle, vol, size, col, c, mode, sv_floor=1e-3):
    Z, Y, X, _ = vol.shape
    ntri, codes = oracle.mc_table()
    cell = [f32(size[0]) / f32(X), f32(size[1]) / f32(Y), f32(size[2]) / f32(Z)]
    words = (vol[..., 0].astype(np.uint16).astype(np.uint32) | (vol[..., 1].astype(np.uint16).astype(np.uint32) << 16))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([X, Y, Z, c, mode, 0 if col is None else 1], np.int32).tobytes())
        f.write(np.array([sv_floor] + cell, np.float32).tobytes())
        f.write(np.ascontiguousarray(ntri, np.uint8).tobytes())
        f.write(np.ascontiguousarray(codes, np.uint8).tobytes())
        f.write(np.ascontiguousarray(words).tobytes())
        if col is not None:
            f.write(np.ascontiguousarray(col, np.uint8).tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    n, m = (int(v) for v in np.frombuffer(raw, np.uint64, 2))
    off = 16
    out = {}
    for name, dtype, count, shape in (("clusters", np.uint32, n, (n,)), ("sums", np.int64, 20 * n, (n, 20)), ("vertices", np.float32, 3 * n, (n, 3)),
                                      ("normals", np.float32, 3 * n, (n, 3)), ("rgb", np.uint8, 3 * n, (n, 3)), ("faces", np.int32, 3 * m, (m, 3)),
                                      ("stats", np.uint64, 12, (12,))):
        out[name] = np.frombuffer(raw, dtype, count, off).reshape(shape)
        off += count * np.dtype(dtype).itemsize
    assert off == len(raw)
    return out


def test_the_kernels_shared_text_equals_the_twin_on_the_host(tmp_path, oracle):
    """hsk_simplify_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program, which is run as a program): every small volume of the GPU list, every cluster size, both modes, zero differences"""
    exe = kit.build_harness("simplify_point", tmp_path)
    for name, (vol, _, size, col) in small_cases().items():
        for c in CLUSTERS:
            for mode in MODES:
                got = run_harness(exe, tmp_path, oracle, vol, size, col, c, mode)
                tw = twin_of(oracle, name, c, mode)
                tag = (name, c, mode)
                assert np.array_equal(got["clusters"], tw["clusters"]), tag
                assert int((got["sums"] != tw["sums"]).sum()) == 0, tag
                assert same_bits(got["vertices"], tw["vertices"]), tag
                assert same_normals(got["normals"], tw["normals"]), tag
                assert np.array_equal(got["faces"], tw["faces"]), tag
                if col is not None:
                    assert np.array_equal(got["rgb"], tw["rgb"]), tag
                assert got["stats"].tolist() == stats_list(tw["stats"]), tag
        st = twin_of(oracle, name, 4, ST.QUADRIC)["stats"]
        print(f"{name}: {st}")
    # the list is not trivial: thousands of faces, every rank, partial clusters, uncoloured clusters
    box = twin_of(oracle, "box", 2, ST.QUADRIC)["stats"]
    assert box["n_out_faces"] > 3000 and all(box["n_rank"][r] > 0 for r in (1, 2, 3))
    assert twin_of(oracle, "box with colour", 2, ST.QUADRIC)["stats"]["n_uncolored"] > 0
    assert twin_of(oracle, "holes", 4, ST.QUADRIC)["stats"]["n_out_faces"] < twin_of(oracle, "box", 4, ST.QUADRIC)["stats"]["n_out_faces"]


# ---- 3. hsk_cluster_vertex on exact planes --------------------------------------------------------------------------------------
N1, N2, N3 = np.array([1, 2, 2]), np.array([2, 1, -2]), np.array([2, -2, 1])     # mutually orthogonal, length 3


def plane_triangle(point, u, v):
    """a triangle that lies exactly on the plane through `point` spanned by the integer directions u, v; normal u x v"""
    p = np.asarray(point, np.int64)
    return np.stack([p + 10 * u, p + 50 * u + 10 * v, p + 10 * u + 60 * v])


def sums_of(triangles, vertices=None):
    """the 16 sums of a cluster whose vertices are `vertices` (default: the triangles' corners) and that every triangle touches"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3, 3)
    pts = tri.reshape(-1, 3) if vertices is None else np.asarray(vertices, np.int64).reshape(-1, 3)
    s = np.zeros(16, np.int64)
    s[0] = len(pts)
    s[1:4] = pts.sum(axis=0)
    for t in tri:
        n = np.cross(t[1] - t[0], t[2] - t[0])
        dn = int(n @ t[0])
        s[4:7] += n
        s[7:13] += [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2]]
        s[13:16] += n * dn
    return s


def test_cluster_vertex_on_exact_planes(hsk):
    corner = np.array([300, -410, 520], np.int64)                # in 1/256 voxel, inside the cell of c = 8 grown by a voxel (+-1280)
    t1, t2, t3 = plane_triangle(corner, N2, N3), plane_triangle(corner, N3, N1), plane_triangle(corner, N1, N2)
    # three orthogonal planes: rank 3, their intersection; only the double solve rounds
    s = sums_of([t1, t2, t3])
    x, rank, clamped = hsk.cluster_vertex(s, 8)
    assert rank == 3 and not clamped and np.abs(x - corner / 256.0).max() < 1e-9
    tx, trank, tcl = ST.cluster_vertex(s[None, :], 8)
    assert np.array_equal(x, tx[0] / 256.0) and trank[0] == 3 and not tcl[0]           # the twin's solve, bit for bit
    # two planes: rank 2, the point of their line nearest the mean
    s = sums_of([t1, t2])
    x, rank, clamped = hsk.cluster_vertex(s, 8)
    mean = s[1:4] / s[0]
    line = corner + N3 * ((mean - corner) @ N3) / 9.0
    assert rank == 2 and not clamped and np.abs(x - line / 256.0).max() < 1e-9
    # one plane: rank 1, the mean projected onto it
    s = sums_of([t1])
    x, rank, clamped = hsk.cluster_vertex(s, 8)
    mean = s[1:4] / s[0]
    proj = mean - N1 * ((mean - corner) @ N1) / 9.0
    assert rank == 1 and not clamped and np.abs(x - proj / 256.0).max() < 1e-9
    # A = 0: rank 0, the mean -- and so does the mean mode whatever A is
    s = sums_of([], vertices=[[10, 20, 30], [11, 22, 33], [12, 24, 37]])
    x, rank, clamped = hsk.cluster_vertex(s, 4)
    assert rank == 0 and not clamped and np.array_equal(x, (s[1:4] / 3.0) / 256.0)
    s = sums_of([t1, t2, t3])
    x, rank, clamped = hsk.cluster_vertex(s, 8, mode=hsk.SIMPLIFY_MEAN)
    assert rank == 0 and not clamped and np.array_equal(x, (s[1:4] / s[0]) / 256.0)
    # a solution outside the grown cell: clamped to it, and the flag set (c = 2: +-(128 * 2 + 256) / 256 = +-2 voxels)
    far = np.array([5000, 100, -100], np.int64)
    s = sums_of([plane_triangle(far, np.array([0, 1, 0]), np.array([0, 0, 1]))], vertices=[[0, 100, -100]])
    x, rank, clamped = hsk.cluster_vertex(s, 2)
    assert rank == 1 and clamped and x.tolist() == [2.0, 100 / 256.0, -100 / 256.0]
    # the axis-aligned triple through the Jacobi's skipped rotations (A is diagonal from the start)
    e = np.eye(3, dtype=np.int64)
    s = sums_of([plane_triangle(corner, e[1], e[2]), plane_triangle(corner, e[2], e[0]), plane_triangle(corner, e[0], e[1])])
    x, rank, clamped = hsk.cluster_vertex(s, 8)
    assert rank == 3 and np.abs(x - corner / 256.0).max() < 1e-9


def test_cluster_vertex_equals_the_twin_on_random_sums(hsk):
    rng = np.random.default_rng(5)
    rows = []
    for _ in range(200):
        k = int(rng.integers(1, 6))
        tri = rng.integers(-600, 600, (k, 3, 3))
        rows.append(sums_of(tri))
    rows = np.array(rows)
    for c in CLUSTERS:
        tx, trank, tcl = ST.cluster_vertex(rows, c)
        for i, s in enumerate(rows):
            x, rank, clamped = hsk.cluster_vertex(s, c)
            assert np.array_equal(x, tx[i] / 256.0) and rank == trank[i] and clamped == tcl[i], (c, i)


# ---- 4. a closed surface stays closed -------------------------------------------------------------------------------------------
def test_a_closed_surface_stays_closed(oracle):
    """identifying vertices and dropping the faces with a repeated vertex commutes with the boundary operator, and the rule merges
    nothing else: every directed edge (a, b) of the output occurs exactly as often as (b, a); the signed volume keeps its sign"""
    vol = sphere_volume()
    assert (vol[..., 1] != 0).all()
    mesh = mesh_of(oracle, "sphere")
    assert directed_edge_balance(mesh["faces"]) == 0
    v_in = signed_volume(mesh["vertices"], mesh["faces"])
    for c in CLUSTERS:
        for mode in MODES:
            tw = twin_of(oracle, "sphere", c, mode)
            assert len(tw["faces"]) > 0 and directed_edge_balance(tw["faces"]) == 0, (c, mode)
            v_out = signed_volume(tw["vertices"], tw["faces"])
            assert v_out * v_in > 0, (c, mode, v_in, v_out)
    # (and an open surface does not pass the same check: the check can fail)
    assert directed_edge_balance(twin_of(oracle, "six faces", 4, ST.QUADRIC)["faces"]) != 0


# ---- 5. C layout, Python mirror, errors without a device, the overflow assertion ---------------------------------------------------
def test_simplify_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, S = _lib.HskSimplifyParams, _lib.HskSimplifyStats
    assert (C.sizeof(P), C.sizeof(S)) == (12, 96)
    assert (ST.QUADRIC, ST.MEAN) == (hsk.SIMPLIFY_QUADRIC, hsk.SIMPLIFY_MEAN) == (_lib.HSK_SIMPLIFY_QUADRIC, _lib.HSK_SIMPLIFY_MEAN)
    assert tuple(n for n, _ in S._fields_) == hsk.kinfu.SIMPLIFY_STATS_FIELDS


def test_argument_errors_that_need_no_device(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    p = L.HskSimplifyParams(9, 9, 9.0)
    lib.hsk_default_simplify_params(None, C.byref(p))
    assert (p.cluster_voxels, p.mode, p.sv_floor) == (4, L.HSK_SIMPLIFY_QUADRIC, f32(1e-3))
    lib.hsk_default_simplify_params(None, None)
    nv, nf = C.c_size_t(77), C.c_size_t(77)
    st = L.HskSimplifyStats(n_clamped=77)
    assert lib.hsk_extract_mesh_simplified(None, None, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), C.byref(st)) == -1
    assert (nv.value, nf.value, st.n_clamped) == (77, 77, 77)
    s = sums_of([plane_triangle([0, 0, 0], N2, N3)])
    assert hsk.cluster_vertex(s, 0, sv_floor=0.0)[1] == 1              # the zeros are the defaults
    for bad in (dict(cluster_voxels=3), dict(cluster_voxels=32), dict(cluster_voxels=-4), dict(mode=2), dict(mode=-1), dict(sv_floor=-0.5),
                dict(sv_floor=1.0), dict(sv_floor=float("nan")), dict(sv_floor=float("inf"))):
        with pytest.raises(hsk.KinfuError):
            hsk.cluster_vertex(s, **bad)
    empty = s.copy()
    empty[0] = 0
    with pytest.raises(hsk.KinfuError):
        hsk.cluster_vertex(empty, 4)
    x, rank, cl = np.zeros(3), C.c_int(), C.c_int()
    assert lib.hsk_cluster_vertex(None, 4, 0, 0.0, x.ctypes.data_as(C.POINTER(C.c_double)), C.byref(rank), C.byref(cl)) == -1
    assert callable(hsk.KinfuTracker.extract_mesh_simplified)


def test_the_overflow_assertions_compile(tmp_path):
    """the shared header's static_asserts (|sum N dN| at c = 16 fits an int64) hold: the header compiles on its own"""
    src = tmp_path / "o.cpp"
    src.write_text('#include "hsk_simplify_point.h"\nint main() { return simp_shift(16) == 4 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "housescan_amd", "csrc"), str(src), "-o", str(tmp_path / "o")])
    subprocess.check_call([str(tmp_path / "o")])
    text = open(os.path.join(ROOT, "housescan_amd", "csrc", "hsk_simplify_point.h")).read()
    assert text.count("static_assert") >= 4
    # the same arithmetic, restated: 5 * 17^3 triangles, |N_i| <= 2^17, |dN| <= 3 * 2^17 * 2304
    assert 5 * 17 ** 3 * 2 ** 17 * (3 * 2 ** 17 * 2304) < 2 ** 63
