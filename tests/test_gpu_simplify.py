"""hsk_extract_mesh_simplified on the GPU: vertices, normals, colours, faces, counts and every statistic bit for bit against the
numpy restatement of the rule (tests/simplify_twin.py) at every cluster size and in both modes, on the small volumes of
tests/test_simplify_host.py and on a scanned room; a closed surface stays closed; a flat plane stays flat; the quadric finds a box's
corners where the mean does not; the call protocol, the count cache, the refusals.  The simplified mesh's tests:
  tests/test_simplify_host.py          the twin pinned by hand and to the kernels' shared text on the host; the small volumes
  tests/test_gpu_simplify.py           this file: cluster rows of one 64-cluster segment, at most 1024 cluster rows
  tests/simplify_cases.py              the wide and tall volumes and the census of what an input reaches
  tests/test_simplify_shapes_host.py   that census asserted on the twin alone
  tests/test_gpu_simplify_shapes.py    the device against the twin on those volumes: many segments, a second scan block"""
import ctypes as C

import numpy as np
import pytest

import simplify_twin as ST
from kit import same_bits, volume_ctx
from mesh_twin import mesh_indexed, same_normals
from simplify_cases import (BOX_DIMS, BOX_SIZE, CLUSTERS, MODES, box_distance, check, directed_edge_balance, grid, mesh_of, signed_volume, small_cases, stats_list, twin_of, volume_of)

pytestmark = pytest.mark.gpu
f32 = np.float32


# ---- 1. parity with the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "sphere", "two walls", "holes", "exact zeros", "six faces", "blob", "empty", "box with colour"])
def test_uploaded_volumes_match_the_twin(hsk, oracle, name):
    vol, dims, size, col = small_cases()[name]
    trk = volume_ctx(hsk, dims, size)
    try:
        if col is not None:
            trk.enable_color()
            trk.upload_color(col)
        trk.upload_tsdf(vol)
        for c in CLUSTERS:
            for mode in MODES:
                _, _, st = check(trk, twin_of(oracle, name, c, mode), c, mode, rgb=col is not None, tag=name)
        print(f"{name}: {st}")
        if col is not None:   # (and without rgb the same context gives the same geometry, no colour, no uncoloured count)
            check(trk, twin_of(oracle, name, 4, ST.QUADRIC), 4, ST.QUADRIC, rgb=False, tag=name)
    finally:
        trk.close()


def test_a_scanned_room_matches_the_twin(hsk, oracle, synth_frames):
    """64^3, a few tracked frames: the read-out runs on the volume with its deferred weights (no flush), the twin on the download"""
    trk = hsk.KinfuTracker(n=64)
    try:
        for k in range(4):
            trk.process_frame(synth_frames(k)[1])
        got = {(c, mode): trk.extract_mesh_simplified(cluster_voxels=c, mode=mode) for c in CLUSTERS for mode in MODES}
        vol = trk.download_tsdf()
        mesh = mesh_indexed(vol, *oracle.mc_table(), size=3.0, normals=False)
        assert len(mesh["faces"]) > 2000
        for (c, mode), (v, f, nrm, _, st) in got.items():
            tw = ST.simplify(vol, *oracle.mc_table(), c=c, mode=mode, size=3.0, mesh=mesh)
            assert same_bits(v, tw["vertices"]) and same_normals(nrm, tw["normals"]) and np.array_equal(f, tw["faces"]), (c, mode)
            assert stats_list(st) == stats_list(tw["stats"]), (c, mode, st, tw["stats"])
        print(got[(4, ST.QUADRIC)][4])
    finally:
        trk.close()


# ---- 2. what the rule promises ----------------------------------------------------------------------------------------------------
def test_a_closed_surface_stays_closed_on_the_device(hsk, oracle):
    vol, dims, size, _ = small_cases()["sphere"]
    trk = volume_ctx(hsk, dims, size)
    try:
        trk.upload_tsdf(vol)
        mesh = mesh_of(oracle, "sphere")
        v_in = signed_volume(mesh["vertices"], mesh["faces"])
        for c in CLUSTERS:
            for mode in MODES:
                v, f, _, _, _ = trk.extract_mesh_simplified(cluster_voxels=c, mode=mode, normals=False)
                assert len(f) > 0 and directed_edge_balance(f) == 0, (c, mode)
                assert signed_volume(v, f) * v_in > 0, (c, mode)
    finally:
        trk.close()


def test_a_flat_plane_stays_flat(hsk, oracle):
    """a tilted plane with an exactly linear stored TSDF, 600 x + 300 y + 1000 z = 29451 in voxel indices.  e: the largest distance
    of the INDEXED mesh's vertices to it.  The mean of a cluster lies in the hull of vertices that are each within e plus one quantum
    (sqrt(3) / 512 voxel covers half a quantum on three axes) of the plane, and the rank-1 correction moves it onto a weighted
    least-squares plane of triangles inside that same slab: every simplified vertex lies within 2 (e + sqrt(3) / 512) voxel"""
    n = 32
    x, y, z = grid((n, n, n))
    t = (600 * x + 300 * y + 1000 * z - 29451).astype(np.int16)
    vol = np.stack([t, np.full(t.shape, 1, np.int16)], axis=-1)
    normal = np.array([600.0, 300.0, 1000.0])
    cell = float(f32(3.0) / f32(n))

    def distance(v):
        g = np.asarray(v, np.float64) / cell - 0.5
        return np.abs(g @ normal - 29451.0) / np.linalg.norm(normal)

    trk = hsk.KinfuTracker(n=n)
    try:
        trk.upload_tsdf(vol)
        vi = trk.extract_mesh_indexed(normals=False, rgb=False)[0]
        e = float(distance(vi).max())
        bound = 2.0 * (e + np.sqrt(3.0) / 512.0)
        for c in CLUSTERS:
            for mode in MODES:
                v, f, _, _, st = trk.extract_mesh_simplified(cluster_voxels=c, mode=mode, normals=False)
                d = float(distance(v).max())
                print(f"c {c} mode {mode}: {len(v)} vertices, {len(f)} faces, farthest {d:.3e} voxel (e {e:.3e}, bound {bound:.3e})")
                assert len(v) > 0 and d <= bound, (c, mode, d, bound)
                assert st["n_rank"] == ([0, len(v), 0, 0] if mode == ST.QUADRIC else [len(v), 0, 0, 0]) and st["n_clamped"] == 0
    finally:
        trk.close()


def test_the_quadric_finds_the_corners_of_a_box(hsk, oracle):
    """a box room in 48^3 whose eight corners lie at voxel index 12 or 36 on every axis: the centres of clusters of 8.  d: the largest
    distance from an analytic corner to the nearest output vertex, in voxels.  Measured (also in DESIGN.md 8k): d_Q = 0 (the three
    walls' planes are exact in this TSDF and the solve returns their intersection), d_M = 2.309, the indexed mesh's own 0"""
    n = 48
    vol = volume_of(box_distance((n, n, n), (12, 12, 12), (36, 36, 36)))
    corners = np.array([[a, b, c] for a in (12, 36) for b in (12, 36) for c in (12, 36)], np.float64)
    cell = float(f32(3.0) / f32(n))

    def farthest(v):
        g = np.asarray(v, np.float64) / cell - 0.5
        return max(float(np.linalg.norm(g - k, axis=1).min()) for k in corners)

    trk = hsk.KinfuTracker(n=n)
    try:
        trk.upload_tsdf(vol)
        d_i = farthest(trk.extract_mesh_indexed(normals=False, rgb=False)[0])
        vq, _, _, _, sq = trk.extract_mesh_simplified(cluster_voxels=8, mode=ST.QUADRIC, normals=False)
        vm, _, _, _, _ = trk.extract_mesh_simplified(cluster_voxels=8, mode=ST.MEAN, normals=False)
        d_q, d_m = farthest(vq), farthest(vm)
        print(f"corner distance in voxels: quadric {d_q:.4f}, mean {d_m:.4f}, indexed mesh {d_i:.4f}; ranks {sq['n_rank']}")
        assert d_q < d_m
    finally:
        trk.close()


# ---- 3. the protocol ---------------------------------------------------------------------------------------------------------------
def test_call_protocol(hsk, oracle, synth_frames):
    trk = hsk.KinfuTracker(n=64)
    try:
        for k in range(4):
            trk.process_frame(synth_frames(k)[1])
        lib, h, L = trk.lib, trk.h, hsk._lib
        p = L.HskSimplifyParams(4, ST.QUADRIC, 0.0)
        before = trk.download_tsdf()
        # counts only, then the fill: the same result
        nv, nf, st0 = C.c_size_t(), C.c_size_t(), L.HskSimplifyStats()
        assert lib.hsk_extract_mesh_simplified(h, C.byref(p), None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), C.byref(st0)) == 0
        v, f, nrm, _, st = trk.extract_mesh_simplified(cluster_voxels=4)
        assert (nv.value, nf.value) == (len(v), len(f)) and len(f) > 100
        assert stats_list(hsk.kinfu.simplify_stats_dict(st0)) == stats_list(st)
        # params NULL is the default: c = 4, the quadric
        vd, fd = np.empty_like(v), np.empty_like(f)
        assert lib.hsk_extract_mesh_simplified(h, None, vd.ctypes.data, None, None, len(vd), C.byref(nv), fd.ctypes.data, len(fd), C.byref(nf), None) == 0
        assert same_bits(vd, v) and np.array_equal(fd, f)
        # a cap one short: an error, the counts set, the caller's memory untouched (guard values inside and behind)
        vb = np.full((len(v) + 1, 3), 7.0, f32)
        nb = np.full((len(v) + 1, 3), 7.0, f32)
        fb = np.full((len(f) + 1, 3), -5, np.int32)
        for cv, cf in ((len(v) - 1, len(f)), (len(v), len(f) - 1)):
            nv.value = nf.value = 0
            rc = lib.hsk_extract_mesh_simplified(h, C.byref(p), vb.ctypes.data, nb.ctypes.data, None, cv, C.byref(nv), fb.ctypes.data, cf, C.byref(nf), None)
            assert rc == -1 and (nv.value, nf.value) == (len(v), len(f))
            assert (vb == 7.0).all() and (nb == 7.0).all() and (fb == -5).all()
        # each subset of the arrays, each written whole and nothing behind it
        for want_v, want_n, want_f in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
            vb[:], nb[:], fb[:] = 7.0, 7.0, -5
            rc = lib.hsk_extract_mesh_simplified(h, C.byref(p), vb.ctypes.data if want_v else None, nb.ctypes.data if want_n else None, None, len(v),
                                                 C.byref(nv), fb.ctypes.data if want_f else None, len(f), C.byref(nf), None)
            assert rc == 0
            assert same_bits(vb[:-1], v) if want_v else (vb == 7.0).all()
            assert same_normals(nb[:-1], nrm) if want_n else (nb == 7.0).all()
            assert np.array_equal(fb[:-1], f) if want_f else (fb == -5).all()
            assert (vb[-1] == 7.0).all() and (nb[-1] == 7.0).all() and (fb[-1] == -5).all()
        # a repeat is identical, also with the other products and another cluster size in between
        trk.extract_cloud()
        trk.extract_mesh_simplified(cluster_voxels=2, mode=ST.MEAN)
        trk.extract_mesh_indexed(rgb=False)
        v2, f2, n2, _, st2 = trk.extract_mesh_simplified(cluster_voxels=4)
        assert same_bits(v2, v) and np.array_equal(f2, f) and same_normals(n2, nrm) and st2 == st
        # nothing the tracker reads was written: the volume is what it was
        assert np.array_equal(trk.download_tsdf(), before)
        # rgb without colour
        cb = np.zeros((len(v), 3), np.uint8)
        assert lib.hsk_extract_mesh_simplified(h, C.byref(p), None, None, cb.ctypes.data, len(v), C.byref(nv), None, 0, C.byref(nf), None) == -3
        with pytest.raises(hsk.KinfuError, match="colour"):
            trk.extract_mesh_simplified(rgb=True)
        # the argument errors on a live context
        for bad in (L.HskSimplifyParams(3, 0, 0.0), L.HskSimplifyParams(32, 0, 0.0), L.HskSimplifyParams(4, 2, 0.0), L.HskSimplifyParams(4, 0, -0.1),
                    L.HskSimplifyParams(4, 0, 1.0), L.HskSimplifyParams(4, 0, float("nan"))):
            assert lib.hsk_extract_mesh_simplified(h, C.byref(bad), None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), None) == -1
        # one more integrated frame: the count cache is voided, the result changes and matches the twin again
        trk.process_frame(synth_frames(4)[1])
        v3, f3, n3, _, st3 = trk.extract_mesh_simplified(cluster_voxels=4)
        assert not (v3.shape == v.shape and same_bits(v3, v))
        tw = ST.simplify(trk.download_tsdf(), *oracle.mc_table(), c=4, size=3.0)
        assert same_bits(v3, tw["vertices"]) and np.array_equal(f3, tw["faces"]) and same_normals(n3, tw["normals"])
        assert stats_list(st3) == stats_list(tw["stats"])
    finally:
        trk.close()


def test_a_slab_of_a_group_is_refused(hsk, synth_frames):
    grp = hsk.KinfuGroup(hsk.default_config(64), device_ids=[0, 0])
    try:
        grp.process_frame(synth_frames(0)[1])
        for i in range(grp.n_slabs()):
            with pytest.raises(hsk.KinfuError, match="slab"):
                grp.slab(i).extract_mesh_simplified(rgb=False)
    finally:
        grp.close()
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        with pytest.raises(hsk.KinfuError, match="slab"):
            part.extract_mesh_simplified()
    finally:
        part.close()
