"""hsk_extract_mesh_simplified on the GPU at the widths and row counts that the volumes of tests/test_gpu_simplify.py do not reach
(tests/simplify_cases.py; what each case reaches is asserted without a GPU by tests/test_simplify_shapes_host.py): cluster rows
of up to nine 64-cluster segments, more than 1024 cluster rows, cube rows of seventeen trips, a top cell layer that the volume's
last plane cuts at every cluster size, a colour volume at a row pitch of 1032, the scratch buffer growing under a live count cache.
Vertices, normals, colours, faces, counts and every statistic bit for bit against the numpy twin; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import simplify_cases as SC
import simplify_twin as ST
from kit import same_bits, volume_ctx
from mesh_twin import mesh_indexed, same_normals
from simplify_cases import CLUSTERS, MODES, check, stats_list

pytestmark = pytest.mark.gpu
f32 = np.float32


def hall_ctx(hsk):
    vol, dims, size, col = SC.shape_cases()["hall"]
    trk = volume_ctx(hsk, dims, size)
    try:
        trk.enable_color()
        trk.upload_color(col)
        trk.upload_tsdf(vol)
    except Exception:
        trk.close()
        raise
    return trk


def test_the_hall_matches_the_twin(hsk, oracle):
    """one context, the cluster sizes in the order 16, 8, 4, 2, 4, 16: on the way down the scratch buffer grows three times under
    a live count cache, on the way back it is reused at another shift; then without rgb; then another volume (a new vol_epoch)"""
    trk = hall_ctx(hsk)
    try:
        for c in (16, 8, 4, 2, 4, 16):
            for mode in MODES:
                _, _, st = check(trk, SC.twin_of(oracle, "hall", c, mode), c, mode, rgb=True, tag="hall")
            print(f"hall c {c}: {st}")
        check(trk, SC.twin_of(oracle, "hall", 4, ST.QUADRIC), 4, ST.QUADRIC, rgb=False, tag="hall without rgb")
        trk.upload_tsdf(SC.shape_cases()["hall flipped"][0])
        _, _, st = check(trk, SC.twin_of(oracle, "hall flipped", 2, ST.QUADRIC), 2, ST.QUADRIC, rgb=True, tag="hall flipped")
        assert st["n_out_vertices"] != SC.twin_of(oracle, "hall", 2, ST.QUADRIC)["stats"]["n_out_vertices"]
    finally:
        trk.close()


def test_the_tall_room_matches_the_twin(hsk, oracle):
    vol, dims, size, _ = SC.shape_cases()["tall"]
    trk = volume_ctx(hsk, dims, size)
    try:
        trk.upload_tsdf(vol)
        for c in CLUSTERS:
            for mode in MODES:
                _, _, st = check(trk, SC.twin_of(oracle, "tall", c, mode), c, mode, tag="tall")
            print(f"tall c {c}: {st}")
    finally:
        trk.close()


def test_a_scanned_wide_volume_matches_the_twin(hsk, oracle, synth_frames):
    """320 x 48 x 40 over 3 m, four frames integrated at their ground-truth poses (no tracking): the read-out runs on the volume
    with its deferred weights, before any download, the twin on the download afterwards; the volume is what it was"""
    trk = volume_ctx(hsk, SC.WIDE_DIMS, SC.WIDE_SIZE)
    try:
        for pose, depth in SC.wide_frames(synth_frames):
            trk.integrate(depth, pose)
        got = {(c, mode): trk.extract_mesh_simplified(cluster_voxels=c, mode=mode) for c in (2, 4) for mode in MODES}
        vol = trk.download_tsdf()
        mesh = mesh_indexed(vol, *oracle.mc_table(), size=SC.WIDE_SIZE, normals=False)
        assert len(mesh["faces"]) > 2000
        for (c, mode), (v, f, nrm, _, st) in got.items():
            tw = ST.simplify(vol, *oracle.mc_table(), c=c, mode=mode, size=SC.WIDE_SIZE, mesh=mesh)
            cs = SC.census(vol, mesh, tw, c)
            assert cs["cseg"] >= 2 and len(cs["segments_used"]) >= 2, (c, cs)       # (the host test's conditions, on THIS volume)
            assert same_bits(v, tw["vertices"]), (c, mode, len(v), len(tw["vertices"]))
            assert same_normals(nrm, tw["normals"]), (c, mode)
            assert f.shape == tw["faces"].shape and np.array_equal(f, tw["faces"]), (c, mode)
            assert stats_list(st) == stats_list(tw["stats"]), (c, mode, st, tw["stats"])
        print(got[(4, ST.QUADRIC)][4])
        # the same calls again after the download (the weights flushed), and nothing the tracker reads was written
        for (c, mode), (v, f, _, _, st) in got.items():
            v2, f2, _, _, st2 = trk.extract_mesh_simplified(cluster_voxels=c, mode=mode)
            assert same_bits(v2, v) and np.array_equal(f2, f) and st2 == st, (c, mode)
        assert np.array_equal(trk.download_tsdf(), vol)
    finally:
        trk.close()


def test_counts_then_an_exact_fill_on_the_hall(hsk, oracle):
    """a counts-only call at c = 2 (no array at all): the totals and every statistic are the twin's; the fill that follows with
    capacities of exactly those totals writes the arrays whole and nothing behind them"""
    tw = SC.twin_of(oracle, "hall", 2, ST.QUADRIC)
    trk = hall_ctx(hsk)
    try:
        lib, h, L = trk.lib, trk.h, hsk._lib
        p = L.HskSimplifyParams(2, ST.QUADRIC, 0.0)
        nv, nf, st0 = C.c_size_t(), C.c_size_t(), L.HskSimplifyStats()
        assert lib.hsk_extract_mesh_simplified(h, C.byref(p), None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), C.byref(st0)) == 0
        assert (nv.value, nf.value) == (len(tw["vertices"]), len(tw["faces"]))
        want = dict(tw["stats"], n_uncolored=0)                                     # (no rgb asked for: nothing counted as uncoloured)
        assert stats_list(hsk.kinfu.simplify_stats_dict(st0)) == stats_list(want), (hsk.kinfu.simplify_stats_dict(st0), want)
        n, m = nv.value, nf.value
        vb, nb = np.full((n + 1, 3), 7.0, f32), np.full((n + 1, 3), 7.0, f32)
        cb, fb = np.full((n + 1, 3), 9, np.uint8), np.full((m + 1, 3), -5, np.int32)
        st1 = L.HskSimplifyStats()
        nv.value = nf.value = 0
        assert lib.hsk_extract_mesh_simplified(h, C.byref(p), vb.ctypes.data, nb.ctypes.data, cb.ctypes.data, n, C.byref(nv), fb.ctypes.data, m,
                                               C.byref(nf), C.byref(st1)) == 0
        assert (nv.value, nf.value) == (n, m)
        assert same_bits(vb[:-1], tw["vertices"]) and same_normals(nb[:-1], tw["normals"])
        assert np.array_equal(cb[:-1], tw["rgb"]) and np.array_equal(fb[:-1], tw["faces"])
        assert (vb[-1] == 7.0).all() and (nb[-1] == 7.0).all() and (cb[-1] == 9).all() and (fb[-1] == -5).all()
        assert stats_list(hsk.kinfu.simplify_stats_dict(st1)) == stats_list(tw["stats"])
    finally:
        trk.close()
