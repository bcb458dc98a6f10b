"""Hole filling on the device (hsk_fill_holes, hsk_download_fill_mask) against the numpy twin
(tests/fill_twin.py): the whole downloaded volume, the mask and the twin-defined stats are EQUAL to the twin's -- the twin runs no
skip logic, so an error in the tiles' skip test shows as a differing word."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import fill_cases as FC
import fill_twin as FT
from kit import dims_of, same_bits, state_of, volume_ctx

pytestmark = pytest.mark.gpu
TWIN_STATS = ("n_unseen", "n_reached", "n_written", "n_written_negative", "iterations_run")


def ctx(hsk, dims, size=AT.DST_SIZE, **over):
    return volume_ctx(hsk, dims, size, **over)


def check_fill(trk, name, twin, box=None, **params):
    """fills the context's volume; the download, the mask and the stats equal the twin's"""
    ref, ref_mask, ref_st = twin
    st = trk.fill_holes(box=box, **params)
    out, mask = trk.download_tsdf(), trk.download_fill_mask()
    print(f"{name}: {st}")
    assert int((out != ref).sum()) == 0, f"{name}: {int((out != ref).any(axis=-1).sum())} words differ"
    assert mask.dtype == np.uint8 and int((mask != ref_mask).sum()) == 0, f"{name}: {int((mask != ref_mask).sum())} mask bytes differ"
    assert {k: st[k] for k in TWIN_STATS} == ref_st, name
    return st


# ---- 1. random volumes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", FC.RANDOM_DIMS)
def test_random_volumes_match_the_twin(hsk, dims):
    """a fifth of the voxels in random states; 46 and 41 planes: the last plane group holds padding planes, which are no voxels; 72 x
    56: X and Y are 8 mod 16, the last tiles are half empty.  The default parameters (4 iterations at these cells, SURFACE, band 2),
    then ALL with 1, 2 and 9 iterations, each from the same upload"""
    X, Y, Z = dims
    vol = FC.random_volume(dims)
    trk = ctx(hsk, dims, size=(3.0 * X / 80, 3.0 * Y / 64, 3.0 * Z / 48))
    try:
        p = trk.default_fill_params()
        assert (p.iterations, p.keep, p.band, p.fill_weight) == (FC.RANDOM_PARAMS[0][0], hsk.FILL_SURFACE, 2, 1)
        for i, (it, keep) in enumerate(FC.RANDOM_PARAMS):
            trk.upload_tsdf(vol)
            params = {} if i == 0 else dict(iterations=it, keep=keep)
            st = check_fill(trk, f"random {dims} {it} {keep}", FC.random_twin(dims, it, keep), **params)
            assert st["n_written"] > 1000
    finally:
        trk.close()


# ---- 2. hand-built shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FC.shapes()))
def test_hand_built_shapes_match_the_twin(hsk, name):
    vol, params, box = FC.shapes()[name]
    trk = ctx(hsk, dims_of(vol))
    try:
        trk.upload_tsdf(vol)
        trk.label_components()
        st = check_fill(trk, name, FC.shape_twin(name), box=box, **params)
        # vol_epoch moves iff something was written: a cached pass reports reuse exactly when nothing was
        assert trk.label_components()[1]["labels_reused"] == (1 if st["n_written"] == 0 else 0)
        if name in ("no source", "no non-source", "an empty box"):
            assert st["n_written"] == 0 and st["n_reached"] == 0 and not trk.download_fill_mask().any()
    finally:
        trk.close()


# ---- 3. the planar wall closes -----------------------------------------------------------------------------------------------------
def boundary_edges_inside(verts, faces, cell, x0, x1, y0, y1):
    """the edges used by exactly one triangle whose two vertices lie strictly inside x0 < x < x1, y0 < y < y1 (voxel units; a
    voxel's centre lies at its index + 0.5)"""
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    uniq, counts = np.unique(e, axis=0, return_counts=True)
    lone = uniq[counts == 1]
    v = verts.astype(np.float64)
    inside = (v[:, 0] > x0 * cell[0]) & (v[:, 0] < x1 * cell[0]) & (v[:, 1] > y0 * cell[1]) & (v[:, 1] < y1 * cell[1])
    return int((inside[lone[:, 0]] & inside[lone[:, 1]]).sum()) if len(lone) else 0


def test_the_planar_wall_closes(hsk):
    """DESIGN.md 8p's property: the wall at z0 = 30.3 voxels with a 12 x 12 column hole, 16 iterations, SURFACE, band 2 -- every one
    of the 144 hole columns has exactly one z crossing, within 0.25 voxel of z0 (the twin measures 30.305 .. 30.321; 24 584 voxels
    reached, 864 written).  The indexed mesh of the filled volume has no boundary edge (an edge of exactly one triangle) with both
    vertices inside the hole's x and y extent.  The unfilled mesh's open rim runs through the centres of the observed columns
    next to the hole, half a voxel OUTSIDE the hole's columns -- a cube needs all eight corners observed --, so the extent is taken
    one and a half voxels wider on every side: the unfilled mesh has boundary edges in it, the filled one none (which says more
    than none inside the hole's columns alone; that is asserted too)"""
    vol, (x0, x1, y0, y1) = FT.planar_wall()
    twin = FC.shape_twin("planar wall")
    dims = dims_of(vol)
    cell = tuple(AT.DST_SIZE[i] / dims[i] for i in range(3))
    wide, hole = (x0 - 1.5, x1 + 1.5, y0 - 1.5, y1 + 1.5), (x0, x1, y0, y1)
    trk = ctx(hsk, dims)
    try:
        trk.upload_tsdf(vol)
        v0, f0 = trk.extract_mesh_indexed(normals=False, rgb=False)[:2]
        open_before = boundary_edges_inside(v0, f0, cell, *wide)
        st = check_fill(trk, "planar wall", twin, iterations=16)
        assert st["n_written"] == twin[2]["n_written"] == 864 and st["n_reached"] == 24584
        out = trk.download_tsdf()
        zs = [FT.column_crossings(out, x, y) for y in range(y0, y1) for x in range(x0, x1)]
        assert len(zs) == 144 and all(len(z) == 1 for z in zs)
        print(f"crossings at {min(z[0] for z in zs):.3f} .. {max(z[0] for z in zs):.3f}")
        assert all(abs(z[0] - 30.3) <= 0.25 for z in zs)
        v1, f1 = trk.extract_mesh_indexed(normals=False, rgb=False)[:2]
        open_after = boundary_edges_inside(v1, f1, cell, *wide)
        print(f"boundary edges about the hole: {open_before} before, {open_after} after; faces {len(f0)} -> {len(f1)}")
        assert open_before > 0 and open_after == 0 and boundary_edges_inside(v1, f1, cell, *hole) == 0 and len(f1) > len(f0)
    finally:
        trk.close()


# ---- 4. deferred weights -----------------------------------------------------------------------------------------------------------
def test_fill_on_a_volume_with_deferred_weights_and_the_scan_goes_on(hsk):
    """24 frames of room 0 integrated at 64^3 leave free-space weights in the summaries; the fill runs BEFORE any download and its
    download equals the twin fed by the download of a second, identically grown context, deferred weights included; one more frame
    then integrates on both, and what the fill did not write stays equal"""
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 300, 12)]
    depths = [hsk.synth_room_depth(0, p) for p in poses]

    def grown(n):
        trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
        for d, p in zip(depths[:n], poses[:n]):
            trk.integrate(d, p)
        return trk

    a, b = grown(24), grown(24)
    try:
        st = b.fill_holes()
        vol = a.download_tsdf()
        assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
        it = FT.default_iterations((3.0 / 64,) * 3)
        ref, ref_mask, ref_st = FT.fill(vol, it)
        print(f"deferred weights: {st}")
        assert b.default_fill_params().iterations == it and {k: st[k] for k in TWIN_STATS} == ref_st and ref_st["n_written"] > 100
        filled = b.download_tsdf()
        assert int((filled != ref).sum()) == 0 and np.array_equal(b.download_fill_mask(), ref_mask)
        assert (filled[ref_mask == 1][:, 1] == 1).all() and np.array_equal(filled[ref_mask == 0], vol[ref_mask == 0])
        for t in (a, b):
            t.integrate(depths[24], poses[24])
        va, vb = a.download_tsdf(), b.download_tsdf()
        assert not np.array_equal(va, vol) and np.array_equal(va[ref_mask == 0], vb[ref_mask == 0])
    finally:
        a.close()
        b.close()


def test_pose_and_maps_stay_and_tracking_goes_on(hsk, synth_frames):
    trk = hsk.KinfuTracker(n=64)
    try:
        for k in range(4):
            trk.process_frame(synth_frames(k)[1])
        before = state_of(trk, False)
        st = trk.fill_holes()
        print(f"mid-scan: {st}")
        assert st["n_written"] > 0
        for a, b in zip(before, state_of(trk, False)):
            assert same_bits(a, b)
        for k in range(4, 8):
            pose, ok = trk.process_frame(synth_frames(k)[1])
            assert ok, f"frame {k} lost tracking after the fill"
    finally:
        trk.close()


# ---- 5. colour ---------------------------------------------------------------------------------------------------------------------
def test_the_colour_volume_stays_bit_for_bit(hsk):
    vol, params, _ = FC.shapes()["hole across x = 16, y = 16, z = 8"]
    trk = ctx(hsk, dims_of(vol))
    try:
        trk.upload_tsdf(vol)
        trk.enable_color()
        rng = np.random.default_rng(5)
        colour = rng.integers(0, 256, vol.shape[:3] + (4,), dtype=np.uint8)
        trk.upload_color(colour)
        before = trk.download_color()
        st = check_fill(trk, "colour", FC.shape_twin("hole across x = 16, y = 16, z = 8"), **params)
        assert st["n_written"] > 0 and trk.download_color().tobytes() == before.tobytes() == colour.tobytes()
    finally:
        trk.close()


# ---- 6. the mask -------------------------------------------------------------------------------------------------------------------
def test_the_mask_is_held_while_the_volume_stands(hsk):
    vol, params, _ = FC.shapes()["hole across x = 16, y = 16, z = 8"]
    ref_mask = FC.shape_twin("hole across x = 16, y = 16, z = 8")[1]
    X, Y, Z = dims_of(vol)
    trk = ctx(hsk, (X, Y, Z))
    try:
        trk.upload_tsdf(vol)
        with pytest.raises(hsk.KinfuError, match="no fill is held"):
            trk.download_fill_mask()
        trk.fill_holes(**params)
        full = trk.download_fill_mask()
        assert np.array_equal(full, ref_mask) and np.array_equal(trk.download_fill_mask(), full)       # held: a second read gives the same
        for lo, hi in (((14, 15, 5), (27, 26, 12)), ((0, 0, 0), (X, Y, 1)), ((13, 0, 7), (17, Y, 9)), ((3, 3, 3), (3, 9, 9))):
            part = trk.download_fill_mask(box=(lo, hi))
            assert part.shape == (hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]) and np.array_equal(part, full[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]])
        with pytest.raises(hsk.KinfuError, match="box"):
            trk.download_fill_mask(box=((0, 0, 0), (X + 1, Y, Z)))
        # a fill that writes nothing holds an all-zero mask at the unchanged epoch
        trk.label_components()
        assert trk.fill_holes(box=((0, 0, 0), (4, 4, 4)))["n_written"] == 0 and not trk.download_fill_mask().any()
        assert trk.label_components()[1]["labels_reused"] == 1
        trk.fill_holes(**params)                                                                          # (everything is filled already: nothing to write)
        trk.upload_tsdf(vol)
        with pytest.raises(hsk.KinfuError, match="no fill is held"):
            trk.download_fill_mask()
        assert trk.lib.hsk_download_fill_mask(trk.h, None, full.ctypes.data) == -3
    finally:
        trk.close()
    trk = hsk.KinfuTracker(n=64)
    try:
        depth, pose = hsk.synth_depth(hsk.synth_pose(0)), hsk.synth_pose(0)
        trk.integrate(depth, pose)
        trk.fill_holes()
        assert trk.download_fill_mask().shape == (64, 64, 64)
        trk.integrate(depth, pose)
        with pytest.raises(hsk.KinfuError, match="no fill is held"):
            trk.download_fill_mask()
    finally:
        trk.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_untouched(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    vol, params, _ = FC.shapes()["hole across x = 16, y = 16, z = 8"]
    X, Y, Z = dims_of(vol)
    trk = ctx(hsk, (X, Y, Z))
    try:
        trk.upload_tsdf(vol)
        trk.label_components()
        for bad in (dict(iterations=0), dict(iterations=256), dict(iterations=-1), dict(keep=2), dict(keep=-1), dict(band=-1), dict(band=9),
                    dict(fill_weight=0), dict(fill_weight=129)):
            st = L.HskFillStats(n_written=77)
            p = hsk.default_fill_params(trk, **bad)
            assert lib.hsk_fill_holes(trk.h, C.byref(p), None, C.byref(st)) == -1 and st.n_written == 77 and lib.hsk_last_error(trk.h), bad
        for lo, hi in (((-1, 0, 0), (X, Y, Z)), ((0, 0, 0), (X, Y + 1, Z)), ((0, 0, 5), (X, Y, 4))):
            with pytest.raises(hsk.KinfuError, match="the box must satisfy"):
                trk.fill_holes(box=(lo, hi))
        with pytest.raises(hsk.KinfuError, match="iterations"):
            trk.fill_holes(iterations=300)
        with pytest.raises(TypeError, match="no field"):
            trk.fill_holes(weight=3)
        assert trk.label_components()[1]["labels_reused"] == 1 and np.array_equal(trk.download_tsdf(), vol)
    finally:
        trk.close()
    # between submit and wait
    trk = hsk.KinfuTracker(n=64)
    try:
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        trk.submit_frame(hsk.synth_depth(hsk.synth_pose(1)))
        st, mask = L.HskFillStats(n_written=77), np.full(64 ** 3, 9, np.uint8)
        assert lib.hsk_fill_holes(trk.h, None, None, C.byref(st)) == -3 and st.n_written == 77 and b"in flight" in lib.hsk_last_error(trk.h)
        assert lib.hsk_download_fill_mask(trk.h, None, mask.ctypes.data) == -3 and (mask == 9).all()
        _, ok = trk.wait_frame()
        assert ok and trk.fill_holes()["n_unseen"] > 0
    finally:
        trk.close()
    # a context that stores part of its volume, and the slabs of a group
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        for call in (lambda t: t.fill_holes(), lambda t: t.download_fill_mask()):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call(part)
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        for i in range(g.n_slabs()):
            for call in (lambda t: t.fill_holes(), lambda t: t.download_fill_mask()):
                with pytest.raises(hsk.KinfuError, match="slab"):
                    call(g.slab(i))
        _, ok = g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))
        assert ok
    finally:
        g.close()
