"""Surface components on the GPU: hsk_label_components, hsk_download_components and hsk_prune_components against the numpy
restatement of the rule (tests/components_twin.py), every label, record, count and volume word EQUAL: the carved room with injected
blobs and random volumes at the sizes that have padding planes and ragged tiles; the shapes that break a tiled union-find; a
volume with deferred weights; prune bit for bit, with and without colour; what pruning is for (cloud, mesh, view, volume image);
nothing else of the context moves and a scan goes on; the errors."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import components_twin as KT
import np_twin as T
import reloc_twin as RT
from components_cases import BLOBS, grow, injected_volume, shapes, speckled, twin_of
from cover_cases import EYE, carved_volume
from kit import dims_of, same_bits, state_of, volume_ctx

pytestmark = pytest.mark.gpu
f32 = np.float32


def ctx(hsk, dims, size=AT.DST_SIZE, **over):
    return volume_ctx(hsk, dims, size, **over)


def check_against_twin(trk, name, vol):
    """labels, records and stats of the context's volume equal the twin's of `vol`"""
    ref_lab, ref_rec = twin_of(name, vol)
    rec, st = trk.label_components()
    lab = trk.download_components()
    print(f"{name}: {st}")
    assert lab.dtype == np.uint32 and int((lab != ref_lab).sum()) == 0, f"{name}: {int((lab != ref_lab).sum())} labels differ"
    assert len(rec) == len(ref_rec) and np.array_equal(rec, ref_rec), f"{name}: the records differ"
    assert {k: st[k] for k in ("n_components", "n_inside", "largest")} == KT.stats(ref_rec), name
    return rec, st


@pytest.fixture(scope="module")
def mv():
    return KT.default_min_voxels(AT.DST_SIZE, AT.DST_DIMS, T.tau_of(AT.DST_SIZE, AT.DST_DIMS, 0.03))


# ---- 1. labels, records and stats against the twin -----------------------------------------------------------------------------
def test_the_injected_room_matches_the_twin(hsk, mv):
    vol = injected_volume()[0]
    trk = ctx(hsk, AT.DST_DIMS)
    try:
        trk.upload_tsdf(vol)
        rec, st = check_against_twin(trk, "injected", vol)
        assert st["labels_reused"] == 0 and trk.label_components()[1]["labels_reused"] == 1
        assert trk.default_prune_params().min_voxels == mv and int((rec["n_voxels"] < mv).sum()) == len(BLOBS)
    finally:
        trk.close()


@pytest.mark.parametrize("dims", [(80, 64, 48), (80, 64, 46), (80, 64, 41), (72, 56, 40)])
def test_random_volumes_match_the_twin(hsk, dims):
    """a fifth of the voxels in random states: thousands of components; 46 and 41 planes: the last plane group holds padding
    planes, which are no voxels and connect nothing; 72 x 56: X and Y are 8 mod 16, the last tiles are half empty"""
    X, Y, Z = dims
    vol = np.ascontiguousarray(speckled(carved_volume(), Z)[:Z, :Y, :X])
    trk = ctx(hsk, dims, size=(3.0 * X / 80, 3.0 * Y / 64, 3.0 * Z / 48))
    try:
        trk.upload_tsdf(vol)
        rec, _ = check_against_twin(trk, f"speckled {dims}", vol)
        assert len(rec) > 2000
    finally:
        trk.close()


# ---- 2. the shapes that break a tiled union-find -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(shapes()))
def test_hand_built_shapes_match_the_twin(hsk, name):
    vol, n = shapes()[name]
    trk = ctx(hsk, dims_of(vol))
    try:
        trk.upload_tsdf(vol)
        rec, st = check_against_twin(trk, name, vol)
        assert st["n_components"] == n
        if n == 0:
            assert (trk.download_components() == KT.NONE).all() and st["n_inside"] == 0 and st["largest"] == 0
    finally:
        trk.close()


# ---- 3. deferred weights, the cached labelling -----------------------------------------------------------------------------------
def test_labels_on_a_volume_with_deferred_weights_and_the_cache(hsk):
    """24 frames of room 0 integrated at 64^3 leave free-space weights in the summaries; the labelling is taken BEFORE any download
    and equals the twin fed by the download of a second, identically grown context -- and the first context's download afterwards
    equals the second's, deferred weights included: the labelling enqueued no flush that changed anything.  A second call gives the same
    bytes and reports labels_reused; after one more frame it does not, and the labels are the twin's again"""
    poses = [hsk.synth_room_pose(0, k, 720) for k in range(0, 300, 12)]
    depths = [hsk.synth_room_depth(0, p) for p in poses]

    def grown(n):
        trk = hsk.KinfuTracker(n=64, init_pose=poses[0])
        for d, p in zip(depths[:n], poses[:n]):
            trk.integrate(d, p)
        return trk

    a, b = grown(24), grown(24)
    try:
        rec, st = b.label_components()
        lab = b.download_components()
        vol = a.download_tsdf()
        assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
        ref_lab = KT.labels(vol)
        ref_rec = KT.records(vol, ref_lab)
        print(f"deferred weights: {st}, the head {rec[:3]}")
        assert int((lab != ref_lab).sum()) == 0 and np.array_equal(rec, ref_rec) and st["n_inside"] == int(KT.inside(vol).sum()) > 1000
        rec2, st2 = b.label_components()
        assert st["labels_reused"] == 0 and st2["labels_reused"] == 1 and rec2.tobytes() == rec.tobytes() and b.download_components().tobytes() == lab.tobytes()
        assert np.array_equal(b.download_tsdf(), vol)
        for t in (a, b):
            t.integrate(depths[24], poses[24])
        rec3, st3 = b.label_components()
        vol3 = a.download_tsdf()
        assert st3["labels_reused"] == 0 and not np.array_equal(vol3, vol)
        assert np.array_equal(b.download_components(), KT.labels(vol3)) and np.array_equal(rec3, KT.records(vol3))
    finally:
        a.close()
        b.close()


# ---- 4. prune, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [KT.UNSEEN, KT.FREE])
@pytest.mark.parametrize("colour", [False, True])
def test_prune_equals_the_twin_bit_for_bit(hsk, mv, fill, colour):
    vol = injected_volume()[0]
    trk = ctx(hsk, AT.DST_DIMS)
    try:
        trk.upload_tsdf(vol)
        col = None
        if colour:
            trk.enable_color()
            col = np.random.default_rng(5).integers(1, 255, vol.shape[:3] + (4,)).astype(np.uint8)
            trk.upload_color(col)
        before = trk.download_tsdf()
        assert np.array_equal(before, vol)
        ref, ref_col, ref_st = KT.prune(before, col, min_voxels=mv, fill=fill)
        st = trk.prune_components(min_voxels=mv, fill=fill)
        after = trk.download_tsdf()
        print(f"fill {fill}, colour {colour}: {st}")
        assert st == ref_st and st["n_pruned"] == len(BLOBS)
        assert int((after != ref).sum()) == 0
        changed = (after != before).any(-1)
        cores = np.logical_or.reduce(injected_volume()[1])
        assert np.array_equal(changed, cores), "exactly the pruned components' words changed"
        if colour:
            got_col = trk.download_color()
            assert np.array_equal(got_col, ref_col) and (got_col[cores] == 0).all() and np.array_equal(got_col[~cores], col[~cores])
        rec, st2 = trk.label_components()                                  # the pruned volume, labelled afresh
        assert st2["labels_reused"] == 0 and np.array_equal(rec, KT.records(ref))
    finally:
        trk.close()


def test_prune_that_prunes_nothing_writes_nothing_and_keep_largest(hsk, mv):
    vol = injected_volume()[0]
    trk = ctx(hsk, AT.DST_DIMS)
    try:
        trk.upload_tsdf(vol)
        rec, _ = trk.label_components()
        st = trk.prune_components(min_voxels=0, keep_largest=0)
        assert st == {"n_components": len(rec), "n_pruned": 0, "n_pruned_voxels": 0, "n_kept_voxels": int(rec["n_voxels"].sum())}
        assert trk.label_components()[1]["labels_reused"] == 1, "vol_epoch moved: cached passes are void"
        assert np.array_equal(trk.download_tsdf(), vol)
        st = trk.prune_components(min_voxels=0, keep_largest=1)
        ref, _, ref_st = KT.prune(vol, None, min_voxels=0, keep_largest=1)
        after = trk.download_tsdf()
        assert st == ref_st and st["n_pruned"] == len(rec) - 1 and np.array_equal(after, ref)
        first = twin_of("injected", vol)[0] == np.uint32(KT.root_lin(rec[:1], AT.DST_DIMS)[0])
        assert np.array_equal(KT.inside(after), first), "exactly the first record's voxels stay INSIDE"
    finally:
        trk.close()


# ---- 5. what it is for ---------------------------------------------------------------------------------------------------------------
def test_the_pruned_room_reads_out_like_the_room_that_never_had_the_blobs(hsk, mv):
    vol, cores = injected_volume()
    base = carved_volume()
    trk, clean, dirty = ctx(hsk, AT.DST_DIMS), ctx(hsk, AT.DST_DIMS), ctx(hsk, AT.DST_DIMS)
    try:
        trk.upload_tsdf(vol)
        clean.upload_tsdf(base)
        dirty.upload_tsdf(vol)
        rec = trk.label_components()[0]
        st = trk.prune_components()                                        # the defaults: min_voxels of the context, UNSEEN
        assert st["n_pruned"] == len(BLOBS)
        pruned = trk.download_tsdf()
        # the cloud: a crossing needs a negative, observed partner (on the twin first)
        want = T.extract_cloud(base, AT.DST_SIZE)
        assert np.array_equal(T.extract_cloud(pruned, AT.DST_SIZE), want)
        cloud = trk.extract_cloud()[0]
        assert same_bits(cloud, clean.extract_cloud()[0]) and same_bits(cloud, want) and len(dirty.extract_cloud()[0]) > len(cloud)
        # the mesh: no vertex inside a blob's box grown by one voxel
        verts = trk.extract_mesh_indexed(rgb=False)[0]
        dverts = dirty.extract_mesh_indexed(rgb=False)[0]
        cell = np.array([f32(AT.DST_SIZE[i]) / f32(AT.DST_DIMS[i]) for i in range(3)], np.float64)
        n_dirty = 0
        for r in rec[rec["n_voxels"] < mv]:
            lo, hi = (r["lo"] - 1) * cell, (r["hi"] + 1) * cell
            assert not np.all((verts >= lo) & (verts <= hi), axis=1).any()
            n_dirty += int(np.all((dverts >= lo) & (dverts <= hi), axis=1).sum())
        assert n_dirty > 100 and len(verts) == len(clean.extract_mesh_indexed(rgb=False)[0])
        # the view: a camera that looked at the large blob sees the wall behind it, at the wall's depth: the hit is the crossing
        # between two samples inside the wall's own band, whose words the prune left bit for bit
        (cx, cy, cz), _ = BLOBS[2]
        pose = RT.look_at(EYE, ((cx + 0.5) * cell[0], (cy + 0.5) * cell[1], (cz + 0.5) * cell[2])).astype(f32)
        kw = dict(width=160, height=120, fx=130.0, fy=130.0, cx=79.5, cy=59.5, pose=pose, rgb=False)
        d_pruned, d_clean, d_dirty = (t.render_view(**kw)["depth"].astype(np.int64) for t in (trk, clean, dirty))
        blob = (d_dirty > 0) & (d_dirty < d_clean - 250)
        print(f"view: {int(blob.sum())} pixels saw the blob; {int((d_pruned != d_clean)[blob].sum())} of them differ from the clean room's depth, {int((d_pruned != d_clean).sum())} of all")
        assert blob.sum() > 50 and (d_clean[blob] > 0).all() and np.array_equal(d_pruned[blob], d_clean[blob])
        # the volume image round-trips the pruned volume
        image = trk.pack_volume()
        clean.unpack_volume(image)
        assert np.array_equal(clean.download_tsdf(), pruned)
    finally:
        for t in (trk, clean, dirty):
            t.close()


# ---- 6. the context otherwise does not move ----------------------------------------------------------------------------------------
def test_pose_and_maps_stay_and_a_scan_goes_on(hsk, synth_frames):
    trk = hsk.KinfuTracker(n=64)
    try:
        for k in range(4):
            trk.process_frame(synth_frames(k)[1])
        vol = trk.download_tsdf()
        # a blob of 27 voxels in the middle of observed free space, uploaded into the scan
        free = (vol[..., 0] == 32767) & (vol[..., 1] != 0)
        room = ~grow(grow(grow(~free)))
        z, y, x = (int(v[len(v) // 2]) for v in np.nonzero(room))
        core = np.zeros(free.shape, bool)
        core[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = True
        ring1 = grow(core) & ~core
        vol[core], vol[ring1], vol[grow(core | ring1) & ~core & ~ring1] = (-20000, 4), (9000, 4), (24000, 4)
        trk.upload_tsdf(vol)
        before = state_of(trk, False)
        rec, _ = trk.label_components()
        trk.download_components()
        st = trk.prune_components()
        print(f"mid-scan: {st}")
        assert st["n_pruned"] >= 1 and (rec["n_voxels"] == 27).any()
        for a, b in zip(before, state_of(trk, False)):
            assert same_bits(a, b)
        assert not KT.inside(trk.download_tsdf())[core].any()
        for k in range(4, 8):
            pose, ok = trk.process_frame(synth_frames(k)[1])
            assert ok, f"frame {k} lost tracking after the prune"
    finally:
        trk.close()


def test_errors_leave_everything_untouched(hsk, mv):
    lib, L = hsk._lib.load(), hsk._lib
    vol = injected_volume()[0]
    trk = ctx(hsk, AT.DST_DIMS)
    try:
        trk.upload_tsdf(vol)
        rec, _ = trk.label_components()
        lab = trk.download_components()
        n = C.c_size_t(0)
        few = np.full(3, 7, KT.COMPONENT_DTYPE)
        st = L.HskComponentStats()
        assert lib.hsk_label_components(trk.h, few.ctypes.data_as(C.POINTER(L.HskComponent)), 3, C.byref(n), C.byref(st)) == -1     # cap below the count
        assert n.value == len(rec) and st.n_components == len(rec) and (few == np.full(1, 7, KT.COMPONENT_DTYPE)[0]).all() and b"cap" in lib.hsk_last_error(trk.h)
        assert lib.hsk_label_components(trk.h, None, 0, None, None) == -1
        assert lib.hsk_download_components(trk.h, None) == -1
        for bad in (dict(keep_largest=-1), dict(keep_largest=4097), dict(fill=2), dict(fill=-1)):
            ps = L.HskPruneStats(n_pruned=77)
            p = hsk.default_prune_params(trk, **bad)
            assert lib.hsk_prune_components(trk.h, C.byref(p), C.byref(ps)) == -1 and ps.n_pruned == 77 and lib.hsk_last_error(trk.h), bad
        with pytest.raises(hsk.KinfuError, match="keep_largest"):
            trk.prune_components(keep_largest=5000)
        assert trk.label_components()[1]["labels_reused"] == 1 and np.array_equal(trk.download_components(), lab) and np.array_equal(trk.download_tsdf(), vol)
        assert trk.prune_components(keep_largest=4096, min_voxels=0)["n_pruned"] == 0
    finally:
        trk.close()
    # between submit and wait
    trk = hsk.KinfuTracker(n=64)
    try:
        trk.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        trk.submit_frame(hsk.synth_depth(hsk.synth_pose(1)))
        n, lab, ps = C.c_size_t(77), np.full(64 ** 3, 9, np.uint32), L.HskPruneStats(n_pruned=77)
        assert lib.hsk_label_components(trk.h, None, 0, C.byref(n), None) == -3 and n.value == 77 and b"in flight" in lib.hsk_last_error(trk.h)
        assert lib.hsk_download_components(trk.h, lab.ctypes.data) == -3 and (lab == 9).all()
        assert lib.hsk_prune_components(trk.h, None, C.byref(ps)) == -3 and ps.n_pruned == 77
        _, ok = trk.wait_frame()
        assert ok and trk.label_components()[1]["n_components"] >= 1
    finally:
        trk.close()
    # a context that stores part of its volume, and the slabs of a group
    part = hsk.KinfuTracker(n=64, own_z0=0, own_z1=32)
    try:
        for call in (lambda t: t.label_components(), lambda t: t.download_components(), lambda t: t.prune_components()):
            with pytest.raises(hsk.KinfuError, match="slab"):
                call(part)
        n = C.c_size_t(77)
        assert lib.hsk_label_components(part.h, None, 0, C.byref(n), None) == -3 and n.value == 77
    finally:
        part.close()
    g = hsk.KinfuGroup(n=64, device_ids=(0, 0))
    try:
        g.process_frame(hsk.synth_depth(hsk.synth_pose(0)))
        for i in range(g.n_slabs()):
            for call in (lambda t: t.label_components(), lambda t: t.download_components(), lambda t: t.prune_components()):
                with pytest.raises(hsk.KinfuError, match="slab"):
                    call(g.slab(i))
        _, ok = g.process_frame(hsk.synth_depth(hsk.synth_pose(1)))
        assert ok
    finally:
        g.close()


def test_a_million_components(hsk):
    """a 128^3 checkerboard: every second voxel INSIDE, no two of them adjacent -- 2^20 components of one voxel, the records in
    the order of their roots; the tables of roots and records at a size no other test reaches"""
    n = 128
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    on = ((x + y + z) & 1) == 0
    vol = np.zeros((n, n, n, 2), np.int16)
    vol[on] = (-9, 2)
    trk = hsk.KinfuTracker(n=n)
    try:
        trk.upload_tsdf(vol)
        rec, st = trk.label_components()
        assert st == {"n_components": n ** 3 // 2, "n_inside": n ** 3 // 2, "largest": 1, "labels_reused": 0}
        lin = np.arange(n ** 3, dtype=np.uint32).reshape(n, n, n)
        assert np.array_equal(trk.download_components(), np.where(on, lin, np.uint32(KT.NONE)))
        assert (rec["n_voxels"] == 1).all() and np.array_equal(rec["root"], np.stack([x[on], y[on], z[on]], -1))
        assert np.array_equal(rec["lo"], rec["root"]) and np.array_equal(rec["hi"], rec["root"] + 1)
        got = trk.prune_components(min_voxels=0, keep_largest=3)
        assert got == {"n_components": n ** 3 // 2, "n_pruned": n ** 3 // 2 - 3, "n_pruned_voxels": n ** 3 // 2 - 3, "n_kept_voxels": 3}
        after = trk.download_tsdf()
        assert int(KT.inside(after).sum()) == 3 and KT.inside(after)[0, 0, 0] and KT.inside(after)[0, 0, 2] and KT.inside(after)[0, 0, 4]
    finally:
        trk.close()
