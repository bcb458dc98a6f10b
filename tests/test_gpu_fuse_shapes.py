"""hsk_fuse_volume on the GPU at the shapes and cell ratios tests/test_gpu_fuse.py does not reach, BIT FOR BIT against the numpy
restatement of the rule (tests/fuse_twin.py): the TSDF pairs, the colour volume, n_fused, n_colored and the footprint box.  The
cases are tests/fuse_cases.py's, each shown by tests/test_fuse_shapes_host.py to reach the path of fuse.hip it is there for:
A  a ragged source (an odd count of plane groups, X across a 64-voxel row) into a ragged destination with three different cells,
   with colour, twice; the destination a whole context afterwards; the source untouched
B  a destination three times coarser than the source: the brick lookup's second to sixth trip, its last lane
C  a footprint of more chunks than the sweep has waves: the persistent stride's second round
D  lone observed cells across brick boundaries and next to the outer shell, under three seeded matrices: what a wrong skip loses
E  the levelled volume's fuse, as hsk_level_config sets it up
F  a tracked source whose free-space weights are still deferred"""
import numpy as np
import pytest

import fuse_twin as FT
import view_twin as VT
from fuse_cases import (DEFER_FRAMES, DEFER_N, SHAPE_NAMES, SWEEP_WAVES, assert_fused, assert_nontrivial, case_of, chunk_index, deferred_case,
                        empty_like_ctx, footprint_of, source_of, twin_of)
from kit import same_bits_nan, volume_ctx

pytestmark = pytest.mark.gpu
f32 = np.float32


def ctx_pair(hsk, c, src_arrays=None):
    """(source context, holding the arrays given; empty destination context) of a case, at the case's one truncation distance"""
    src = volume_ctx(hsk, c.sdims, c.ssize, color=c.colour, trunc_dist_m=c.trunc)
    try:
        if src_arrays is not None:
            src.upload_tsdf(src_arrays[0])
            if c.colour:
                src.upload_color(src_arrays[1])
        return src, volume_ctx(hsk, c.ddims, c.dsize, color=c.colour, trunc_dist_m=c.trunc)
    except Exception:
        src.close()
        raise


# ---- B .. E: one fuse into an empty destination -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SHAPE_NAMES if not n.startswith("A ")])
def test_fuse_matches_the_twin(hsk, name):
    c = case_of(name)
    ref_t, ref_c, ref_s = twin_of(name)
    assert ref_s["n_fused"] > 0
    box = footprint_of(name)
    if name == "C slab":
        # the chunks of the stride's second round hold voxels that take a sample, so a wave that stopped after its first is seen
        z, y, x = np.nonzero(ref_s["fused"])
        later = int((chunk_index(box, x, y, z) >= SWEEP_WAVES).sum())
        assert later >= 10000, f"only {later} fused voxels in chunks {SWEEP_WAVES} and up"
    src, dst = ctx_pair(hsk, c, source_of(name))
    try:
        st = dst.fuse_from(src, c.m)
        print(f"{name}: {st}")
        assert_fused(dst, st, ref_t, ref_c, ref_s, box, name)
        if name == "C slab":
            # (4 x 2048 is launch_fuse_sweep's grid cap, fuse.hip: a change of the cap fails here, not the point of the test)
            assert st["chunks_total"] > SWEEP_WAVES == 4 * 2048
        if name.startswith("D lone") or name.startswith("B b") or name.startswith("B l"):
            assert 0 < st["chunks_swept"] < st["chunks_total"], f"{name}: the skip test does not bite: {st}"
    finally:
        src.close()
        dst.close()


# ---- A: ragged on both sides, with colour, twice; the destination a whole context; the source untouched --------------------------------
def test_ragged_volumes_twice_and_the_fused_context_equals_a_fresh_one(hsk):
    first, again = case_of("A ragged both"), case_of("A again")
    s_tsdf, s_col = source_of("A ragged both")
    src, dst = ctx_pair(hsk, first, (s_tsdf, s_col))
    fresh = volume_ctx(hsk, first.ddims, first.dsize, color=True, trunc_dist_m=first.trunc)
    try:
        for name, c in (("A ragged both", first), ("A again", again)):
            ref_t, ref_c, ref_s = twin_of(name)
            assert_nontrivial(ref_t, ref_s, s_tsdf, name)
            st = dst.fuse_from(src, c.m)
            print(f"{name}: {st}")
            assert_fused(dst, st, ref_t, ref_c, ref_s, footprint_of(name), name)
        # the source is untouched
        assert np.array_equal(src.download_tsdf(), s_tsdf) and np.array_equal(src.download_color(), s_col)
        # the destination is a whole context: test_gpu_fuse.py's test 4 at the ragged shape
        tsdf, col = dst.download_tsdf(), dst.download_color()
        fresh.upload_tsdf(tsdf)
        fresh.upload_color(col)
        for a, b in zip(dst.extract_cloud_attrs(), fresh.extract_cloud_attrs()):
            assert same_bits_nan(np.asarray(a), np.asarray(b)), "cloud"
        assert dst.extract_cloud(cap=0)[1] > 1000
        mesh = dst.extract_mesh_indexed()
        for a, b in zip(mesh, fresh.extract_mesh_indexed()):
            assert same_bits_nan(np.asarray(a), np.asarray(b)), "indexed mesh"
        assert len(mesh[0]) > 1000
        pose = hsk.synth_pose(0)                 # in front of the volume's z = 0 face, looking in
        va = dst.render_view(pose=pose, mode=VT.COLOR_LIT, vmap=True, nmap=True)
        vb = fresh.render_view(pose=pose, mode=VT.COLOR_LIT, vmap=True, nmap=True)
        print(f"view: {va['n_hit']} hits")
        assert va["n_hit"] > 1000
        for key in va:
            assert same_bits_nan(np.asarray(va[key]), np.asarray(vb[key])), f"view: {key}"
        depth = hsk.synth_depth(pose)
        dst.integrate(depth, pose)
        fresh.integrate(depth, pose)
        assert dst.integrate_coarse_counts() == fresh.integrate_coarse_counts()
        ta, tb = dst.download_tsdf(), fresh.download_tsdf()
        assert np.array_equal(ta, tb) and not np.array_equal(ta, tsdf)
    finally:
        src.close()
        dst.close()
        fresh.close()


# ---- F: a source with deferred free-space weights ---------------------------------------------------------------------------------------
def test_a_source_with_deferred_weights(hsk, synth_frames):
    """two identical 64^3 trackers take four frames of the scripted stream; one is downloaded for the twin (which writes its
    deferred weights back), the other is the source as the tracker left it: the fuse writes them back itself, and what the source
    holds afterwards is what the first one held"""
    c = deferred_case()

    def tracked():
        trk = hsk.KinfuTracker(n=DEFER_N, trunc_dist_m=c.trunc)
        for k in range(DEFER_FRAMES):
            trk.process_frame(synth_frames(k)[1])
        return trk

    a, b = tracked(), tracked()
    dst = volume_ctx(hsk, c.ddims, c.dsize, trunc_dist_m=c.trunc)
    try:
        vol = a.download_tsdf()
        assert (vol[..., 1] > 1).any() and (vol[..., 0] < 0).any()
        ref_t, _, ref_s = FT.fuse(empty_like_ctx(c.ddims, False)[0], c.dsize, vol, c.ssize, c.m)
        assert_nontrivial(ref_t, ref_s, vol, "F deferred")
        st = dst.fuse_from(b, c.m)
        print(f"F deferred: {st}")
        assert_fused(dst, st, ref_t, None, ref_s, FT.footprint(c.sdims, c.ssize, c.ddims, c.dsize, c.m), "F deferred")
        assert np.array_equal(b.download_tsdf(), vol)
    finally:
        a.close()
        b.close()
        dst.close()
