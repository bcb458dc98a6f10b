"""The fusion shape cases without a GPU (tests/fuse_cases.py): every case is shown, on the numpy twin (tests/fuse_twin.py) and on
the binary64 restatement of a chunk's reach (fuse_cases.chunk_bricks) alone, to reach the path of fuse.hip it is there for -- so
that tests/test_gpu_fuse_shapes.py cannot pass on an input that misses it -- and hsk_fuse_footprint equals the twin's footprint
for each of them.  The slab's twin result is not made here (its footprint and chunk count need no sweep)."""
import numpy as np
import pytest

import fuse_twin as FT
from fuse_cases import (LONE_CORNERS, LONE_DST, PREVIOUS, RAG_DST, RAG_SRC, SHAPE_NAMES, SWEEP_WAVES, assert_nontrivial, before_of, case_of, chunk_grid,
                        chunk_index, crafted, crafted_colour, deferred_case, footprint_of, lone_cell_counts, lone_cells, reach_of, source_of, twin_of)

SWEPT_ON_THE_HOST = [n for n in SHAPE_NAMES if n != "C slab"]


def chunks_with_fused(name):
    """the sweep's chunk numbers that hold a voxel the twin fused"""
    z, y, x = np.nonzero(twin_of(name)[2]["fused"])
    return np.unique(chunk_index(footprint_of(name), x, y, z)).tolist()


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
def test_crafted_volumes_are_what_they_say():
    vol, col = crafted((72, 40, 50), 21), crafted_colour((72, 40, 50), 22)
    assert vol.shape == (50, 40, 72, 2) and vol.dtype == np.int16 and col.shape == (50, 40, 72, 4) and col.dtype == np.uint8
    assert vol[..., 0].min() == -32767 and vol[..., 0].max() == 32767
    w = vol[..., 1]
    assert set(np.unique(w).tolist()) == {0, 1, 2, 3, 4, 5} and 0.02 < (w == 0).mean() < 0.04
    assert (vol[..., 0][w == 0] != 0).any()                        # (a hole keeps its raw value: a rule that read it would show)
    assert 0.08 < (col[..., 3] == 0).mean() < 0.12 and col[..., 3].max() <= 40
    assert np.array_equal(vol, crafted((72, 40, 50), 21)) and not np.array_equal(vol, crafted((72, 40, 50), 20))
    lone = lone_cells((72, 40, 50), LONE_CORNERS, 26)
    assert int((lone[..., 1] > 0).sum()) == 8 * len(LONE_CORNERS)
    for x, y, z in LONE_CORNERS:
        assert (lone[z:z + 2, y:y + 2, x:x + 2, 1] > 0).all()


def test_the_lone_cells_are_where_the_skip_test_has_its_edges():
    """the first and the last interior cell; cells across a brick boundary (voxels 8k - 1 | 8k) on one, two and three axes, two of
    each at least; cells inside one brick; every cube at least four voxels from the next"""
    dims = RAG_SRC[0]
    assert LONE_CORNERS[0] == (1, 1, 1) and LONE_CORNERS[1] == tuple(d - 3 for d in dims)
    across = [sum(v % 8 == 7 for v in c) for c in LONE_CORNERS]
    for k in (0, 1, 2, 3):
        assert across.count(k) >= 2, (k, across)
    for i, a in enumerate(LONE_CORNERS):
        for b in LONE_CORNERS[i + 1:]:
            assert max(abs(a[k] - b[k]) for k in range(3)) >= 2 + 4, (a, b)


# ---- the footprint of every case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPE_NAMES + ("F deferred",))
def test_footprint_matches_the_twin(hsk, name):
    from housescan_amd import products
    c = deferred_case() if name == "F deferred" else case_of(name)
    box = FT.footprint(c.sdims, c.ssize, c.ddims, c.dsize, c.m)
    assert products.fuse_footprint(c.sdims, c.ssize, c.ddims, c.dsize, c.m) == box, name
    assert box != (0,) * 6
    largest = float(max(max(FT.cells(c.sdims, c.ssize)), max(FT.cells(c.ddims, c.dsize))))
    assert float(c.trunc) >= 2.1 * largest * (1 - 1e-6), f"{name}: trunc_dist_m {c.trunc} is below 2.1 x the largest cell: the two contexts' distances would differ"


@pytest.mark.parametrize("name", SWEPT_ON_THE_HOST)
def test_the_footprint_and_the_reach_hold_what_the_twin_fuses(name):
    """the twin sweeps every voxel: what it fuses lies in the footprint, and in chunks whose reach holds an observed brick"""
    st = twin_of(name)[2]
    assert st["n_fused"] > 0 and FT.box_contains(footprint_of(name), st["box"])
    reach = reach_of(name)
    c0, cn = chunk_grid(footprint_of(name))
    assert len(reach) == cn[0] * cn[1] * cn[2]
    for k in chunks_with_fused(name):
        assert reach[k].nb > 0 and reach[k].observed, (name, k, reach[k])
    if name in PREVIOUS:
        assert np.array_equal(before_of(name)[0], twin_of(PREVIOUS[name])[0])


# ---- A: ragged on both sides ----------------------------------------------------------------------------------------------------------
def test_case_a_is_ragged_and_its_fused_voxels_reach_every_ragged_edge():
    (sx, sy, sz), (dx, dy, dz) = RAG_SRC[0], RAG_DST[0]
    # k_fuse_bricks: an odd number of plane groups (the last brick layer has one), a wave across two brick rows, a last block partly
    # past n_threads
    groups = (sz + 3) // 4
    assert groups % 2 == 1 and sx % 64 != 0 and (sx * (sy // 8) * ((sz + 7) // 8)) % 256 != 0
    # k_fuse_sweep: lanes that leave in x and in y, a chunk that ends inside a plane group
    assert dx % 16 != 0 and dy % 16 != 0 and dz % 16 != 0 and dz % 4 != 0
    cs, cd = FT.cells(*RAG_SRC), FT.cells(*RAG_DST)
    assert len({float(v) for v in cd}) == 3 and cd[0] != cs[0] and cd[2] != cs[2]      # (2.7 / 72 is the source's 1.5 / 40 too)
    first, again = twin_of("A ragged both"), twin_of("A again")
    src = source_of("A ragged both")
    for name, ref in (("A ragged both", first), ("A again", again)):
        st = ref[2]
        assert_nontrivial(ref[0], st, src[0], name)
        assert 0 < st["n_colored"] < st["n_fused"], name
        print(f"{name}: fused {st['n_fused']} of {st['fused'].size}, coloured {st['n_colored']}, box {st['box']}, chunks {len(reach_of(name))}, "
              f"most bricks {max(r.nb for r in reach_of(name))}")
        f = st["fused"]
        assert f[dz - 1].sum() >= 100, name                           # the last plane: the first of its group
        assert f[:, :, dx - 4:].sum() >= 100, name                    # the last 16-byte row of the last, half-filled chunk column
        b = st["box"]                                                   # Ws == 0 leaves voxels alone inside the swept region
        assert st["n_fused"] < 0.9 * (b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4])
    assert again[2]["fused"][:, 64:].sum() >= 1000                   # the half-filled last chunk row in y: the second placement's
    before = before_of("A again")
    f = again[2]["fused"]
    assert (f & (before[0][..., 1] > 0)).sum() >= 1000, "few merges onto a weight"
    s_col_w = again[1][..., 3].astype(int) - before[1][..., 3]
    assert ((s_col_w > 0) & (before[1][..., 3] > 0)).sum() >= 1000 and ((s_col_w > 0) & (before[1][..., 3] == 0)).sum() >= 1000
    assert again[1][..., 3].max() == 64                                # the colour weight saturates somewhere


# ---- B: a destination coarser than the source ---------------------------------------------------------------------------------------
def test_case_b_needs_the_lookups_later_trips():
    for name in ("B brick 285", "B last lane"):
        st = twin_of(name)[2]
        held = chunks_with_fused(name)
        assert held == [0], (name, held)
        r = reach_of(name)[0]
        assert r.lo == (0, 0, 0) and r.n == (7, 7, 7) and r.nb == 343 and (r.nb + 63) // 64 == 6
        assert r.observed and min(r.observed) >= 64, (name, r)      # nothing for the first trip to see
        print(f"{name}: fused {st['n_fused']}, box {st['box']}, chunk 0 reaches {r.nb} bricks, observed {r.observed}")
    assert twin_of("B brick 285")[2]["n_fused"] == 8 and reach_of("B brick 285")[0].observed == [285]
    last = twin_of("B last lane")[2]
    assert last["n_fused"] == 1 and last["box"] == (15, 16, 15, 16, 15, 16)
    r = reach_of("B last lane")[0]
    assert r.observed == [r.nb - 1] and r.nb % 64 != 0                # the last lane of the last, partial trip
    ref = twin_of("B dense, turned")
    assert_nontrivial(ref[0], ref[2], source_of("B dense, turned")[0], "B dense, turned", share=0.01)   # (64000 voxels against 2 M)
    assert ref[2]["n_fused"] >= 0.5 * 40 ** 3
    nbs = [r.nb for r in reach_of("B dense, turned")]
    print(f"B dense, turned: fused {ref[2]['n_fused']}, bricks per chunk {min(nbs)} .. {max(nbs)}")
    assert sum(1 for v in nbs if v > 64) >= 20 and max(nbs) > 1024      # (of 27 chunks; the turned volume's corner chunks reach less)


# ---- C: more chunks than waves ----------------------------------------------------------------------------------------------------------
def test_case_c_has_more_chunks_than_the_sweep_has_waves():
    c = case_of("C slab")
    c0, cn = chunk_grid(footprint_of("C slab"))
    print(f"C slab: footprint {footprint_of('C slab')}, chunks {cn}")
    assert c0 == [0, 0, 0] and cn == [91, 91, 1] and cn[0] * cn[1] * cn[2] > SWEEP_WAVES
    assert c.ddims[0] % 16 == 8 and footprint_of("C slab")[1] > c.ddims[0] - 8       # the last chunk column: half filled, and inside the footprint


# ---- D: lone cells ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SHAPE_NAMES if n.startswith("D lone")])
def test_case_d_every_lone_cell_inside_is_fused_and_little_else(name):
    c = case_of(name)
    assert all(abs(float(a) - 2 * float(b)) < 1e-6 for a, b in zip(FT.cells(c.sdims, c.ssize), FT.cells(*LONE_DST)))
    counts = lone_cell_counts(name)
    st = twin_of(name)[2]
    print(f"{name}: fused {st['n_fused']}, per cell (inside, fused) {counts}")
    for corner, (inside, n) in zip(LONE_CORNERS, counts):
        assert n >= 1 or not inside, f"{name}: the cell at {corner} maps inside the destination and no voxel took its sample"
    assert sum(1 for _, n in counts if n >= 1) >= 8
    assert 0 < st["n_fused"] < 200
    reach = reach_of(name)
    seen = sum(1 for r in reach if r.observed)
    print(f"   {len(chunks_with_fused(name))} chunks hold fused voxels, {seen} of {len(reach)} reach an observed brick")
    assert 0 < seen < len(reach)                                        # the skip test has chunks to leave and chunks to keep


# ---- E: the levelled volume ---------------------------------------------------------------------------------------------------------------
def test_case_e_is_the_levelled_volumes_fuse():
    c = case_of("E levelled")
    ref = twin_of("E levelled")
    cs, cd = FT.cells(c.sdims, c.ssize), FT.cells(c.ddims, c.dsize)
    assert len({float(v) for v in cs}) == 3 and sum(float(a) != float(b) for a, b in zip(cs, cd)) >= 2
    assert all(d % 8 == 0 for d in c.ddims[:2])
    assert_nontrivial(ref[0], ref[2], source_of("E levelled")[0], "E levelled")
    assert ref[2]["n_fused"] > 10000
    print(f"E levelled: {c.sdims} -> {c.ddims} over {c.dsize}, trunc {c.trunc}, fused {ref[2]['n_fused']}, most bricks {max(r.nb for r in reach_of('E levelled'))}")
