"""The simplified mesh's shape cases (tests/simplify_cases.py) without a GPU: the conditions that make them worth running.  The
bookkeeping around the shared arithmetic -- who owns which cluster, where a cluster's output number comes from, where a cube
row's faces start -- exists only in the kernels (housescan_amd/csrc/simplify.hip), on 64-wide segments and 1024-row scan blocks.
Here the twin's result on every case is counted (simplify_cases.census) and the counts asserted: an input that stays inside the
first segment, the first scan block or whole cells fails HERE, so that tests/test_gpu_simplify_shapes.py cannot pass on an input
that misses the code it is there for.  The thresholds are conditions, not measurements; the counts are printed."""
import numpy as np
import pytest

import simplify_cases as SC
import simplify_twin as ST
from kit import same_bits
from mesh_twin import mesh_indexed
from simplify_cases import CLUSTERS, MODES


def census_of(oracle, name, c):
    """the census of a case at one cluster size; the clusters and the faces are the same in both modes (the mode moves vertices)"""
    q, m = (SC.twin_of(oracle, name, c, mode) for mode in MODES)
    assert np.array_equal(q["clusters"], m["clusters"]) and np.array_equal(q["faces"], m["faces"])
    cs = SC.census(SC.shape_cases()[name][0], SC.mesh_of(oracle, name), q, c)
    print(f"{name} c {c}: {cs} {q['stats']}")
    return cs, q["stats"]


@pytest.mark.parametrize("c", CLUSTERS)
def test_the_hall_leaves_the_first_segment(oracle, c):
    """1032 x 24 x 21 at every cluster size: more than one 64-cluster segment to a cluster row, a row with a segment of 64
    referenced clusters (rank 63), referenced clusters on either side of a segment edge and a surviving face across one, some in
    the last, partial segment, some in the top cell layer, which the volume's last plane cuts (21 is a multiple of no cell); at c = 2
    and 4 rows with an empty segment between two that are not (the carry runs over it).  At c = 2 the cube rows' trips of
    k_simp_faces.  THE RULE: a face belongs to the cube that its three corners' edges share (simplify_cases.face_cubes), its trip
    is that cube's x >> 6, its cube row the cube's (y, z); a face survives when its corners' clusters (lower corner >> s) are
    three; a cube row counts when its surviving faces lie in three or more distinct trips and a trip between two of them holds
    none -- and, the stronger form asserted with it, no vertex of the indexed mesh has its edge's lower corner on one of the
    cube row's four grid rows within that trip, which is what the kernel's `any == 0` test skips a trip for: the write pass's
    `base` is carried over it"""
    cs, st = census_of(oracle, "hall", c)
    assert cs["cseg"] >= 2 and cs["cx"] > 64
    assert cs["rows_full"] >= 1
    assert cs["at_63"] >= 1 and cs["at_64"] >= 1
    assert cs["in_last"] >= 1 and cs["cx"] % 64 != 0
    assert cs["top_layer"] >= 1 and cs["top_partial"]
    assert cs["faces_across"] >= 1
    if c in (2, 4):
        assert cs["rows_gap"] >= 5
    if c == 2:
        assert cs["trip_rows"] >= 1 and cs["trip_rows_skipped"] >= 1
    # (the rule's own branches: every rank but 0, uncoloured clusters at the small cells)
    assert all(st["n_rank"][r] > 0 for r in (1, 2, 3))
    assert st["n_uncolored"] > 0 or c == 16


def test_the_flipped_hall_has_other_counts(oracle):
    """one voxel's sign flipped in front of the first wall: the totals that a count cache would keep are no longer right"""
    a, b = (SC.twin_of(oracle, name, 2, ST.QUADRIC) for name in ("hall", "hall flipped"))
    assert len(b["vertices"]) != len(a["vertices"]) and len(b["faces"]) != len(a["faces"])
    cs, _ = census_of(oracle, "hall flipped", 2)
    assert cs["cseg"] >= 2 and cs["at_63"] >= 1 and cs["at_64"] >= 1 and cs["faces_across"] >= 1


@pytest.mark.parametrize("c", CLUSTERS)
def test_the_tall_room_leaves_the_first_scan_block(oracle, c):
    """24 x 72 x 61: at c = 2 more than 1024 cluster rows with output clusters on both sides of row 1024 (launch_scan_rows' second
    block on cl_cnt / tc_cnt); at every c a top cell layer that the last plane cuts (61 is odd), with output clusters in it"""
    cs, _ = census_of(oracle, "tall", c)
    assert cs["top_layer"] >= 1 and cs["top_partial"]
    if c == 2:
        assert cs["crows"] > 1024 and cs["rows_below"] >= 1 and cs["rows_1024"] >= 1


def test_the_scanned_wide_volume_leaves_the_first_segment(oracle, synth_frames):
    """the oracle's integrate of the GPU test's frames at the same poses: more than 2000 input faces; at c = 2 and c = 4 more than
    one segment to a cluster row and referenced clusters in at least two of them"""
    vol = SC.wide_oracle_volume(oracle, synth_frames)
    mesh = mesh_indexed(vol, *oracle.mc_table(), size=SC.WIDE_SIZE, normals=False)
    assert len(mesh["faces"]) > 2000
    for c in (2, 4):
        tw = ST.simplify(vol, *oracle.mc_table(), c=c, size=SC.WIDE_SIZE, mesh=mesh)
        cs = SC.census(vol, mesh, tw, c)
        print(f"scanned wide {SC.WIDE_DIMS}, {SC.WIDE_FRAMES} frames, c {c}: {cs} {tw['stats']}")
        assert cs["cseg"] >= 2 and len(cs["segments_used"]) >= 2


def test_the_census_can_fail(oracle):
    """the counts are not satisfied by anything: the box of tests/test_simplify_host.py, 72 x 40 x 24, meets none of the hall's"""
    from simplify_cases import mesh_of, small_cases, twin_of
    cs = SC.census(small_cases()["box"][0], mesh_of(oracle, "box"), twin_of(oracle, "box", 2, ST.QUADRIC), 2)
    assert cs["cseg"] == 1 and cs["rows_full"] == cs["rows_gap"] == cs["at_63"] == cs["at_64"] == cs["faces_across"] == 0
    assert cs["rows_1024"] == 0 and not cs["top_partial"] and cs["trip_rows"] == 0
    # (and the cube of a face is the cube: every face of the box lies in a cube that marching cubes emits there)
    vol = small_cases()["box"][0]
    cube = SC.face_cubes(mesh_of(oracle, "box")["edges"], mesh_of(oracle, "box")["faces"])
    t = vol[..., 0] < 0
    x, y, z = cube[:, 0], cube[:, 1], cube[:, 2]
    corners = np.stack([t[z + dz, y + dy, x + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], axis=1)
    assert (corners.any(axis=1) & ~corners.all(axis=1)).all()
    assert not same_bits(SC.twin_of(oracle, "hall", 2, ST.QUADRIC)["vertices"], SC.twin_of(oracle, "hall", 2, ST.MEAN)["vertices"])
