"""The room partition without a GPU: the numpy twin (tests/partition_twin.py) pinned by hand-computed cases -- the door of the two
rooms at the threshold where one core becomes two, the ties at the corner eight tiles share and on a mirror plane of voxels, the
dropping of small cores and the cap of 1024 --, its G against reach_twin's field seeded at every kept core voxel, its frontier
form against whole-grid Jacobi sweeps; the kernels' shared text (housescan_amd/csrc/hsk_part_point.h) compiled for the host with
the sanitizers, relaxing tile after tile in three visiting orders, against the twin -- zero differences --, and G of its keys against the reach
harness's field on one ragged grid (the two are one relaxation text); hsk_merge_rooms; the
defaults; the C layout of the new structs and their Python mirror; the argument errors that need no device.  The scenes and
constants here are the GPU tests' too."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import clearance_twin as CL
import kit
import partition_twin as PT
import reach_twin as RE
from partition_cases import DOOR_THRESHOLD, MIRROR_DIMS, RAGGED, d2_of, mirror_rooms, ragged_case, serpentine_core_d2, twin_partition
from reach_cases import CORNER_DIMS, SERPENTINE_DIMS, TILE, WEIGHTS, corridors, run_harness as reach_harness, serpentine, tile_corner, two_rooms

f32 = np.float32


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------------


# ---- 1. the door of two rooms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", WEIGHTS)
def test_the_door_of_two_rooms(weight):
    """a wall at x = 40 with a door 16 x 30: at core_d2 = the largest D in the door plane the core runs through the door, one
    above it there are two cores; the door's voxels go to the room of the smaller root and the faces lie on their far side"""
    d2 = d2_of("two rooms", two_rooms(False), weight, 4096)
    thr = DOOR_THRESHOLD[weight]
    assert d2[:, :, 40].max() == thr
    one, n_one = PT.kept_roots(PT.core_labels(d2, thr), 1)
    assert n_one == 1 and len(one) == 1
    labels = PT.core_labels(d2, thr + 1)
    two, n_two = PT.kept_roots(labels, 1)
    assert n_two == 2 and len(two) == 2
    if weight == (1, 1, 1):
        assert [(labels == r).sum() for r in two] == [99534, 96462]
    p = twin_partition("two rooms", d2, weight, thr + 1, min(weight), 1)
    assert p["stats"] == {"n_cores": 2, "n_rooms": 2, "n_dropped": 0, "n_passable": 80 * 64 * 48 - 64 * 48 + 480, "n_assigned": 243168, "n_doors": 1}
    assert p["rooms"]["n_voxels"].tolist() == [123360, 119808] and (p["ids"] == PT.UNASSIGNED).sum() == 0
    door = p["doors"][0]
    assert (door["a"], door["b"], door["n_faces"].tolist(), door["lo"].tolist(), door["hi"].tolist()) == (0, 1, [480, 0, 0], [40, 24, 0], [41, 40, 30])
    assert door["sum2"].tolist() == [480 * 81, 2 * 30 * sum(range(24, 40)), 2 * 16 * sum(range(30))] and door["max_d2"] == thr
    assert p["rooms"]["root"].tolist() == [[0, 0, 0], [41 + 8, 0, 0]] or weight != (1, 1, 1)
    assert (p["ids"][:30, 24:40, 40] == 0).all() and (p["ids"][:, :, :40] == 0).all() and (p["ids"][:, :, 41:] == 1).all()
    assert p["rooms"]["n_core_voxels"].tolist() == [(labels == r).sum() for r in two]


def test_two_sealed_rooms_have_no_door():
    for weight in WEIGHTS:
        d2 = d2_of("two sealed rooms", two_rooms(True), weight, 4096)
        p = twin_partition("two sealed rooms", d2, weight, DOOR_THRESHOLD[weight] + 1, min(weight), 1)
        assert (p["stats"]["n_rooms"], p["stats"]["n_doors"], len(p["doors"])) == (2, 0, 0)
        assert p["rooms"]["n_voxels"].tolist() == [40 * 64 * 48, 39 * 64 * 48] and (p["ids"][:, :, 40] == PT.BLOCKED).all()


# ---- 2. ties ------------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_root():
    d2 = d2_of("tile corner", tile_corner(), (1, 1, 1))
    p = twin_partition("tile corner", d2, (1, 1, 1), 4, 1, 1)
    assert p["rooms"]["n_voxels"].tolist() == [1473, 1473] and p["doors"]["n_faces"].tolist() == [[2, 2, 2]] and p["stats"]["n_doors"] == 1
    tx, ty, tz = TILE
    # the cube on the corner: a voxel of it is a face move from the cube's voxel in one chamber's tile and an edge move from the
    # other's, so the cube splits four and four; the scene is its own reflection through the corner, and no voxel ties with its image
    cube = p["ids"][tz - 1:tz + 1, ty - 1:ty + 1, tx - 1:tx + 1]
    assert cube.tolist() == [[[0, 0], [0, 1]], [[0, 1], [1, 1]]]
    image, held = p["ids"][::-1, ::-1, ::-1], p["ids"] < PT.NONE
    assert np.array_equal(held, image < PT.NONE) and np.array_equal(p["ids"][held], 1 - image[held])
    assert p["rooms"]["root"][0].tolist() < p["rooms"]["root"][1].tolist() and p["rooms"]["n_core_voxels"][0] == p["rooms"]["n_core_voxels"][1]
    for weight in WEIGHTS:
        vol = mirror_rooms()
        d2 = d2_of("mirror rooms", vol, weight)
        q = twin_partition("mirror rooms", d2, weight, 9 * min(weight), min(weight), 1)
        X = MIRROR_DIMS[0]
        plane = q["ids"][:, :, X // 2]
        assert q["stats"]["n_rooms"] == 2 and (plane < PT.NONE).sum() == 16 and (plane[plane < PT.NONE] == 0).all()
        assert np.array_equal(q["cost"], q["cost"][:, :, ::-1]) and q["rooms"]["n_voxels"][0] - q["rooms"]["n_voxels"][1] == 16
        left, right = q["ids"][:, :, :X // 2], q["ids"][:, :, X // 2 + 1:][:, :, ::-1]
        assert np.array_equal(left < PT.NONE, right < PT.NONE) and (left[left < PT.NONE] == 0).all() and (right[right < PT.NONE] == 1).all()
        assert q["doors"]["n_faces"].tolist() == [[16, 0, 0]] and q["doors"]["lo"].tolist() == [[X // 2, 6, 4]] and q["doors"]["hi"].tolist() == [[X // 2 + 1, 10, 8]]


# ---- 3. G is the reach field; the frontier form is the Jacobi form ---------------------------------------------------------------------------
def test_g_is_the_reach_field_seeded_at_every_kept_core_voxel():
    cases = [("tile corner", d2_of("tile corner", tile_corner(), (1, 1, 1)), (1, 1, 1), 4, 1, 1)]
    vol, d2, par = ragged_case(RAGGED[0], (16, 25, 44), 8)
    cases.append((f"speckled {RAGGED[0]}", d2, (16, 25, 44), par["core_d2"], par["min_d2"], 8))
    for name, d2, weight, core_d2, min_d2, min_core in cases:
        p = twin_partition(name, d2, weight, core_d2, min_d2, min_core)
        seeds = [(int(x), int(y), int(z)) for z, y, x in np.argwhere(p["cost"] == 0)]
        ref, used = RE.field(d2, weight, min_d2, RE.MAX_COST, seeds)
        assert used == len(seeds) == p["rooms"]["n_core_voxels"].sum() and np.array_equal(p["cost"], ref)
        assert ((p["ids"] == PT.BLOCKED) == (ref == RE.BLOCKED)).all() and ((p["ids"] == PT.UNASSIGNED) == (ref == RE.UNREACHED)).all()


def small_cases():
    rng = np.random.default_rng(15)
    for trial in range(6):
        dims = tuple(int(v) for v in rng.integers(2, 12, 3))
        d2 = rng.choice(np.array([0, 1, 3, 50, CL.FAR], np.uint32), dims[::-1], p=[0.2, 0.1, 0.1, 0.3, 0.3])
        yield dims, d2


def test_the_frontier_relaxation_equals_whole_grid_sweeps():
    n = 0
    for dims, d2 in small_cases():
        for weight in WEIGHTS:
            for core_d2, min_d2, min_core, max_cost in ((50, 1, 1, RE.MAX_COST), (50, 3, 2, RE.MAX_COST), (3, 3, 1, RE.MAX_COST), (50, 1, 1, 3 * RE.costs(weight)[14]),
                                                        (50, 1, 1, 0)):
                key, roots, n_cores = PT.field(d2, weight, core_d2, min_d2, min_core, max_cost)
                assert key.dtype == np.uint64 and np.array_equal(key, PT.field_jacobi(d2, weight, core_d2, min_d2, min_core, max_cost)), (dims, weight, core_d2)
                assert ((key == PT.KEY_BLOCKED) == (d2 < min_d2)).all() and n_cores >= len(roots)
                n += 1
    assert n == 60


# ---- 4. dropping and the cap; the scenes are what the tests say ----------------------------------------------------------------------------
def test_the_scenes_are_what_the_tests_say():
    want = {(RAGGED[0], (1, 1, 1)): (97, 500, 214), (RAGGED[0], (16, 25, 44)): (16, 586, 17), (RAGGED[1], (1, 1, 1)): (169, 752, 468),
            (RAGGED[1], (16, 25, 44)): (18, 843, 17)}
    for (dims, weight), (kept, cores, n_doors) in want.items():
        vol, d2, par = ragged_case(dims, weight, 8)
        p = twin_partition(f"speckled {dims}", d2, weight, **par)
        st = p["stats"]
        assert (st["n_rooms"], st["n_cores"], st["n_dropped"], st["n_doors"]) == (kept, cores, cores - kept, n_doors), (dims, weight, st)
        assert st["n_passable"] > st["n_assigned"] >= 100000 and np.all(np.diff(p["rooms"]["n_voxels"].astype(np.int64)) <= 0)
        assert p["rooms"]["n_core_voxels"].min() >= 8 and p["rooms"]["n_voxels"].sum() == st["n_assigned"]
    vol, d2, par = ragged_case(RAGGED[1], (16, 25, 44), 1)
    with pytest.raises(PT.TooManyRooms) as e:
        PT.field(d2, (16, 25, 44), 9 * 16, 16, 1, RE.MAX_COST)
    assert e.value.args == (1121, 1121)
    # the serpentine: only the end chambers hold a core, and the corridor between them is passable
    vol, walls = serpentine()
    for weight in WEIGHTS:
        d2 = d2_of("serpentine", vol, weight, 256)
        p = twin_partition("serpentine", d2, weight, serpentine_core_d2(weight), min(weight), 1)
        X = SERPENTINE_DIMS[0]
        assert p["stats"]["n_rooms"] == p["stats"]["n_cores"] == 2 and p["stats"]["n_doors"] == 1 and (p["ids"] == PT.UNASSIGNED).sum() == 0
        cores = p["cost"] == 0
        assert cores[:, :, :walls[0]].any() and cores[:, :, walls[-1] + 1:].any() and not cores[:, :, walls[0]:walls[-1] + 1].any()
        assert walls[1] < p["doors"]["lo"][0][0] and p["doors"]["hi"][0][0] <= walls[-2] + 1, "the rooms meet mid-way"
    # the corridors: with core_d2 = min_d2 every free voxel is a core voxel
    vol, _ = corridors()
    d2 = d2_of("corridors", vol, (1, 1, 1))
    p = twin_partition("corridors", d2, (1, 1, 1), 1, 1, 1)
    tx = TILE[0]
    assert p["stats"]["n_rooms"] == 2 and p["rooms"]["n_voxels"].tolist() == [2 * tx, 2 * tx - 2] and (p["cost"][p["ids"] < PT.NONE] == 0).all()
    assert p["stats"]["n_doors"] == 0


# ---- 5. the kernels' shared text on the host -------------------------------------------------------------------------------------------------
def run_harness(exe, tmp_path, d2, weight, core_d2, min_d2, min_core, max_cost, order, radius=0, points=()):
    Z, Y, X = d2.shape
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for part in (np.array([X, Y, Z], np.int32), np.array(list(weight) + [core_d2, min_d2, min_core, max_cost, order, radius, len(points)], np.uint32),
                     np.array([x + X * (y + Y * z) for x, y, z in points], np.uint32), np.ascontiguousarray(d2, np.uint32)):
            f.write(np.ascontiguousarray(part).tobytes())
    kit.run_harness(exe, src, dst)
    raw = open(dst, "rb").read()
    counts = dict(zip(("n_cores", "n_kept", "n_passable", "n_rounds", "n_tiles", "n_first"), (int(v) for v in np.frombuffer(raw, np.uint64, 6))))
    if counts["n_kept"] > PT.MAX_ROOMS:
        assert len(raw) == 48
        return None, None, counts, None
    n = X * Y * Z
    key = np.frombuffer(raw, np.uint64, n, 48).reshape(Z, Y, X)
    roots = np.frombuffer(raw, np.uint32, counts["n_kept"], 48 + 8 * n)
    at = 48 + 8 * n + 4 * counts["n_kept"]
    found = np.frombuffer(raw[at:], np.uint64, len(points))
    assert at + 8 * len(points) == len(raw)
    return key, roots, counts, found


def host_cases():
    """name -> (clearance field, weight, core_d2, min_d2, min_core_voxels)"""
    out = {}
    for w in WEIGHTS:
        out[f"two rooms {w}"] = (d2_of("two rooms", two_rooms(False), w, 4096), w, DOOR_THRESHOLD[w] + 1, min(w), 1)
        vol, d2, par = ragged_case(RAGGED[0], w, 8)
        out[f"speckled {RAGGED[0]} {w}"] = (d2, w, par["core_d2"], par["min_d2"], 8)
        out[f"mirror rooms {w}"] = (d2_of("mirror rooms", mirror_rooms(), w), w, 9 * min(w), min(w), 1)
        out[f"serpentine {w}"] = (d2_of("serpentine", serpentine()[0], w, 256), w, serpentine_core_d2(w), min(w), 1)
    out["tile corner"] = (d2_of("tile corner", tile_corner(), (1, 1, 1)), (1, 1, 1), 4, 1, 1)
    out["corridors"] = (d2_of("corridors", corridors()[0], (1, 1, 1)), (1, 1, 1), 1, 1, 1)
    for i, (dims, d2) in enumerate(small_cases()):
        out[f"small {i}"] = (d2, (16, 25, 44), 50, 3, 2)
    return out


def test_the_kernels_text_makes_the_twins_partition_on_the_host_in_any_tile_order(tmp_path):
    """hsk_part_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program): the cores by the union-find, rounds of tile relaxations on 64-bit keys, one tile after the other, with the worklist as
    it was filled, reversed and shuffled -- the keys, the roots, the counts and the lookups against the twin, zero differences"""
    exe = kit.build_harness("part_point", tmp_path)
    rng = np.random.default_rng(19)
    for name, (d2, weight, core_d2, min_d2, min_core) in host_cases().items():
        p = twin_partition(name, d2, weight, core_d2, min_d2, min_core)
        Z, Y, X = d2.shape
        points = [tuple(int(v) for v in rng.integers(0, (X, Y, Z))) for _ in range(40)]
        lin = np.arange(X * Y * Z, dtype=np.uint32).reshape(Z, Y, X)
        rounds = []
        for order in (0, 1, 2):
            key, roots, counts, found = run_harness(exe, tmp_path, d2, weight, core_d2, min_d2, min_core, RE.MAX_COST, order, order + 1, points)
            print(f"{name} order {order}: {counts}")
            assert int((key != p["key"]).sum()) == 0, (name, order)
            assert (counts["n_cores"], counts["n_kept"], counts["n_passable"]) == (p["stats"]["n_cores"], p["stats"]["n_rooms"], p["stats"]["n_passable"])
            assert sorted(roots.tolist()) == sorted(int(lin[r[2], r[1], r[0]]) for r in p["rooms"]["root"])
            want = PT.lookup(p["ids"], weight, (1.0 * X, 1.0 * Y, 1.0 * Z), [(x + 0.5, y + 0.5, z + 0.5) for x, y, z in points], order + 1)
            rank = {int(lin[r[2], r[1], r[0]]): i for i, r in enumerate(p["rooms"]["root"])}
            got = [rank[int(k) & 0xFFFFFFFF] if (int(k) >> 32) <= RE.MAX_COST else PT.NONE for k in found]
            assert got == want.tolist(), (name, order)
            rounds.append(counts["n_rounds"])
        if name.startswith("serpentine"):
            assert min(rounds) >= 5
    # max_cost: the keys above it are not propagated; the cap: counted, nothing made
    d2, weight, core_d2, min_d2, min_core = host_cases()["serpentine (16, 25, 44)"]
    full = twin_partition("serpentine (16, 25, 44)", d2, weight, core_d2, min_d2, min_core)
    cap = int(np.sort(full["cost"][full["cost"] <= RE.MAX_COST])[full["cost"].size // 2])
    key, _, counts, _ = run_harness(exe, tmp_path, d2, weight, core_d2, min_d2, min_core, cap, 2)
    capped = PT.field(d2, weight, core_d2, min_d2, min_core, cap)[0]
    assert np.array_equal(key, capped) and (key == PT.KEY_UNASSIGNED).sum() >= 1000
    assert np.array_equal(key, np.where((full["cost"] <= RE.MAX_COST) & (full["cost"] > cap), PT.KEY_UNASSIGNED, full["key"]))
    vol, d2, par = ragged_case(RAGGED[1], (16, 25, 44), 1)
    key, _, counts, _ = run_harness(exe, tmp_path, d2, (16, 25, 44), 9 * 16, 16, 1, RE.MAX_COST, 0)
    assert key is None and (counts["n_cores"], counts["n_kept"], counts["n_rounds"]) == (1121, 1121, 0)


def test_the_two_harnesses_run_one_relaxation(tmp_path):
    """the tile relaxation is one text (hsk_reach_point.h) with two value policies: on a grid of 2 x 2 x 2 tiles, every one ragged,
    G of the partition harness's keys is the field the reach harness makes when every kept core voxel is a seed, bit for bit --
    the markers included (a key's G is the reach field's marker)"""
    exes = {}
    for name in ("part_point", "reach_point"):
        exes[name] = kit.build_harness(name, tmp_path)
    dims, weight = (40, 12, 11), (16, 25, 44)
    assert all(t < d < 2 * t for d, t in zip(dims, TILE))
    d2 = np.random.default_rng(23).choice(np.array([0, 1, 3, 50, CL.FAR], np.uint32), dims[::-1], p=[0.25, 0.25, 0.2, 0.15, 0.15])
    key, roots, counts, _ = run_harness(exes["part_point"], tmp_path, d2, weight, 50, 1, 2, RE.MAX_COST, 2)         # (singleton cores are dropped)
    g_of_key = (key >> np.uint64(32)).astype(np.uint32)
    seeds = [(int(x), int(y), int(z)) for z, y, x in np.argwhere(g_of_key == 0)]
    assert 2 <= counts["n_kept"] < counts["n_cores"] and 2 * counts["n_kept"] <= len(seeds) <= RE.MAX_SEEDS
    g, st, used, rounds, tiles, _ = reach_harness(exes["reach_point"], tmp_path, d2, weight, 1, RE.MAX_COST, 1, seeds)
    assert used == len(seeds) and int((g != g_of_key).sum()) == 0
    assert st["n_passable"] == counts["n_passable"] and ((g > 0) & (g <= RE.MAX_COST)).sum() >= 1000 and (g == RE.UNREACHED).sum() >= 1
    assert (g == RE.BLOCKED).sum() == (d2 < 1).sum() and min(tiles, counts["n_tiles"]) >= 8


# ---- 6. merge, defaults, layout, errors without a device ----------------------------------------------------------------------------------
def test_merge_rooms(hsk):
    vol, d2, par = ragged_case(RAGGED[0], (1, 1, 1), 8)
    p = twin_partition(f"speckled {RAGGED[0]}", d2, (1, 1, 1), **par)
    n = p["stats"]["n_rooms"]
    doors = p["doors"]
    seen = set()
    for merge_d2 in (0, 1, 2, 3, 4, 5, 9, 16, 17, CL.FAR):
        got = hsk.merge_rooms(doors, n, merge_d2)
        assert got.dtype == np.uint32 and np.array_equal(got, PT.merge(doors, n, merge_d2)) and (got <= np.arange(n)).all() and (got[got] == got).all()
        seen.add(len(set(got.tolist())))
    assert 1 in seen or min(seen) < n and max(seen) == n and len(seen) >= 3
    assert hsk.merge_rooms(doors[:0], 5, 0).tolist() == [0, 1, 2, 3, 4] and len(hsk.merge_rooms(doors[:0], 0, 0)) == 0
    chain = np.zeros(3, PT.DOOR_DTYPE)
    chain["a"], chain["b"], chain["max_d2"] = [2, 0, 3], [3, 2, 4], [9, 9, 8]
    assert hsk.merge_rooms(chain, 5, 9).tolist() == [0, 1, 0, 0, 4] == PT.merge(chain, 5, 9).tolist()
    lib = hsk._lib.load()
    out = np.full(4, 7, np.uint32)
    assert lib.hsk_merge_rooms(chain.ctypes.data, 3, 4, 9, out.ctypes.data) == -1 and (out == 7).all(), "room 4 is not below 4"
    assert lib.hsk_merge_rooms(None, 3, 4, 9, out.ctypes.data) == -1 and lib.hsk_merge_rooms(chain.ctypes.data, 3, 5, 9, None) == -1 and (out == 7).all()
    with pytest.raises(hsk.KinfuError):
        hsk.merge_rooms(chain, 4, 9)


def test_default_parameters(hsk):
    cube = CL.default_params((3.0, 3.0, 3.0), (256,) * 3)
    want = PT.default_params(cube, (3.0, 3.0, 3.0), (256,) * 3)
    p = hsk.default_partition_params()
    assert (p.core_d2, p.min_d2, p.min_core_voxels, p.max_cost, p.flags, p.pad) == (want["core_d2"], 1, want["min_core_voxels"], RE.MAX_COST, 0, 0)
    assert p.core_d2 == hsk.clearance_d2(hsk.default_clearance_params(), 0.5) == 1821 and p.min_core_voxels == 9710
    assert hsk.default_partition_params(clearance=hsk.default_clearance_params(max_d2=100)).core_d2 == 100          # clamped to max_d2
    q = hsk.default_partition_params(core_d2=7, min_d2=2, min_core_voxels=3, max_cost=99)
    assert (q.core_d2, q.min_d2, q.min_core_voxels, q.max_cost) == (7, 2, 3, 99)
    with pytest.raises(TypeError, match="no field"):
        hsk.default_partition_params(flags=1)
    hsk._lib.load().hsk_default_partition_params(None, None, None)


def test_partition_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    names = {"hsk_partition_params": (_lib.HskPartitionParams, None), "hsk_room": (_lib.HskRoom, hsk.kinfu.ROOM_DTYPE), "hsk_door": (_lib.HskDoor, hsk.kinfu.DOOR_DTYPE),
             "hsk_partition_stats": (_lib.HskPartitionStats, None)}
    for cls, dtype in names.values():
        if dtype is not None:
            for field, _ in cls._fields_:
                assert dtype.fields[field][1] == getattr(cls, field).offset
            assert dtype.itemsize == C.sizeof(cls) and dtype == PT.ROOM_DTYPE or dtype == PT.DOOR_DTYPE
    consts = ["HSK_PARTITION_MAX_ROOMS", "HSK_PARTITION_MAX_RADIUS", "HSK_ROOM_UNASSIGNED", "HSK_ROOM_OUTSIDE", "HSK_ROOM_BLOCKED", "HSK_ROOM_NONE"]
    assert [C.sizeof(c) for c, _ in names.values()] == [24, 88, 72, 56]
    assert (PT.MAX_ROOMS, PT.MAX_RADIUS, PT.UNASSIGNED, PT.OUTSIDE, PT.BLOCKED, PT.NONE) == tuple(getattr(_lib, c) for c in consts)
    assert (hsk.kinfu.ROOM_UNASSIGNED, hsk.kinfu.ROOM_OUTSIDE, hsk.kinfu.ROOM_BLOCKED, hsk.kinfu.ROOM_NONE) == (PT.UNASSIGNED, PT.OUTSIDE, PT.BLOCKED, PT.NONE)
    assert tuple(n for n, _ in _lib.HskPartitionParams._fields_)[:4] == hsk.kinfu.PARTITION_FIELDS


def test_null_contexts_are_refused(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    st = L.HskPartitionStats(n_cores=77)
    out = np.full(8, 9, np.uint32)
    recs, doors = np.full(2, 9, PT.ROOM_DTYPE), np.full(2, 9, PT.DOOR_DTYPE)
    pts = np.zeros((2, 3), f32)
    n = C.c_size_t(5)
    assert lib.hsk_build_partition(None, None, None, recs.ctypes.data, 2, C.byref(n), C.byref(st)) == -1 and (st.n_cores, n.value) == (77, 5)
    assert lib.hsk_partition_doors(None, doors.ctypes.data, 2, C.byref(n)) == -1 and n.value == 5
    assert lib.hsk_download_partition(None, None, out.ctypes.data) == -1 and lib.hsk_download_partition_cost(None, None, out.ctypes.data) == -1
    assert lib.hsk_partition_at(None, pts.ctypes.data, 2, 0, out.ctypes.data) == -1
    assert lib.hsk_partition_floor(None, None, 1, 0, 1, None, out.ctypes.data, recs.ctypes.data, 2, C.byref(n), doors.ctypes.data, 2, C.byref(n), C.byref(st)) == -1
    assert lib.hsk_release_partition(None) == -1 and lib.hsk_partition_tiles_relaxed(None, None, None, None) == -1
    assert (out == 9).all() and (recs["n_voxels"] == 9).all() and (doors["a"] == 9).all() and (st.n_cores, n.value) == (77, 5)
    for name in ("default_partition_params", "build_partition", "partition_doors", "download_partition", "download_partition_cost", "partition_at",
                 "partition_floor", "release_partition", "partition_tiles_relaxed"):
        assert callable(getattr(hsk.KinfuTracker, name))
