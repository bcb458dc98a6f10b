"""The reach field without a GPU: the numpy twin (tests/reach_twin.py) pinned by hand-computed cases -- an empty box in closed form,
a wall with a door, the cost tables -- and cross-checked with whole-grid Jacobi sweeps and, where it happens to import, with
scipy.sparse.csgraph.dijkstra; the kernels' shared text (housescan_amd/csrc/hsk_reach_point.h) compiled for the host with the
sanitizers, relaxing tile after tile in three visiting orders, against the twin -- zero differences; the path rule;
hsk_rank_views_reach and hsk_reach_metres; the C layout of the new structs and their Python mirror; the argument errors that need
no device.  The scenes and constants here are the GPU tests' too."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import clearance_twin as CL
import kit
import reach_twin as RE
from clearance_cases import SCENE_DEFAULTS, twin_field
from components_cases import speckled
from cover_cases import EYE, carved_volume
from reach_cases import (FREE_WORD, SERPENTINE_DIMS, SOLID_WORD, TILE, WEIGHTS, check_path, corridors, free_volume, hand_d2, header_constant, run_harness, serpentine, staircase, tile_corner, twin_reach)

f32 = np.float32


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------------


# ---- 1. the twin against hand-computed cases ------------------------------------------------------------------------------------------------
def test_the_cost_tables():
    assert sorted(set(RE.costs((1, 1, 1))) - {0}) == [16, 23, 28]
    assert sorted(set(RE.costs((16, 25, 44))) - {0}) == [64, 80, 102, 106, 124, 133, 148]
    c = RE.costs((16, 25, 44))
    assert c[13] == 0 and c[14] == 64 and c[16] == 80 and c[22] == 106 and c[26] == 148 and c[0] == 148 and c == c[::-1]
    assert max(RE.costs((1024, 1024, 1024))) == 887 and RE.MAX_COST + 887 < 2 ** 32


def test_an_empty_box_has_the_chamfer_distance_in_closed_form():
    dims = (13, 11, 7)
    d2 = np.full(dims[::-1], CL.FAR, np.uint32)
    seed = (4, 6, 2)
    g, used = RE.field(d2, (1, 1, 1), 1, RE.MAX_COST, [seed])
    zz, yy, xx = np.indices(dims[::-1])
    d = np.sort(np.stack([abs(xx - seed[0]), abs(yy - seed[1]), abs(zz - seed[2])]), axis=0)          # c <= b <= a
    assert used == 1 and np.array_equal(g, 16 * (d[2] - d[1]) + 23 * (d[1] - d[0]) + 28 * d[0])
    assert np.array_equal(g, RE.field_jacobi(d2, (1, 1, 1), 1, RE.MAX_COST, [seed]))
    two, used2 = RE.field(d2, (1, 1, 1), 1, RE.MAX_COST, [seed, (12, 0, 6), seed])
    far = np.sort(np.stack([abs(xx - 12), abs(yy - 0), abs(zz - 6)]), axis=0)
    assert used2 == 3 and np.array_equal(two, np.minimum(g, 16 * (far[2] - far[1]) + 23 * (far[1] - far[0]) + 28 * far[0]))
    capped, _ = RE.field(d2, (1, 1, 1), 1, 64, [seed])
    assert np.array_equal(capped, np.where(g <= 64, g, RE.UNREACHED)) and (capped == 64).any() and (capped == RE.UNREACHED).any()
    assert RE.stats(capped) == {"n_passable": 13 * 11 * 7, "n_reached": int((g <= 64).sum()), "max_cost_seen": 64}


def test_a_wall_with_a_door():
    """9 x 5 x 1, a wall at x = 4 with a door at y = 2, the seed at (0, 2): straight through the door 8 moves; to the far corner
    (8, 0) the path must leave the door by a face move -- the diagonal would cut the jamb's corner --: 4 + 1 face moves, two
    diagonals, one face move"""
    vol = free_volume((9, 5, 1))
    vol[0, :, 4] = SOLID_WORD
    vol[0, 2, 4] = FREE_WORD
    d2 = hand_d2(vol, (1, 1, 1))
    g, used = RE.field(d2, (1, 1, 1), 1, RE.MAX_COST, [(0, 2, 0)])
    assert used == 1 and g[0, 2, 8] == 8 * 16 and g[0, 0, 8] == 64 + 16 + 2 * 23 + 16 == 142 and g[0, 4, 8] == 142
    assert g[0, 2, 4] == 64 and g[0, 1, 5] == 64 + 16 + 16 and g[0, 1, 3] == 32 + 23 and (g[0, [0, 1, 3, 4], 4] == RE.BLOCKED).all()
    assert RE.path(g, (1, 1, 1), (8, 0, 0)).tolist() == [[0, 2, 0], [1, 2, 0], [2, 2, 0], [3, 2, 0], [4, 2, 0], [5, 2, 0], [6, 1, 0], [7, 0, 0], [8, 0, 0]]
    assert len(RE.path(g, (1, 1, 1), (4, 0, 0))) == 0 and len(RE.path(g, (1, 1, 1), (9, 0, 0))) == 0
    shut = vol.copy()
    shut[0, 2, 4] = SOLID_WORD
    g2, _ = RE.field(hand_d2(shut, (1, 1, 1)), (1, 1, 1), 1, RE.MAX_COST, [(0, 2, 0), (4, 2, 0)])          # the second seed lies on a solid
    assert (g2[0, :, 5:] == RE.UNREACHED).all() and (g2[0, :, :4] <= RE.MAX_COST).all() and _ == 1


def test_the_box_rule_keeps_a_path_from_slipping_between_solids_that_touch_by_an_edge():
    d2 = hand_d2(staircase(), (1, 1, 1))
    g, _ = RE.field(d2, (1, 1, 1), 1, RE.MAX_COST, [(2, 12, 6)])
    zz, yy, xx = np.indices(g.shape)
    assert (g[xx - yy > 8] == RE.UNREACHED).all() and (g[xx - yy < 8] <= RE.MAX_COST).all() and (g[xx - yy == 8] == RE.BLOCKED).all()
    assert (xx - yy > 8).sum() > 1000


# ---- 2. the twin against other shortest-path codes ------------------------------------------------------------------------------------------
def small_cases():
    rng = np.random.default_rng(5)
    for trial in range(6):
        dims = tuple(int(v) for v in rng.integers(1, 12, 3))
        d2 = rng.choice(np.array([0, 1, 3, 50, CL.FAR], np.uint32), dims[::-1], p=[0.2, 0.1, 0.1, 0.3, 0.3])
        seeds = [tuple(int(rng.integers(0, n)) for n in dims) for _ in range(3)]
        yield dims, d2, seeds


def test_the_frontier_relaxation_equals_whole_grid_sweeps():
    n = 0
    for dims, d2, seeds in small_cases():
        for weight in WEIGHTS:
            for min_d2, max_cost in ((1, RE.MAX_COST), (3, RE.MAX_COST), (1, 5 * RE.costs(weight)[14]), (1, 0)):
                got, used = RE.field(d2, weight, min_d2, max_cost, seeds)
                assert got.dtype == np.uint32 and np.array_equal(got, RE.field_jacobi(d2, weight, min_d2, max_cost, seeds)), (dims, weight, min_d2, max_cost)
                assert ((got == RE.BLOCKED) == (d2 < min_d2)).all() and used == sum(1 for x, y, z in seeds if d2[z, y, x] >= min_d2)
                n += 1
    assert n == 48


def test_the_twin_against_scipy_where_it_imports():
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import dijkstra
    except ImportError:
        return
    cases = [(d2, seeds) for _, d2, seeds in small_cases()] + [(hand_d2(serpentine()[0], (1, 1, 1)), [(2, 2, 2)])]
    for d2, seeds in cases:
        for weight in WEIGHTS:
            Z, Y, X = d2.shape
            ok = RE.allowed(RE.passable(d2, 1)).reshape(27, -1)
            c = RE.costs(weight)
            rows, cols, vals = [], [], []
            for m, (dx, dy, dz) in enumerate(RE.MOVES):
                src = np.flatnonzero(ok[m])
                rows.append(src), cols.append(src + dx + X * (dy + Y * dz)), vals.append(np.full(src.size, c[m], np.float64))
            graph = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(d2.size, d2.size)).tocsr()
            used = [x + X * (y + Y * z) for x, y, z in seeds if d2[z, y, x] >= 1]
            got, _ = RE.field(d2, weight, 1, RE.MAX_COST, seeds)
            if not used:
                assert not (got <= RE.MAX_COST).any()
                continue
            dist = dijkstra(graph, indices=sorted(set(used)), min_only=True).reshape(d2.shape)
            want = np.where(np.isfinite(dist), dist, float(RE.UNREACHED))
            want[d2 < 1] = RE.BLOCKED
            assert np.array_equal(got, want.astype(np.uint32))


# ---- 3. the kernels' shared text on the host ---------------------------------------------------------------------------------------------


def host_cases():
    """name -> (clearance field, weight, min_d2, seeds): the carved room at the default parameters; a ragged speckled volume, the
    serpentine, the staircase, the tile corner and the one-voxel corridors as the GPU tests build them, the hand-computed cases;
    all but the carved room with both weight sets"""
    d = SCENE_DEFAULTS
    carved = twin_field("carved", carved_volume(), d["weight"], d["max_d2"], CL.UNKNOWN)
    out = {"carved": (carved, d["weight"], RE.default_params(d)["min_d2"], RE.seed_voxels(AT.DST_SIZE, AT.DST_DIMS, [EYE]))}
    rag = np.ascontiguousarray(speckled(carved_volume(), 41)[:41, :56, :72])
    for w in WEIGHTS:
        out[f"speckled 72 x 56 x 41 {w}"] = (hand_d2(rag, w), w, min(w), [(30, 30, 20), (71, 55, 40), (0, 0, 0)])
        out[f"serpentine {w}"] = (hand_d2(serpentine()[0], w), w, min(w), [(2, 2, 2)])
        out[f"staircase {w}"] = (hand_d2(staircase(), w), w, min(w), [(2, 12, 6)])
        out[f"tile corner {w}"] = (hand_d2(tile_corner(), w), w, min(w), [(4, 3, 3)])
        # the hand-computed cases of the tests above, and the one-voxel corridors with their seeds on tile faces (few voxels each)
        out[f"small: empty box {w}"] = (np.full((7, 11, 13), CL.FAR, np.uint32), w, min(w), [(4, 6, 2)])
        door = free_volume((9, 5, 1))
        door[0, :, 4] = SOLID_WORD
        door[0, 2, 4] = FREE_WORD
        out[f"small: wall with a door {w}"] = (hand_d2(door, w), w, min(w), [(0, 2, 0)])
        vol, seeds = corridors()
        for name, seed in seeds.items():
            out[f"small: corridor {name} {w}"] = (hand_d2(vol, w), w, min(w), [seed])
    return out


def test_the_kernels_text_makes_the_twins_field_on_the_host_in_any_tile_order(tmp_path):
    """hsk_reach_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program): rounds of tile relaxations, one tile after the other, with the worklist as it was filled, reversed and shuffled --
    the field, the counts and the paths against the twin, zero differences"""
    assert TILE == (32, 8, 8) and (header_constant("REACH_MAX_SEEDS"), header_constant("REACH_MAX_ROUNDS")) == (RE.MAX_SEEDS, 65536)
    exe = kit.build_harness("reach_point", tmp_path)
    rng = np.random.default_rng(9)
    for name, (d2, weight, min_d2, seeds) in host_cases().items():
        ref, used = twin_reach(name, d2, weight, min_d2, RE.MAX_COST, seeds)
        reached = np.argwhere(ref <= RE.MAX_COST)
        goals = [tuple(int(v) for v in reached[i][::-1]) for i in rng.integers(0, len(reached), 4)] + [tuple(int(v) for v in b[::-1]) for b in np.argwhere(ref == RE.BLOCKED)[:1]]
        rounds, ok = [], RE.allowed(ref != RE.BLOCKED)
        for order in (0, 1, 2):
            g, st, n_used, n_rounds, n_tiles, paths = run_harness(exe, tmp_path, d2, weight, min_d2, RE.MAX_COST, order, seeds, goals)
            print(f"{name} order {order}: {st}, {n_rounds} rounds, {n_tiles} tiles relaxed")
            assert int((g != ref).sum()) == 0, (name, order)
            assert st == RE.stats(ref) and n_used == used and st["n_reached"] >= (10 if name.startswith("small") else 1000)
            for p, goal in zip(paths, goals):
                assert np.array_equal(p, RE.path(ref, weight, goal))
                if len(p):
                    check_path(ref, ok, weight, p, goal)
            assert all((len(p) > 0) == (ref[v[2], v[1], v[0]] <= RE.MAX_COST) for p, v in zip(paths, goals))
            if "corridor" in name:
                assert st["n_reached"] == (2 * TILE[0] if "face" in name else 2 * TILE[0] - 2), "the seed's whole corridor is reached, across the face or round the corner"
            rounds.append(n_rounds)
        if name.startswith("serpentine"):
            assert min(rounds) >= 5
    # the caps: a max_cost that occurs in the field, and 0
    d2, weight, min_d2, seeds = host_cases()["serpentine (16, 25, 44)"]
    full, _ = twin_reach("serpentine (16, 25, 44)", d2, weight, min_d2, RE.MAX_COST, seeds)
    cap = int(np.sort(full[full <= RE.MAX_COST])[full.size // 8])
    for max_cost in (cap, 0):
        g, st, *_ = run_harness(exe, tmp_path, d2, weight, min_d2, max_cost, 2, seeds)
        assert np.array_equal(g, np.where((full <= RE.MAX_COST) & (full > max_cost), RE.UNREACHED, full)) and st["max_cost_seen"] == max_cost
    # no usable seed: nothing is relaxed
    g, st, n_used, n_rounds, n_tiles, _ = run_harness(exe, tmp_path, d2, weight, min_d2, RE.MAX_COST, 0, [(10, 0, 0)])
    assert d2[0, 0, 10] == 0 and (n_used, n_rounds, n_tiles, st["n_reached"]) == (0, 0, 0, 0)


def test_the_scenes_are_what_the_tests_say():
    vol, seeds = corridors()
    free = vol[..., 0] > 0
    tx, ty, tz = TILE
    assert free.sum() == 2 * tx + (tx - 1) + 1 + (tx - 2) and all(free[z, y, x] for x, y, z in seeds.values())
    for x, y, z in list(seeds.values())[:4]:                     # one voxel wide: a seed has at most two free face neighbours
        assert sum(bool(free[z + c, y + b, x + a]) for a, b, c in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
                   if 0 <= x + a < free.shape[2] and 0 <= y + b < free.shape[1] and 0 <= z + c < free.shape[0]) <= 2
    vol, walls = serpentine()
    assert len(walls) >= 4 and all(s >= 3 * t for s, t in zip(SERPENTINE_DIMS[:2], TILE[:2]))
    ref, _ = twin_reach("serpentine (1, 1, 1)", hand_d2(vol, (1, 1, 1)), (1, 1, 1), 1, RE.MAX_COST, [(2, 2, 2)])
    X, Y, Z = SERPENTINE_DIMS
    # (between two walls, 14 voxels apart, the path crosses Y - 6 voxels of y: 14 diagonal moves and Y - 20 face moves, not 14 face moves)
    assert RE.MAX_COST >= ref[2, 2, X - 2] > 16 * (X - 4) + (len(walls) - 1) * (14 * 23 + (Y - 20) * 16 - 14 * 16) and (ref != RE.UNREACHED).all()
    corner, _ = twin_reach("tile corner (16, 25, 44)", hand_d2(tile_corner(), (16, 25, 44)), (16, 25, 44), 16, RE.MAX_COST, [(4, 3, 3)])
    far = corner[TILE[2]:, TILE[1]:, TILE[0]:]
    assert (far <= RE.MAX_COST).sum() > 500 and (far == RE.UNREACHED).sum() == 0 and (corner <= RE.MAX_COST).sum() >= 1000
    assert (corner <= RE.MAX_COST).sum() == (far <= RE.MAX_COST).sum() + (corner[:TILE[2], :TILE[1], :TILE[0]] <= RE.MAX_COST).sum() + 6
    assert corner[TILE[2], TILE[1], TILE[0]] == corner[TILE[2] - 1, TILE[1] - 1, TILE[0] - 1] + 148          # across the corner by the diagonal move


# ---- 4. defaults, metres, ranking, layout, errors without a device ------------------------------------------------------------------------
def test_default_parameters_and_metres(hsk):
    d = SCENE_DEFAULTS
    want = RE.default_params(d)
    assert want["min_d2"] in (1024, 1025) and want["max_cost"] == 0xF0000000
    cp = hsk.default_clearance_params(weight=d["weight"], max_d2=d["max_d2"], flags=d["flags"], unit_m=d["unit_m"])
    p = hsk.default_reach_params(clearance=cp)
    assert (p.min_d2, p.max_cost, p.flags, p.pad) == (want["min_d2"], want["max_cost"], 0, 0)
    cube = hsk.default_reach_params()
    assert cube.min_d2 == RE.default_params(CL.default_params((3.0, 3.0, 3.0), (256,) * 3))["min_d2"] == hsk.clearance_d2(hsk.default_clearance_params(), 0.3)
    assert hsk.default_reach_params(clearance=hsk.default_clearance_params(max_d2=100)).min_d2 == 100          # clamped to max_d2
    q = hsk.default_reach_params(min_d2=7, max_cost=99)
    assert (q.min_d2, q.max_cost) == (7, 99)
    with pytest.raises(TypeError, match="no field"):
        hsk.default_reach_params(flags=1)
    lib = hsk._lib.load()
    lib.hsk_default_reach_params(None, None, None)
    for g in (0, 1, 16, 4580, 22676, RE.MAX_COST):
        assert f32(lib.hsk_reach_metres(C.byref(cp), g)) == RE.metres(d["unit_m"], g) == hsk.reach_metres(cp, g)
    assert lib.hsk_reach_metres(C.byref(cp), 16) == d["unit_m"]
    for g in (RE.UNREACHED, RE.OUTSIDE, RE.BLOCKED, RE.MAX_COST + 1):
        assert np.isnan(lib.hsk_reach_metres(C.byref(cp), g)) and np.isnan(hsk.reach_metres(cp, g))
    assert np.isnan(lib.hsk_reach_metres(None, 5))
    m = hsk.reach_metres(cp, np.array([0, 1600, RE.BLOCKED], np.uint32))
    assert m[0] == 0 and abs(m[1] - 0.9375) < 1e-6 and np.isnan(m[2])


def test_rank_views_reach(hsk):
    rng = np.random.default_rng(12)
    n = 80
    s = np.zeros(n, hsk.kinfu.VIEW_SCORE_DTYPE)
    s["gain"], s["n_frontier"] = rng.integers(0, 6, n), rng.integers(0, 3, n)
    s["eye_state"] = rng.choice([0, 0, 0, 1, 2, 3], n)
    g = rng.choice(np.array([0, 5, 99, 100, 101, RE.MAX_COST, RE.UNREACHED, RE.OUTSIDE, RE.BLOCKED], np.uint32), n)
    for max_g in (100, 0, RE.MAX_COST):
        got = hsk.rank_views_reach(s, g, max_g)
        assert np.array_equal(got, RE.rank_views_reach(s, g, max_g)) and sorted(got.tolist()) == list(range(n))
        behind = (g > RE.MAX_COST) | (g > max_g)
        k = int((~behind).sum())
        plain = hsk.rank_views(s).tolist()
        assert 0 < k < n and got[:k].tolist() == [i for i in plain if not behind[i]] and got[k:].tolist() == [i for i in plain if behind[i]]
    assert np.array_equal(hsk.rank_views_reach(s, np.zeros(n, np.uint32)), hsk.rank_views(s))
    assert len(hsk.rank_views_reach(s[:0], g[:0], 5)) == 0
    lib = hsk._lib.load()
    order = np.full(n, 7, np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert lib.hsk_rank_views_reach(None, g.ctypes.data_as(u32p), 1, n, order.ctypes.data_as(u32p)) == -1
    assert lib.hsk_rank_views_reach(s.ctypes.data_as(C.POINTER(hsk._lib.HskViewScore)), None, 1, n, order.ctypes.data_as(u32p)) == -1
    assert lib.hsk_rank_views_reach(s.ctypes.data_as(C.POINTER(hsk._lib.HskViewScore)), g.ctypes.data_as(u32p), 1, n, None) == -1
    assert (order == 7).all()
    with pytest.raises(ValueError):
        hsk.rank_views_reach(s, g[:3], 5)


def test_reach_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, S = _lib.HskReachParams, _lib.HskReachStats
    assert (C.sizeof(P), C.sizeof(S)) == (16, 40)
    assert (RE.UNREACHED, RE.OUTSIDE, RE.BLOCKED, RE.MAX_COST, RE.MAX_SEEDS) == (_lib.HSK_REACH_UNREACHED, _lib.HSK_REACH_OUTSIDE, _lib.HSK_REACH_BLOCKED,
                                                                                 _lib.HSK_REACH_MAX_COST, _lib.HSK_REACH_MAX_SEEDS)
    assert (hsk.kinfu.REACH_UNREACHED, hsk.kinfu.REACH_OUTSIDE, hsk.kinfu.REACH_BLOCKED, hsk.kinfu.REACH_MAX_COST) == (RE.UNREACHED, RE.OUTSIDE, RE.BLOCKED, RE.MAX_COST)
    assert tuple(n for n, _ in P._fields_)[:2] == hsk.kinfu.REACH_FIELDS


def test_null_contexts_are_refused(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    st = L.HskReachStats(n_reached=77)
    out = np.full(8, 9, np.uint32)
    vox = np.full(6, 9, np.int32)
    pts = np.zeros((2, 3), f32)
    n = C.c_size_t(5)
    assert lib.hsk_build_reach(None, None, None, pts.ctypes.data, 2, C.byref(st)) == -1 and st.n_reached == 77
    assert lib.hsk_download_reach(None, None, out.ctypes.data) == -1
    assert lib.hsk_reach_at(None, pts.ctypes.data, 2, out.ctypes.data) == -1
    assert lib.hsk_reach_path(None, pts.ctypes.data, vox.ctypes.data, 2, C.byref(n)) == -1 and n.value == 5
    assert lib.hsk_reach_floor(None, None, 1, 0, 1, None, pts.ctypes.data, 2, out.ctypes.data, C.byref(st)) == -1 and st.n_reached == 77
    assert lib.hsk_release_reach(None) == -1 and lib.hsk_reach_tiles_relaxed(None, None, None) == -1
    assert (out == 9).all() and (vox == 9).all()
    for name in ("default_reach_params", "build_reach", "download_reach", "reach_at", "reach_path", "reach_floor", "release_reach"):
        assert callable(getattr(hsk.KinfuTracker, name))
