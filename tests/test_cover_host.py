"""Scan coverage without a GPU: the kernels' work on one ray (housescan_amd/csrc/hsk_cover_point.h, compiled for the host) against
the numpy twin (tests/cover_twin.py), ray for ray; hsk_rank_views against the twin; the property DESIGN.md 8i claims for the
half-tau step, shown on the twin; the C layout of the new structs and their Python mirror; hsk_default_probe; the argument errors
that need no device."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import cover_twin as CT
import kit
import np_twin as T
import reloc_twin as RT
from align_cases import scene
from cover_cases import AWAY, TOWARDS, carved_volume, probe_40x30
from kit import blocked

f32 = np.float32


def odd_translations():
    out = []
    for i, bad in enumerate((np.nan, np.inf, -np.inf)):
        m = np.array(TOWARDS, f32)
        m[i, 3] = bad
        out.append(m)
    m = np.array(TOWARDS, f32)
    m[:3, 3] = np.nan
    return out + [m]


def view_cases():
    """[(probe, {name: pose})]: the views of the rule's classes and eye states, grouped by the probe they are seen through"""
    full = {"towards the patch": TOWARDS, "away from the patch": AWAY,
            "from outside the grid, looking in": RT.look_at((-0.5, 1.5, 1.5), (1.5, 1.5, 1.5)),
            "from 40 m away": RT.look_at((40.0, 1.5, 1.5), (1.5, 1.5, 1.5)),
            "from the unobserved margin": RT.look_at((0.1, 1.5, 1.5), (1.5, 1.5, 1.5))}
    for i, m in enumerate(odd_translations()):
        full[f"odd translation {i}"] = m
    short = {"far_m short of every wall": RT.look_at((1.5, 1.5, 1.6), (2.7, 1.5, 1.6))}
    wall = {"the eye inside a wall's band": RT.look_at((0.26, 1.5, 1.5), (1.5, 1.5, 1.5))}
    return [(probe_40x30(), full), (probe_40x30(far_m=0.6), short), (probe_40x30(near_m=0.0), wall)]


def run_harness(exe, tmp_path, vol, pr, poses):
    poses = np.asarray(poses, f32).reshape(-1, 4, 4)
    path = tmp_path / "in.bin"
    with open(path, "wb") as f:
        for part in (np.array(AT.DST_DIMS, np.int32), np.array(AT.DST_SIZE, f32), np.array([pr["width"], pr["height"]], np.int32),
                     np.array([pr[k] for k in ("fx", "fy", "cx", "cy", "near_m", "far_m", "step_m")], f32), np.uint32(len(poses)), poses, blocked(vol)):
            f.write(np.ascontiguousarray(part).tobytes())
    out = kit.run_harness(exe, path, text=True)
    rows = [np.array(line.split(), np.int64) for line in out.strip().splitlines()]
    assert len(rows) == len(poses)
    return [(int(r[0]), r[1:].reshape(pr["height"], pr["width"], 3)) for r in rows]


# ---- 1. the kernels' work on one ray, compiled for the host ------------------------------------------------------------------
def test_the_kernels_ray_function_equals_the_twin_on_the_host(tmp_path):
    """the text every lane of k_cover_rays runs, built for the host with the address and undefined-behaviour sanitizers (their
    runtime linked into the program): class, depth and gain of every ray and every pose's eye_state against the twin, zero
    differences; a NaN or an infinity in a pose's translation makes its rays OUTSIDE and reads nothing out of bounds"""
    exe = kit.build_harness("cover_point", tmp_path)
    vol = carved_volume()
    S = CT.states(vol)
    assert ((S == CT.UNSEEN).sum(), (S == CT.FREE).sum(), (S == CT.SOLID).sum()) == (100980, 106556, 38224)
    seen_cls, seen_eye, scores = set(), set(), {}
    for pr, cases in view_cases():
        got = run_harness(exe, tmp_path, vol, pr, list(cases.values()))
        for (name, pose), (eye, px) in zip(cases.items(), got):
            ref = CT.ray_walk(vol, AT.DST_SIZE, pr, pose)
            sc = CT.score(vol, AT.DST_SIZE, pr, [pose])[0]
            print(f"{name}: {sc}")
            for k, key in enumerate(("cls", "depth_mm", "gain")):
                diff = int((px[..., k] != ref[key].astype(np.int64)).sum())
                assert diff == 0, f"{name}: {diff} rays differ in {key}"
            assert eye == int(sc["eye_state"]) == CT.eye_state(vol, AT.DST_SIZE, pose), name
            assert sum(int(sc[c]) for c in CT.CLASSES) == pr["width"] * pr["height"]
            assert int(sc["gain"]) == int(ref["gain"].sum()) and (ref["gain"][ref["cls"] != CT.FRONTIER] == 0).all()
            assert (ref["depth_mm"][~np.isin(ref["cls"], (CT.HIT, CT.FRONTIER))] == 0).all()
            seen_cls |= set(np.unique(ref["cls"]).tolist())
            seen_eye.add(eye)
            scores[name] = sc
    assert seen_cls == {CT.HIT, CT.FRONTIER, CT.OPEN, CT.BLIND, CT.OUTSIDE} and seen_eye == {CT.FREE, CT.UNSEEN, CT.SOLID, CT.NOWHERE}
    t = scores["towards the patch"]
    # the twin's own figures, pinned (the issue quotes 820 / 380 / 2804 for a view it does not fix: the target and the principal
    # point are the test's; through cx = 20, cy = 15 the twin gives 820 / 380 / 2784, through this probe from near_m = 0.4 820 / 380 / 2892)
    assert (int(t["n_hit"]), int(t["n_frontier"]), int(t["gain"]), int(t["eye_state"])) == (829, 371, 2764, CT.FREE)
    assert t["n_open"] == t["n_blind"] == t["n_outside"] == 0
    assert scores["away from the patch"]["n_hit"] == 1200
    assert scores["from outside the grid, looking in"]["n_blind"] == 1200 and scores["from outside the grid, looking in"]["eye_state"] == CT.NOWHERE
    assert scores["from 40 m away"]["n_outside"] == 1200
    assert scores["far_m short of every wall"]["n_open"] == 1200
    assert scores["the eye inside a wall's band"]["n_blind"] == 1200 and scores["the eye inside a wall's band"]["eye_state"] == CT.SOLID
    assert scores["from the unobserved margin"]["eye_state"] == CT.UNSEEN
    for i in range(4):
        assert scores[f"odd translation {i}"]["n_outside"] == 1200 and scores[f"odd translation {i}"]["eye_state"] == CT.NOWHERE


# ---- 2. hsk_rank_views ---------------------------------------------------------------------------------------------------------
def test_rank_views_equals_the_twin_ties_and_eye_states_included(hsk):
    rng = np.random.default_rng(11)
    s = np.zeros(300, CT.VIEW_SCORE_DTYPE)
    s["gain"] = rng.integers(0, 6, len(s))                      # few values: equal gains with equal and with different n_frontier
    s["n_frontier"] = rng.integers(0, 4, len(s))
    s["n_hit"] = rng.integers(0, 1000, len(s))                  # (no part of the key)
    s["eye_state"] = rng.choice([0, 0, 0, 1, 2, 3], len(s))
    s["gain"][7] = 1 << 40                                      # beyond 32 bits
    s["eye_state"][7] = 0
    s["gain"][8], s["eye_state"][8] = 1 << 41, 2                # the largest gain, where nobody can stand
    ref = CT.rank(s)
    got = hsk.rank_views(s)
    assert got.dtype == np.uint32 and np.array_equal(got, ref)
    free = s["eye_state"][got] == 0
    n_free = int(free.sum())
    assert 0 < n_free < len(s) and free[:n_free].all() and not free[n_free:].any() and got[0] == 7 and got[n_free] == 8
    for part in (got[:n_free], got[n_free:]):
        g, f = s["gain"][part].astype(np.int64), s["n_frontier"][part].astype(np.int64)
        assert (np.diff(g) <= 0).all()
        same = np.diff(g) == 0
        assert same.sum() > 10 and (np.diff(f)[same] <= 0).all()
        same_all = same & (np.diff(f) == 0)
        assert same_all.sum() > 5 and (np.diff(part.astype(np.int64))[same_all] > 0).all()
    assert len(hsk.rank_views(s[:0])) == 0
    assert hsk._lib.load().hsk_rank_views(None, 3, None) == -1


# ---- 3. the property of the half-tau step, on the twin ------------------------------------------------------------------------
def inside_views():
    eyes = ((1.0, 1.5, 1.4), (2.0, 0.8, 2.2), (1.6, 2.2, 0.8), (0.6, 1.9, 2.3))
    targets = ((2.7, 1.5, 1.4), (0.3, 1.2, 1.6), (1.5, 0.35, 1.5), (1.5, 2.6, 1.2), (1.4, 1.5, 0.4), (1.7, 1.3, 2.65), (2.7, 2.6, 2.65), (0.3, 0.35, 0.4))
    return [RT.look_at(e, t) for e in eyes for t in targets]


def test_fully_scanned_walls_show_no_frontier_at_half_tau_and_the_patch_ranks_first():
    """the scene without the patch: no view from inside the room has a FRONTIER ray at a step of 0.5 tau -- the SOLID band behind
    a surface is one tau thick -- while a step of 1.3 tau steps over it; with the patch, the view towards it ranks first among the
    25 views of a lattice of yaw and pitch around it, and the view away from it ranks behind it"""
    whole = scene()[0]
    pr = probe_40x30(near_m=0.4)
    views = inside_views()
    sc = CT.score(whole, AT.DST_SIZE, pr, views)
    print(f"0.5 tau: frontier rays {int(sc['n_frontier'].sum())}, hits {int(sc['n_hit'].sum())} of {1200 * len(views)}")
    assert (sc["eye_state"] == CT.FREE).all() and (sc["n_frontier"] == 0).all() and (sc["gain"] == 0).all() and (sc["n_hit"] > 0).all()
    long_step = CT.score(whole, AT.DST_SIZE, probe_40x30(near_m=0.4, step_tau=1.3), views)
    print(f"1.3 tau: frontier rays {int(long_step['n_frontier'].sum())}")
    assert long_step["n_frontier"].sum() > 100
    carved = carved_volume()
    L = RT.lattice(TOWARDS, 0.0, 0, np.radians(35.0), 2)
    assert len(L) == 25
    sc = CT.score(carved, AT.DST_SIZE, pr, list(L) + [AWAY])
    order = CT.rank(sc)
    print(f"best view {order[0]}: {sc[order[0]]}; away: {sc[25]}")
    assert order[0] == 12 and (int(sc["n_hit"][12]), int(sc["n_frontier"][12]), int(sc["gain"][12])) == (820, 380, 2892)
    assert sc["gain"][25] == 0 and list(order).index(25) > 0


# ---- 4. header, C layout, Python mirror ---------------------------------------------------------------------------------------
def test_cover_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    B, V, P, S = _lib.HskVoxelBox, _lib.HskCoverage, _lib.HskProbe, _lib.HskViewScore
    assert C.sizeof(S) == 32 and C.sizeof(V) == 80 and hsk.kinfu.VIEW_SCORE_DTYPE.itemsize == 32 and CT.VIEW_SCORE_DTYPE == hsk.kinfu.VIEW_SCORE_DTYPE
    assert [n for n, _ in S._fields_] == list(CT.CLASSES) + ["eye_state", "gain"]
    assert (_lib.HSK_RAY_HIT, _lib.HSK_RAY_FRONTIER, _lib.HSK_RAY_OPEN, _lib.HSK_RAY_BLIND, _lib.HSK_RAY_OUTSIDE) == (CT.HIT, CT.FRONTIER, CT.OPEN, CT.BLIND, CT.OUTSIDE)
    assert (_lib.HSK_EYE_FREE, _lib.HSK_EYE_UNSEEN, _lib.HSK_EYE_SOLID, _lib.HSK_EYE_OUTSIDE) == (CT.FREE, CT.UNSEEN, CT.SOLID, CT.NOWHERE)
    assert tuple(n for n, _ in P._fields_) == hsk.kinfu.PROBE_FIELDS


# ---- 5. hsk_default_probe --------------------------------------------------------------------------------------------------------
def test_default_probe_without_a_context(hsk):
    cfg = hsk.default_config(256)
    p = hsk.default_probe()
    tau = T.tau_of(tuple(cfg.vol_size_m), (cfg.vol_x, cfg.vol_y, cfg.vol_z), cfg.trunc_dist_m)
    assert (p.width, p.height) == (cfg.width >> 2, cfg.height >> 2) == (160, 120)
    assert (p.fx, p.fy, p.cx, p.cy) == (f32(cfg.fx) / f32(4), f32(cfg.fy) / f32(4), f32(cfg.cx) / f32(4), f32(cfg.cy) / f32(4))
    assert (p.near_m, p.far_m) == (f32(0.4), f32(3.5)) and p.step_m == f32(0.5) * f32(tau)
    q = hsk.default_probe(width=7, height=5, step_m=0.25)
    assert (q.width, q.height, q.step_m, q.fx) == (7, 5, 0.25, p.fx)
    with pytest.raises(TypeError, match="no field"):
        hsk.default_probe(depth=3)
    hsk._lib.load().hsk_default_probe(None, None)
    assert CT.n_samples(CT.probe(*(getattr(p, k) for k in hsk.kinfu.PROBE_FIELDS))) == int(np.floor((3.5 - float(f32(0.4))) / float(p.step_m))) + 1


# ---- 6. the argument errors that need no device ----------------------------------------------------------------------------------
def test_null_contexts_are_refused(hsk):
    lib = hsk._lib.load()
    L = hsk._lib
    eye = np.eye(4, dtype=f32)
    one = np.zeros(1, CT.VIEW_SCORE_DTYPE)
    cov = L.HskCoverage(n_unseen=77)
    p = hsk.default_probe()
    assert lib.hsk_coverage_census(None, None, C.byref(cov)) == -1 and cov.n_unseen == 77
    assert lib.hsk_score_views(None, C.byref(p), eye.ctypes.data, 1, one.ctypes.data_as(C.POINTER(L.HskViewScore))) == -1 and not one["gain"].any()
    cls = np.full((p.height, p.width), 9, np.uint8)
    assert lib.hsk_render_coverage(None, C.byref(p), eye.ctypes.data_as(C.POINTER(C.c_float)), cls.ctypes.data, None, None, None) == -1 and (cls == 9).all()
    for name in ("coverage", "score_views", "render_coverage"):
        assert callable(getattr(hsk.KinfuTracker, name))
    assert callable(hsk.default_probe) and callable(hsk.rank_views)
