"""Cloud normals without a GPU: the rule's text for one point (housescan_amd/csrc/hsk_normal_point.h, compiled for the host) against
the numpy twin (tests/normals_twin.py, its two forms asserted equal on the way) on every case of tests/normals_cases.py, byte for
byte; the library's host mirror hsk_normal_solve against the twin's solve; what the rule promises -- outputs that do not depend on
the order of the points, an oblique plane's normal, the surfel import that normal feeds, a sphere, a thin wall whose faces turn to
their own rooms --, shown on the twin; the defaults and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import kit
import normals_cases as NC
import normals_twin as NT
import planes_twin as PT
import splat_cases as SC
import splat_twin as ST

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{case name: (case, the twin's five outputs, the harness's)} of every case, each computed once"""
    tmp = tmp_path_factory.mktemp("normals")
    exe = kit.build_harness("normal_point", tmp)
    out = {}
    for i, c in enumerate(NC.all_cases()):
        src, dst = tmp / f"in{i}.bin", tmp / f"out{i}.bin"
        NC.write_harness_input(src, c)
        kit.run_harness(exe, src, dst)
        assert c["name"] not in out
        out[c["name"]] = (c, NC.twin(c), NC.read_harness_output(dst, len(c["xyz"])))
    return out


def test_the_harness_equals_the_twin_on_every_case(results):
    """the text every lane of k_normal_gather runs, built for the host with the address and undefined-behaviour sanitizers: normals,
    curvature, counts, classes and counters against the twin"""
    seen = np.zeros(5, np.int64)
    for name, (c, ref, got) in results.items():
        for what, a, b in zip(("normals", "curvature", "neighbours", "classes"), ref, got):
            assert kit.same_bits(a, b), f"{name}: {what} differ at {np.argwhere(np.asarray(a != b))[:5].tolist()}"
        assert ref[4] == got[4], f"{name}: {ref[4]} != {got[4]}"
        assert sum(ref[4][k] for k in NT.STATS[:5]) == len(c["xyz"]), name
        seen += np.bincount(ref[3], minlength=5)
    assert (seen > 0).all(), seen                              # every class of the rule occurs


def test_the_cases_mean_what_their_names_say(results):
    _, (_, _, cnt, cls, st), _ = results["neighbours at exactly the radius"]
    assert cnt[0] == 1 + len(NC.ON_BOUNDARY) and cls[0] == NT.OK
    _, (_, _, cnt, cls, st), _ = results["neighbours one step past the radius"]
    assert cnt[0] == 1 and cls[0] == NT.SPARSE
    _, (_, _, cnt, cls, st), _ = results["duplicated points"]
    assert (cnt == 15).all() and st["n_ok"] == 15 and st["n_cells"] == 1
    _, (_, _, cnt, cls, st), _ = results["4096 points, each in a cell of its own"]
    assert (cnt == 1).all() and st["n_sparse"] == st["n_cells"] == st["n_pairs"] == 4096
    _, (_, _, cnt, cls, st), _ = results["300 points in one cell"]
    assert (cnt == 300).all() and st["n_ok"] == 300 and st["n_cells"] == 1 and st["n_pairs"] == 90000
    _, (nrm, curv, cnt, cls, st), _ = results["300 points in one cell, 64 allowed"]
    assert (cnt == 65).all() and st["n_crowded"] == 300 and st["n_pairs"] == 300 * 65 and not nrm.any() and not curv.any()
    for name in ("a collinear run", "three coincident points"):
        _, (nrm, curv, cnt, cls, st), _ = results[name]
        assert (cls == NT.DEGENERATE).all() and not nrm.any() and not curv.any(), name
    _, (nrm, _, cnt, cls, st), _ = results["NaN, Inf and points out of reach among valid ones"]
    assert st["n_invalid"] == 6 and (cls[20:26] == NT.INVALID).all() and not cnt[20:26].any() and st["n_ok"] > 30
    _, (_, _, cnt, cls, st), _ = results["no valid point"]
    assert st["n_invalid"] == 6 and st["n_cells"] == 0 and st["n_pairs"] == 0
    _, (_, _, cnt, cls, st), _ = results["neighbours in all 27 cells, and round a cell's corner"]
    assert cnt[13] == 27 and st["n_cells"] == 27 + 8 and (cnt[27:] == 8).all()
    c, (_, _, cnt, cls, st), _ = results["coordinates at +-64 m, r_q = 4"]
    assert (cnt == 9).all() and st["n_ok"] == 72 and np.abs(c["xyz"]).max() == 64.0 and NT.radius_q(c["params"]["radius_m"]) == 4
    c, (_, _, cnt, cls, st), _ = results["r_q = 1024"]
    assert NT.radius_q(c["params"]["radius_m"]) == 1024 and st["n_ok"] == 900 and cnt.max() > 400


def test_the_orientation_cases(results):
    up, down = [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]
    for name, want in (("a flat patch, no viewpoint", up), ("a flat patch, one viewpoint below", down),
                       ("a flat patch, a viewpoint in the tangent plane", up), ("a flat patch, two equidistant viewpoints", down)):
        _, (nrm, curv, _, cls, _), _ = results[name]
        assert (cls == NT.OK).all() and (nrm == np.array(want, f32)).all() and not curv.any(), name
    c, (nrm, _, _, cls, _), _ = results["a sphere, 256 viewpoints"]
    d = c["viewpoints"].astype(f64)[None] - c["xyz"].astype(f64)[:, None]
    near = d[np.arange(len(d)), np.argmin((d * d).sum(-1), axis=1)]
    assert (cls == NT.OK).all() and ((nrm.astype(f64) * near).sum(-1) > 0).all()


def test_the_host_mirror_equals_the_twins_solve(hsk, results):
    """hsk_normal_solve through the library, on the sums of every case's first points that are solved"""
    done = 0
    for name, (c, (nrm, curv, cnt, cls, _), _) in results.items():
        ok = NT.valid(c["xyz"])
        sums, _ = NT.sums_grid(NT.quantise(c["xyz"], ok), ok, NT.radius_q(c["params"]["radius_m"]))
        for i in np.flatnonzero((cls == NT.OK) | (cls == NT.DEGENERATE))[:24]:
            got = hsk.normal_solve(sums[i], c["xyz"][i], c["viewpoints"], c["params"]["line_rel"])
            assert kit.same_bits(got[0], nrm[i]) and kit.same_bits(got[1], curv[i]) and got[2] == cls[i], (name, i)
            done += 1
    assert done > 300
    with pytest.raises(hsk.KinfuError, match="normal_solve"):
        hsk.normal_solve([0] * 10, [0, 0, 0])                      # no neighbour at all
    with pytest.raises(hsk.KinfuError, match="normal_solve"):
        hsk.normal_solve([3, 0, 0, 0, 1 << 40, 0, 0, 0, 0, 0], [0, 0, 0])
    with pytest.raises(hsk.KinfuError, match="normal_solve"):
        hsk.normal_solve([3, 0, 0, 0, 2, 0, 0, 2, 0, 0], [0, 0, 0], line_rel=float("nan"))
    with pytest.raises(hsk.KinfuError, match="normal_solve"):
        hsk.normal_solve([3, 0, 0, 0, 2, 0, 0, 2, 0, 0], [0, 0, 0], viewpoints=[[0, float("inf"), 0]])
    assert hsk._lib.load().hsk_normal_solve(None, None, None, 0, 0.001, None, None, None) == -1


def test_shuffling_the_cloud_permutes_the_outputs_and_changes_no_bit(results):
    for name in ("6000 random points", "a box corner", "a thin wall", "NaN, Inf and points out of reach among valid ones"):
        c, ref, _ = results[name]
        order = np.random.default_rng(5).permutation(len(c["xyz"]))
        got = NT.estimate(c["xyz"][order], c["viewpoints"], c["params"])
        assert all(kit.same_bits(a[order], b) for a, b in zip(ref[:4], got[:4])) and ref[4] == got[4], name


def test_the_oblique_plane(results):
    """The plane of tests/splat_cases.py (30 degrees, 40 mm spacing) at radius 3 s = 0.12 m.  A grid point inside the plane has the
    29 grid points within 3 spacings as neighbours (the 3-4-5 triangle is out of reach: 9 + 0 <= 9, 4 + 4 <= 9, 9 + 1 > 9: 1 + 4 * 3 +
    4 * 2 + 8 = 29), a corner a quarter of them and the axes: 11.  The points lie on the plane up to binary32 rounding of their
    coordinates and the 1 / 4096 m grid: at most 0.125 mm off it along each axis, over a lever of 0.12 m -- a tilt of at most
    atan(2 * 0.125e-3 * sqrt(3) / 0.12) = 0.21 degrees in the worst case of everything conspiring; the issue's bound is 0.2, what the rule
    gave when the issue was written 0.074.  Curvature: (0.125e-3 / 0.12)^2 is about 1e-6 <= 1e-5."""
    c, (nrm, curv, cnt, cls, st), _ = results["the oblique plane"]
    true = NC.oblique_plane()[1]
    assert st["n_ok"] == len(c["xyz"]) and cnt.min() == 11 and cnt.max() == 29
    cos = np.clip((nrm.astype(f64) * true).sum(-1) / np.linalg.norm(nrm.astype(f64), axis=1), -1.0, 1.0)
    angle = np.degrees(np.arccos(cos))
    print(f"largest angle to the true normal {angle.max():.4f} degrees, largest curvature {curv.max():.3g}")
    assert angle.max() <= 0.2 and curv.max() <= 1e-5


def test_the_estimated_normals_feed_the_surfel_import(results):
    """the chain: the oblique plane through splat_twin.splat in SURFEL mode with the ESTIMATED normals, held to the bound
    tests/test_splat_host.py holds the true normals to (1.0 mm)"""
    c, (nrm, _, _, _, _), _ = results["the oblique plane"]
    case = SC.oblique_cases()[0]
    assert kit.same_bits(case["xyz"], c["xyz"]) and case["params"]["mode"] == ST.SURFEL
    ref = SC.oblique_depth(case["cam"]) * 1000.0
    err = {}
    for what, normals in (("estimated", nrm), ("true", case["normals"])):
        img, st = ST.splat(case["xyz"], normals, case["pose"], SC.CAMS[case["cam"]], case["params"])
        err[what] = np.abs(img.astype(f64) - ref).max()
        assert st["n_pixels"] == img.size and st["n_backfacing"] == 0, what
    print(f"surfel: largest depth error {err['estimated']:.3f} mm with the estimated normals, {err['true']:.3f} mm with the true ones")
    assert err["estimated"] <= 1.0


def test_a_sphere_seen_from_its_centre(results):
    """Normals are radial and point inward.  DERIVED bound: the neighbours of a point lie on a cap of chord radius r = 0.12 m of a
    sphere of R = 0.5 m, within its sag r^2 / 2R = 14.4 mm of the tangent plane; a plane through them tilts against the tangent plane
    by at most atan(sag / r) = 6.9 degrees, however unevenly the cap is sampled."""
    c, (nrm, curv, cnt, cls, st), _ = results["a sphere seen from its centre"]
    assert st["n_ok"] == len(c["xyz"])
    inward = np.array(NC.SPHERE_CENTRE) - c["xyz"].astype(f64)
    inward /= np.linalg.norm(inward, axis=1)[:, None]
    cos = (nrm.astype(f64) * inward).sum(-1)
    print(f"largest angle to the radius {np.degrees(np.arccos(cos.min())):.3f} degrees, curvature {curv.min():.3g} .. {curv.max():.3g}")
    assert cos.min() >= np.cos(np.arctan(0.12 / (2 * 0.5))) and (curv > 0).all() and (curv <= f32(1.0 / 3.0)).all()


def test_a_box_corner_has_curvature_where_its_faces_meet(results):
    c, (nrm, curv, cnt, cls, st), _ = results["a box corner"]
    assert st["n_ok"] == len(c["xyz"])
    d = c["xyz"].astype(f64) - 1.0                                # the corner at the origin, the faces in the coordinate planes
    on = (d < 1e-6).sum(axis=1)                                   # 1: a face's point, 2: on an edge, 3: the corner
    inner = (on == 1) & (np.sort(d, axis=1)[:, 1] > 0.07)         # a face's points further than the radius from the other faces
    assert inner.sum() > 100 and (curv[inner] == 0).all() and (np.abs(nrm[inner]).max(axis=1) == 1).all()
    assert (curv[on == 2] > 1e-2).all() and (curv[on == 3] > 5e-2).all() and curv.max() <= f32(1.0 / 3.0)


def test_a_thin_walls_faces_turn_to_their_own_rooms(results):
    c, (nrm, curv, cnt, cls, st), _ = results["a thin wall"]
    face = NC.thin_wall()[1]
    assert st["n_ok"] == 882 and cnt.min() >= 5
    assert (nrm[face == 0] == np.array([-1, 0, 0], f32)).all() and (nrm[face == 1] == np.array([1, 0, 0], f32)).all()
    recs, labels, bad = PT.detect(c["xyz"], nrm)
    assert bad == 0 and len(recs) == 2 and [int(r["n_inliers"]) for r in recs] == [441, 441]
    a, b = recs[0]["abcd"][:3].astype(f64), recs[1]["abcd"][:3].astype(f64)
    assert a @ b < -0.999 and (np.bincount(labels[face == 0], minlength=2).max() == 441)


def test_the_defaults_and_the_python_surface(hsk):
    p = hsk.default_normal_params()
    ref = NT.params()
    assert f32(p.radius_m) == ref["radius_m"] == f32(3.0) * (f32(3.0) / f32(512.0))
    assert (p.min_neighbours, p.max_neighbours, f32(p.line_rel), p.flags, p.pad) == (8, 4096, f32(1e-3), 0, 0)
    assert NT.default_radius(1e-5) == f32(1.0) / f32(1024.0) and NT.default_radius(0.2) == 0.25
    q = hsk.default_normal_params(radius_m=0.125, max_neighbours=100)
    assert (q.radius_m, q.min_neighbours, q.max_neighbours) == (0.125, 8, 100)
    for refused in ("flags", "pad", "radius"):
        with pytest.raises(TypeError, match="no field"):
            hsk.default_normal_params(**{refused: 0})
    from housescan_amd import _lib, kinfu
    assert C.sizeof(_lib.HskNormalParams) == 24 and C.sizeof(_lib.HskNormalStats) == 32
    assert tuple(n for n, _ in _lib.HskNormalStats._fields_) == NT.STATS
    assert tuple(n for n, _ in _lib.HskNormalParams._fields_)[:4] == kinfu.NORMAL_FIELDS
    assert (hsk.NORMAL_OK, hsk.NORMAL_INVALID, hsk.NORMAL_SPARSE, hsk.NORMAL_CROWDED, hsk.NORMAL_DEGENERATE) == (NT.OK, NT.INVALID, NT.SPARSE, NT.CROWDED, NT.DEGENERATE)
    lib = _lib.load()
    lib.hsk_default_normal_params(None, None)
    out = np.full(3, 9, f32)
    assert lib.hsk_estimate_normals(None, None, 0, None, 0, None, out.ctypes.data, None, None, None, None) == -1 and (out == 9).all()
    assert callable(hsk.KinfuTracker.estimate_normals)
    nrm, curv, cls = hsk.normal_solve([4, 0, 0, 0, 8, 0, 0, 8, 0, 0], [0.1, 0.2, 0.3])      # four points of a square in the plane z = 0
    assert (nrm == np.array([0, 0, 1], f32)).all() and curv == 0 and cls == hsk.NORMAL_OK
    nrm, _, _ = hsk.normal_solve([4, 0, 0, 0, 8, 0, 0, 8, 0, 0], [0.1, 0.2, 0.3], viewpoints=[[0, 0, -1]])
    assert (nrm == np.array([0, 0, -1], f32)).all()
