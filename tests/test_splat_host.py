"""Cloud import without a GPU: the kernel's work on one point and one pixel (housescan_amd/csrc/hsk_splat_point.h, compiled for the
host) against the numpy twin (tests/splat_twin.py) on every case of tests/splat_cases.py, byte for byte; what the rule promises --
a watertight image of a regular grid, the depth error of an oblique plane in both modes, an image that does not depend on the
order of the points --, shown on the twin; the defaults and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import kit
import splat_cases as SC
import splat_twin as ST

f32 = np.float32


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{case name: (case, the twin's (image, stats), the harness's)} of every case, each computed once"""
    tmp = tmp_path_factory.mktemp("splat")
    exe = kit.build_harness("splat_point", tmp)
    out = {}
    for i, c in enumerate(SC.all_cases()):
        src, dst = tmp / f"in{i}.bin", tmp / f"out{i}.bin"
        SC.write_harness_input(src, c)
        kit.run_harness(exe, src, dst)
        key = f"{c['cam']}: {c['name']}"
        assert key not in out
        out[key] = (c, SC.twin(c), SC.read_harness_output(dst, c))
    return out


def test_the_harness_equals_the_twin_on_every_case(results):
    """the text every lane of k_splat_points runs, built for the host with the address and undefined-behaviour sanitizers: every
    image and every counter against the twin"""
    seen = {k: 0 for k in ST.STATS}
    for key, (c, (img, st), (got_img, got_st)) in results.items():
        assert kit.same_bits(img, got_img), f"{key}: {int((img != got_img).sum())} pixels differ"
        assert st == got_st, f"{key}: {st} != {got_st}"
        assert sum(st[k] for k in ST.STATS[:5]) == len(c["xyz"]), key
        for k in ST.STATS:
            seen[k] += st[k]
    assert all(v > 0 for v in seen.values()), seen            # every class of the rule occurs


def one(results, cam, name):
    return results[f"{cam}: {name}"]


@pytest.mark.parametrize("cam", ["68x52", "64x48"])
def test_the_geometry_cases_mean_what_their_names_say(results, cam):
    w, h = SC.CAMS[cam]["width"], SC.CAMS[cam]["height"]
    _, (img, st), _ = one(results, cam, "footprints clipped by each border and corner")
    assert st["n_splatted"] == 8 and st["n_outside"] == 0
    assert all(img[v, u] == 1000 for v in (0, h - 1) for u in (0, w - 1)) and img[h // 2, 0] == img[h // 2, w - 1] == img[0, w // 2] == img[h - 1, w // 2] == 1000
    _, (img, st), _ = one(results, cam, "footprints that miss the image by one pixel, and their neighbours that do not")
    assert (st["n_outside"], st["n_splatted"]) == (4, 4)
    assert img[h // 2, 0] and img[h // 2, w - 1] and img[0, w // 2] and img[h - 1, w // 2] and not img[h // 2, 1] and not img[1, w // 2]
    _, (img, st), _ = one(results, cam, "half-widths at both clamps")
    assert st["n_splatted"] == 2 and int((img == 7000).sum()) == 1 and int((img == 150).sum()) == 17 * 17
    _, (img, st), _ = one(results, cam, "z at near_m and far_m, and one step outside")
    assert (st["n_splatted"], st["n_clipped"]) == (2, 2) and (img == 100).any() and (img == 8000).any()
    _, (img, st), _ = one(results, cam, "z_mm = 65535")
    assert (st["n_clipped"], st["n_splatted"] + st["n_outside"]) == (1, 2) and (img == 65535).any()
    _, (img, st), _ = one(results, cam, "points behind the camera and in its plane")
    assert (st["n_clipped"], st["n_splatted"]) == (3, 1)
    _, (img, st), _ = one(results, cam, "NaN and Inf coordinates")
    assert (st["n_invalid"], st["n_splatted"]) == (9, 1)
    c, (img, st), _ = one(results, cam, "4096 points on one pixel")
    assert (st["n_splatted"], st["n_pixels"]) == (4096, 1) and img.max() == int(ST.mm(f32(c["xyz"][:, 2].min())))
    _, (img, st), _ = one(results, cam, "equal z_mm on one pixel")
    assert st["n_pixels"] == 1 and img.max() == 1000
    a, b = one(results, cam, "near before far")[1], one(results, cam, "far before near")[1]
    assert kit.same_bits(a[0], b[0]) and a[1] == b[1] and set(np.unique(a[0])) == {0, 1000, 2000}
    c, (img, st), _ = one(results, cam, "surfel: grazing normals reach the clamp")
    lo, hi = 1000 - 75, 1000 + 75                                  # z -+ 2 half_m = 1 -+ 0.075 m
    assert st["n_splatted"] == 2 and img[img != 0].min() == lo and img.max() == hi
    _, (img, st), _ = one(results, cam, "surfel: back-facing points")
    assert (st["n_backfacing"], st["n_splatted"]) == (2, 1)
    _, (img, st), _ = one(results, cam, "surfel: zero and NaN normals are disc points")
    assert st["n_splatted"] == 3 and set(np.unique(img)) == {0, 1000}
    _, (img, st), _ = one(results, cam, "surfel: one disc and one surfel offer on a pixel")
    assert st["n_splatted"] == 2 and len(np.unique(img)) > 3 and (img == 1000).any()
    _, (img, st), _ = one(results, cam, "surfel without normals given to a disc call")
    assert set(np.unique(img)) == {0, 1000}


def test_a_regular_grid_is_watertight_as_it_lies_and_turned_in_its_plane(results):
    """DERIVED: a grid of spacing s at depth z projects to a grid of spacing d = fx s / z pixels.  Every pixel centre lies within
    d / sqrt(2) (half the cell's diagonal) of a grid point in the Euclidean sense, whatever the grid's rotation in its plane, so
    within d / sqrt(2) on either image axis; the footprint's half-width is fx (0.5 s cover) / z = 0.75 d > d / sqrt(2) with the
    default cover (1.5 >= sqrt(2)), and neither clamp bites (0.5 <= 1.5 px <= 8).  So every pixel is owned, and by points at z only."""
    cam = SC.CAMS["68x52"]
    d = float(cam["fx"]) * SC.WATER_S / SC.WATER_Z
    assert 0.5 <= 0.75 * d <= 8.0
    for spin in (0, 30):
        _, (img, st), _ = one(results, "68x52", f"watertight grid turned by {spin} degrees")
        assert st["n_pixels"] == img.size and (img == int(round(SC.WATER_Z * 1000))).all(), spin


def test_an_oblique_plane_is_exact_in_surfel_mode_and_bounded_in_disc_mode(results):
    """The plane z = z0 + x tan(30 deg), sampled by a grid of spacing s with its normals.  SURFEL: a pixel's offers are its ray's
    depth on the points' tangent planes, which all are the plane itself, so the image is the analytic depth z* up to the rounding
    to a millimetre (0.5 mm) and float error: 1 mm.  The clamp z +- 2 half_m is never reached (below).
    DISC, DERIVED: a point p owns pixel u only if |u0 - u| <= fx half_m / z_p, that is |x_p - rx z_p| <= half_m with rx = (u - cx) /
    fx (no clamp bites: 0.5 <= fx half_m / z <= 8 over the view).  On the plane z_p - z* = (x_p - rx z*) tan = ((x_p - rx z_p) + rx
    (z_p - z*)) tan, so |z_p - z*| <= half_m tan / (1 - |rx| tan), which is <= half_m tan (1 + |rx|) while |rx| <= (1 - tan) / tan =
    0.73 (here max |rx| = 0.56); the plane does not vary along v.  Every pixel has an owner (the grid is denser than the watertight
    one), every offer lies within the bound of z*, so the smallest does; the rounding adds 0.5 mm: the issue's bound
    half_m tan 30 (1 + max |u - cx| / fx) + 1 mm."""
    cam = SC.CAMS["68x52"]
    ref = SC.oblique_depth("68x52") * 1000.0
    tan = np.tan(np.radians(SC.OBLIQUE_DEG))
    half = 0.5 * SC.OBLIQUE_S * 1.5
    rx_max = float(np.abs(np.arange(cam["width"]) - float(cam["cx"])).max() / float(cam["fx"]))
    assert rx_max <= (1 - tan) / tan and half * tan / (1 - rx_max * tan) < 2 * half
    z = ref / 1000.0
    assert (float(cam["fx"]) * half / z.max() >= 0.5) and (float(cam["fx"]) * half / z.min() <= 8.0)
    _, (img, st), _ = one(results, "68x52", "oblique plane, surfel")
    err = np.abs(img.astype(np.float64) - ref)
    print(f"surfel: largest error {err.max():.3f} mm")
    assert st["n_pixels"] == img.size and err.max() <= 1.0
    _, (img, st), _ = one(results, "68x52", "oblique plane, disc")
    err = np.abs(img.astype(np.float64) - ref)
    bound = (half * tan * (1.0 + rx_max)) * 1000.0 + 1.0
    print(f"disc: largest error {err.max():.3f} mm, bound {bound:.3f} mm")
    assert st["n_pixels"] == img.size and err.max() <= bound


def test_shuffling_the_cloud_changes_no_pixel_and_no_counter(results):
    for key in ("640x480: 6000 points at the sensor's resolution", "68x52: 257 points, surfel", "68x52: oblique plane, surfel"):
        c, (img, st), _ = results[key]
        order = np.random.default_rng(5).permutation(len(c["xyz"]))
        d = dict(c, xyz=c["xyz"][order], normals=c["normals"][order])
        img2, st2 = SC.twin(d)
        assert kit.same_bits(img, img2) and st == st2, key


def test_the_defaults_and_the_python_surface(hsk):
    p = hsk.default_splat_params()
    ref = ST.params()
    assert p.mode == hsk.SPLAT_DISC == ST.DISC and hsk.SPLAT_SURFEL == ST.SURFEL
    assert all(f32(getattr(p, k)) == ref[k] for k in ("point_size_m", "cover", "min_half_px", "max_half_px", "near_m", "far_m"))
    assert p.point_size_m == f32(3.0) / f32(512.0) and p.cover >= np.sqrt(2.0)
    q = hsk.default_splat_params(mode=hsk.SPLAT_SURFEL, far_m=3)
    assert (q.mode, q.far_m, q.cover) == (1, 3.0, 1.5)
    with pytest.raises(TypeError, match="no field"):
        hsk.default_splat_params(size=3)
    from housescan_amd import _lib, house, kinfu
    assert C.sizeof(_lib.HskSplatParams) == 28 and C.sizeof(_lib.HskSplatStats) == 24 and kinfu.SPLAT_STATS_DTYPE.names == ST.STATS
    assert tuple(n for n, _ in _lib.HskSplatParams._fields_) == kinfu.SPLAT_FIELDS
    lib = _lib.load()
    lib.hsk_default_splat_params(None, None)
    depth = np.full(4, 9, np.uint16)
    eye = np.eye(4, dtype=f32)
    assert lib.hsk_splat_cloud(None, None, None, 0, eye.ctypes.data_as(C.POINTER(C.c_float)), None, depth.ctypes.data, None) == -1 and (depth == 9).all()
    assert lib.hsk_import_cloud(None, None, None, 0, None, 0, None, None) == -1
    assert callable(hsk.KinfuTracker.splat_cloud) and callable(hsk.KinfuTracker.import_cloud) and callable(house.import_room)
