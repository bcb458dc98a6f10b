"""The clouds, cameras and parameters of the cloud import's tests, shared by the host test (tests/test_splat_host.py: the harness
against the twin) and the device test (tests/test_gpu_splat.py: hsk_splat_cloud against the twin).  A case is a dict: name, cam
(a key of CAMS), params (splat_twin.params), pose [4, 4] binary32, xyz [n, 3] binary32 in world coordinates, normals [n, 3] or None."""
import numpy as np

import reloc_twin as RT
import splat_twin as ST

f32, f64 = np.float32, np.float64

# 68 x 52: a multiple of 4 and of neither 8 nor 16; 640 x 480: the sensor's
CAMS = {"68x52": ST.camera(68, 52, 60.0, 60.0, 33.5, 25.5), "64x48": ST.camera(64, 48, 52.5, 52.5, 31.5, 23.5),
        "640x480": ST.camera(640, 480, 525.0, 525.0, 319.5, 239.5)}
EYE = np.eye(4, dtype=f32)
OBLIQUE = RT.look_at((0.4, 2.1, 0.3), (1.6, 1.2, 2.0)).astype(f32)      # a general rigid pose: no zero in its rotation
GRID_PASS = 1024 * 256                                                    # the points one pass of k_splat_points' grid covers


def at_pixel(cam, u, v, z):
    """the camera point that projects to (u, v) at depth z"""
    return [(f64(u) - f64(cam["cx"])) / f64(cam["fx"]) * z, (f64(v) - f64(cam["cy"])) / f64(cam["fy"]) * z, z]


def case(name, cam, params, pose, xyz, normals=None):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    return dict(name=name, cam=cam, params=params, pose=np.asarray(pose, f32).reshape(4, 4), xyz=xyz,
                normals=None if normals is None else np.ascontiguousarray(normals, f32).reshape(-1, 3))


def to_world(pose, pts):
    m = np.asarray(pose, f64)
    return (np.asarray(pts, f64).reshape(-1, 3) @ m[:3, :3].T + m[:3, 3]).astype(f32)


def random_cloud(n, seed, pose=OBLIQUE):
    """n points in a box around the view's frustum, a few of them behind the camera, beside the image or not finite"""
    rng = np.random.default_rng(seed)
    pc = np.stack([rng.uniform(-1.6, 1.6, n), rng.uniform(-1.3, 1.3, n), rng.uniform(-0.5, 3.0, n)], 1)
    xyz = to_world(pose, pc)
    if n >= 16:
        xyz[rng.integers(0, n, n // 16), rng.integers(0, 3, n // 16)] = rng.choice([np.nan, np.inf, -np.inf], n // 16)
    nrm = rng.normal(size=(n, 3)).astype(f32)
    if n >= 16:
        nrm[rng.integers(0, n, n // 16)] = 0
        nrm[rng.integers(0, n, n // 16), 1] = np.nan
    return xyz, nrm


def count_cases(cam="68x52"):
    """the point counts around a wave, a block, and beyond one pass of the grid"""
    out = []
    for n in (0, 1, 63, 64, 65, 257):
        xyz, nrm = random_cloud(n, 100 + n)
        out.append(case(f"{n} points, disc", cam, ST.params(0.05), OBLIQUE, xyz))
        out.append(case(f"{n} points, surfel", cam, ST.params(0.05, mode=ST.SURFEL), OBLIQUE, xyz, nrm))
    return out


def many_points_case():
    n = GRID_PASS + 333
    xyz, nrm = random_cloud(n, 7)
    return case(f"{n} points: beyond one pass of the grid", "64x48", ST.params(0.004, mode=ST.SURFEL, max_half_px=1.0), OBLIQUE, xyz, nrm)


def geometry_cases(cam="68x52"):
    c = CAMS[cam]
    w, h = c["width"], c["height"]
    um, vm = w // 2, h // 2
    p = ST.params(0.05)                                       # at z = 1 a half-width of fx 0.0375: 2.25 px (60), 1.97 px (52.5)
    ru = float(c["fx"]) * 0.0375
    out = []
    border = [(0.3, vm), (w - 0.7, vm), (um, 0.3), (um, h - 0.7), (0.3, 0.3), (w - 0.7, 0.3), (0.3, h - 0.7), (w - 0.7, h - 0.7)]
    out.append(case("footprints clipped by each border and corner", cam, p, EYE, [at_pixel(c, u, v, 1.0) for u, v in border]))
    # u0 + ru = -0.5: the last pixel covered is -1 -- a miss by one pixel; u0 + ru = 0.5: pixel 0 is covered; likewise on every side
    miss = [(-0.5 - ru, vm), (w - 0.5 + ru, vm), (um, -0.5 - ru), (um, h - 0.5 + ru)]
    touch = [(0.5 - ru, vm), (w - 1.5 + ru, vm), (um, 0.5 - ru), (um, h - 1.5 + ru)]
    out.append(case("footprints that miss the image by one pixel, and their neighbours that do not", cam, p, EYE,
                    [at_pixel(c, u, v, 1.0) for u, v in miss + touch]))
    out.append(case("half-widths at both clamps", cam, p, EYE, [at_pixel(c, um - 10, vm, 7.0), at_pixel(c, um + 10, vm, 0.15)]))
    near, far = f32(0.1), f32(8.0)
    out.append(case("z at near_m and far_m, and one step outside", cam, p, EYE,
                    [[0, 0, near], [2.0, 0, far], [0, 0.01, np.nextafter(near, f32(0))], [0, 0.5, np.nextafter(far, f32(9))]]))
    edge = f32(65.535)
    out.append(case("z_mm = 65535", cam, ST.params(0.05, far_m=65.535), EYE, [[0, 0, edge], [3, 0, f32(65.5346)], [0, 3, np.nextafter(edge, f32(70))]]))
    out.append(case("points behind the camera and in its plane", cam, p, EYE, [[0, 0, -1.0], [0.1, 0.1, 0.0], [0, 0, -0.0], [0, 0, 1.0]]))
    bad = [[v if k == a else 0.5 for k in range(3)] for a in range(3) for v in (np.nan, np.inf, -np.inf)]
    out.append(case("NaN and Inf coordinates", cam, p, EYE, bad + [[0, 0, 1.0]]))
    rng = np.random.default_rng(3)
    one = [at_pixel(c, um + 0.1, vm - 0.2, z) for z in rng.uniform(1.0, 2.0, 4096)]
    out.append(case("4096 points on one pixel", cam, ST.params(0.0005), EYE, one))
    out.append(case("equal z_mm on one pixel", cam, ST.params(0.0005), EYE, [at_pixel(c, um, vm, 1.0001), at_pixel(c, um, vm, 1.0002), at_pixel(c, um, vm, 0.9998)]))
    a, b = at_pixel(c, um, vm, 1.0), at_pixel(c, um + 3, vm + 3, 2.0)
    out.append(case("near before far", cam, p, EYE, [a, b]))
    out.append(case("far before near", cam, p, EYE, [b, a]))
    s = ST.params(0.05, mode=ST.SURFEL)
    q = at_pixel(c, um, vm, 1.0)
    out.append(case("surfel: grazing normals reach the clamp", cam, s, EYE, [q, at_pixel(c, um + 12, vm, 1.0)], [[1.0, 0.0, -0.01], [-1.0, 0.0, -0.01]]))
    out.append(case("surfel: back-facing points", cam, s, EYE, [q, at_pixel(c, um + 12, vm, 1.0), at_pixel(c, um - 12, vm, 1.0)],
                    [[0, 0, 1.0], [0.3, 0.1, -1.0], [-1.0, 0.0, 0.0]]))
    out.append(case("surfel: zero and NaN normals are disc points", cam, s, EYE, [q, at_pixel(c, um + 12, vm, 1.0), at_pixel(c, um - 12, vm, 1.0)],
                    [[0, 0, 0], [np.nan, 0, -1.0], [0, np.inf, -1.0]]))
    out.append(case("surfel: one disc and one surfel offer on a pixel", cam, s, EYE, [q, at_pixel(c, um + 2, vm, 0.98)], [[0, 0, 0], [0.5, 0.0, -1.0]]))
    out.append(case("surfel without normals given to a disc call", cam, p, EYE, [q], [[0.5, 0.0, -1.0]]))
    return out


def plane_grid(s, tilt_deg, spin_deg, z0, extent):
    """a regular grid of spacing s on the plane through (0, 0, z0) whose normal is tilted by tilt_deg from the view axis (about the
    image's y axis), the grid turned by spin_deg in the plane -> (camera points [n, 3], the unit normal facing the camera)"""
    k = int(np.ceil(extent / s))
    a, b = np.meshgrid(np.arange(-k, k + 1) * s, np.arange(-k, k + 1) * s, indexing="ij")
    cs, sn = np.cos(np.radians(spin_deg)), np.sin(np.radians(spin_deg))
    a, b = cs * a - sn * b, sn * a + cs * b
    ct, st = np.cos(np.radians(tilt_deg)), np.sin(np.radians(tilt_deg))
    pts = np.stack([a * ct, b, z0 + a * st], -1).reshape(-1, 3)
    return pts, np.array([st, 0.0, -ct])


WATER_Z, WATER_S = 1.5, 0.05
OBLIQUE_Z0, OBLIQUE_S, OBLIQUE_DEG = 1.5, 0.04, 30.0


def watertight_cases(cam="68x52"):
    """a fronto-parallel grid of spacing s filling the view at depth z, as it lies and turned by 30 degrees in its plane; DISC,
    point_size_m = s, the default cover"""
    out = []
    for spin in (0.0, 30.0):
        pts, _ = plane_grid(WATER_S, 0.0, spin, WATER_Z, 2.0)
        out.append(case(f"watertight grid turned by {spin:g} degrees", cam, ST.params(WATER_S), EYE, pts))
    return out


def oblique_cases(cam="68x52"):
    """a plane tilted by 30 degrees against the image plane, as a grid of spacing s with its normals: SURFEL and DISC"""
    pts, n = plane_grid(OBLIQUE_S, OBLIQUE_DEG, 0.0, OBLIQUE_Z0, 3.2)
    nrm = np.tile(n, (len(pts), 1))
    return [case("oblique plane, surfel", cam, ST.params(OBLIQUE_S, mode=ST.SURFEL), EYE, pts, nrm),
            case("oblique plane, disc", cam, ST.params(OBLIQUE_S), EYE, pts, nrm)]


def oblique_depth(cam):
    """the analytic depth of the oblique plane along every pixel's ray, in metres [h, w]: z = z0 / (1 - rx tan(tilt))"""
    c = CAMS[cam]
    rx = (np.arange(c["width"], dtype=f64) - f64(c["cx"])) / f64(c["fx"])
    z = OBLIQUE_Z0 / (1.0 - rx * np.tan(np.radians(OBLIQUE_DEG)))
    return np.tile(z, (c["height"], 1))


def room_case(cam="640x480"):
    xyz, nrm = random_cloud(6000, 11)
    return case("6000 points at the sensor's resolution", cam, ST.params(0.03, mode=ST.SURFEL), OBLIQUE, xyz, nrm)


def all_cases():
    return (count_cases() + geometry_cases("68x52") + geometry_cases("64x48") + watertight_cases() + oblique_cases() + [room_case(), many_points_case()])


def write_harness_input(path, c):
    cam, p = CAMS[c["cam"]], c["params"]
    with open(path, "wb") as f:
        for part in (np.array([cam["width"], cam["height"], p["mode"], 0 if c["normals"] is None else 1], np.int32),
                     np.array([cam[k] for k in ("fx", "fy", "cx", "cy")] + [p[k] for k in ("point_size_m", "cover", "min_half_px", "max_half_px", "near_m", "far_m")], f32),
                     c["pose"], np.uint32(len(c["xyz"])), c["xyz"], c["normals"] if c["normals"] is not None else np.zeros(0, f32)):
            f.write(np.ascontiguousarray(part).tobytes())


def read_harness_output(path, c):
    cam = CAMS[c["cam"]]
    raw = np.fromfile(path, np.uint8)
    px = cam["width"] * cam["height"]
    assert len(raw) == px * 2 + 24
    return raw[:px * 2].view(np.uint16).reshape(cam["height"], cam["width"]), dict(zip(ST.STATS, raw[px * 2:].view(np.uint32).tolist()))


def twin(c):
    return ST.splat(c["xyz"], c["normals"], c["pose"], CAMS[c["cam"]], c["params"])
