"""The clouds, viewpoints and parameters of the cloud normals' tests, shared by the host test (tests/test_normals_host.py: the harness
against the twin) and the device test (tests/test_gpu_normals.py: hsk_estimate_normals against the twin).  A case is a dict: name,
xyz [n, 3] binary32, viewpoints [v, 3] binary32 or None, params (normals_twin.params).  Where a case is about the grid, its points
are given on the q grid (q / 4096 is exact in binary32 for |q| <= 2^18).  The gather kernel takes one trip over the cloud whatever
its size, so there is no case beyond one pass of its grid."""
import numpy as np

import normals_twin as NT
import splat_cases as SC

f32, f64, i64 = np.float32, np.float64, np.int64
BRUTE_MAX = 3000                                              # the clouds small enough for the twin's all-pairs form


def case(name, xyz, params, viewpoints=None):
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    return dict(name=name, xyz=xyz, params=params, viewpoints=None if viewpoints is None else np.ascontiguousarray(viewpoints, f32).reshape(-1, 3))


def from_q(q):
    return (np.asarray(q, f64).reshape(-1, 3) / 4096.0).astype(f32)


def rq_params(r_q, **kw):
    return NT.params(f32(r_q) / f32(4096.0), **kw)


def jittered_plane(n, seed, spacing=0.02):
    """n points of a tilted plane on a jittered lattice of the spacing given: a few neighbours each, none coincident"""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(np.sqrt(max(n, 1))))
    a, b = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    ab = (np.stack([a, b], -1).reshape(-1, 2)[:n] + rng.uniform(-0.3, 0.3, (n, 2))) * spacing
    return np.stack([0.5 + ab[:, 0], -0.2 + ab[:, 1], 1.0 + 0.4 * ab[:, 0] - 0.25 * ab[:, 1]], 1)


def count_cases():
    """the point counts around a wave and a block"""
    return [case(f"{n} points", jittered_plane(n, 100 + n), NT.params(0.05, min_neighbours=3)) for n in (0, 1, 2, 3, 63, 64, 65, 257)]


R9 = 9                                                        # 81 = 9^2 = 4^2 + 4^2 + 7^2; 82 = 9^2 + 1 = 3^2 + 3^2 + 8^2
ON_BOUNDARY = [(9, 0, 0), (-9, 0, 0), (0, 9, 0), (0, -9, 0), (0, 0, 9), (0, 0, -9), (4, 4, 7), (-4, 7, -4)]
PAST_BOUNDARY = [(9, 1, 0), (0, -9, 1), (1, 0, 9), (3, 3, 8), (-8, 3, -3)]


def boundary_cases():
    """neighbours of the first point at exactly r_q^2 and at r_q^2 + 1, on each axis and on a diagonal"""
    c = np.array([1234, -777, 4001], i64)
    return [case("neighbours at exactly the radius", from_q([c] + [c + np.array(d) for d in ON_BOUNDARY]), rq_params(R9, min_neighbours=3)),
            case("neighbours one step past the radius", from_q([c] + [c + np.array(d) for d in PAST_BOUNDARY]), rq_params(R9, min_neighbours=3))]


def class_cases():
    out = []
    five = from_q([(0, 0, 0), (30, 0, 0), (0, 30, 0), (30, 30, 2), (15, 14, 1)])
    out.append(case("duplicated points", np.repeat(five, 3, axis=0), rq_params(64, min_neighbours=3)))
    g = np.arange(16) * 40                                     # r_q = 20: a point per cell, two radii apart
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) - 300
    out.append(case("4096 points, each in a cell of its own", from_q(lattice), rq_params(20)))
    rng = np.random.default_rng(17)
    blob = rng.integers(0, 200, (300, 3))                      # q + 2^18 in [256 * 1024, 256 * 1024 + 200): one cell at r_q = 1024
    out.append(case("300 points in one cell", from_q(blob), rq_params(1024, max_neighbours=512)))
    out.append(case("300 points in one cell, 64 allowed", from_q(blob), rq_params(1024, max_neighbours=64)))
    out.append(case("a collinear run", from_q(np.arange(20)[:, None] * np.array([1, 2, 3]) + 50), rq_params(40, min_neighbours=3)))
    out.append(case("three coincident points", from_q([(5, 6, 7)] * 3), rq_params(8, min_neighbours=3)))
    patch = jittered_plane(40, 5)
    bad = np.array([[np.nan, 0.5, 1.0], [0.5, np.inf, 1.0], [0.5, 0.5, -np.inf], [np.nextafter(f32(64), f32(65)), 0, 0], [0, -64.5, 0], [0, 0, 1e30]])
    mixed = np.concatenate([patch[:20], bad, patch[20:]])
    out.append(case("NaN, Inf and points out of reach among valid ones", mixed, NT.params(0.05, min_neighbours=3)))
    out.append(case("no valid point", bad, NT.params(0.05, min_neighbours=3)))
    return out


def cell_cases():
    out = []
    # r_q = 16, a point in the middle of its cell (q = 8: (q + 2^18) % 16 = 8): offsets -9, 0, +8 reach the cells below, its own and above
    p = np.array([8, 8, 8], i64)
    offs = np.stack(np.meshgrid([-9, 0, 8], [-9, 0, 8], [-9, 0, 8], indexing="ij"), -1).reshape(-1, 3)
    # ... and a point at its cell's lowest corner (q = 4000 = 250 * 16), neighbours in the eight cells that meet there
    c = np.array([4000, 4000, 4000], i64)
    corner = np.stack(np.meshgrid([-1, 0], [-1, 0], [-1, 0], indexing="ij"), -1).reshape(-1, 3)
    out.append(case("neighbours in all 27 cells, and round a cell's corner", from_q(np.concatenate([p + offs, c + corner])), rq_params(16, min_neighbours=3)))
    # +-64 m on every axis at r_q = 4: the largest cell coordinate (2^17), negative q, the key's top bits; a 3 x 3 patch inwards each
    pts = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                far = np.array([sx, sy, sz], i64) * (1 << 18)
                for a in range(3):
                    for b in range(3):
                        pts.append(far - np.array([sx * a, sy * b, 0], i64))
    out.append(case("coordinates at +-64 m, r_q = 4", from_q(pts), rq_params(4, min_neighbours=3)))
    a, b = np.meshgrid(np.arange(30) * 82, np.arange(30) * 82, indexing="ij")         # 2 cm spacing over 0.6 m
    wide = np.stack([a.reshape(-1) - 900, b.reshape(-1) + 300, (a.reshape(-1) // 4) + (b.reshape(-1) // 8)], 1)
    out.append(case("r_q = 1024", from_q(wide), rq_params(1024)))
    return out


def flat_patch():
    """a 9 x 9 patch of the plane z = 1 (its normal is exactly (0, 0, 1): the matrix has no z in it)"""
    a, b = np.meshgrid(np.arange(9) * 40, np.arange(9) * 40, indexing="ij")
    return from_q(np.stack([a.reshape(-1), b.reshape(-1), np.full(81, 4096)], 1))


def sphere(n=2000, radius=0.5, centre=(0.3, -0.2, 1.5)):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1) * radius + np.array(centre)


SPHERE_CENTRE = (0.3, -0.2, 1.5)


def orientation_cases():
    p = rq_params(100, min_neighbours=3)
    flat = flat_patch()
    mid = [160.0 / 4096.0, 160.0 / 4096.0]
    rng = np.random.default_rng(23)
    return [case("a flat patch, no viewpoint", flat, p),
            case("a flat patch, one viewpoint below", flat, p, [mid + [0.0]]),
            case("a flat patch, a viewpoint in the tangent plane", flat, p, [[2.0, -1.0, 1.0]]),
            case("a flat patch, two equidistant viewpoints", flat, p, [mid + [0.0], mid + [2.0]]),
            case("a sphere, 256 viewpoints", sphere(), NT.params(0.12), rng.uniform(-2.0, 3.0, (256, 3)))]


def oblique_plane():
    """splat_cases' oblique plane (30 degrees, 40 mm spacing) -> (points, its unit normal facing the camera at the origin)"""
    return SC.plane_grid(SC.OBLIQUE_S, SC.OBLIQUE_DEG, 0.0, SC.OBLIQUE_Z0, 3.2)


def box_corner(k=16, s=0.02):
    """the three faces of a box that meet at (1, 1, 1), k x k points of spacing s each, the shared edges and corner once per face"""
    a, b = np.meshgrid(np.arange(k) * s, np.arange(k) * s, indexing="ij")
    a, b, o = a.reshape(-1), b.reshape(-1), np.zeros(k * k)
    return np.concatenate([np.stack([a, b, o], 1), np.stack([a, o, b], 1), np.stack([o, a, b], 1)]) + 1.0


def thin_wall():
    """two 21 x 21 grids of 1 cm spacing 3 cm apart -> (points, face [n]: 0 at x = 1, 1 at x = 1.03)"""
    u, v = np.meshgrid(np.arange(21) * 0.01 + 0.2, np.arange(21) * 0.01 + 0.1, indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    pts = np.concatenate([np.stack([np.full(441, 1.0), v, u], 1), np.stack([np.full(441, 1.03), v, u], 1)])
    return pts, np.repeat([0, 1], 441)


WALL_VIEWPOINTS = [[-0.5, 0.2, 0.3], [2.53, 0.2, 0.3]]        # 1.5 m to either side of the wall


def shape_cases():
    pts, _ = oblique_plane()
    return [case("the oblique plane", pts, NT.params(3.0 * SC.OBLIQUE_S), [[0.0, 0.0, 0.0]]),
            case("a sphere seen from its centre", sphere(), NT.params(0.12), [SPHERE_CENTRE]),
            case("a box corner", box_corner(), NT.params(0.06)),
            case("a thin wall", thin_wall()[0], NT.params(0.02, min_neighbours=5), WALL_VIEWPOINTS),
            case("6000 random points", SC.random_cloud(6000, 11)[0], NT.params(0.25))]


def all_cases():
    return count_cases() + boundary_cases() + class_cases() + cell_cases() + orientation_cases() + shape_cases()


def twin(c):
    """the twin's result; on a cloud small enough both of its forms, asserted equal"""
    out = NT.estimate(c["xyz"], c["viewpoints"], c["params"])
    if len(c["xyz"]) <= BRUTE_MAX:
        other = NT.estimate(c["xyz"], c["viewpoints"], c["params"], form="brute")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:4], other[:4])) and out[4] == other[4], c["name"]
    return out


def write_harness_input(path, c):
    p, vp = c["params"], c["viewpoints"]
    with open(path, "wb") as f:
        for part in (np.array([len(c["xyz"]), 0 if vp is None else len(vp), p["min_neighbours"], p["max_neighbours"]], np.uint32),
                     np.array([p["radius_m"], p["line_rel"]], f32), c["xyz"], vp if vp is not None else np.zeros(0, f32)):
            f.write(np.ascontiguousarray(part).tobytes())


def read_harness_output(path, n):
    raw = np.fromfile(path, np.uint8)
    assert len(raw) == n * 21 + 32
    cuts = np.cumsum([0, 12 * n, 4 * n, 4 * n, n])
    normals, curv, counts, cls = (raw[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:]))     # (copies: aligned whatever n is)
    tail = raw[cuts[-1]:].copy()
    st = dict(zip(NT.STATS[:6], tail[:24].view(np.uint32).tolist()), n_pairs=int(tail[24:].view(np.uint64)[0]))
    return normals.view(f32).reshape(n, 3), curv.view(f32), counts.view(np.uint32), cls, st
