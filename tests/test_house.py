"""Host-side room stitching (include/hshouse.h; SURVEY.md 8f-2, BASELINE configs[0]) -- CPU only.

The reference records NO expected outputs for this chain: its pins are inputs (corner tables,
tests/golden/room_corners.json), one property (cuboidFromParams identity, FitCuboidBFGS.hs:134-140, tolerance
1e-6), the self-test acceptance `err <= 1` (FitCuboidBFGS.hs:278), the 4-corners-per-face assertion with the
1e-4 plane tolerance (Main.hs:1881-1882) and `proj == proj2` (Main.hs:2637).  Those are what is checked here,
next to independent numpy restatements of each numeric piece.
"""
import json
import os

import numpy as np
import pytest

from kit import ROOT

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "room_corners.json")))


@pytest.fixture(scope="module")
def H(hsk):
    from housescan_amd import house
    return house


# ---------------------------------------------------------------------------------------------------- numpy twins
def quat_matrix(q):
    """standard (column-vector) rotation of a scalar-first quaternion, normalised first"""
    a, b, c, d = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def cuboid_twin(p, rotate_around=False):
    x, y, z, a, b, c = p[:6]
    R = quat_matrix(p[6:])
    local = np.array([[sx * a / 2, sy * b / 2, sz * c / 2] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    ctr = np.array([x, y, z])
    if rotate_around:  # cuboidFromParamsRotateAround: spawn at the centre, rotate about it
        return ((local + ctr) - ctr) @ R.T + ctr
    return local @ R.T + ctr


def rodrigues(axis, angle):
    k = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def nm_twin(f, start, steps, eps, maxit):
    """GSL multimin nmsimplex2 driven like hmatrix-gsl's minimize (size test after every iteration); the centre and
    the squared size are carried incrementally, as GSL does, so the comparison can be exact"""
    n = len(start)
    P = n + 1
    x = np.tile(np.asarray(start, float), (P, 1))
    for i in range(n):
        x[i + 1, i] = start[i] + steps[i]
    y = np.array([f(r) for r in x])
    state = {}

    def full_center():
        state["c"] = np.array([sum(x[i, j] for i in range(P)) / P for j in range(n)])

    def full_size():
        ss = 0.0
        for i in range(P):
            t = 0.0
            for j in range(n):
                t += (x[i, j] - state["c"][j]) ** 2
            ss += np.sqrt(t) ** 2
        state["S2"] = ss / P

    def trial(coeff, corner):
        xc = (1 - coeff) * P / (P - 1.0) * state["c"] + (P * coeff - 1.0) / (P - 1.0) * x[corner]
        return xc, f(xc)

    def replace(i, xn, val):
        d2 = xmcd = 0.0
        for j in range(n):
            delta = xn[j] - x[i, j]
            d2 += delta * delta
            xmcd += (x[i, j] - state["c"][j]) * delta
        d = np.sqrt(d2)
        state["S2"] += (2.0 / P) * xmcd + ((P - 1.0) / P) * (d * d / P)
        a = 1.0 / P
        state["c"] = (state["c"] - a * x[i]) + a * xn
        x[i], y[i] = xn, val

    full_center()
    full_size()
    it = 0
    while it < maxit:
        it += 1
        hi, lo = 0, 0
        dhi = dlo = y[0]
        dshi = y[1]
        for i in range(1, P):
            if y[i] < dlo:
                dlo, lo = y[i], i
            elif y[i] > dhi:
                dshi, dhi, hi = dhi, y[i], i
            elif y[i] > dshi:
                dshi = y[i]
        xc, val = trial(-1.0, hi)
        if np.isfinite(val) and val < dlo:
            xc2, val2 = trial(-2.0, hi)
            if np.isfinite(val2) and val2 < dlo:
                replace(hi, xc2, val2)
            else:
                replace(hi, xc, val)
        elif not np.isfinite(val) or val > dshi:
            if np.isfinite(val) and val <= dhi:
                replace(hi, xc, val)
            xc2, val2 = trial(0.5, hi)
            if np.isfinite(val2) and val2 <= dhi:
                replace(hi, xc2, val2)
            else:
                for i in range(P):
                    if i != lo:
                        x[i] = 0.5 * (x[i] + x[lo])
                        y[i] = f(x[i])
                full_center()
                full_size()
        else:
            replace(hi, xc, val)
        if state["S2"] <= 0:
            full_size()
        if np.sqrt(state["S2"]) < eps:
            break
    k = int(np.argmin(y))
    return x[k], y[k], it


def box_room(dims, n_per_face=400, seed=0):
    """an axis-aligned box room centred on the origin: (cloud, planes in PCL form, hull polygons)"""
    rng = np.random.default_rng(seed)
    a, b, c = dims
    half = np.array([a, b, c]) / 2
    cloud, planes, hulls = [], [], []
    for axis in range(3):
        for s in (-1, 1):
            u, v = [i for i in range(3) if i != axis]
            pts = np.zeros((n_per_face, 3))
            pts[:, axis] = s * half[axis]
            pts[:, u] = rng.uniform(-half[u], half[u], n_per_face)
            pts[:, v] = rng.uniform(-half[v], half[v], n_per_face)
            cloud.append(pts)
            nrm = np.zeros(3)
            nrm[axis] = 1.0
            planes.append([*nrm, -s * half[axis]])   # n.x + d = 0 on the face
            poly = np.zeros((4, 3))
            poly[:, axis] = s * half[axis]
            poly[:, u] = [-half[u], half[u], half[u], -half[u]]
            poly[:, v] = [-half[v], -half[v], half[v], half[v]]
            hulls.append(poly)
    return np.concatenate(cloud), np.array(planes), hulls


def moved(cloud, planes, hulls, R, t):
    """apply p' = R p + t to a room description (planes stay in PCL form)"""
    c2 = cloud @ R.T + t
    h2 = [h @ R.T + t for h in hulls]
    p2 = []
    for a, b, c, d in planes:
        n2 = R @ np.array([a, b, c])
        p2.append([*n2, d - n2 @ t])
    return c2, np.array(p2), h2


# ---------------------------------------------------------------------------------------------------------- tests
def test_cuboid_from_params_matches_twin_and_identity_property(H):
    """FitCuboidBFGS.hs:134-140: spawning at the origin then translating == spawning at the centre and rotating
    about it, to 1e-6 summed over the corners"""
    rng = np.random.default_rng(1)
    for _ in range(200):
        p = np.concatenate([rng.uniform(-50, 50, 3), rng.uniform(-20, 20, 3), rng.uniform(-3, 3, 4)])
        if abs(p[6:].sum()) == 0:
            continue
        got = H.cuboid_from_params(p)
        assert np.abs(got - cuboid_twin(p)).max() < 1e-10
        assert np.linalg.norm(got - cuboid_twin(p, rotate_around=True), axis=1).sum() < 1e-6


def test_cuboid_corner_order_and_quaternion_convention(H):
    # identity quaternion (scalar FIRST): corners in the order ---, --+, -+-, -++, +--, +-+, ++-, +++
    c = H.cuboid_from_params([1, 2, 3, 2, 4, 6, 1, 0, 0, 0])
    want = np.array([[sx, 2 * sy, 3 * sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], float) + [1, 2, 3]
    assert np.array_equal(c, want)
    # 90 degrees about z, unnormalised: (x, y) -> (-y, x)
    c = H.cuboid_from_params([0, 0, 0, 2, 4, 6, 3, 0, 0, 3])
    assert np.allclose(c[7], [-2, 1, 3], atol=1e-12)


def test_guess_dims_and_errfuns(H):
    p = np.array([0.3, -0.2, 0.1, 2.0, 3.0, 4.0, 0.9, 0.1, -0.2, 0.3])
    c = H.cuboid_from_params(p)
    assert np.allclose(H.guess_dims(c), [2, 3, 4], atol=1e-12)
    assert H.errfun(c, p) < 1e-24 and H.errfun(c, p, closest=True) < 1e-24
    shuffled = c[[3, 1, 7, 0, 2, 6, 5, 4]]
    assert H.errfun(shuffled, p, closest=True) < 1e-24 and H.errfun(shuffled, p) > 1.0
    q = p.copy()
    q[0] += 0.5
    assert abs(H.errfun(c, q) - 8 * 0.25) < 1e-12


def test_nelder_mead_matches_twin_iteration_for_iteration(H):
    def rosen(x):
        return float(100 * (x[1] - x[0] ** 2) ** 2 + (1 - x[0]) ** 2)

    for maxit in (1, 2, 5, 17, 60, 400):
        x, fv, it = H.nm_minimize(rosen, [-1.2, 1.0], [0.5, 0.5], eps=1e-10, maxit=maxit)
        xt, ft, itt = nm_twin(rosen, [-1.2, 1.0], [0.5, 0.5], 1e-10, maxit)
        assert it == itt
        assert np.array_equal(x, xt) and fv == ft
    x, fv, it = H.nm_minimize(rosen, [-1.2, 1.0], [0.5, 0.5], eps=1e-10, maxit=5000)
    assert np.allclose(x, [1, 1], atol=1e-6) and it < 5000

    def quad5(x):
        return float(np.sum((np.asarray(x) - np.arange(5)) ** 2 * (1 + np.arange(5))))

    x, fv, it = H.nm_minimize(quad5, np.zeros(5), np.ones(5), eps=1e-9, maxit=5000)
    xt, ft, itt = nm_twin(quad5, np.zeros(5), np.ones(5), 1e-9, 5000)
    assert it == itt and np.array_equal(x, xt) and np.allclose(x, np.arange(5), atol=1e-6)


def test_nelder_mead_survives_non_finite_values(H):
    def f(x):
        return float("nan") if x[0] > 2.0 else float((x[0] - 1.5) ** 2 + (x[1] + 0.5) ** 2)

    x, fv, it = H.nm_minimize(f, [0.0, 0.0], [3.0, 1.0], eps=1e-9, maxit=2000)
    assert np.allclose(x, [1.5, -0.5], atol=1e-6)


@pytest.mark.parametrize("arg_order", [0, 1])
def test_fit_recovers_random_cuboids_reference_acceptance(H, arg_order):
    """the reference's own smoke test (FitCuboidBFGS.hs:266-282): random a,b,c in [1,10], random rotation, corner at
    the origin; it flags err > 1.  Closest-corner association can stall in a local minimum, so -- like the reference,
    which only prints -- require the bulk to pass, and every pass to be a real fit."""
    rng = np.random.default_rng(7)
    good = 0
    trials = 60
    for _ in range(trials):
        a, b, c = rng.uniform(1, 10, 3)
        pts = np.array([[x, y, z] for x in (0, a) for y in (0, b) for z in (0, c)])
        R = rodrigues(rng.uniform(0, 3, 3) + 1e-3, np.radians(rng.uniform(0, 360)))
        pts = pts @ R.T
        p, steps, err = H.fit_cuboid(pts, H.FIT_FROM_CENTER, arg_order)
        assert steps <= 2000 and np.isfinite(err)
        good += err <= 1.0
        if err < 1e-6:
            assert np.allclose(sorted(np.abs(p[3:6])), sorted([a, b, c]), atol=1e-2)
    # measured over 200 draws: 0.56 (as named) / 0.71 (as passed) of the fits pass the reference's err <= 1
    assert good >= (0.4, 0.55)[arg_order] * trials, good


def test_fit_two_stage_on_the_reference_corner_tables(H):
    """Main.hs:2346-2413 and :2531-2540 (hand-clicked, noisy corners of real rooms): the two-stage fit ends with a
    room-sized box whose RMSE is far below the room size; stage 2 never makes stage 1 worse"""
    rooms = dict(FIXTURE["dev_rooms_mean_relative"])
    rooms["test_room1"] = FIXTURE["test_room1_absolute"]
    for name, corners in rooms.items():
        c = np.array(corners, np.float32).astype(np.float64)
        p1, s1, e1 = H.fit_cuboid(c, H.FIT_FROM_CENTER, H.FIT_AS_PASSED)
        p, steps, err = H.fit_cuboid(c, H.FIT_FROM_CENTER_FIRST, H.FIT_AS_PASSED)
        assert steps >= s1 and steps <= 4000
        assert err <= e1 + 1e-9, name
        assert np.sqrt(err) < 0.6, (name, np.sqrt(err))
        assert np.all(np.abs(p[3:6]) > 0.7) and np.all(np.abs(p[3:6]) < 6.0), (name, p[3:6])
        assert np.linalg.norm(p[:3] - c.mean(axis=0)) < 0.5


def test_example_cuboid_ordered_fit(H):
    """FitCuboidBFGS.hs:29-41, :255-268: the 2x1x1 example rotated 20 degrees about (1,2,3), ordered association"""
    ex = FIXTURE["example_cuboid"]
    pts = np.array(ex["unrotated"], float) @ rodrigues(ex["axis"], np.radians(ex["degrees"])).T
    for order in (0, 1):
        p, steps, err = H.fit_cuboid(pts, H.FIT_ORDERED, order)
        assert np.isfinite(err) and steps <= 2000
    p, steps, err = H.fit_cuboid(pts, H.FIT_ORDERED, H.FIT_AS_NAMED)
    assert err < 1e-6 and np.allclose(np.abs(p[3:6]), [2, 1, 1], atol=1e-3)


def test_plane_corner(H):
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = rng.normal(size=(3, 3))
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        d = rng.uniform(-3, 3, 3)
        eq = np.concatenate([n, d[:, None]], axis=1).astype(np.float32)
        got = H.plane_corner(*eq)
        want = np.linalg.solve(eq[:, :3].astype(np.float64), eq[:, 3].astype(np.float64)).astype(np.float32)
        assert got is not None and np.array_equal(got, want) or np.allclose(got, want, rtol=2e-6, atol=2e-6)
    assert H.plane_corner([1, 0, 0, 1], [1, 0, 0, 2], [0, 1, 0, 0]) is None          # parallel walls
    assert H.plane_corner([1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3]).tolist() == [1, 2, 3]


def test_fit_plane_total_least_squares(H):
    rng = np.random.default_rng(5)
    n = np.array([0.3, -0.5, 0.81])
    n /= np.linalg.norm(n)
    basis = np.linalg.svd(n[None])[2][1:]
    pts = (rng.uniform(-2, 2, (500, 2)) @ basis) + 0.7 * n + rng.normal(0, 1e-3, (500, 1)) * n
    eq = H.fit_plane(pts)
    assert abs(np.linalg.norm(eq[:3]) - 1) < 1e-6
    assert abs(abs(eq[:3] @ n) - 1) < 1e-5 and abs(abs(eq[3]) - 0.7) < 1e-3
    assert eq[np.argmax(np.abs(eq[:3]))] > 0     # the documented sign choice
    with pytest.raises(H.HouseError):
        H.fit_plane(pts[:2])


def test_rotation_between_normals(H):
    rng = np.random.default_rng(9)
    for _ in range(30):
        a, b = rng.normal(size=3), rng.normal(size=3)
        a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
        R = H.rotation_between(a, b)
        assert np.allclose(a.astype(np.float32) @ R, b, atol=2e-6)            # row vector from the right
        assert np.allclose(R @ R.T, np.eye(3), atol=2e-6) and abs(np.linalg.det(R) - 1) < 1e-5
    assert np.array_equal(H.rotation_between([0, 1, 0], [0, 1, 0]), np.eye(3, dtype=np.float32))
    with pytest.raises(H.HouseError):
        H.rotation_between([0, 1, 0], [0, -1, 0])


def test_lstsq_distances_against_numpy(H):
    # consistent chain 10 -> 20 -> 30, node 0 is the first node of the smallest key
    pos, rmse = H.lstsq_distances({(10, 20): 2.0, (20, 30): 3.0})
    assert list(pos) == [10, 20, 30] and np.allclose(list(pos.values()), [0, 2, 5], atol=1e-12) and rmse < 1e-6
    # inconsistent triangle, with the reference's RMSE = sqrt(||Ax-b||_2 / m)
    d = {(1, 2): 1.0, (2, 3): 1.0, (1, 3): 2.6, (3, 4): -0.5}
    pos, rmse = H.lstsq_distances(d)
    nodes = [1, 2, 3, 4]
    A = np.zeros((len(d), 4))
    b = np.zeros(len(d))
    for r, ((i, j), v) in enumerate(sorted(d.items())):
        A[r, nodes.index(i)], A[r, nodes.index(j)], b[r] = -1, 1, v
    x = np.linalg.lstsq(A[:, 1:], b, rcond=None)[0]
    assert np.allclose([pos[k] for k in nodes], [0, *x], atol=1e-12)
    assert abs(rmse - np.sqrt(np.linalg.norm(A[:, 1:] @ x - b) / len(d))) < 1e-12
    # node numbering follows the SORTED keys, not the insertion order
    pos, _ = H.lstsq_distances({(7, 9): 1.0, (3, 7): 4.0})
    assert list(pos) == [3, 7, 9] and np.allclose(list(pos.values()), [0, 4, 5], atol=1e-12)
    # negative distances, and the reverse key as a separate constraint
    pos, rmse = H.lstsq_distances({(1, 2): -2.0, (2, 1): 2.0})
    assert list(pos) == [1, 2] and np.allclose(list(pos.values()), [0, -2], atol=1e-12) and rmse < 1e-6


def test_group_connected_components(H):
    edges = [((1, 2), "a"), ((5, 6), "b"), ((2, 3), "c"), ((9, 9), "d"), ((6, 7), "e"), ((3, 1), "f")]
    comps = H.group_connected_components(edges)
    assert [sorted(x[1] for x in c) for c in comps] == [["a", "c", "f"], ["b", "e"], ["d"]]
    assert H.group_connected_components([]) == []
    rng = np.random.default_rng(2)
    e = [((int(a), int(b)), k) for k, (a, b) in enumerate(rng.integers(0, 40, (30, 2)))]
    comps = H.group_connected_components(e)
    assert sorted(k for c in comps for _, k in c) == list(range(30))
    seen = []
    for c in comps:        # components are vertex-disjoint and internally connected
        verts = set(v for (a, b), _ in c for v in (a, b))
        assert all(verts.isdisjoint(s) for s in seen)
        seen.append(verts)
        reach, frontier = set(), {next(iter(verts))}
        while frontier:
            reach |= frontier
            frontier = {w for (a, b), _ in c for v, w in ((a, b), (b, a)) if v in reach} - reach
        assert reach == verts


def test_show_float_is_haskell_show(H):
    cases = {1.0: "1.0", 0.1: "0.1", 0.5: "0.5", -3.25: "-3.25", 1.0e-2: "1.0e-2", 5.0e-2: "5.0e-2", 12345678.0: "1.2345678e7",
             1.0e7: "1.0e7", 9999999.0: "9999999.0", 0.0: "0.0", 100.0: "100.0", 6.0: "6.0", 1.5e-5: "1.5e-5",
             -0.80041015: "-0.80041015", 2.601904: "2.601904", 123.456: "123.456", 3.0e10: "3.0e10"}
    for v, s in cases.items():
        assert H.show_float(v) == s, (v, H.show_float(v), s)
    rng = np.random.default_rng(4)
    for v in np.concatenate([rng.normal(0, 10, 200), rng.normal(0, 1e-4, 50), rng.normal(0, 1e9, 50)]).astype(np.float32):
        s = H.show_float(float(v))
        assert np.float32(float(s)) == v                     # round trip
        assert "." in s and not s.endswith(".")


def _oriented_room(house, dims, R, t, seed, name):
    cloud, planes, hulls = box_room(dims, seed=seed)
    c2, p2, h2 = moved(cloud, planes, hulls, R, t)
    return house.add_room(name, c2, p2, h2), c2


def test_load_makes_normals_inward_and_keeps_identity_projection(H):
    hs = H.House()
    cloud, planes, hulls = box_room((4, 2.5, 3))
    flipped = planes.copy()
    flipped[::2] *= -1
    rid = hs.add_room("r", cloud, flipped, hulls)
    ids, eq = hs.room_planes(rid)
    assert len(ids) == 6 and len(set(ids)) == 6
    mean = hs.room_mean(rid)
    for pid, e in zip(ids, eq):
        bm = hs.plane_bounds(pid).mean(axis=0)
        assert (mean - bm) @ e[:3] > 0                       # inward
        assert abs(bm @ e[:3] - e[3]) < 1e-5                 # n.x = d on the wall
    assert np.array_equal(hs.room_projection(rid), np.eye(4, dtype=np.float32))
    assert hs.room_projection_to_string(rid) == ",".join(["1.0" if i % 5 == 0 else "0.0" for i in range(16)])
    hs.close()


def test_projection_tracks_every_rigid_edit(H):
    """projTest (Main.hs:2543-2639): applying the exported 4x4 to the cloud as loaded gives the cloud as shown"""
    hs = H.House()
    R0 = rodrigues([1, 2, 0.5], 0.4)
    rid, original = _oriented_room(hs, (4, 2.5, 3), R0, np.array([1.0, -2.0, 0.5]), 0, "a")
    hs.rotate_kinfu_room(rid)
    hs.auto_align_floor(rid)
    hs.translate_room(rid, [6, 0, -3])
    hs.rotate_room(rid, rodrigues([0, 1, 0], np.pi / 2).T.astype(np.float32))
    hs.room_auto_align_axis(rid, [1, 0, 0])
    M = hs.room_projection(rid).astype(np.float64)
    assert np.allclose(M[3], [0, 0, 0, 1]) and abs(np.linalg.det(M[:3, :3]) - 1) < 1e-5
    want = original @ M[:3, :3].T + M[:3, 3]
    assert np.abs(hs.room_cloud(rid) - want).max() < 2e-5
    # planes moved with the room: every hull vertex still satisfies its plane, normals still inward
    ids, eq = hs.room_planes(rid)
    for pid, e in zip(ids, eq):
        b = hs.plane_bounds(pid)
        assert np.abs(b @ e[:3] - e[3]).max() < 2e-5
        assert (hs.room_mean(rid) - b.mean(axis=0)) @ e[:3] > 0
    # after the two alignments one wall normal is +Y and another +X, to binary32 accuracy
    assert np.abs(eq[:, :3] @ [0, 1, 0]).max() > 1 - 1e-5 and np.abs(eq[:, :3] @ [1, 0, 0]).max() > 1 - 1e-5
    hs.close()


def test_remove_ceiling_keeps_ties_and_rejects_tiny_clouds(H):
    hs = H.House()
    ys = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8], float)     # n/5 = 2: the limit is the 2nd largest y = 8
    cloud = np.stack([np.arange(10.0), ys, np.zeros(10)], axis=1)
    rid = hs.add_room("r", cloud, np.zeros((0, 4)), [])
    hs.remove_ceiling(rid)
    assert len(hs.room_cloud(rid)) == 10                      # both 8s survive (<= limit)
    cloud[:, 1] = np.arange(10.0)
    rid = hs.add_room("r2", cloud, np.zeros((0, 4)), [])
    hs.remove_ceiling(rid)
    assert sorted(hs.room_cloud(rid)[:, 1]) == list(range(9))  # only y = 9 is above the 2nd largest (8)
    rid = hs.add_room("r3", cloud[:4], np.zeros((0, 4)), [])
    with pytest.raises(H.HouseError, match="k must be >= 1"):
        hs.remove_ceiling(rid)
    hs.close()


def test_suggest_points_and_cuboid_fit_replace_planes(H):
    hs = H.House()
    dims = (4.0, 2.5, 3.0)
    R0 = rodrigues([0.2, 1, 0.1], 0.3)
    rid, _ = _oriented_room(hs, dims, R0, np.array([0.5, 0.2, -0.3]), 1, "a")
    n, adopted = hs.suggest_points(rid)
    assert (n, adopted) == (8, True)                           # 20 triples, 12 of them parallel pairs -> 8 corners
    cids, corners = hs.room_corners(rid)
    assert len(cids) == 8 and not hs.room_corners(rid, suggested=True)[0]
    want = cuboid_twin([0, 0, 0, *dims, 1, 0, 0, 0]) @ R0.T + [0.5, 0.2, -0.3]
    for c in corners:
        assert np.linalg.norm(want - c, axis=1).min() < 1e-5
    old_planes, _ = hs.room_planes(rid)
    p, steps, rmse = hs.fit_cuboid_to_room(rid, H.FIT_AS_PASSED)
    assert rmse < 1e-4 and steps <= 4000
    assert np.allclose(sorted(np.abs(p[3:6])), sorted(dims), atol=1e-3)
    new_ids, eq = hs.room_planes(rid)
    assert len(new_ids) == 6 and not set(new_ids) & set(old_planes)
    cids2, corners2 = hs.room_corners(rid)
    assert cids2 == cids                                       # corner ids are re-used (Main.hs:1837)
    for pid, e in zip(new_ids, eq):                            # Main.hs:1881-1882: four corners on every face, 1e-4
        b = hs.plane_bounds(pid)
        assert b.shape == (4, 3) and np.abs(b @ e[:3] - e[3]).max() < 1e-4
        assert sum(np.abs(corners2 @ e[:3] - e[3]) < 1e-4) == 4
        # polygon order: consecutive vertices share an edge (never the face diagonal)
        edges = np.linalg.norm(np.roll(b, -1, axis=0) - b, axis=1)
        assert edges.max() < np.linalg.norm(b[0] - b[2]) - 1e-3
    # second call on a room that already has 8 corners only fills the suggestions
    n, adopted = hs.suggest_points(rid)
    assert n == 8 and not adopted and len(hs.room_corners(rid, suggested=True)[0]) == 8
    hs.close()


def test_argument_order_quirk_for_rooms_centred_on_the_origin(H):
    """AS_PASSED hands stage 1's solution to nmsimplex2 as the STEP SIZES of stage 2 (FitCuboidBFGS.hs:201): when the
    corner mean is ~0 the simplex has no extent along the centre and the centre stays at the literal start 0.01"""
    c = cuboid_twin([0, 0, 0, 4, 2.5, 3, 1, 0, 0, 0]) @ rodrigues([0.2, 1, 0.1], 0.3).T
    p, _, err = H.fit_cuboid(c, H.FIT_FROM_CENTER_FIRST, H.FIT_AS_PASSED)
    assert np.allclose(p[:3], 0.01, atol=1e-6) and abs(err - 8 * 3e-4) < 1e-5
    p, _, err = H.fit_cuboid(c, H.FIT_FROM_CENTER_FIRST, H.FIT_AS_NAMED)
    assert np.allclose(p[:3], 0, atol=1e-6) and err < 1e-10
    p, _, err = H.fit_cuboid(c + [2.0, 1.0, -3.0], H.FIT_FROM_CENTER_FIRST, H.FIT_AS_PASSED)
    assert np.allclose(p[:3], [2, 1, -3], atol=1e-6) and err < 1e-10


def test_fit_needs_exactly_eight_corners(H):
    hs = H.House()
    cloud, planes, hulls = box_room((2, 2, 2))
    rid = hs.add_room("r", cloud, planes, hulls)
    with pytest.raises(H.HouseError, match="need 8"):
        hs.fit_cuboid_to_room(rid)
    hs.set_room_corners(rid, np.zeros((9, 3)))
    with pytest.raises(H.HouseError, match="exactly 8"):
        hs.fit_cuboid_to_room(rid)
    hs.close()


def test_reference_corner_tables_give_four_corners_per_face(H):
    """every hand-clicked corner table of the reference goes through fitCuboidToRoom's face assertion"""
    rooms = dict(FIXTURE["dev_rooms_mean_relative"])
    rooms["test_room1"] = FIXTURE["test_room1_absolute"]
    hs = H.House()
    for name, corners in rooms.items():
        c = np.array(corners, np.float32)
        rid = hs.add_room(name, c, np.zeros((0, 4)), [])
        hs.set_room_corners(rid, c)
        p, steps, rmse = hs.fit_cuboid_to_room(rid, H.FIT_AS_PASSED)
        ids, eq = hs.room_planes(rid)
        assert len(ids) == 6 and rmse < 0.6
        # opposite faces are parallel, adjacent ones orthogonal
        G = np.abs(eq[:, :3] @ eq[:, :3].T)
        assert np.allclose(np.sort(G, axis=1)[:, -2:], 1, atol=1e-5) and np.allclose(np.sort(G, axis=1)[:, :4], 0, atol=1e-5)
    hs.close()


ROOM_A_AT = [0.7, -0.3, 0.4]
ROOM_B_AT = [7.3, 0.4, -0.9]


def _two_room_house(H, gap_axis=0):
    """rooms A (4 x 2.5 x 3) and B (3 x 2.5 x 3), axis aligned, B displaced arbitrarily; returns ids and wall ids"""
    hs = H.House()
    a, _ = _oriented_room(hs, (4, 2.5, 3), np.eye(3), np.array(ROOM_A_AT), 0, "/scan/rooma/cloud_downsampled.pcd")
    b, _ = _oriented_room(hs, (3, 2.5, 3), np.eye(3), np.array(ROOM_B_AT), 1, "/scan/roomb/cloud_downsampled.pcd")
    for r in (a, b):
        assert hs.suggest_points(r) == (8, True)
        hs.fit_cuboid_to_room(r, H.FIT_AS_PASSED)
    return hs, a, b


def _wall(hs, room, axis, sign):
    """the wall of `room` whose mean lies furthest along sign*axis"""
    ids, eq = hs.room_planes(room)
    best = max(ids, key=lambda p: sign * hs.plane_bounds(p).mean(axis=0)[axis])
    return best


def test_connect_walls_guesses_axis_and_refuses_mismatches(H):
    hs, a, b = _two_room_house(H)
    wa, wb = _wall(hs, a, 0, +1), _wall(hs, b, 0, -1)
    assert hs.connect_walls(wa, wb, H.OPPOSITE, 0.1)
    assert not hs.connect_walls(wb, wa, H.OPPOSITE, 0.2)       # the pair is already connected, either order
    assert hs.connected_walls() == [(H.AXIS_X, H.OPPOSITE, pytest.approx(0.1), wa, wb)]
    with pytest.raises(H.HouseError, match="Could not guess axis"):
        hs.connect_walls(_wall(hs, a, 1, +1), _wall(hs, b, 2, +1))
    with pytest.raises(H.HouseError, match="not walls"):
        hs.connect_walls(wa, 99999)
    hs.disconnect_walls(wb, wa)
    assert hs.connected_walls() == []
    # newest connection first; re-fitting a room drops the connections that named its old walls (Main.hs:1843-1847)
    hs.connect_walls(wa, wb, H.OPPOSITE, 0.1)
    hs.connect_walls(_wall(hs, a, 2, +1), _wall(hs, b, 2, +1), H.SAME)
    assert [w[0] for w in hs.connected_walls()] == [H.AXIS_Z, H.AXIS_X]
    hs.fit_cuboid_to_room(b, H.FIT_AS_PASSED)
    assert hs.connected_walls() == []
    hs.close()


def test_optimize_room_positions_two_rooms(H):
    """configs[0]: two rooms, one shared wall (10 cm thick), floors and one side wall flush"""
    hs, a, b = _two_room_house(H)
    before_a = hs.corner_mean(a).copy()
    hs.connect_walls(_wall(hs, a, 0, +1), _wall(hs, b, 0, -1), H.OPPOSITE, 0.1)   # A's +x wall backs B's -x wall
    hs.connect_walls(_wall(hs, a, 1, -1), _wall(hs, b, 1, -1), H.SAME)            # floors level
    hs.connect_walls(_wall(hs, a, 2, -1), _wall(hs, b, 2, -1), H.SAME)            # -z walls flush
    rm = hs.optimize_room_positions()
    assert np.all(rm < 1e-6)
    assert np.allclose(hs.corner_mean(a), before_a, atol=1e-6)                     # the first room stays where it is
    ca, cb = hs.room_corners(a)[1], hs.room_corners(b)[1]
    assert abs((cb[:, 0].min() - ca[:, 0].max()) - 0.1) < 1e-5                     # wall thickness between them
    assert abs(cb[:, 1].min() - ca[:, 1].min()) < 1e-5 and abs(cb[:, 2].min() - ca[:, 2].min()) < 1e-5
    Mb = hs.room_projection(b)
    assert np.allclose(Mb[:3, :3], np.eye(3), atol=1e-6)
    assert np.allclose(Mb[:3, 3], [0.7 + 4 / 2 + 0.1 + 3 / 2 - 7.3, -0.3 - 0.4, 0.4 + 0.9], atol=2e-5)
    # running it again changes nothing (idempotent)
    hs.optimize_room_positions()
    assert np.allclose(hs.room_projection(b), Mb, atol=2e-6)
    hs.close()


def test_optimize_room_positions_overconstrained_ring_and_components(H):
    """three rooms in a row with an inconsistent extra constraint: least squares spreads the error; an unconnected
    pair forms its own component and is solved separately"""
    hs = H.House()
    rooms = []
    for k, x in enumerate([0.0, 5.0, 11.0, 30.0, 41.0]):
        r, _ = _oriented_room(hs, (3, 2.5, 3), np.eye(3), np.array([x, 0.0, 0.0]), k, f"/s/r{k}/walls/c.pcd")
        assert hs.suggest_points(r) == (8, True)
        hs.fit_cuboid_to_room(r, H.FIT_AS_PASSED)
        rooms.append(r)
    r0, r1, r2, r3, r4 = rooms
    hs.connect_walls(_wall(hs, r0, 0, +1), _wall(hs, r1, 0, -1), H.OPPOSITE, 0.1)
    hs.connect_walls(_wall(hs, r1, 0, +1), _wall(hs, r2, 0, -1), H.OPPOSITE, 0.1)
    hs.connect_walls(_wall(hs, r0, 0, -1), _wall(hs, r2, 0, -1), H.SAME)           # contradicts the chain
    hs.connect_walls(_wall(hs, r3, 0, +1), _wall(hs, r4, 0, -1), H.OPPOSITE, 0.2)  # separate component
    rm = hs.optimize_room_positions()
    assert rm[0] > 0.1 and np.isnan(rm[1]) and np.isnan(rm[2])
    x = [hs.corner_mean(r)[0] for r in rooms]
    # expected by numpy: unknowns c1, c2 relative to c0 = 0; rows c1 = 3.1, c2 - c1 = 3.1, c2 = 0
    A = np.array([[1, 0], [-1, 1], [0, 1]], float)
    sol = np.linalg.lstsq(A, np.array([3.1, 3.1, 0.0]), rcond=None)[0]
    # the connections were consed, so the LAST one made is the first listed: its first room is the anchor
    anchor = 30.0
    assert abs((x[4] - x[3]) - 3.2) < 1e-5
    assert np.allclose([x[1] - x[0], x[2] - x[0]], sol, atol=1e-5)
    # reference behaviour (Main.hs:2151-2152): EVERY component's node 0 lands on the first listed room's old centre
    assert abs(x[3] - anchor) < 1e-5 and abs(x[0] - anchor) < 1e-5
    hs.close()


def test_xf_export_round_trip(H, tmp_path):
    from housescan_amd import products as P
    hs, a, b = _two_room_house(H)
    hs.rotate_room(b, rodrigues([0, 1, 0], 0.3).T.astype(np.float32))
    hs.export_all_room_xf_files(str(tmp_path / "xf"))
    assert sorted(os.listdir(tmp_path / "xf")) == ["rooma.xf", "roomb.xf"]      # takeFileName . takeDirectory of the path's dir
    for r, f in ((a, "rooma.xf"), (b, "roomb.xf")):
        text = open(tmp_path / "xf" / f).read()
        assert text == hs.room_projection_to_xf_format(r) and text.count("\n") == 4
        assert np.array_equal(P.read_xf(str(tmp_path / "xf" / f)), hs.room_projection(r))
        csv = hs.room_projection_to_string(r)
        assert np.array_equal(np.array(csv.split(","), np.float32).reshape(4, 4), hs.room_projection(r))
    hs.close()


def test_load_room_directory_written_by_the_products(H, tmp_path):
    """the seam of SURVEY.md 8f-1: a directory produced by products.write_room_dir loads, and the chain runs on it"""
    from housescan_amd import products as P
    rng = np.random.default_rng(0)
    dims = np.array([3.2, 2.4, 2.8])
    # a dense box-room cloud in a KinFu-like frame (tilted, off-centre), like hsk_extract_cloud would give
    cloud, _, _ = box_room(dims, n_per_face=6000, seed=3)
    cloud += rng.normal(0, 0.002, cloud.shape)
    R0 = rodrigues([1, 0.3, 0.2], 0.15)
    cloud = (cloud @ R0.T + [1.5, 1.5, 1.6]).astype(np.float32)
    planes, n_down = P.write_room_dir(str(tmp_path / "room" / "walls"), cloud, leaf=0.05, dist_thresh=0.02, min_fraction=0.05)
    assert len(planes) == 6
    hs = H.House()
    rid = hs.load_room(str(tmp_path / "room" / "walls"))
    assert len(hs.room_cloud(rid)) == n_down
    assert np.array_equal(hs.room_cloud(rid), H.read_pcd_xyz(str(tmp_path / "room" / "walls" / "cloud_downsampled.pcd")))
    hs.rotate_kinfu_room(rid)
    hs.auto_align_floor(rid)
    n, adopted = hs.suggest_points(rid)
    assert (n, adopted) == (8, True)
    p, steps, rmse = hs.fit_cuboid_to_room(rid, H.FIT_AS_PASSED)
    assert rmse < 0.02 and np.allclose(sorted(np.abs(p[3:6])), sorted(dims), atol=0.03)
    # the floor (largest +Y-facing wall after the alignment) is level
    ids, eq = hs.room_planes(rid)
    assert np.abs(eq[:, :3] @ [0, 1, 0]).max() > 0.999
    with pytest.raises(H.HouseError):
        hs.load_room(str(tmp_path / "nowhere"))
    hs.close()


def test_ply_points_round_trip(H, tmp_path):
    pts = np.random.default_rng(0).normal(size=(1000, 3)).astype(np.float32)
    H.write_ply_points(str(tmp_path / "c.ply"), pts)
    head = open(tmp_path / "c.ply", "rb").read(200)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 1000\n")
    assert np.array_equal(H.read_ply_points(str(tmp_path / "c.ply")), pts)


def test_pcd_reader_ascii_and_binary(H, tmp_path):
    from housescan_amd import products as P
    pts = np.random.default_rng(1).normal(size=(257, 3)).astype(np.float32)
    P.write_pcd(str(tmp_path / "b.pcd"), pts)
    assert np.array_equal(H.read_pcd_xyz(str(tmp_path / "b.pcd")), pts)
    with open(tmp_path / "a.pcd", "w") as f:
        f.write("# .PCD v0.7\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH 3\nHEIGHT 1\n"
                "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS 3\nDATA ascii\n1 2 3 0\n-0.5 0.25 1e-3 0\n4 5 6 0\n")
    assert H.read_pcd_xyz(str(tmp_path / "a.pcd")).tolist() == [[1, 2, 3], [-0.5, 0.25, np.float32(1e-3)], [4, 5, 6]]
    with open(tmp_path / "bad.pcd", "w") as f:
        f.write("VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 5\nHEIGHT 1\nPOINTS 5\nDATA ascii\n1 2 3\n")
    with pytest.raises(H.HouseError, match="truncated"):
        H.read_pcd_xyz(str(tmp_path / "bad.pcd"))
