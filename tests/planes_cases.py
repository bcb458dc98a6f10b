"""The plane tests' clouds, their twin results and the rule's bar on the scene."""
import numpy as np

import align_twin as AT
import planes_twin as PT

f32 = np.float32
HALF_CELL_M = 0.5 * 3.0 / 80          # half the smallest cell of the 80 x 64 x 48 scene: 18.75 mm
DIST_M, COS_MIN = 0.02, 0.8660254037844387

_CACHE = {}


def scene_cloud():
    """(volume, points, normals) of the analytic scene at 80 x 64 x 48, made once"""
    if "scene" not in _CACHE:
        vol = PT.scene_volume()
        _CACHE["scene"] = (vol,) + PT.scene_cloud(vol)
    return _CACHE["scene"]


def odd_cloud():
    """the scene's cloud with the odd points mixed in: NaN and infinite coordinates and normals, a point far away, |x| just
    either side of 64, a zero normal, a normal that is not a unit vector"""
    if "odd" not in _CACHE:
        _, ps, ns = scene_cloud()
        ps, ns = ps.copy(), ns.copy()
        below, above = np.nextafter(f32(64), f32(0)), np.nextafter(f32(64), f32(np.inf))
        ps[5], ps[7, 1], ps[9], ps[11], ps[13, 2], ps[15, 0] = np.nan, np.nan, 1e9, np.inf, -np.inf, -1e30
        ns[17], ns[19, 2], ns[21, 0], ns[23] = np.nan, np.inf, -np.inf, 0.0
        ps[25, 0], ps[27, 0], ps[29, 1], ps[31, 2], ps[33, 0], ps[35, 1] = below, above, -below, -above, 64.0, -64.0
        ns[37] = ns[37] * f32(3.0)
        ns[39, 1] = 1e30
        _CACHE["odd"] = (ps, ns)
    return _CACHE["odd"]


def twin_scene():
    """the twin's detection on the scene (a), made once"""
    if "twin_scene" not in _CACHE:
        _, ps, ns = scene_cloud()
        _CACHE["twin_scene"] = PT.detect(ps, ns)
    return _CACHE["twin_scene"]


def twin_wall():
    """the thin wall (b) and the twin's detection on it, made once"""
    if "twin_wall" not in _CACHE:
        ps, ns, face = PT.thin_wall()
        _CACHE["twin_wall"] = (ps, ns, face) + PT.detect(ps, ns)
    return _CACHE["twin_wall"]


def score_planes_for_tests(n_planes):
    """n_planes planes for the scoring tests: the room's faces as the twin found them, then planes of seed points of the odd
    cloud (some of them invalid: NaN planes), then a NaN plane and an infinite one"""
    ps, ns = odd_cloud()
    rec = twin_scene()[0]
    planes = [r["abcd"] for r in rec]
    rng = PT.Lcg(11)
    with np.errstate(all="ignore"):
        while len(planes) < n_planes:
            i = rng.next() % 64 if len(planes) % 3 == 0 else rng.next() % len(ps)
            planes.append(np.append(ns[i], -PT.dot3(*ns[i], *ps[i])).astype(f32))
    planes = np.array(planes[:n_planes], f32)
    if n_planes > 2:
        planes[-1], planes[-2] = np.nan, (np.inf, 0.0, 0.0, 1.0)
    return planes


def assert_scene_bar(rec, what):
    """(a)'s bar: six planes, each within half the smallest cell of one of the room's faces and within 1 degree of its inward
    normal, every face once"""
    faces = PT.room_faces()
    assert len(rec) == 6, what
    seen = set()
    for r in rec:
        p = r["abcd"].astype(np.float64)
        assert abs(np.linalg.norm(p[:3]) - 1.0) < 1e-6
        ang = np.degrees(np.arccos(np.clip(faces[:, :3] @ p[:3], -1.0, 1.0)))
        i = int(np.argmin(ang))
        # the plane lies within the bar of the face: the largest distance from it of the face's four corners
        lo, hi = np.array(AT.ROOM)
        axis = i // 2
        at = -faces[i, 3] * faces[i, axis]
        corners = np.array([[at if c == axis else (lo[c], hi[c])[(k >> (c if c < axis else c - 1)) & 1] for c in range(3)] for k in range(4)])
        off = np.abs(corners @ p[:3] + p[3]).max()
        print(f"{what}: plane {r['abcd']} with {r['n_inliers']} points: face {i}, {ang[i]:.4f} degrees, at most {off * 1e3:.3f} mm from it")
        assert ang[i] <= 1.0 and off <= HALF_CELL_M
        seen.add(i)
    assert seen == set(range(6)), what
