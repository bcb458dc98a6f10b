"""The levelling tests' tilted and jittered clouds, their twin results and the bar on an upright frame."""
import numpy as np

import level_twin as LT
from kit import same_bits

f32 = np.float32
ANGLE_BAR_DEG = 0.25                  # at that error a 5 m wall strays 22 mm: one cell of a 512-voxel house

_CACHE = {}


def tilted(scene, tilt, trunc=0.03):
    """(volume, points, normals, cell weights, R) of a scene of LT.SCENES under a tilt of LT.TILTS, made once"""
    key = (scene, tilt, trunc)
    if key not in _CACHE:
        dims, size = LT.SCENES[scene]
        R = LT.TILTS[tilt] if isinstance(tilt, str) else LT.rot(*tilt)
        _CACHE[key] = LT.scene(dims, size, R, trunc) + (LT.cell_weights(dims, size), R)
    return _CACHE[key]


def twin_of(scene, tilt, **params):
    key = ("twin", scene, tilt, tuple(sorted(params.items())))
    if key not in _CACHE:
        _, ps, ns, w, _ = tilted(scene, tilt)
        _CACHE[key] = LT.estimate(ps, ns, w, **params)
    return _CACHE[key]


def jittered(n, seed=5):
    """n points for the stage tests: the tilted scene's cloud repeated with a jitter on points and normals, the edge cases first"""
    _, ps, ns, _, _ = tilted("80x64x48", "a")
    eps, ens = LT.edge_cloud()
    rng = np.random.default_rng(seed)
    reps = -(-max(n - len(eps), 1) // len(ps))
    P = np.tile(ps, (reps, 1)) + rng.normal(0, 0.004, (reps * len(ps), 3)).astype(f32)
    N = np.tile(ns, (reps, 1)) + rng.normal(0, 0.02, (reps * len(ps), 3)).astype(f32)
    pick = rng.permutation(len(P))[:max(n - len(eps), 0)]
    return np.concatenate([eps, P[pick]])[:n].astype(f32), np.concatenate([ens, N[pick]])[:n].astype(f32)


def assert_same_upright(got, ref, what):
    for name in ("n_points", "n_invalid", "n_axis", "n_walls", "found"):
        assert got[name] == ref[name], (what, name, got[name], ref[name])
    for name in ("level", "box_lo", "box_hi"):
        assert same_bits(got[name], ref[name]), (what, name, got[name], ref[name])
    for name in ("floor_m", "ceiling_m"):
        assert same_bits(f32(got[name]), f32(ref[name])), (what, name, got[name], ref[name])
