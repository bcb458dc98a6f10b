"""The volumes the fill tests share (tests/test_fill_host.py on the host, tests/test_gpu_fill.py on the device), each with the
parameters it is filled with, and the twin's result of each, computed once."""
import numpy as np

import fill_twin as FT
from components_cases import speckled
from cover_cases import carved_volume

_CACHE = {}
RANDOM_DIMS = [(80, 64, 48), (80, 64, 46), (80, 64, 41), (72, 56, 40)]
# (iterations, keep) of the random volumes: the default of their 3.75 cm cells -- 4, SURFACE -- then ALL with 1, 2 and 9 iterations
RANDOM_PARAMS = [(4, FT.SURFACE), (1, FT.ALL), (2, FT.ALL), (9, FT.ALL)]


def random_volume(dims):
    X, Y, Z = dims
    key = ("random", dims)
    if key not in _CACHE:
        _CACHE[key] = np.ascontiguousarray(speckled(carved_volume(), Z)[:Z, :Y, :X])
    return _CACHE[key]


def ramp(shape, x_zero=15.4, tau=3.0, weight=2):
    """a volume observed everywhere: a wall whose zero lies at x = x_zero voxels"""
    Z, Y, X = shape
    vol = np.zeros((Z, Y, X, 2), np.int16)
    x = np.arange(X, dtype=np.float64)
    vol[..., 0] = np.rint(np.clip((x_zero - x) / tau, -1.0, 1.0) * 32767).astype(np.int16)[None, None, :]
    vol[..., 1] = weight
    return vol


def shapes():
    """name -> (volume, dict of fill parameters, box or None)"""
    if "shapes" in _CACHE:
        return _CACHE["shapes"]
    out = {}
    wall, _ = FT.planar_wall()
    out["planar wall"] = (wall, dict(iterations=16), None)
    # the wall at z = 8.3 of a 40 x 40 x 16 grid: its hole spans x, y = 14 .. 25 and z = 4 .. 15 -- across the tile faces x = 16,
    # y = 16 and z = 8 together
    low, _ = FT.planar_wall(Z=16, z0=8.3, hole_from=4)
    out["hole across x = 16, y = 16, z = 8"] = (low, dict(iterations=8), None)
    six = ramp((20, 24, 32))                                    # 20 planes: a plane group of its own for the last four
    for z, y, x in ((slice(6, 12), slice(8, 16), slice(0, 4)), (slice(6, 12), slice(8, 16), slice(28, 32)), (slice(6, 12), slice(0, 4), slice(10, 22)),
                    (slice(6, 12), slice(20, 24), slice(10, 22)), (slice(0, 3), slice(8, 16), slice(10, 22)), (slice(17, 20), slice(8, 16), slice(10, 22))):
        six[z, y, x] = 0
    out["a hole on each grid face"] = (six, dict(iterations=6, keep=FT.ALL), None)   # (ALL: the x faces lie far from the crossing)
    one = ramp((12, 24, 32))
    one[5, 11, 15] = 0
    out["one unknown voxel"] = (one, dict(iterations=3), None)
    out["no source"] = (np.zeros((12, 24, 32, 2), np.int16), dict(iterations=5), None)
    out["no non-source"] = (ramp((12, 24, 32)), dict(iterations=5), None)
    low_raw = ramp((8, 16, 16), x_zero=7.6)
    low_raw[2:6, 4:12, 4:12] = 0
    low_raw[1, 4:12, 4:12] = (-32768, 1)                        # sources that an upload can hold and no integrate writes
    low_raw[3:5, 3, 4:12] = (-32768, 3)
    out["a source with raw -32768"] = (low_raw, dict(iterations=6, keep=FT.ALL), None)
    out["a box through the hole"] = (wall, dict(iterations=16), ((0, 0, 0), (20, 40, 48)))
    out["an empty box"] = (wall, dict(iterations=3), ((5, 5, 5), (5, 30, 30)))
    out["band 0"] = (low, dict(iterations=8, band=0), None)
    out["band 8"] = (low, dict(iterations=8, band=8), None)
    out["fill_weight 128"] = (low, dict(iterations=8, fill_weight=128), None)
    small = np.zeros((8, 16, 16, 2), np.int16)
    small[0:2, 0:3, 0:3] = (-9000, 1)
    small[6:8, 13:16, 12:16] = (15000, 2)
    out["255 iterations"] = (small, dict(iterations=255, keep=FT.ALL), None)
    _CACHE["shapes"] = out
    return out


def twin_of(key, vol, params, box=None):
    """the twin's (volume, mask, stats), computed once per key; nobody writes into the arrays"""
    if ("twin", key) not in _CACHE:
        _CACHE[("twin", key)] = FT.fill(vol, box=box, **params)
    return _CACHE[("twin", key)]


def shape_twin(name):
    vol, params, box = shapes()[name]
    return twin_of(("shape", name), vol, params, box)


def random_twin(dims, iterations, keep):
    return twin_of(("random", dims, iterations, keep), random_volume(dims), dict(iterations=iterations, keep=keep))
