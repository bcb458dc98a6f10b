"""The clearance tests' scene parameters, lookup points and twin fields, made once per process."""
import numpy as np

import clearance_twin as CL

f32 = np.float32
SCENE_DEFAULTS = {"weight": (16, 25, 44), "max_d2": 11378, "flags": CL.UNKNOWN, "unit_m": f32(0.009375)}
# the kernels' seams (hsk_clear_point.h; read back from the header below): a row mask's words, an axis pass's segments
MASK_BITS, AXIS_SEG = 64, 16
_CACHE = {}


def twin_field(name, vol, weight, max_d2, flags):
    """the twin's field of a named volume, made once per (name, parameters)"""
    key = (name, tuple(weight), int(max_d2), int(flags))
    if key not in _CACHE:
        _CACHE[key] = CL.field(vol, weight, max_d2, flags)
    return _CACHE[key]


def lookup_points(size_m, dims, seed=3):
    """points at voxel centres, on voxel faces, outside the grid and non-finite"""
    rng = np.random.default_rng(seed)
    cell = np.array([f32(size_m[i]) / f32(dims[i]) for i in range(3)], f32)
    idx = rng.integers(0, dims, (40, 3))
    centres = ((idx + 0.5) * cell).astype(f32)
    faces = (idx * cell).astype(f32)
    edge = np.array([[0.0, 0.0, 0.0], size_m, [size_m[0], 1.0, 1.0], [1.0, -0.0, 1.0], [2.99 * size_m[0] / 3.0, 1.0, 1.0]], f32)
    odd = np.array([[-0.01, 1.0, 1.0], [1.0, 1.0, 40.0], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf], [1e30, 1e30, 1e30], [np.nan] * 3], f32)
    return np.concatenate([centres, faces, edge, odd])
