"""The alignment tests' analytic scene (a room seen from inside with a box on its floor) and its poses, made once per process."""
import numpy as np

import align_twin as AT
import np_twin as T

f32 = np.float32
TAU = T.tau_of(AT.DST_SIZE, AT.DST_DIMS, 0.03)
HALF_CELL_M = 0.5 * 3.0 / 80          # half the smallest destination cell: 18.75 mm
M_TRUE = AT.rigid(2.5, (40.0, -30.0, 20.0))
PERTURBED = (AT.rigid(2.0, (150.0, -100.0, 120.0)) @ M_TRUE).astype(f32)

_CACHE = {}


def scene():
    """(destination volume, source points, source normals), made once"""
    if "scene" not in _CACHE:
        ps, ns = AT.source_cloud(M_TRUE)
        _CACHE["scene"] = (AT.scene_volume(AT.DST_DIMS, AT.DST_SIZE, TAU), ps, ns)
    return _CACHE["scene"]
