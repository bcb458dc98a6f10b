"""The coverage tests' carved volume, its eye points and probe, made once per process."""
import numpy as np

import cover_twin as CT
import reloc_twin as RT
from align_cases import TAU, scene

f32 = np.float32
PATCH = (slice(16, 28), slice(25, 42), slice(61, 80))        # (z, y, x): a never-observed patch cut into the x = 2.7 m wall
PATCH_CENTRE = (2.64375, 1.5703125, 1.375)
EYE = (1.0, 1.5, 1.4)

_CACHE = {}


def carved_volume():
    """the 80 x 64 x 48 scene with the patch set to (0, 0)"""
    if "carved" not in _CACHE:
        vol = scene()[0].copy()
        vol[PATCH] = 0
        _CACHE["carved"] = vol
    return _CACHE["carved"]


def probe_40x30(near_m=0.1, far_m=3.5, step_tau=0.5, w=40, h=30):
    return CT.probe(w, h, 33.0, 33.0, (w - 1) / 2, (h - 1) / 2, near_m, far_m, f32(step_tau) * f32(TAU))


TOWARDS = RT.look_at(EYE, PATCH_CENTRE)
AWAY = RT.look_at(EYE, (0.3, 1.5, 1.4))
