"""The relocalisation tests' room and thick-wall volumes, displaced pose pairs and score cases, made once per process."""
import numpy as np

import align_twin as AT
import np_twin as T
import reloc_twin as RT
from align_cases import M_TRUE, PERTURBED, scene

f32 = np.float32
# the room of the relocalisation tests: align_twin's scene at 160 x 128 x 96 over 3 m (three different cells)
ROOM_DIMS, ROOM_SIZE = (160, 128, 96), (3.0, 3.0, 3.0)
ROOM_TAU = T.tau_of(ROOM_SIZE, ROOM_DIMS, 0.03)        # 65.6 mm: 2.1 times the largest cell
HALF_CELL_M = 0.5 * 3.0 / 160                           # half the smallest cell: 9.4 mm
# (last pose: eye, target; the truth's offset in the last camera's frame: shift, yaw and pitch in degrees)
DISPLACED = (((2.05, 1.62, 2.13), (1.0, 0.6, 1.2), (0.47, -0.18, 0.34), 33.0, -12.0),
             ((1.9, 1.5, 0.9), (0.9, 0.7, 1.4), (-0.36, 0.23, -0.45), -37.0, 9.0))

_CACHE = {}


def room_volume():
    if "room" not in _CACHE:
        _CACHE["room"] = AT.scene_volume(ROOM_DIMS, ROOM_SIZE, ROOM_TAU)
    return _CACHE["room"]


def displaced_pair(case):
    eye, target, t, yaw, pitch = DISPLACED[case]
    last = RT.look_at(eye, target)
    return last.astype(f32), RT.displaced(last, t, yaw, pitch)


def thick_wall_volume():
    """the 80 x 64 x 48 scene with the four outermost planes in x, which the scene leaves unobserved, observed as solid (-1,
    weight 1): the scene itself holds no sample F <= -1 (it stops observing a truncation distance behind a surface), a grown
    volume does"""
    if "thick" not in _CACHE:
        vol = scene()[0].copy()
        assert (vol[:, :, :4, 1] == 0).all()
        vol[:, :, :4] = (-32767, 1)
        _CACHE["thick"] = vol
    return _CACHE["thick"]


def score_cases():
    """(points, {name: pose}) on that volume: the truth, a perturbed pose, one that puts every point outside, one that pushes the
    cloud half a metre through the walls (points in free space and in unseen voxels) and one that pushes it 0.2 m into the
    solid wall (points behind a surface)"""
    _, ps, _ = scene()
    odd = ps.copy()
    odd[5], odd[7, 1], odd[9], odd[11], odd[13, 2], odd[15, 0] = np.nan, np.nan, 1e9, np.inf, -np.inf, -1e30
    away = np.eye(4)
    away[:3, 3] = (40.0, 0.0, 0.0)
    push = np.eye(4)
    push[:3, 3] = (0.5, 0.4, -0.45)
    wall = np.eye(4)
    wall[0, 3] = -0.2
    return odd, {"truth": M_TRUE.astype(f32), "perturbed": PERTURBED, "outside": (away @ M_TRUE).astype(f32), "pushed": (push @ M_TRUE).astype(f32),
                 "into the wall": (wall @ M_TRUE).astype(f32)}
