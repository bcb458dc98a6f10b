"""The partition tests' rooms, their parameters and twin partitions, made once per process."""
import numpy as np

import clearance_twin as CL
import partition_twin as PT
import reach_twin as RE
from components_cases import speckled
from cover_cases import carved_volume
from reach_cases import FREE_WORD, SOLID_WORD

_CACHE = {}
DOOR_THRESHOLD = {(1, 1, 1): 64, (16, 25, 44): 1600}          # the largest D in the door plane of two_rooms(False)
RAGGED = ((72, 56, 41), (80, 64, 46))


def clear_params(weight, scale=16):
    """the hand-built volumes' clearance parameters: flags 0 and a cap of `scale` times the largest weight"""
    return dict(weight=tuple(weight), max_d2=scale * max(weight), flags=0)


def d2_of(name, vol, weight, scale=16):
    """the twin's clearance field of a named volume, made once"""
    key = ("d2", name, tuple(weight), scale)
    if key not in _CACHE:
        cp = clear_params(weight, scale)
        _CACHE[key] = CL.field(vol, cp["weight"], cp["max_d2"], 0)
    return _CACHE[key]


def twin_partition(name, d2, weight, core_d2, min_d2, min_core_voxels, max_cost=RE.MAX_COST):
    """the twin's partition of a named clearance field, made once per (name, parameters)"""
    key = ("partition", name, tuple(weight), int(core_d2), int(min_d2), int(min_core_voxels), int(max_cost))
    if key not in _CACHE:
        _CACHE[key] = PT.partition(d2, weight, core_d2, min_d2, min_core_voxels, max_cost)
    return _CACHE[key]


def ragged(dims):
    X, Y, Z = dims
    return np.ascontiguousarray(speckled(carved_volume(), Z)[:Z, :Y, :X])


def ragged_case(dims, weight, min_core_voxels):
    """the speckled carved room cut to dims -> (volume, clearance field, partition parameters as keywords)"""
    vol = ragged(dims)
    return vol, d2_of(f"speckled {dims}", vol, weight), dict(core_d2=4 * min(weight), min_d2=min(weight), min_core_voxels=min_core_voxels, max_cost=RE.MAX_COST)


MIRROR_DIMS = (67, 16, 12)

MIRROR_PAD = 5          # solid planes behind the far wall that make X a multiple of 8, which a context's volume must be


def mirror_rooms(pad=0):
    """odd X, mirror-symmetric about the plane x = 33 OF voxels: two chambers joined by a corridor 4 x 4 voxels wide, which holds
    no core at core_d2 = 9 min(weight); every passable voxel of the plane is as far from one core as from the other.  `pad` more
    solid planes behind the far wall change no clearance (flags 0: the border is no obstacle)"""
    X, Y, Z = MIRROR_DIMS
    vol = np.zeros((Z, Y, X + pad, 2), np.int16)
    vol[...] = SOLID_WORD
    vol[1:Z - 1, 1:Y - 1, 1:25] = FREE_WORD
    vol[1:Z - 1, 1:Y - 1, X - 25:X - 1] = FREE_WORD
    vol[4:8, 6:10, 25:X - 25] = FREE_WORD
    assert np.array_equal(vol[:, :, :X], vol[:, :, :X][:, :, ::-1])
    return vol


def serpentine_core_d2(weight):
    """a threshold at which only the serpentine's two end chambers -- 10 and 15 voxels deep, the others 13 between two walls --
    hold a core: 8 voxels from the nearest wall"""
    return 64 * weight[0]
