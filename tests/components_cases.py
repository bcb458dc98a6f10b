"""The component tests' volumes: speckled, with injected blobs, the hand-built shapes, and their twin results, made once per process."""
import numpy as np

import components_twin as KT
from cover_cases import carved_volume

IN = (-1000, 3)          # an INSIDE voxel: (tsdf, weight)
_CACHE = {}


def empty(dims):
    X, Y, Z = dims
    return np.zeros((Z, Y, X, 2), np.int16)


def fill(vol, zs, ys, xs, word=IN):
    vol[zs, ys, xs] = word
    return vol


def snake():
    """64 x 64 x 32: a one-voxel-wide path through every tile of 16 x 16 x 8 -- a serpentine of the rows y = 1, 3, .., 63 in each of
    the planes z = 2, 10, 18, 26, joined by columns at alternating ends: the longest parent chains, every merge on one component"""
    vol = empty((64, 64, 32))
    planes = list(range(2, 32, 8))
    for k, z in enumerate(planes):
        for i, y in enumerate(range(1, 64, 2)):
            fill(vol, z, y, slice(1, 63))
            if i > 0:
                fill(vol, z, y - 1, 62 if i % 2 == 1 else 1)
        if k + 1 < len(planes):
            fill(vol, slice(z, z + 9), 63 if k % 2 == 0 else 1, 1)
    return vol


def shapes():
    """{name: (volume, number of components)}: the shapes that break a tiled union-find, each small and built by hand"""
    if "shapes" in _CACHE:
        return _CACHE["shapes"]
    out = {"snake": (snake(), 1)}
    u = empty((32, 32, 8))                                   # a U that leaves the tile x < 16 and re-enters it
    fill(u, 3, 3, slice(10, 21)), fill(u, 3, 9, slice(10, 21)), fill(u, 3, slice(3, 10), 20)
    out["u"] = (u, 1)
    e = empty((32, 32, 16))                                  # blocks that touch along an edge (at a tile corner) and at a corner only
    fill(e, slice(4, 8), slice(12, 16), slice(12, 16)), fill(e, slice(4, 8), slice(16, 20), slice(16, 20)), fill(e, slice(8, 12), slice(20, 24), slice(20, 24))
    out["edge and corner"] = (e, 3)
    s = empty((48, 48, 24))                                  # three bars through the middle tile: a tile face crossed in each of six directions
    fill(s, 12, 24, slice(10, 39)), fill(s, 12, slice(10, 39), 24), fill(s, slice(2, 23), 24, 24)
    out["six directions"] = (s, 1)
    a = empty((32, 24, 12))
    a[...] = IN
    out["every voxel"] = (a, 1)
    out["empty"] = (empty((32, 24, 12)), 0)
    g = empty((32, 24, 10))                                  # members on all six grid faces (10 planes: the last group has padding)
    for z, y, x in ((0, 5, 5), (9, 5, 5), (4, 0, 9), (4, 23, 9), (5, 11, 0), (5, 11, 31), (9, 23, 31), (0, 0, 0)):
        fill(g, z, y, x)
    fill(g, 9, 22, 31)
    out["grid faces"] = (g, 8)
    w = empty((32, 24, 12))                                  # tsdf == 0 and weight == 0 voxels between two blocks separate them
    fill(w, slice(2, 6), slice(2, 6), slice(4, 8)), fill(w, slice(2, 6), slice(2, 6), slice(9, 13))
    fill(w, slice(2, 4), slice(2, 6), 8, (0, 5)), fill(w, slice(4, 6), slice(2, 6), 8, (-5, 0))
    out["separators"] = (w, 2)
    _CACHE["shapes"] = out
    return out


def speckled(vol, seed):
    """test_gpu_cover's: a fifth of the voxels in a random state -- thousands of components"""
    rng = np.random.default_rng(seed)
    out = vol.copy()
    pick = rng.random(vol.shape[:3]) < 0.2
    n = int(pick.sum())
    out[pick, 0] = rng.choice(np.array([32767, 1200, 0, -1, -32767], np.int16), n)
    out[pick, 1] = rng.choice(np.array([0, 0, 1, 7], np.int16), n)
    return out


# the blobs injected into the carved room: centre and radii in voxels (x, y, z) -- across tile faces (48, 32, 16 are multiples of
# the tile), inside one tile, a large one, and half of one on the grid's face y = 63
BLOBS = (((48, 32, 16), (3.0, 3.0, 2.5)), ((30, 40, 30), (2.2, 2.2, 2.2)), ((56, 20, 33), (5.0, 4.0, 4.0)), ((20, 45, 13), (3.0, 2.5, 2.0)),
         ((40, 63, 24), (4.0, 2.0, 3.0)))


def grow(m):
    """a mask and its 26 neighbours"""
    out = m.copy()
    Z, Y, X = m.shape
    p = np.pad(m, 1)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= p[dz:dz + Z, dy:dy + Y, dx:dx + X]
    return out


def injected_volume():
    """(volume, [core mask per blob]): the carved room with closed blobs -- a negative core inside a band of two rings of positive
    partial values -- written only over voxels that were never observed or plain free space (asserted): nothing a wall's crossing
    hangs on is touched"""
    if "injected" not in _CACHE:
        base = carved_volume()
        vol = base.copy()
        Z, Y, X = vol.shape[:3]
        z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
        cores = []
        for (cx, cy, cz), (rx, ry, rz) in BLOBS:
            core = ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 + ((z - cz) / rz) ** 2 < 1.0
            ring1 = grow(core) & ~core
            ring2 = grow(core | ring1) & ~core & ~ring1
            touched = core | ring1 | ring2
            plain = ((base[..., 0] == 0) & (base[..., 1] == 0)) | ((base[..., 0] == 32767) & (base[..., 1] != 0))
            assert plain[touched].all(), "a blob touches a wall's band"
            vol[core] = (-20000, 4)
            vol[ring1] = (9000, 4)
            vol[ring2] = (24000, 4)
            cores.append(core)
        _CACHE["injected"] = (vol, cores)
    return _CACHE["injected"]


def twin_of(name, vol):
    """labels and records of a volume, made once per name"""
    if ("twin", name) not in _CACHE:
        lab = KT.labels(vol)
        _CACHE[("twin", name)] = (lab, KT.records(vol, lab))
    return _CACHE[("twin", name)]
