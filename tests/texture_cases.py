"""The small cases of baked textures, shared by tests/test_texture_host.py (the kernel's text on the CPU) and
tests/test_gpu_texture.py (the kernel): volumes as hsk_download_tsdf hands them out, [Z, Y, X, 2] int16, colour volumes
[Z, Y, X, 4] uint8, and hand-made meshes in volume coordinates.  The twin's results are made once and left unchanged."""
import numpy as np

import texture_twin as TT
from test_simplify_host import BOX_DIMS, BOX_SIZE, grid, small_cases

f32 = np.float32
_CACHE = {}

# ---- the analytic wall: a TSDF exactly linear in x around a wall at voxel coordinate 15.3, a colour ramp ---------------------------
WALL_DIMS, WALL_SIZE = (32, 32, 32), (3.0, 3.0, 3.0)
WALL_X = 15.3          # in voxel indices (the voxel centres' coordinate)
WALL_SLOPE = 4000      # stored units per voxel: 0.3 * 4000 is an integer, so every stored value near the wall is exact
WALL_TAU_VOXELS = 32767.0 / WALL_SLOPE     # one unit of F (the stored value / 32767) is this many voxels
WALL_CELL = float(f32(3.0) / f32(32))


def wall_volume():
    x, _, _ = grid(WALL_DIMS)
    t = np.clip(np.rint((x - WALL_X) * WALL_SLOPE), -32767, 32767).astype(np.int16)
    near = np.abs(x - WALL_X) < 8
    assert np.array_equal(t[near].astype(np.float64), ((x - WALL_X) * WALL_SLOPE)[near].round())
    return np.stack([t, np.full(t.shape, 2, np.int16)], axis=-1)


def wall_colour():
    x, y, z = grid(WALL_DIMS)
    return np.stack([4 * y, 8 * z, np.full(x.shape, 100.0), np.full(x.shape, 3.0)], axis=-1).astype(np.uint8)


def wall_mesh(offset_voxels):
    """two triangles that tile the square y, z in [5, 25] voxels of the plane `offset_voxels` in front of the wall"""
    px = (WALL_X + offset_voxels + 0.5) * WALL_CELL
    lo, hi = (5 + 0.5) * WALL_CELL, (25 + 0.5) * WALL_CELL
    v = np.array([[px, lo, lo], [px, hi, lo], [px, hi, hi], [px, lo, hi]], f32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def unseen_wall_volume():
    """the wall, never observed around the plane x = 25.3: every sample there has a tap without weight"""
    v = wall_volume()
    v[:, :, 22:29, 1] = 0
    return v


# ---- a hand-made mesh in the box volume: every block size, an odd bucket, skipped faces, a face outside the volume ------------------
def hand_mesh():
    """at the box volume's default density (one texel per 0.0375 m): longest edges of 2, 8, 20 and 40 texels -> sides 8, 16, 32, 64
    (and a face far too large for 64: still 64); sizes 8 and 32 hold an odd number of faces; five skipped faces"""
    c = float(f32(BOX_SIZE[0]) / f32(BOX_DIMS[0]))
    x0, y0, z0 = 66.6 + 0.5, 6.0, 5.0                                     # on the wall x = 66.6 (voxel indices), in voxels
    v, f = [], []

    def tri(a, e, at):
        """a right triangle with legs e (voxels) in the wall's plane at (y, z) = at, pushed a voxels off the wall"""
        n = len(v)
        v.extend([[(x0 + a) * c, (y0 + at[0]) * 0.04, (z0 + at[1]) * 0.05], [(x0 + a) * c, (y0 + at[0]) * 0.04 + e * c, (z0 + at[1]) * 0.05],
                  [(x0 + a) * c, (y0 + at[0]) * 0.04, (z0 + at[1]) * 0.05 + e * c]])
        f.append([n, n + 1, n + 2])

    tri(0.2, 2 / np.sqrt(2), (0, 0))      # side 8
    tri(-0.3, 8 / np.sqrt(2), (2, 0))     # side 16
    tri(0.4, 8 / np.sqrt(2), (2, 6))      # side 16
    tri(0.1, 20 / np.sqrt(2), (8, 0))     # side 32
    tri(0.0, 40 / np.sqrt(2), (1, 1))     # side 64
    tri(0.3, 90 / np.sqrt(2), (0, 0))     # side 64: too large for any block, and it leaves the volume
    f.append([1, 2, 0])                   # face 0 again from another corner: another rotation (side 8)
    f.append([4, 5, 3])                   # side 16, rotation 2
    f.append([2, 0, 1])                   # side 8: three faces of side 8 in all
    f.append([0, 0, 1])                   # skipped: a repeated index
    f.append([0, 1, 1000])                # skipped: an index out of range
    f.append([0, -1, 1])                  # skipped: a negative index
    n = len(v)
    v.extend([[0.5, 0.5, 0.5]] * 3)
    f.append([n, n + 1, n + 2])           # skipped: L2 = 0
    n = len(v)
    v.extend([[9.0, 9.0, 9.0], [9.2, 9.0, 9.0], [9.0, 9.2, 9.0]])
    f.append([n, n + 1, n + 2])           # outside the volume: owned texels, nothing projected
    n = len(v)
    v.extend([[0.5, 0.5, np.nan], [0.6, 0.5, 0.5], [0.5, 0.6, 0.5]])
    f.append([n, n + 1, n + 2])           # skipped: a coordinate that is not finite
    return np.array(v, f32), np.array(f, np.int32)


def box_case():
    vol, dims, size, col = small_cases()["box with colour"]
    return vol, col, size


def blocked(vol):
    """a host volume [Z, Y, X, 2] as the device stores it: 64-B blocks of 4 x-adjacent voxels by 4 planes, the pair in one word"""
    Z, Y, X, _ = vol.shape
    out = np.zeros(X * Y * ((Z + 3) & ~3), np.uint32)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    idx = ((((z >> 2) * Y + y) * (X // 4) + (x >> 2)) * 16) + (z & 3) * 4 + (x & 3)
    out[idx.reshape(-1)] = ((vol[..., 0].astype(np.int64) & 0xffff) | ((vol[..., 1].astype(np.int64) & 0xffff) << 16)).reshape(-1)
    return out


def twin_bake(key, vol, col, size, v, f, **params):
    """the twin's bake of a named case, made once and left unchanged"""
    if key not in _CACHE:
        _CACHE[key] = TT.bake(vol, col, size, v, f, **params)
    return _CACHE[key]


def info_list(info):
    return [info[n] for n in TT.INFO_FIELDS if n != "n_blocks"] + list(info["n_blocks"])


def owner_of_texels(tw):
    """per texel of a twin result the face that owns it (-1: none), from the charts alone"""
    H, W = tw["mask"].shape
    own = np.full((H, W), -1, np.int64)
    for i, (x0, y0, s, hr) in enumerate(tw["charts"].tolist()):
        if s < 0:
            continue
        j, k = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")     # j the row, k the column
        mine = (k + j <= s - 2) if (hr & 255) == 0 else (k + j > s - 2)
        sl = own[y0:y0 + s, x0:x0 + s]
        assert (sl[mine] == -1).all()                                       # no two faces own one texel
        sl[mine] = i
    return own
