"""The small cases of baked textures, shared by tests/test_texture_host.py (the kernel's text on the CPU) and
tests/test_gpu_texture.py (the kernel): volumes as hsk_download_tsdf hands them out, [Z, Y, X, 2] int16, colour volumes
[Z, Y, X, 4] uint8, and hand-made meshes in volume coordinates.  The twin's results are made once and left unchanged."""
import numpy as np

import texture_twin as TT
from kit import volume_ctx
from simplify_cases import BOX_DIMS, BOX_SIZE, grid, small_cases

f32 = np.float32


def resolved(vol, size, texels_per_metre=0.0, atlas_width=0, n_iter=4, f_tol=0.01, max_offset_m=0.0):
    """the parameters as hsk_bake_texture resolves them: the zeros replaced by the defaults"""
    Z, Y, X, _ = vol.shape
    cell = TT.cells((X, Y, Z), size)
    return (f32(texels_per_metre) if texels_per_metre else f32(1) / min(cell), atlas_width or 1024, n_iter, f32(f_tol),
            f32(max_offset_m) if max_offset_m else f32(4) * max(cell))


def differing(got, tw, rgb=True):
    """the differing bytes of a bake against the twin's: every output, the charts and the info"""
    n = 0
    for name in ("normal_rgb", "mask") + (("rgb",) if rgb else ()):
        assert got[name].shape == tw[name].shape, (name, got[name].shape, tw[name].shape)
        n += int((got[name] != tw[name]).sum())
    n += int((np.ascontiguousarray(got["uv"]).view(np.uint32) != tw["uv"].view(np.uint32)).sum())
    n += int((np.asarray(got["charts"]).view(np.int32).reshape(-1, 4) != tw["charts"].view(np.int32).reshape(-1, 4)).sum())
    n += sum(a != b for a, b in zip(info_list(got["info"]), info_list(tw["info"])))
    return n


def check_wall(got):
    """every texel inside a face is projected, lies within f_tol tau of the wall and has the ramp's colour there within one level:
    trilinear interpolation of a linear function is exact up to the float rounding and the one rounding to uint8"""
    inside = (got["mask"] & 3) == 3
    assert inside.sum() > 1500 and ((got["mask"][inside] & 4) != 0).all()
    g = got["points"][inside].astype(np.float64) / WALL_CELL - 0.5             # in voxel indices
    assert np.abs(g[:, 0] - WALL_X).max() <= 0.01 * WALL_TAU_VOXELS
    want = np.stack([4 * g[:, 1], 8 * g[:, 2], np.full(len(g), 100.0)], axis=1)
    assert ((got["mask"][inside] & 8) != 0).all() and np.abs(got["rgb"][inside].astype(np.float64) - want).max() <= 1.0
    # the normal is +x: (255, 128, 128)
    assert ((got["mask"][inside] & 16) != 0).all() and (got["normal_rgb"][inside] == (255, 128, 128)).all()


def check_failed(got, v, colored):
    """owned texels, none projected, every one at its P0 -- in the mesh's plane -- and, with colour, the ramp there or nothing"""
    owned = (got["mask"] & 1) != 0
    assert owned.sum() > 1500 and ((got["mask"][owned] & 4) == 0).all()
    assert (got["points"][owned][:, 0] == v[0, 0]).all()
    inside = (got["mask"] & 3) == 3
    if colored:
        g = got["points"][inside].astype(np.float64) / WALL_CELL - 0.5
        want = np.stack([4 * g[:, 1], 8 * g[:, 2], np.full(len(g), 100.0)], axis=1)
        assert ((got["mask"][inside] & 8) != 0).all() and np.abs(got["rgb"][inside].astype(np.float64) - want).max() <= 1.0
    else:
        assert ((got["mask"][owned] & 8) == 0).all() and (got["rgb"] == 0).all()


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


def loaded(hsk, vol, col, size):
    Z, Y, X, _ = vol.shape
    trk = volume_ctx(hsk, (X, Y, Z), size)
    if col is not None:
        trk.enable_color()
        trk.upload_color(col)
    trk.upload_tsdf(vol)
    return trk
