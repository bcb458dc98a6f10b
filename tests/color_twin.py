"""numpy restatement of the colour path (housescan_amd/csrc/color.hip, DESIGN.md "Colour"): the colour update of one frame on
the integrate's own projection (np_twin._project), the band hsk_enable_color puts in effect, and the colour pick and normal
of hsk_extract_cloud_attrs.  Extent, cell and intrinsics are arguments, per axis: nothing here knows a cube or a camera.
Whole volumes: every plane stored and owned."""
import numpy as np

import mesh_twin as MT
from np_twin import _Grid, _project, tau_of

f32 = np.float32
_PLANES = 32  # planes projected at a time (memory only: the result does not depend on it)


def band_of(dims, size3, band_m, trunc):
    """hsk_enable_color's band: band_m when positive, else twice the largest cell; at most the integrate's tau"""
    cell = [f32(size3[i]) / f32(dims[i]) for i in range(3)]
    b = f32(band_m) if band_m > 0 else f32(2.0) * max(cell)
    return min(b, tau_of(size3, dims, trunc))


def integrate_color(col, size3, scaled, rgb, fx, fy, cx, cy, pose, band, max_w):
    """one frame's colour update of `col` ([Z, Y, X, 4] uint8 (r, g, b, w), in place): a voxel whose pixel is in the image with
    D_s != 0 and -band < sdf < band takes c' = (c w + p + ((w + 1) >> 1)) // (w + 1), w' = min(w + 1, max_w).
    Returns the number of voxels coloured"""
    Z, Y, X, _ = col.shape
    band = f32(band)
    n = 0
    for z0 in range(0, Z, _PLANES):
        nz = min(_PLANES, Z - z0)
        ok, u, v, Ds, sdf, _, _, _ = _project((X, Y, Z), size3, scaled, fx, fy, cx, cy, pose, z0, nz)
        upd = ok & (Ds != 0) & (sdf > -band) & (sdf < band)
        iz, iy, ix = np.nonzero(upd)
        if len(iz) == 0:
            continue
        n += len(iz)
        p = rgb[v[iz, iy, ix], u[iz, iy, ix]].astype(np.int64)
        blk = col[z0:z0 + nz]
        c = blk[iz, iy, ix, :3].astype(np.int64)
        w = blk[iz, iy, ix, 3].astype(np.int64)
        w1 = w + 1
        blk[iz, iy, ix, :3] = ((c * w[:, None] + p + (w1 >> 1)[:, None]) // w1[:, None]).astype(np.uint8)
        blk[iz, iy, ix, 3] = np.minimum(w1, max_w).astype(np.uint8)
    return n


def cut_edges(tsdf):
    """the cloud's items in its order (plane, row, x, axis): voxel a = (z, y, x) and its +axis neighbour b, both observed,
    neither at 32767, of opposite strict signs -> (z, y, x, axis, bz, by, bx)"""
    Z, Y, X, _ = tsdf.shape
    t = tsdf[..., 0].astype(np.int32)
    valid = (tsdf[..., 1] != 0) & (t != 32767)
    M = np.zeros((Z, Y, X, 3), bool)
    for k, ax in enumerate((2, 1, 0)):  # k = 0: the +x neighbour (array axis 2), 1: +y, 2: +z
        sa, sb = [slice(None)] * 3, [slice(None)] * 3
        sa[ax], sb[ax] = slice(0, -1), slice(1, None)
        sa, sb = tuple(sa), tuple(sb)
        a, b = t[sa], t[sb]
        M[sa + (k,)] = valid[sa] & valid[sb] & (((a > 0) & (b < 0)) | ((a < 0) & (b > 0)))
    z, y, x, k = np.nonzero(M)
    return z, y, x, k, z + (k == 2), y + (k == 1), x + (k == 0)


def pick_color(t, col, a, b):
    """the colour rule of an edge between voxels a and b (index tuples (z, y, x)): the (r, g, b, w) of the one with the smaller
    |tsdf| (a on a tie), of the other when that one has weight 0 -> (first, other, pick), [n, 4] each"""
    ta, tb = np.abs(t[a]), np.abs(t[b])
    ca, cb = col[a], col[b]
    take_a = (ta <= tb)[:, None]
    first = np.where(take_a, ca, cb)
    other = np.where(take_a, cb, ca)
    return first, other, np.where((first[:, 3] == 0)[:, None], other, first)


def np_attrs(tsdf, col, xyz, size=3.0):
    """per point of the cloud (voxel order: plane, row, x, axis): the normal of the raycast on the TSDF and the colour of the
    selection rule -> (normals, rgb, n_uncolored).  `size`: one extent for a cube, or one per axis"""
    Z, Y, X, _ = tsdf.shape
    size3 = (size,) * 3 if np.isscalar(size) else tuple(size)
    z, y, x, k, bz, by, bx = cut_edges(tsdf)
    assert len(z) == len(xyz)
    _, _, pick = pick_color(tsdf[..., 0].astype(np.int32), col, (z, y, x), (bz, by, bx))
    unc = pick[:, 3] == 0
    rgb = np.where(unc[:, None], 0, pick[:, :3]).astype(np.uint8)
    with np.errstate(all="ignore"):
        nrm = MT.normal_at(_Grid(tsdf, size3, Z, 0), xyz, (X, Y, Z))
    return nrm, rgb, int(unc.sum())
