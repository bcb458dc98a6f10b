"""numpy restatement of hsk_extract_mesh_indexed (include/hskinfu.h): the edge-keyed vertex list, the faces, and per vertex
the normal and colour rules of hsk_extract_cloud_attrs, from a downloaded volume and the oracle's marching-cubes table
(oracle.mc_table()).  Whole volumes: every plane stored and owned."""
import numpy as np

from kit import same_bits
from np_twin import _Grid, _vox

f32 = np.float32
_AXIS = np.array([0, 0, 1, 0, 2, 0, 0, 0])  # b ^ a (1, 2 or 4) -> the edge's axis


def _corner(c):
    return c & 1, (c >> 1) & 1, c >> 2  # (dx, dy, dz)


def mesh_indexed(vol, ntri, codes, size=3.0, col=None, normals=True):
    """vol [Z, Y, X, 2] int16 (tsdf, weight), col [Z, Y, X, 4] uint8 or None ->
    dict(vertices [n, 3] f32, faces [m, 3] int32, edges [n, 4] (z, y, x, axis), normals [n, 3] f32 or None,
         rgb [n, 3] uint8 or None, n_uncolored)"""
    Z, Y, X, _ = vol.shape
    t = vol[..., 0].astype(np.int32)
    w = vol[..., 1] != 0
    valid = np.ones((Z - 1, Y - 1, X - 1), bool)
    m8 = np.zeros((Z - 1, Y - 1, X - 1), np.int32)
    for c in range(8):
        dx, dy, dz = _corner(c)
        sl = (slice(dz, Z - 1 + dz), slice(dy, Y - 1 + dy), slice(dx, X - 1 + dx))
        valid &= w[sl]
        m8 |= (t[sl] < 0).astype(np.int32) << c
    emit = valid & (m8 != 0) & (m8 != 255)
    # a vertex per cut edge of an emitted cube, keyed by the edge's lower corner and axis
    E = np.zeros((Z, Y, X, 3), bool)
    for a in range(8):
        for axis in range(3):
            b = a | (1 << axis)
            if b == a:
                continue
            cut = emit & ((((m8 >> a) ^ (m8 >> b)) & 1) != 0)
            dx, dy, dz = _corner(a)
            E[dz:Z - 1 + dz, dy:Y - 1 + dy, dx:X - 1 + dx, axis] |= cut
    ez, ey, ex, ek = np.nonzero(E)  # (plane, row, x, axis) order
    nv = len(ez)
    ids = np.full(E.shape, -1, np.int64)
    ids[ez, ey, ex, ek] = np.arange(nv)
    bz, by, bx = ez + (ek == 2), ey + (ek == 1), ex + (ek == 0)
    G = _Grid(vol, (size,) * 3 if np.isscalar(size) else tuple(size), Z, 0)   # (one extent for a cube, or one per axis)
    Fa = t[ez, ey, ex].astype(f32) / f32(32767)
    Fb = t[bz, by, bx].astype(f32) / f32(32767)
    wt = (Fa / (Fa - Fb)).astype(f32)
    verts = np.empty((nv, 3), f32)
    for ax, (ga, gb) in enumerate(((ex, bx), (ey, by), (ez, bz))):
        pa = ((ga.astype(f32) + f32(0.5)) * G.cell[ax]).astype(f32)
        pb = ((gb.astype(f32) + f32(0.5)) * G.cell[ax]).astype(f32)
        verts[:, ax] = pa + wt * (pb - pa)
    # faces: emitted cubes in voxel order, then table order; each corner the id of its edge
    cz, cy, cx = np.nonzero(emit)
    m = m8[cz, cy, cx]
    F = np.full((len(m), 5, 3), -1, np.int64)
    for k in range(5):
        for q in range(3):
            code = codes[m, k, q]
            a, b = code & 15, code >> 4
            axis = _AXIS[a ^ b]
            F[:, k, q] = ids[cz + (a >> 2), cy + ((a >> 1) & 1), cx + (a & 1), axis]
    faces = F[np.arange(5)[None, :] < ntri[m][:, None]]
    assert (faces >= 0).all()
    out = dict(vertices=verts, faces=faces.astype(np.int32), edges=np.stack([ez, ey, ex, ek], axis=1), normals=None, rgb=None,
               n_uncolored=0)
    if normals:
        out["normals"] = normal_at(G, verts, (X, Y, Z))
    if col is not None:
        ta, tb = np.abs(t[ez, ey, ex]), np.abs(t[bz, by, bx])
        ca, cb = col[ez, ey, ex], col[bz, by, bx]
        take_a = ta <= tb
        first = np.where(take_a[:, None], ca, cb)
        other = np.where(take_a[:, None], cb, ca)
        pick = np.where((first[:, 3] == 0)[:, None], other, first)
        unc = pick[:, 3] == 0
        out["rgb"] = np.where(unc[:, None], 0, pick[:, :3]).astype(np.uint8)
        out["n_uncolored"] = int(unc.sum())
    return out


def normal_at(G, xyz, dims):
    """the raycast's normal at each point: central differences of the trilinear TSDF one cell either side, scaled by 1 / |n|;
    NaN x 3 where floor(p / cell) is not within (1, dims - 2) on every axis"""
    p = [xyz[:, i].copy() for i in range(3)]
    deep = np.ones(len(xyz), bool)
    for i in range(3):
        q = _vox(p[i], G.cell[i])
        deep &= (q > 1) & (q < dims[i] - 2)
    n = []
    for i in range(3):
        hi = [c.copy() for c in p]
        lo = [c.copy() for c in p]
        hi[i] = (hi[i] + G.cell[i]).astype(f32)
        lo[i] = (lo[i] - G.cell[i]).astype(f32)
        n.append((G.trilinear(hi) - G.trilinear(lo)).astype(f32))
    with np.errstate(all="ignore"):
        ninv = f32(1) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    nrm = np.full((len(xyz), 3), np.nan, f32)
    for i in range(3):
        nrm[deep, i] = (n[i] * ninv)[deep]
    return nrm


def same_normals(a, b):
    """NaN in the same places, every other component bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(a[~np.isnan(a)], b[~np.isnan(b)])
