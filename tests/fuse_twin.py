"""numpy restatement of volume fusion (include/hskinfu.h "Volume fusion"), written from the rule's text: binary32
throughout, one rounding per written operator, rint ties-to-even, correctly rounded division; the integer merges in int64.  The
twin sweeps EVERY destination voxel -- no footprint, no skip test -- so it also says what those may not change.

Volumes are the host arrays of hsk_download_tsdf / hsk_download_color: [Z, Y, X, 2] int16 (tsdf, weight) and [Z, Y, X, 4] uint8
(r, g, b, w)."""
import numpy as np

f32 = np.float32
MAX_WEIGHT = 128


def cells(dims, size):
    """the contexts' binary32 cells: size / dims per axis (dims = (X, Y, Z))"""
    return [f32(size[i]) / f32(dims[i]) for i in range(3)]


def is_rigid(m):
    m = np.asarray(m, f32).reshape(4, 4)
    if not (m[3, 0] == 0 and m[3, 1] == 0 and m[3, 2] == 0 and m[3, 3] == 1):
        return False
    R = m[:3, :3].astype(np.float64)
    for i in range(3):
        for j in range(3):
            g = (R[0, i] * R[0, j] + R[1, i] * R[1, j]) + R[2, i] * R[2, j]
            if not abs(g - (1.0 if i == j else 0.0)) <= 1e-4:
                return False
    return True


def invert_rigid(m):
    """step 1: (R^T, -R^T t) in binary64 from the binary32 entries, rounded once"""
    m = np.asarray(m, f32).reshape(4, 4)
    if not is_rigid(m):
        raise ValueError("not rigid")
    R, t = m[:3, :3].astype(np.float64), m[:3, 3].astype(np.float64)
    inv = np.zeros((4, 4), f32)
    inv[:3, :3] = m[:3, :3].T
    for i in range(3):
        inv[i, 3] = f32(-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]))
    inv[3, 3] = 1
    return inv


def footprint(src_dims, src_size, dst_dims, dst_size, m):
    """hsk_fuse_footprint: the image of the source's interior [cell, (dims - 1) cell] under m (the box of its corners'
    images, binary64), padded by one destination cell, clipped; all zeros when empty"""
    m = np.asarray(m, f32).reshape(4, 4)
    if not is_rigid(m):
        raise ValueError("not rigid")
    R, t = m[:3, :3].astype(np.float64), m[:3, 3].astype(np.float64)
    cs = [np.float64(c) for c in cells(src_dims, src_size)]
    cd = [np.float64(c) for c in cells(dst_dims, dst_size)]
    lo = [cs[i] for i in range(3)]
    hi = [np.float64(src_dims[i] - 1) * cs[i] for i in range(3)]
    mn, mx = [np.inf] * 3, [-np.inf] * 3
    for c in range(8):
        p = [hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]]
        for i in range(3):
            q = ((R[i, 0] * p[0] + R[i, 1] * p[1]) + R[i, 2] * p[2]) + t[i]
            mn[i], mx[i] = min(mn[i], q), max(mx[i], q)
    box = []
    for i in range(3):
        if not np.isfinite(mn[i]) or not np.isfinite(mx[i]):
            return (0,) * 6
        a = max(np.floor(mn[i] / cd[i]) - 1.0, 0.0)
        b = min(np.floor(mx[i] / cd[i]) + 2.0, float(dst_dims[i]))
        if not a < b:
            return (0,) * 6
        box += [int(a), int(b)]
    return tuple(box)


def _vox_of(p, cell):
    with np.errstate(all="ignore"):
        q = np.floor((p / cell).astype(f32))
    g = np.where(q >= 0, np.minimum(q, f32(1.0e6)), f32(-1))   # (a NaN is not >= 0)
    return g.astype(np.int64)


def sample(src, src_size, ps):
    """step 3's sample at the points ps = (px, py, pz) (binary32 arrays of one shape): (ok, Fs, Ws, voxel) -- ok: not the NaN
    of the outer shell; Fs binary32; Ws the smallest weight of the eight taps; voxel: the (x, y, z) that contain the points,
    clamped to the interior (the colour rule's voxel where ok)"""
    Z, Y, X, _ = src.shape
    dims = (X, Y, Z)
    cell = cells(dims, src_size)
    g = [_vox_of(ps[i], cell[i]) for i in range(3)]
    ok = np.ones(ps[0].shape, bool)
    for i in range(3):
        ok &= (g[i] > 0) & (g[i] < dims[i] - 1)
    g = [np.clip(g[i], 1, dims[i] - 2) for i in range(3)]
    vox = [x.copy() for x in g]
    fr = []
    with np.errstate(all="ignore"):
        for i in range(3):
            vc = ((g[i].astype(f32) + f32(0.5)) * cell[i]).astype(f32)
            g[i] = np.where(ps[i] < vc, g[i] - 1, g[i])
            vc = ((g[i].astype(f32) + f32(0.5)) * cell[i]).astype(f32)
            fr.append(((ps[i] - vc).astype(f32) / cell[i]).astype(f32))
        a, b, c = fr
        one = f32(1)
        x, y, z = g

        def tap(dx, dy, dz):
            v = src[z + dz, y + dy, x + dx]
            return (v[..., 0].astype(f32) / f32(32767)).astype(f32), v[..., 1].astype(np.int64)

        taps = {(dx, dy, dz): tap(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
        F = lambda k: taps[k][0]  # noqa: E731
        res = F((0, 0, 0)) * (one - a) * (one - b) * (one - c)
        res = res + F((0, 0, 1)) * (one - a) * (one - b) * c
        res = res + F((0, 1, 0)) * (one - a) * b * (one - c)
        res = res + F((0, 1, 1)) * (one - a) * b * c
        res = res + F((1, 0, 0)) * a * (one - b) * (one - c)
        res = res + F((1, 0, 1)) * a * (one - b) * c
        res = res + F((1, 1, 0)) * a * b * (one - c)
        res = res + F((1, 1, 1)) * a * b * c
    assert res.dtype == f32
    Ws = np.minimum.reduce([w for _, w in taps.values()])
    return ok, res, Ws, vox


def fuse(dst, dst_size, src, src_size, m, dst_color=None, src_color=None, max_w=64, planes=16):
    """dst <- dst (+) resample(src) under m (source -> destination).  -> (tsdf, colour or None, stats): the new destination
    arrays (the inputs are not changed) and dict(n_fused, n_colored, fused: the bool mask [Z, Y, X] of voxels that took a
    sample, box: the bounding box of that mask (x0 x1 y0 y1 z0 z1, half-open) or None).  Colour is merged iff both colour
    volumes are given."""
    inv = invert_rigid(m)
    A, b = inv[:3, :3], inv[:3, 3]
    Z, Y, X, _ = dst.shape
    cd = cells((X, Y, Z), dst_size)
    out = dst.copy()
    colour = dst_color is not None and src_color is not None
    out_c = dst_color.copy() if dst_color is not None else None
    fused = np.zeros((Z, Y, X), bool)
    n_colored = 0
    pdx = ((np.arange(X).astype(f32) + f32(0.5)) * cd[0]).astype(f32)[None, None, :]
    pdy = ((np.arange(Y).astype(f32) + f32(0.5)) * cd[1]).astype(f32)[None, :, None]
    for z0 in range(0, Z, planes):
        z1 = min(Z, z0 + planes)
        pdz = ((np.arange(z0, z1).astype(f32) + f32(0.5)) * cd[2]).astype(f32)[:, None, None]
        with np.errstate(all="ignore"):
            ps = [(((A[i, 0] * pdx + A[i, 1] * pdy).astype(f32) + (A[i, 2] * pdz).astype(f32)).astype(f32) + b[i]).astype(f32)
                  for i in range(3)]
        ps = [np.broadcast_to(p, (z1 - z0, Y, X)) for p in ps]
        ok, Fs, Ws, vox = sample(src, src_size, ps)
        take = ok & (Ws > 0)
        with np.errstate(all="ignore"):
            q = np.rint((Fs * f32(32767)).astype(f32))
        q = np.clip(np.where(take, q, 0), -32767, 32767).astype(np.int64)
        d = out[z0:z1]
        rd, Wd = d[..., 0].astype(np.int64), d[..., 1].astype(np.int64)
        n = rd * Wd + q * Ws
        W = np.maximum(Wd + Ws, 1)
        raw = np.sign(n) * ((2 * np.abs(n) + W) // (2 * W))
        d[..., 0] = np.where(take, raw, rd).astype(np.int16)
        d[..., 1] = np.where(take, np.minimum(W, MAX_WEIGHT), Wd).astype(np.int16)
        fused[z0:z1] = take
        if colour:
            cs = src_color[vox[2], vox[1], vox[0]].astype(np.int64)
            dc = out_c[z0:z1]
            cdv = dc.astype(np.int64)
            ws, wd = cs[..., 3], cdv[..., 3]
            mix = take & (ws != 0)
            w = np.maximum(wd + ws, 1)
            for ch in range(3):
                c = (cdv[..., ch] * wd + cs[..., ch] * ws + (w >> 1)) // w
                dc[..., ch] = np.where(mix, c, cdv[..., ch]).astype(np.uint8)
            dc[..., 3] = np.where(mix, np.minimum(w, max_w), wd).astype(np.uint8)
            n_colored += int(mix.sum())
    box = None
    if fused.any():
        zz, yy, xx = np.nonzero(fused)
        box = (int(xx.min()), int(xx.max()) + 1, int(yy.min()), int(yy.max()) + 1, int(zz.min()), int(zz.max()) + 1)
    return out, out_c, {"n_fused": int(fused.sum()), "n_colored": n_colored, "fused": fused, "box": box}


def box_contains(outer, inner):
    return inner is None or all(outer[2 * i] <= inner[2 * i] and inner[2 * i + 1] <= outer[2 * i + 1] for i in range(3))


def crossings(vol, size):
    """the zero crossings of a volume along x, y and z between neighbouring observed voxels (one value < 0, the other >= 0), at
    the linear interpolation of the two values -> [n, 3] float64 points"""
    Z, Y, X, _ = vol.shape
    cell = [float(c) for c in cells((X, Y, Z), size)]
    F = vol[..., 0].astype(np.float64)
    W = vol[..., 1]
    zc, yc, xc = np.meshgrid((np.arange(Z) + 0.5) * cell[2], (np.arange(Y) + 0.5) * cell[1], (np.arange(X) + 0.5) * cell[0], indexing="ij")
    P = np.stack([xc, yc, zc], -1)
    pts = []
    for axis in range(3):                      # array axis 0 = z, 1 = y, 2 = x
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        Fa, Fb = F[lo], F[hi]
        cut = (W[lo] > 0) & (W[hi] > 0) & ((Fa < 0) != (Fb < 0))
        s = Fa[cut] / (Fa[cut] - Fb[cut])
        pts.append(P[lo][cut] + s[:, None] * (P[hi][cut] - P[lo][cut]))
    return np.concatenate(pts)


def rot_about(axis, deg, centre, shift=(0.0, 0.0, 0.0)):
    """a rigid matrix: the rotation by `deg` about `axis` through `centre`, then the translation `shift` (binary32)"""
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    R = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    R = np.array(R, np.float64)
    ce = np.asarray(centre, np.float64)
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = ce - R @ ce + np.asarray(shift, np.float64)
    return m.astype(f32)


def translation(t):
    m = np.eye(4, dtype=f32)
    m[:3, 3] = np.asarray(t, f32)
    return m
