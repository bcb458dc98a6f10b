"""numpy restatement of baked textures (include/hskinfu.h "Baked textures"), written from the rule's text: the
layout in integers and binary64, the texel rule in binary32 with one rounding per written operator, sums left-associated,
correctly rounded division and square root.  Vectorised over the texels of the atlas.

A volume is the host array of hsk_download_tsdf: [Z, Y, X, 2] int16 (tsdf, weight); a colour volume [Z, Y, X, 4] uint8
(r, g, b, w)."""
import numpy as np

f32 = np.float32
OWNED, INSIDE, PROJECTED, COLORED, NORMAL = 1, 2, 4, 8, 16
SIDES = (8, 16, 32, 64)
MAX_SIDE = 16384
CHART_DTYPE = np.dtype([("x0", np.int32), ("y0", np.int32), ("s", np.int32), ("half_rot", np.int32)])
INFO_FIELDS = ("width", "height", "n_faces_charted", "n_faces_skipped", "n_blocks", "n_owned", "n_inside", "n_projected", "n_colored", "n_normal")


class TooHigh(Exception):
    """the atlas would be higher than 16384 texels; .height is the height the mesh needs"""

    def __init__(self, height):
        super().__init__(f"H = {height}")
        self.height = height


# ---- the layout -------------------------------------------------------------------------------------------------------------------
def face_sides(vertices, faces, tpm):
    """-> (side [m] int, 0: skipped; rot [m] int): the block side and the corner opposite the longest edge of every face"""
    v = np.asarray(vertices, f32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = len(v)
    ok = ((f >= 0) & (f < n)).all(axis=1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    p = v[np.where(ok[:, None], f, 0)].astype(np.float64) if n else np.zeros((len(f), 3, 3))
    ok &= np.isfinite(p).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        d = p[:, [1, 2, 0], :] - p                                      # edge k joins corners k and k + 1 mod 3
        e2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        e2 = np.where(ok[:, None], e2, 0.0)
        kmax = np.argmax(e2, axis=1)                                    # (the first of equals: the lowest edge)
        L2 = e2[np.arange(len(f)), kmax]
        ok &= L2 > 0
        T = L2 * (np.float64(tpm) * np.float64(tpm))
    side = np.full(len(f), 64, np.int64)
    for s in (32, 16, 8):
        side = np.where(np.float64((s - 5) ** 2) >= T, s, side)
    return np.where(ok, side, 0), np.where(ok, (kmax + 2) % 3, 0)


def morton6(m):
    x = (m & 1) | ((m >> 1) & 2) | ((m >> 2) & 4)
    y = ((m >> 1) & 1) | ((m >> 2) & 2) | ((m >> 3) & 4)
    return x, y


def layout(vertices, faces, tpm, W=0):
    """-> dict: W, H, blocks (a list of (x0, y0, s, faceA, faceB, rotA, rotB)), charts [m] CHART_DTYPE, uv [m, 3, 2] float32 and
    the info counts; raises TooHigh"""
    W = W or 1024
    assert 64 <= W <= MAX_SIDE and W % 64 == 0
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    side, rot = face_sides(vertices, f, tpm)
    cols = W // 64
    off, blocks = 0, []
    charts = np.full(len(f), -1, np.int32).repeat(4).view(CHART_DTYPE)
    n_blocks = [0, 0, 0, 0]
    for s in (64, 32, 16, 8):
        ids = np.flatnonzero(side == s)
        for k in range(0, len(ids), 2):
            st, (tx, ty) = off >> 6, morton6(off & 63)
            x0, y0 = 64 * (st % cols) + 8 * tx, 64 * (st // cols) + 8 * ty
            pair = [int(i) for i in ids[k:k + 2]]
            blocks.append((x0, y0, s, pair[0], pair[1] if len(pair) > 1 else -1, int(rot[pair[0]]), int(rot[pair[1]]) if len(pair) > 1 else 0))
            for half, i in enumerate(pair):
                charts[i] = (x0, y0, s, half | (int(rot[i]) << 8))
            n_blocks[SIDES.index(s)] += 1
            off += (s // 8) ** 2
    supers = (off + 63) >> 6
    H = 64 * ((supers + cols - 1) // cols)
    info = dict(width=W, height=H, n_faces_charted=int((side > 0).sum()), n_faces_skipped=int((side == 0).sum()), n_blocks=n_blocks,
                n_owned=0, n_inside=0, n_projected=0, n_colored=0, n_normal=0)
    if H > MAX_SIDE:
        raise TooHigh(H)
    uv = np.zeros((len(f), 3, 2), f32)
    for i in np.flatnonzero(side > 0):
        x0, y0, s, hr = (int(v) for v in charts[i])
        half, r = hr & 255, hr >> 8
        for j, (cx, cy) in enumerate(((1, 1), (s - 4, 1), (1, s - 4))):
            x, y = (x0 + s - cx, y0 + s - cy) if half else (x0 + cx, y0 + cy)
            uv[i, (j + r) % 3] = (f32(np.float64(x) / np.float64(W)), f32(np.float64(1.0) - np.float64(y) / np.float64(H)))
    return dict(W=W, H=H, blocks=blocks, charts=charts, uv=uv, info=info)


# ---- the texel rule ---------------------------------------------------------------------------------------------------------------
def cells(dims, size):
    return [f32(size[i]) / f32(dims[i]) for i in range(3)]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def sample(vol, cell, p):
    """the trilinear sample's cell and taps at the points p = (px, py, pz) -> dict: inn, the lower corner g, the fractions fr, the
    eight values f[dx, dy, dz] and the smallest weight"""
    Z, Y, X, _ = vol.shape
    dims = (X, Y, Z)
    g, fr = [], []
    inn = np.ones(p[0].shape, bool)
    for i in range(3):
        q = np.floor(p[i] / cell[i])
        gi = np.where(q >= 0, np.minimum(q, f32(1.0e6)), f32(-1)).astype(np.int64)      # (a NaN is not >= 0)
        inn &= (gi > 0) & (gi < dims[i] - 1)
        gi = np.clip(gi, 1, dims[i] - 2)
        gi = np.where(p[i] < (gi.astype(f32) + f32(0.5)) * cell[i], gi - 1, gi)
        fr.append((p[i] - (gi.astype(f32) + f32(0.5)) * cell[i]) / cell[i])
        g.append(gi)
    f, w = {}, []
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                t = vol[g[2] + dz, g[1] + dy, g[0] + dx]
                f[dx, dy, dz] = t[..., 0].astype(f32) / f32(32767)
                w.append(t[..., 1].astype(np.int64))
    assert all(a.dtype == f32 for a in fr) and f[0, 0, 0].dtype == f32
    return dict(inn=inn, g=g, fr=fr, f=f, minw=np.minimum.reduce(w))


def blend(sm):
    f, (A, B, C), one = sm["f"], sm["fr"], f32(1)
    F = f[0, 0, 0] * (one - A) * (one - B) * (one - C)
    F = F + f[0, 0, 1] * (one - A) * (one - B) * C
    F = F + f[0, 1, 0] * (one - A) * B * (one - C)
    F = F + f[0, 1, 1] * (one - A) * B * C
    F = F + f[1, 0, 0] * A * (one - B) * (one - C)
    F = F + f[1, 0, 1] * A * (one - B) * C
    F = F + f[1, 1, 0] * A * B * (one - C)
    F = F + f[1, 1, 1] * A * B * C
    return F


def gradient(sm, cell):
    f, (a1, b1, c1), one = sm["f"], sm["fr"], f32(1)
    a0, b0, c0 = one - a1, one - b1, one - c1
    sx = ((((f[1, 0, 0] - f[0, 0, 0]) * b0 * c0 + (f[1, 0, 1] - f[0, 0, 1]) * b0 * c1) + (f[1, 1, 0] - f[0, 1, 0]) * b1 * c0) + (f[1, 1, 1] - f[0, 1, 1]) * b1 * c1)
    sy = ((((f[0, 1, 0] - f[0, 0, 0]) * a0 * c0 + (f[0, 1, 1] - f[0, 0, 1]) * a0 * c1) + (f[1, 1, 0] - f[1, 0, 0]) * a1 * c0) + (f[1, 1, 1] - f[1, 0, 1]) * a1 * c1)
    sz = ((((f[0, 0, 1] - f[0, 0, 0]) * a0 * b0 + (f[0, 1, 1] - f[0, 1, 0]) * a0 * b1) + (f[1, 0, 1] - f[1, 0, 0]) * a1 * b0) + (f[1, 1, 1] - f[1, 1, 0]) * a1 * b1)
    return [sx / cell[0], sy / cell[1], sz / cell[2]]


def texel_tables(lay):
    """per texel of the atlas: face (-1: unowned), half, s, the texel's place (i, j) in its block, rotation"""
    W, H = lay["W"], lay["H"]
    face = np.full((H, W), -1, np.int64)
    half, side, bi, bj, rot = (np.zeros((H, W), np.int64) for _ in range(5))
    for (x0, y0, s, fa, fb, ra, rb) in lay["blocks"]:
        j, i = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        a = i + j <= s - 2
        sl = (slice(y0, y0 + s), slice(x0, x0 + s))
        face[sl], half[sl], rot[sl] = np.where(a, fa, fb), np.where(a, 0, 1), np.where(a, ra, rb)
        side[sl], bi[sl], bj[sl] = s, i, j
    return face, half, side, bi, bj, rot


def bake(vol, col, size, vertices, faces, texels_per_metre=0.0, atlas_width=0, n_iter=4, f_tol=0.01, max_offset_m=0.0):
    """-> dict: layout()'s W, H, charts, uv, info (with the texel counts), rgb / normal_rgb [H, W, 3] uint8 (rgb zeros without col),
    mask [H, W] uint8, and points [H, W, 3] float32, the final point of every owned texel (0 elsewhere)"""
    Z, Y, X, _ = vol.shape
    cell = cells((X, Y, Z), size)
    tpm = f32(texels_per_metre) if texels_per_metre else f32(1) / min(cell)
    mo = f32(max_offset_m) if max_offset_m else f32(4) * max(cell)
    max2, tol = mo * mo, f32(f_tol)
    v = np.asarray(vertices, f32).reshape(-1, 3)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    lay = layout(v, fc, tpm, atlas_width)
    W, H = lay["W"], lay["H"]
    face, half, side, bi, bj, rot = (a.reshape(-1) for a in texel_tables(lay))
    own = np.flatnonzero(face >= 0)
    face, half, side, bi, bj, rot = (a[own] for a in (face, half, side, bi, bj, rot))
    one = f32(1)
    with np.errstate(all="ignore"):
        x, y = bi.astype(f32) + f32(0.5), bj.astype(f32) + f32(0.5)
        x, y = np.where(half == 1, side.astype(f32) - x, x), np.where(half == 1, side.astype(f32) - y, y)
        d = (side - 5).astype(f32)
        bu, bv = (x - one) / d, (y - one) / d
        bw = (one - bu) - bv
        c0, c1, c2 = (v[fc[face, (rot + j) % 3]] for j in range(3)) if len(own) else (np.zeros((0, 3), f32),) * 3
        P0 = [(c0[:, a] + bu * (c1[:, a] - c0[:, a])) + bv * (c2[:, a] - c0[:, a]) for a in range(3)]
        mask = np.full(len(own), OWNED, np.int64) | np.where((bu >= 0) & (bv >= 0) & (bw >= 0), INSIDE, 0)
        P = [a.copy() for a in P0]
        active, projected = np.ones(len(own), bool), np.zeros(len(own), bool)
        for it in range(n_iter + 1):
            sm = sample(vol, cell, P)
            active &= sm["inn"] & (sm["minw"] > 0)
            F = blend(sm)
            hit = active & (np.abs(F) <= tol)
            projected |= hit
            active &= ~hit
            if it == n_iter:
                break
            g = gradient(sm, cell)
            gg = dot3(g, g)
            active &= gg > 0
            t = F / gg
            Q = [P[a] - t * g[a] for a in range(3)]
            e = [Q[a] - P0[a] for a in range(3)]
            active &= dot3(e, e) <= max2
            P = [np.where(active, Q[a], P[a]) for a in range(3)]
        P = [np.where(projected, P[a], P0[a]) for a in range(3)]
        mask |= np.where(projected, PROJECTED, 0)
        sm = sample(vol, cell, P)
        rgb = np.zeros((len(own), 3), np.uint8)
        if col is not None:
            A, B, C = sm["fr"]
            gx, gy, gz = sm["g"]
            sw, sc = np.zeros(len(own), f32), [np.zeros(len(own), f32) for _ in range(3)]
            for dx in (0, 1):
                for dy in (0, 1):
                    for dz in (0, 1):
                        wt = (A if dx else one - A) * (B if dy else one - B) * (C if dz else one - C)
                        cw = col[gz + dz, gy + dy, gx + dx]
                        wt = np.where(cw[:, 3] > 0, wt, f32(0))
                        sw = sw + wt
                        sc = [sc[k] + wt * cw[:, k].astype(f32) for k in range(3)]
            colored = sm["inn"] & (sw > 0)
            for k in range(3):
                lvl = np.minimum(255, np.where(colored, sc[k] / sw + f32(0.5), f32(0)).astype(np.int64))
                rgb[:, k] = np.where(colored, lvl, 0)
            mask |= np.where(colored, COLORED, 0)
        g = gradient(sm, cell)
        gg = dot3(g, g)
        has_n = sm["inn"] & (sm["minw"] > 0) & (gg > 0)
        ln = np.sqrt(gg)
        nrm = np.zeros((len(own), 3), np.uint8)
        for k in range(3):
            lvl = np.rint(((g[k] / ln) * f32(0.5) + f32(0.5)) * f32(255))
            nrm[:, k] = np.where(has_n, lvl, 0).astype(np.int64)
        mask |= np.where(has_n, NORMAL, 0)
    for a in P0 + P + [bu, bv, bw]:
        assert a.dtype == f32
    out = dict(W=W, H=H, charts=lay["charts"], uv=lay["uv"], blocks=lay["blocks"])
    full = {"rgb": np.zeros((H * W, 3), np.uint8), "normal_rgb": np.zeros((H * W, 3), np.uint8), "mask": np.zeros(H * W, np.uint8),
            "points": np.zeros((H * W, 3), f32)}
    full["rgb"][own], full["normal_rgb"][own], full["mask"][own], full["points"][own] = rgb, nrm, mask, np.stack(P, axis=1) if len(own) else 0
    out.update(rgb=full["rgb"].reshape(H, W, 3), normal_rgb=full["normal_rgb"].reshape(H, W, 3), mask=full["mask"].reshape(H, W),
               points=full["points"].reshape(H, W, 3))
    info = dict(lay["info"])
    for name, bit in (("n_owned", OWNED), ("n_inside", INSIDE), ("n_projected", PROJECTED), ("n_colored", COLORED), ("n_normal", NORMAL)):
        info[name] = int(((mask & bit) != 0).sum())
    out["info"] = info
    return out
