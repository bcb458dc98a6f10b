"""numpy restatement of keyframe textures (include/hskinfu.h "Keyframe textures"), written from the rule's text over
tests/texture_twin.py: the layout, the points, the normal map and the low mask bits are the texture twin's bake; the keyframe
lookup is binary32 with one rounding per written operator, sums left-associated, correctly rounded division and square root,
vectorised over the texels and sequential over the keyframes in ascending index.

A keyframe is a dict: depth (h, w) uint16 millimetres, rgb (h, w, 3) uint8, pose (4, 4) float32 camera-to-world, intr [4] float32
(fx fy cx cy)."""
import numpy as np

import texture_twin as TT

f32 = np.float32
KEYFRAME, BEST, BLEND, NONE = 32, 0, 1, 255
KINFO_FIELDS = ("n_keyframes", "n_keyed", "n_fallback", "n_uncolored", "n_pairs_seen", "n_pairs_occluded")


def default_params(cell_max):
    """hsk_default_keytex_params: stated choices"""
    return dict(mode=BEST, z_min_m=0.3, z_max_m=4.0, cos_min=0.2, border_px=4.0, occlusion_tol_m=float(f32(3) * f32(cell_max)), blend_floor=0.5,
                fallback_volume=1)


def keyframe(depth, rgb, pose, intr):
    return dict(depth=np.ascontiguousarray(depth, np.uint16), rgb=np.ascontiguousarray(rgb, np.uint8), pose=np.asarray(pose, f32).reshape(4, 4),
                intr=np.asarray(intr, f32).reshape(4))


def unit_normals(vol, cell, P):
    """the gradient over its length at the points P, as texture_twin.bake forms the normal -> (n [3] arrays, has_n)"""
    sm = TT.sample(vol, cell, P)
    g = TT.gradient(sm, cell)
    gg = TT.dot3(g, g)
    has_n = sm["inn"] & (sm["minw"] > 0) & (gg > 0)
    ln = np.sqrt(gg)
    return [g[k] / ln for k in range(3)], has_n


def geometry(kf, q, n, kp):
    """steps 1 to 3 -> dict: ok, zc, weight, iu, iv, a, b (meaningful where ok)"""
    R, t = kf["pose"][:3, :3], kf["pose"][:3, 3]
    fx, fy, cx, cy = kf["intr"]
    h, w = kf["depth"].shape
    d = [q[i] - t[i] for i in range(3)]
    xc, yc, zc = (TT.dot3(d, [R[0, j], R[1, j], R[2, j]]) for j in range(3))
    ok = (zc >= f32(kp["z_min_m"])) & (zc <= f32(kp["z_max_m"]))
    r2 = TT.dot3(d, d)
    c = -TT.dot3(n, d) / np.sqrt(r2)
    ok &= c >= f32(kp["cos_min"])
    u, v = fx * (xc / zc) + cx, fy * (yc / zc) + cy
    bd = f32(kp["border_px"])
    ok &= (u >= bd) & (u <= f32(w - 1) - bd) & (v >= bd) & (v <= f32(h - 1) - bd)
    iu = np.minimum(np.where(ok, u, 0).astype(np.int64), w - 2)
    iv = np.minimum(np.where(ok, v, 0).astype(np.int64), h - 2)
    out = dict(ok=ok, zc=zc, weight=c / r2, iu=iu, iv=iv, a=u - iu.astype(f32), b=v - iv.astype(f32))
    for name in ("zc", "weight", "a", "b"):
        assert out[name].dtype == f32, name
    return out


def taps(kf, g, kp):
    """steps 4 and 5 -> (visible, val [3] float32 arrays)"""
    tol = f32(kp["occlusion_tol_m"])
    vis = np.ones(g["ok"].shape, bool)
    for dj in (0, 1):
        for di in (0, 1):
            D = kf["depth"][g["iv"] + dj, g["iu"] + di]
            vis &= (D != 0) & (np.abs(g["zc"] - D.astype(f32) * f32(0.001)) <= tol)
    val = []
    for ch in range(3):
        c = kf["rgb"][..., ch].astype(f32)
        c00, c10, c01, c11 = c[g["iv"], g["iu"]], c[g["iv"], g["iu"] + 1], c[g["iv"] + 1, g["iu"]], c[g["iv"] + 1, g["iu"] + 1]
        top, bot = c00 + g["a"] * (c10 - c00), c01 + g["a"] * (c11 - c01)
        val.append(top + g["b"] * (bot - top))
        assert val[-1].dtype == f32
    return vis, val


def lookup(keyframes, q, n, kp):
    """the keyframe rule at the points q with unit normals n -> dict: keyed, rgb [m, 3] uint8, source [m] uint8, seen, occluded"""
    m = len(q[0])
    best = np.full(m, -1, np.int64)
    wmax = np.zeros(m, f32)
    bval = [np.zeros(m, f32) for _ in range(3)]
    seen = occluded = 0
    passing = []
    with np.errstate(all="ignore"):
        for k, kf in enumerate(keyframes):
            g = geometry(kf, q, n, kp)
            vis, val = taps(kf, g, kp)
            seen += int(g["ok"].sum())
            occluded += int((g["ok"] & ~vis).sum())
            ok = g["ok"] & vis
            passing.append((ok, g["weight"], val))
            take = ok & ((best < 0) | (g["weight"] > wmax))
            best = np.where(take, k, best)
            wmax = np.where(take, g["weight"], wmax)
            bval = [np.where(take, val[c], bval[c]) for c in range(3)]
        if kp["mode"] == BLEND:
            floor_w = f32(kp["blend_floor"]) * wmax
            sw, s = np.zeros(m, f32), [np.zeros(m, f32) for _ in range(3)]
            for ok, wk, val in passing:
                use = ok & (wk >= floor_w)
                sw = np.where(use, sw + wk, sw)
                s = [np.where(use, s[c] + wk * val[c], s[c]) for c in range(3)]
            bval = [np.where(sw > 0, s[c] / sw, bval[c]) for c in range(3)]
        keyed = best >= 0
        rgb = np.stack([np.minimum(255, np.where(keyed, bval[c] + f32(0.5), f32(0)).astype(np.int64)) for c in range(3)], axis=1).astype(np.uint8)
    return dict(keyed=keyed, rgb=rgb, source=np.where(keyed, best, NONE).astype(np.uint8), seen=seen, occluded=occluded)


def bake(vol, col, size, vertices, faces, keyframes, keytex=None, **params):
    """-> texture_twin.bake's dict (mask with KEYFRAME, COLORED only where the colour volume coloured the texel) plus source [H, W]
    uint8 and kinfo"""
    base = TT.bake(vol, col, size, vertices, faces, **params)
    Z, Y, X, _ = vol.shape
    cell = TT.cells((X, Y, Z), size)
    kp = default_params(max(cell))
    kp.update(keytex or {})
    H, W = base["mask"].shape
    mask, rgb = base["mask"].reshape(-1).copy(), base["rgb"].reshape(-1, 3).copy()
    source = np.full(H * W, NONE, np.uint8)
    idx = np.flatnonzero(mask & TT.NORMAL)
    P = [base["points"].reshape(-1, 3)[idx, a] for a in range(3)]
    with np.errstate(all="ignore"):
        n, has_n = unit_normals(vol, cell, P)
    assert has_n.all()
    lk = lookup(keyframes, P, n, kp)
    keyed = np.zeros(H * W, bool)
    keyed[idx] = lk["keyed"]
    source[idx] = lk["source"]
    if not (kp["fallback_volume"] and col is not None):
        rgb[:] = 0
        mask &= ~np.uint8(TT.COLORED)
    rgb[idx[lk["keyed"]]] = lk["rgb"][lk["keyed"]]
    mask[keyed] = (mask[keyed] & ~np.uint8(TT.COLORED)) | np.uint8(KEYFRAME)
    out = dict(base, rgb=rgb.reshape(H, W, 3), mask=mask.reshape(H, W), source=source.reshape(H, W))
    info = dict(base["info"])
    info["n_colored"] = int(((mask & TT.COLORED) != 0).sum())
    out["info"] = info
    owned = int(((mask & TT.OWNED) != 0).sum())
    out["kinfo"] = dict(n_keyframes=len(keyframes), n_keyed=int(keyed.sum()), n_fallback=info["n_colored"],
                        n_uncolored=owned - int(keyed.sum()) - info["n_colored"], n_pairs_seen=lk["seen"], n_pairs_occluded=lk["occluded"])
    return out
