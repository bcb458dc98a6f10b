"""numpy twin of the cloud import's rule (housescan_amd/csrc/hsk_splat_point.h; include/hskinfu.h "Cloud import"):
the same operations in the same order, every one rounded to binary32, vectorised over the points.  splat() is hsk_splat_cloud's
image and counters for one view."""
import numpy as np

f32 = np.float32
DISC, SURFEL = 0, 1
INVALID, CLIPPED, BACKFACING, OUTSIDE, DONE = range(5)
STATS = ("n_invalid", "n_clipped", "n_backfacing", "n_outside", "n_splatted", "n_pixels")
FLT_MAX = np.finfo(f32).max
EMPTY = 0xFFFFFFFF


def camera(width, height, fx, fy, cx, cy):
    return dict(width=int(width), height=int(height), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy))


def params(point_size_m=None, mode=DISC, cover=1.5, min_half_px=0.5, max_half_px=8.0, near_m=0.1, far_m=8.0):
    """hsk_default_splat_params without a context, the keywords over it"""
    ps = f32(3.0) / f32(512.0) if point_size_m is None else f32(point_size_m)
    return dict(mode=int(mode), point_size_m=ps, cover=f32(cover), min_half_px=f32(min_half_px), max_half_px=f32(max_half_px),
                near_m=f32(near_m), far_m=f32(far_m))


def half_m(p):
    return (f32(0.5) * p["point_size_m"]) * p["cover"]


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def finite(x):
    return np.abs(x) <= FLT_MAX            # (a NaN fails the comparison)


def mm(z):
    d = np.rint(z * f32(1000.0))
    d = np.where(~(d >= f32(1.0)), f32(1.0), d)
    d = np.where(~(d <= f32(65535.0)), f32(65535.0), d)
    return d.astype(np.int64)


def span(c, r, n):
    a, b = np.ceil(c - r), np.floor(c + r)
    last = f32(n - 1)
    ok = (b >= f32(0.0)) & (a <= last)
    a = np.where(a < f32(0.0), f32(0.0), a)
    b = np.where(b > last, last, b)
    lo, hi = np.where(ok, a, 0).astype(np.int64), np.where(ok, b, 0).astype(np.int64)
    return ok & (lo <= hi), lo, hi


def points(xyz, normals, pose, cam, p):
    """splat_point for every point -> (class [n], the footprints and planes of all points as a dict of [n] arrays)"""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    m = np.asarray(pose, f32).reshape(4, 4)
    R, t = m[:3, :3], m[:3, 3]
    h = half_m(p)
    with np.errstate(all="ignore"):
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        cls = np.full(len(xyz), DONE, np.int64)
        fin = finite(x) & finite(y) & finite(z)
        dx, dy, dz = x - t[0], y - t[1], z - t[2]
        xc = dot3(dx, dy, dz, R[0, 0], R[1, 0], R[2, 0])
        yc = dot3(dx, dy, dz, R[0, 1], R[1, 1], R[2, 1])
        zc = dot3(dx, dy, dz, R[0, 2], R[1, 2], R[2, 2])
        inside = (zc >= p["near_m"]) & (zc <= p["far_m"])
        surfel = np.zeros(len(xyz), bool)
        ncx = ncy = ncz = pn = z_lo = z_hi = np.zeros(len(xyz), f32)
        if p["mode"] == SURFEL and normals is not None:
            nrm = np.ascontiguousarray(normals, f32).reshape(-1, 3)
            nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
            has = finite(nx) & finite(ny) & finite(nz) & ~((nx == 0) & (ny == 0) & (nz == 0))
            ncx = dot3(nx, ny, nz, R[0, 0], R[1, 0], R[2, 0])
            ncy = dot3(nx, ny, nz, R[0, 1], R[1, 1], R[2, 1])
            ncz = dot3(nx, ny, nz, R[0, 2], R[1, 2], R[2, 2])
            pn = dot3(ncx, ncy, ncz, xc, yc, zc)
            surfel = has
            band = f32(2.0) * h
            z_lo, z_hi = zc - band, zc + band
        back = surfel & ~(pn < f32(0.0))
        u0, v0 = cam["fx"] * (xc / zc) + cam["cx"], cam["fy"] * (yc / zc) + cam["cy"]
        ru, rv = (cam["fx"] * h) / zc, (cam["fy"] * h) / zc
        ru = np.minimum(np.maximum(ru, p["min_half_px"]), p["max_half_px"])
        rv = np.minimum(np.maximum(rv, p["min_half_px"]), p["max_half_px"])
        oku, u_lo, u_hi = span(u0, ru, cam["width"])
        okv, v_lo, v_hi = span(v0, rv, cam["height"])
        z_mm = mm(zc)
    cls[~(oku & okv)] = OUTSIDE
    cls[back] = BACKFACING
    cls[~inside] = CLIPPED
    cls[~fin] = INVALID
    return cls, dict(u_lo=u_lo, u_hi=u_hi, v_lo=v_lo, v_hi=v_hi, z_mm=z_mm, surfel=surfel, ncx=ncx, ncy=ncy, ncz=ncz, pn=pn, z_lo=z_lo, z_hi=z_hi)


def offers(cam, f, idx, u, v):
    """splat_offer of the points idx at their pixels (u, v)"""
    out = f["z_mm"][idx].copy()
    s = f["surfel"][idx]
    if s.any():
        i = idx[s]
        with np.errstate(all="ignore"):
            rx, ry = (u[s].astype(f32) - cam["cx"]) / cam["fx"], (v[s].astype(f32) - cam["cy"]) / cam["fy"]
            zs = f["pn"][i] / dot3(f["ncx"][i], f["ncy"][i], f["ncz"][i], rx, ry, f32(1.0))
            zs = np.where(~(zs >= f["z_lo"][i]), f["z_lo"][i], zs)
            zs = np.where(~(zs <= f["z_hi"][i]), f["z_hi"][i], zs)
            out[s] = mm(zs)
    return out


def splat(xyz, normals, pose, cam, p):
    """-> (depth (height, width) uint16, stats dict): a pixel holds the smallest depth offered to it, 0 without an offer"""
    cls, f = points(xyz, normals, pose, cam, p)
    w, h = cam["width"], cam["height"]
    zbuf = np.full(w * h, EMPTY, np.int64)
    live = np.flatnonzero(cls == DONE)
    if len(live):
        nu, nv = f["u_hi"][live] - f["u_lo"][live], f["v_hi"][live] - f["v_lo"][live]
        for dv in range(int(nv.max()) + 1):
            for du in range(int(nu.max()) + 1):
                sel = (du <= nu) & (dv <= nv)
                if not sel.any():
                    continue
                idx = live[sel]
                u, v = f["u_lo"][idx] + du, f["v_lo"][idx] + dv
                np.minimum.at(zbuf, v * w + u, offers(cam, f, idx, u, v))
    depth = np.where(zbuf == EMPTY, 0, zbuf).astype(np.uint16).reshape(h, w)
    st = {name: int((cls == k).sum()) for k, name in enumerate(STATS[:5])}
    st["n_pixels"] = int((depth != 0).sum())
    return depth, st
