"""numpy restatement of a section view (include/hskinfu.h "Section views"), written from the rule's text:
binary32 throughout, one rounding per written operator, no contraction, correctly rounded / and sqrt.  Steps 1-7 (ray, box,
clip, march, hit, cut, class) stand here in full; the voxel look-up and the trilinear sample are np_twin's (A.6), the Lambert
term of a point light and the colour look-up view_twin's (8b).  Also the two host-side operations: a house section in a
room's frame (binary64, rounded once) and the composite of several views."""
import numpy as np

import view_twin as VT
from np_twin import _Grid, _vox, tau_of

f32 = np.float32
PINHOLE, ORTHO = 0, 1
HIT, CUT, BACKGROUND = 1, 2, 0


def section(width, height, fx, fy, cx, cy, pose, projection=PINHOLE, clip=(), mode=VT.LAMBERT, light=(0.0, 0.0, 0.0),
            light_in_camera=True, light_directional=False, background=(0, 0, 0), cut_rgb=(255, 96, 0)):
    """a section as a dict (the fields of hsk_section, follow = 0)"""
    return dict(width=int(width), height=int(height), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy),
                pose=np.asarray(pose, f32).reshape(4, 4).copy(), projection=int(projection),
                clip=[tuple(f32(v) for v in pl) for pl in clip], mode=int(mode), light=tuple(f32(v) for v in light),
                light_in_camera=bool(light_in_camera), light_directional=bool(light_directional),
                background=tuple(int(v) for v in background), cut_rgb=tuple(int(v) for v in cut_rgb))


def rays(sec):
    """step 1 -> o[3], d[3], each (H, W) float32"""
    W, H = sec["width"], sec["height"]
    R, t = sec["pose"][:3, :3], sec["pose"][:3, 3]
    x = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W))
    rx = ((x - sec["cx"]) / sec["fx"]).astype(f32)
    ry = ((y - sec["cy"]) / sec["fy"]).astype(f32)
    lat = [(R[i, 0] * rx + R[i, 1] * ry).astype(f32) for i in range(3)]
    if sec["projection"] == ORTHO:
        o = [(lat[i] + t[i]).astype(f32) for i in range(3)]
        d = [np.full((H, W), R[i, 2], f32) for i in range(3)]
    else:
        o = [np.full((H, W), t[i], f32) for i in range(3)]
        d = [(lat[i] + R[i, 2] * f32(1.0)).astype(f32) for i in range(3)]
    with np.errstate(all="ignore"):
        inv = (f32(1) / np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(f32))).astype(f32)
    d = [(d[i] * inv).astype(f32) for i in range(3)]
    d = [np.where(d[i] == 0, f32(1e-15), d[i]).astype(f32) for i in range(3)]
    return o, d


def box(o, d, size):
    """step 2 -> t_box, t_exit"""
    sz = [f32(s) for s in size]
    zero = f32(0)
    with np.errstate(all="ignore"):
        tmin = [((np.where(d[i] > 0, zero, sz[i]) - o[i]) / d[i]).astype(f32) for i in range(3)]
        tmax = [((np.where(d[i] > 0, sz[i], zero) - o[i]) / d[i]).astype(f32) for i in range(3)]
    t_box = np.fmax(np.fmax(np.fmax(tmin[0], tmin[1]), tmin[2]), zero).astype(f32)
    t_exit = np.fmin(np.fmin(tmax[0], tmax[1]), tmax[2]).astype(f32)
    return t_box, t_exit


def clip_rays(o, d, t_box, t_exit, planes):
    """step 3 -> t_start, t_exit, alive"""
    t_start, t_exit = t_box.copy(), t_exit.copy()
    alive = np.ones(t_box.shape, bool)
    for (a, b, c, e) in planes:
        s0 = (((a * o[0] + b * o[1]).astype(f32) + c * o[2]).astype(f32) + e).astype(f32)
        sd = ((a * d[0] + b * d[1]).astype(f32) + c * d[2]).astype(f32)
        with np.errstate(all="ignore"):
            tp = ((-s0) / sd).astype(f32)
        t_start = np.where(sd > 0, np.fmax(t_start, tp), t_start).astype(f32)
        t_exit = np.where(sd < 0, np.fmin(t_exit, tp), t_exit).astype(f32)
        alive &= ~((sd == 0) & (s0 < 0))
    return t_start, t_exit, alive


def march(vol, size, trunc, o, d, t_start, marching):
    """step 4: A.6's loop with D2 / D3 from t_start along o + d * time for the rays of `marching` -> vmap, nmap (3, H, W)"""
    Z, Y, X, _ = vol.shape
    G = _Grid(vol, size, Z, 0)
    cell, dims = G.cell, (X, Y, Z)
    tau = tau_of(size, dims, trunc)
    sz = [f32(s) for s in size]
    step = tau * f32(0.8)
    max_time = f32(3) * ((sz[0] + sz[1]) + sz[2])
    H, W = t_start.shape
    vm = np.full((3, H, W), np.nan, f32)
    nm = np.full((3, H, W), np.nan, f32)
    alive = marching.copy()
    tc = t_start.astype(f32).copy()

    def point(tt, sel):
        return [(o[k][sel] + d[k][sel] * tt).astype(f32) for k in range(3)]

    while True:
        alive &= tc < max_time
        if not alive.any():
            break
        sel = np.nonzero(alive)
        tcur = tc[sel]
        tn = (tcur + step).astype(f32)
        far = point(tn, sel)
        g = [_vox(far[k], cell[k]) for k in range(3)]
        inside = np.ones(len(tcur), bool)
        for k in range(3):
            inside &= (g[k] >= 0) & (g[k] < dims[k])
        # far sample outside the grid: the ray ends
        alive[sel[0][~inside], sel[1][~inside]] = False
        keep = np.nonzero(inside)[0]
        sel = (sel[0][keep], sel[1][keep])
        tcur, tn = tcur[keep], tn[keep]
        g = [gk[keep] for gk in g]
        near = point(tcur, sel)
        pv = [np.clip(_vox(near[k], cell[k]), 0, dims[k] - 1) for k in range(3)]
        r_near = G.at(pv[0], pv[1], pv[2])
        r_far = G.at(g[0], g[1], g[2])
        back = (r_near < 0) & (r_far > 0)
        cross = (r_near > 0) & (r_far < 0)
        if cross.any():
            c = np.nonzero(cross)[0]
            csel = (sel[0][c], sel[1][c])
            tcc = tcur[c]
            p_far, p_near = point(tn[c], csel), point(tcc, csel)
            Ftdt, Ft = G.trilinear(p_far), G.trilinear(p_near)
            with np.errstate(all="ignore"):
                Ts = (tcc - ((step * Ft).astype(f32) / (Ftdt - Ft).astype(f32)).astype(f32)).astype(f32)
                good = ~np.isnan(Ftdt) & ~np.isnan(Ft) & (Ts >= (tcc - step).astype(f32)) & (Ts <= (tcc + f32(2.0) * step).astype(f32))
            gi = np.nonzero(good)[0]
            if len(gi):
                gsel = (csel[0][gi], csel[1][gi])
                vtx = point(Ts[gi], gsel)
                for k in range(3):
                    vm[k][gsel] = vtx[k]
                q = [_vox(p_near[k][gi], cell[k]) for k in range(3)]     # the near sample's voxel, unclamped
                deep = np.ones(len(gi), bool)
                for k in range(3):
                    deep &= (q[k] > 1) & (q[k] < dims[k] - 2)
                di = np.nonzero(deep)[0]
                if len(di):
                    dsel = (gsel[0][di], gsel[1][di])
                    base = [vtx[k][di] for k in range(3)]
                    n = []
                    for k in range(3):
                        hi, lo = [b.copy() for b in base], [b.copy() for b in base]
                        hi[k] = (hi[k] + cell[k]).astype(f32)
                        lo[k] = (lo[k] - cell[k]).astype(f32)
                        n.append((G.trilinear(hi) - G.trilinear(lo)).astype(f32))
                    with np.errstate(all="ignore"):   # (a zero gradient: 0 * inf = NaN, no normal)
                        ninv = (f32(1) / np.sqrt(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]).astype(f32))).astype(f32)
                        for k in range(3):
                            nm[k][dsel] = (n[k] * ninv).astype(f32)
        ended = back | cross
        alive[sel[0][ended], sel[1][ended]] = False
        tc[sel[0][~ended], sel[1][~ended]] = tn[~ended]
    return vm, nm


def brightness(vm, nm, sec):
    """step 9 (int32; meaningful on hits)"""
    if not sec["light_directional"]:
        return VT.brightness(vm, nm, sec["pose"], sec["light"], sec["light_in_camera"])
    R = sec["pose"][:3, :3]
    l = [f32(v) for v in sec["light"]]
    if sec["light_in_camera"]:
        l = [f32(f32(f32(R[i, 0] * l[0]) + f32(R[i, 1] * l[1])) + f32(R[i, 2] * l[2])) for i in range(3)]
    with np.errstate(all="ignore"):
        s = f32(f32(f32(l[0] * l[0]) + f32(l[1] * l[1])) + f32(l[2] * l[2]))
        dot = ((l[0] * nm[0] + l[1] * nm[1]).astype(f32) + l[2] * nm[2]).astype(f32)
        w = (dot * f32(f32(1) / np.sqrt(s))).astype(f32)
        w = np.where(w > 0, w, f32(0)).astype(f32)
        w = np.where((s == 0) | np.isnan(nm[0]), f32(0), w).astype(f32)
        br = 50 + (f32(205) * w).astype(f32).astype(np.int32)
    return np.minimum(255, br)


def depth_of(p, pose, valid):
    """step 8 (8b step 3): along the optical axis from the camera's t, millimetres, 0 outside 1..65535"""
    R, t = pose[:3, :3], pose[:3, 3]
    with np.errstate(all="ignore"):
        zc = ((R[0, 2] * (p[0] - t[0]) + R[1, 2] * (p[1] - t[1])).astype(f32) + R[2, 2] * (p[2] - t[2])).astype(f32)
        dd = np.rint((zc * f32(1000)).astype(f32))
        return np.where(valid & (dd >= 1) & (dd <= 65535), dd, 0).astype(np.uint16)


def render(vol, size, trunc, sec, color=None):
    """-> dict(rgb, depth, vmap, nmap, cls (H, W: HIT / CUT / BACKGROUND), n_hit, n_cut, n_uncolored, raw_hit: what the march
    found before the planes and the cut were applied)"""
    Z, Y, X, _ = vol.shape
    dims = (X, Y, Z)
    o, d = rays(sec)
    t_box, t_exit = box(o, d, size)
    t_start, t_exit, alive = clip_rays(o, d, t_box, t_exit, sec["clip"])
    with np.errstate(all="ignore"):
        marching = alive & (t_start < t_exit)
    vm, nm = march(vol, size, trunc, o, d, t_start, marching)
    raw_hit = ~np.isnan(vm[0])
    # step 5
    hit = raw_hit.copy()
    for (a, b, c, e) in sec["clip"]:
        with np.errstate(all="ignore"):
            s = (((a * vm[0] + b * vm[1]).astype(f32) + c * vm[2]).astype(f32) + e).astype(f32)
        hit &= s >= 0
    # step 6
    G = _Grid(vol, size, Z, 0)
    raised = marching & (t_start > t_box)
    ts = np.where(raised, t_start, f32(0)).astype(f32)
    ps = [(o[k] + d[k] * ts).astype(f32) for k in range(3)]
    pv = [np.clip(_vox(ps[k], G.cell[k]), 0, dims[k] - 1) for k in range(3)]
    cut = raised & (G.at(pv[0], pv[1], pv[2]) < 0)
    # step 7
    hit &= ~cut
    vm = np.where(hit[None], vm, f32(np.nan)).astype(f32)
    nm = np.where(hit[None], nm, f32(np.nan)).astype(f32)
    H, W = hit.shape
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:] = np.asarray(sec["background"], np.uint8)
    mode = sec["mode"]
    n_unc = 0
    if mode in (VT.LAMBERT, VT.COLOR_LIT):
        br = brightness(vm, nm, sec)
    if mode == VT.LAMBERT:
        rgb[hit] = br[hit][:, None].astype(np.uint8)
    elif mode == VT.NORMALS:
        has_n = hit & ~np.isnan(nm[0])
        for i in range(3):
            c = np.rint(((nm[i] * f32(0.5) + f32(0.5)).astype(f32) * f32(255)).astype(f32))
            rgb[..., i][has_n] = c[has_n].astype(np.int32).astype(np.uint8)
    else:
        g = []
        for i in range(3):
            with np.errstate(all="ignore"):
                q = np.floor((vm[i] / G.cell[i]).astype(f32))
            g.append(np.clip(np.where(hit, q, 0), 0, dims[i] - 1).astype(np.int64))
        cw = color[g[2], g[1], g[0]]
        unc = hit & (cw[..., 3] == 0)
        n_unc = int(unc.sum())
        c = np.where(unc[..., None], 0, cw[..., :3]).astype(np.int64)
        if mode == VT.COLOR_LIT:
            c = (c * br[..., None].astype(np.int64) + 127) // 255
        rgb[hit] = c[hit].astype(np.uint8)
    rgb[cut] = np.asarray(sec["cut_rgb"], np.uint8)
    depth = depth_of(vm, sec["pose"], hit)
    depth[cut] = depth_of(ps, sec["pose"], cut)[cut]
    cls = np.where(cut, CUT, np.where(hit, HIT, BACKGROUND)).astype(np.int8)
    return dict(rgb=rgb, depth=depth, vmap=vm, nmap=nm, cls=cls, n_hit=int(hit.sum()), n_cut=int(cut.sum()), n_uncolored=n_unc,
                raw_hit=raw_hit)


def in_room(sec, room_xf):
    """hsk_section_in_room: M = room -> house (4x4, rigid); binary64 from the binary32 inputs, sums left to right, one rounding"""
    M = np.asarray(room_xf, f32).reshape(4, 4).astype(np.float64)
    R, t = M[:3, :3], M[:3, 3]

    def direction(v):
        return np.array([(R[0, i] * v[0] + R[1, i] * v[1]) + R[2, i] * v[2] for i in range(3)])

    def point(p):
        return direction([p[0] - t[0], p[1] - t[1], p[2] - t[2]])

    out = dict(sec)
    P = sec["pose"].astype(np.float64)
    pose = np.eye(4, dtype=f32)
    for c in range(3):
        pose[:3, c] = direction(P[:3, c]).astype(f32)
    pose[:3, 3] = point(P[:3, 3]).astype(f32)
    out["pose"] = pose
    planes = []
    for pl in sec["clip"]:
        n = [float(v) for v in pl]
        abc = [f32((n[0] * R[0, j] + n[1] * R[1, j]) + n[2] * R[2, j]) for j in range(3)]
        planes.append((abc[0], abc[1], abc[2], f32(((n[0] * t[0] + n[1] * t[1]) + n[2] * t[2]) + n[3])))
    out["clip"] = planes
    if not sec["light_in_camera"]:
        l = [float(v) for v in sec["light"]]
        out["light"] = tuple(f32(v) for v in (direction(l) if sec["light_directional"] else point(l)))
    return out


def composite(rgbs, depths, background):
    """hsk_composite_views: the smallest non-zero depth wins, the lowest index on a tie"""
    dep = np.stack([np.asarray(x, np.uint16) for x in depths]).astype(np.int64)
    key = np.where(dep == 0, 1 << 20, dep)
    idx = np.argmin(key, axis=0)                       # (the first of equal minima)
    none = (dep == 0).all(axis=0)
    H, W = none.shape
    yy, xx = np.mgrid[0:H, 0:W]
    out_d = np.where(none, 0, dep[idx, yy, xx]).astype(np.uint16)
    out_i = np.where(none, -1, idx).astype(np.int32)
    out_rgb = None
    if rgbs is not None:
        col = np.stack([np.asarray(c, np.uint8) for c in rgbs])
        out_rgb = col[idx, yy, xx]
        out_rgb[none] = np.asarray(background, np.uint8)
    return out_rgb, out_d, out_i


def to_struct(sec, _lib):
    """the dict as an `_lib.HskSection`"""
    s = _lib.HskSection()
    v = s.view
    v.width, v.height = sec["width"], sec["height"]
    v.fx, v.fy, v.cx, v.cy = float(sec["fx"]), float(sec["fy"]), float(sec["cx"]), float(sec["cy"])
    v.pose[:] = [float(x) for x in sec["pose"].reshape(16)]
    v.follow, v.mode = 0, sec["mode"]
    v.light[:] = [float(x) for x in sec["light"]]
    v.light_in_camera = int(sec["light_in_camera"])
    v.background[:] = list(sec["background"])
    s.projection, s.light_directional, s.n_clip = sec["projection"], int(sec["light_directional"]), len(sec["clip"])
    for c, pl in enumerate(sec["clip"]):
        s.clip[c][:] = [float(x) for x in pl]
    s.cut_rgb[:] = list(sec["cut_rgb"])
    return s


def from_struct(s):
    v = s.view
    return section(v.width, v.height, v.fx, v.fy, v.cx, v.cy, np.array(v.pose, f32).reshape(4, 4), s.projection,
                   [tuple(s.clip[c]) for c in range(s.n_clip)], v.mode, tuple(v.light), bool(v.light_in_camera),
                   bool(s.light_directional), tuple(v.background), tuple(s.cut_rgb))


def look(eye, target, up):
    """a cam->world pose at `eye` whose z axis points at `target`; x = up x z, y = z x x"""
    z = np.asarray(target, float) - np.asarray(eye, float)
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4, dtype=f32)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P

