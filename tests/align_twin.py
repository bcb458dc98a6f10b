"""numpy restatement of volume alignment (include/hskinfu.h "Volume alignment"), written from the rule's text:
binary32 unless said, one rounding per written operator, sums left-associated, correctly rounded division and square root; the
28 sums are integers in units of 2^-26, added exactly.  The solve, the sines and cosines and the pose update are np_twin's (the
tracker's).  Also the analytic scene of the alignment tests: a room seen from inside with a box on its floor.

A volume is the host array of hsk_download_tsdf: [Z, Y, X, 2] int16 (tsdf, weight)."""
import numpy as np

import np_twin as T

f32 = np.float32
f64 = np.float64
CONVERGED, MAX_ITERS, FEW, DEGENERATE, DIVERGED = 0, 1, 2, 3, 4
STATUS = ("converged", "max_iters", "few", "degenerate", "diverged")
DEFAULTS = dict(max_iters=30, J=3, cos_gate=0.5, max_points=262144, min_points=256, eps_rot=1e-5, eps_trans_m=1e-5, max_rot=0.2)


def cells(dims, size):
    return [f32(size[i]) / f32(dims[i]) for i in range(3)]


def dot3(a, b):
    return ((a[0] * b[0] + a[1] * b[1]).astype(f32) + a[2] * b[2]).astype(f32)


def subsample(n, max_points):
    """-> (stride, the indices used)"""
    stride = max(1, -(-n // max_points))
    return stride, np.arange(0, n, stride)


def _vox_of(p, cell):
    with np.errstate(all="ignore"):
        q = np.floor((p / cell).astype(f32))
    return np.where(q >= 0, np.minimum(q, f32(1.0e6)), f32(-1)).astype(np.int64)   # (a NaN is not >= 0)


def probe(vol, size, a):
    """8d step 3's sample at the points a = (ax, ay, az), with the gradient of 8f step 2 -> (ok, F, Ws, (gx, gy, gz)); ok: not
    the NaN of the outer shell"""
    Z, Y, X, _ = vol.shape
    dims = (X, Y, Z)
    cell = cells(dims, size)
    g = [_vox_of(a[i], cell[i]) for i in range(3)]
    ok = np.ones(a[0].shape, bool)
    for i in range(3):
        ok &= (g[i] > 0) & (g[i] < dims[i] - 1)
    g = [np.clip(g[i], 1, dims[i] - 2) for i in range(3)]
    one = f32(1)
    with np.errstate(all="ignore"):
        fr = []
        for i in range(3):
            vc = ((g[i].astype(f32) + f32(0.5)) * cell[i]).astype(f32)
            g[i] = np.where(a[i] < vc, g[i] - 1, g[i])
            vc = ((g[i].astype(f32) + f32(0.5)) * cell[i]).astype(f32)
            fr.append(((a[i] - vc).astype(f32) / cell[i]).astype(f32))
        (A, B, C), (x, y, z) = fr, g
        a0, a1, b0, b1, c0, c1 = one - A, A, one - B, B, one - C, C
        f, w = {}, []
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    v = vol[z + dz, y + dy, x + dx]
                    f[dx, dy, dz] = (v[..., 0].astype(f32) / f32(32767)).astype(f32)
                    w.append(v[..., 1].astype(np.int64))
        F = f[0, 0, 0] * a0 * b0 * c0
        F = F + f[0, 0, 1] * a0 * b0 * c1
        F = F + f[0, 1, 0] * a0 * b1 * c0
        F = F + f[0, 1, 1] * a0 * b1 * c1
        F = F + f[1, 0, 0] * a1 * b0 * c0
        F = F + f[1, 0, 1] * a1 * b0 * c1
        F = F + f[1, 1, 0] * a1 * b1 * c0
        F = F + f[1, 1, 1] * a1 * b1 * c1
        gx = ((((f[1, 0, 0] - f[0, 0, 0]) * b0 * c0 + (f[1, 0, 1] - f[0, 0, 1]) * b0 * c1) + (f[1, 1, 0] - f[0, 1, 0]) * b1 * c0)
              + (f[1, 1, 1] - f[0, 1, 1]) * b1 * c1) / cell[0]
        gy = ((((f[0, 1, 0] - f[0, 0, 0]) * a0 * c0 + (f[0, 1, 1] - f[0, 0, 1]) * a0 * c1) + (f[1, 1, 0] - f[1, 0, 0]) * a1 * c0)
              + (f[1, 1, 1] - f[1, 0, 1]) * a1 * c1) / cell[1]
        gz = ((((f[0, 0, 1] - f[0, 0, 0]) * a0 * b0 + (f[0, 1, 1] - f[0, 1, 0]) * a0 * b1) + (f[1, 0, 1] - f[1, 0, 0]) * a1 * b0)
              + (f[1, 1, 1] - f[1, 1, 0]) * a1 * b1) / cell[2]
    for v in (F, gx, gy, gz):
        assert v.dtype == f32
    return ok, F, np.minimum.reduce(w), (gx, gy, gz)


def rows(vol, size, tau, ps, ns, M, J, cos_gate):
    """steps 1-4 for the points ps with normals ns ([n, 3] binary32) at M -> (used [n] bool, row [7, n] binary32)"""
    M = np.asarray(M, f32).reshape(4, 4)
    R, t = M[:3, :3], M[:3, 3]
    tau, gate = f32(tau), f32(cos_gate)
    x, y, z = (np.ascontiguousarray(ps[:, i], f32) for i in range(3))
    u, v, w = (np.ascontiguousarray(ns[:, i], f32) for i in range(3))
    n_pts = len(x)
    with np.errstate(all="ignore"):
        p = [(((R[i, 0] * x + R[i, 1] * y).astype(f32) + R[i, 2] * z).astype(f32) + t[i]).astype(f32) for i in range(3)]
        n = [((R[i, 0] * u + R[i, 1] * v).astype(f32) + R[i, 2] * w).astype(f32) for i in range(3)]
        best = np.full(n_pts, f32(2))          # |F| of the running best (a valid probe has |F| < 1)
        bF, bc, bs = (np.zeros(n_pts, f32) for _ in range(3))
        bd = [np.zeros(n_pts, f32) for _ in range(3)]
        for j in [0] + [s * k for k in range(1, J + 1) for s in (1, -1)]:
            sj = f32(f32(j) * tau)
            a = [(p[i] + (sj * n[i]).astype(f32)).astype(f32) for i in range(3)]
            ok, F, Ws, g = probe(vol, size, a)
            gg = dot3(g, g)
            ln = np.sqrt(gg).astype(f32)
            nd = [(g[i] / ln).astype(f32) for i in range(3)]
            cj = dot3(n, nd)
            aF = np.abs(F)
            take = ok & (Ws > 0) & (aF < 1) & (gg > 0) & (cj >= gate) & (aF < best)     # (strictly smaller: the earliest on a tie)
            best = np.where(take, aF, best)
            bF, bc, bs = np.where(take, F, bF), np.where(take, cj, bc), np.where(take, sj, bs).astype(f32)
            bd = [np.where(take, nd[i], bd[i]) for i in range(3)]
        used = best < 2
        c = [f32(size[i]) * f32(0.5) for i in range(3)]
        q = [(p[i] - c[i]).astype(f32) for i in range(3)]
        cr = [((q[1] * bd[2]).astype(f32) - (q[2] * bd[1]).astype(f32)).astype(f32),
              ((q[2] * bd[0]).astype(f32) - (q[0] * bd[2]).astype(f32)).astype(f32),
              ((q[0] * bd[1]).astype(f32) - (q[1] * bd[0]).astype(f32)).astype(f32)]
        r = ((bs * bc).astype(f32) - (bF * tau).astype(f32)).astype(f32)
    row = np.stack(cr + bd + [r]).astype(f32)
    return used, row


def sums(used, row):
    """step 5: the 28 sums (binary64) and n_used.  Every term is rint(product 2^26), an integer; they are added as integers
    and the total converted once (exact below 2^53 units)"""
    rw = row[:, used].astype(f64)
    out = []
    pairs = [(a, b) for a in range(6) for b in range(a, 7)] + [(6, 6)]
    for a, b in pairs:
        q = np.rint((rw[a] * rw[b]) * 67108864.0)
        out.append(float(int(q.astype(np.int64).sum())) * (1.0 / 67108864.0))
    return np.array(out, f64), int(used.sum())


def iteration(vol, size, tau, ps, ns, M, J=3, cos_gate=0.5):
    used, row = rows(vol, size, tau, ps, ns, M, J, cos_gate)
    s, n = sums(used, row)
    return s, n, used


def step(sums27, M, centre):
    """step 6's solve and centred pose update -> (M_next, x6, ok); a singular system: M, zeros, False"""
    M = np.asarray(M, f32).reshape(4, 4)
    x6, ok = T.icp_solve(np.asarray(sums27, f64)[:27])
    if not ok:
        return M.copy(), np.zeros(6, f32), False
    c = np.asarray(centre, f32)
    P = M.copy()
    P[:3, 3] = (M[:3, 3] - c).astype(f32)
    P = T.pose_update(P, x6)
    out = M.copy()
    out[:3, :3] = P[:3, :3]
    out[:3, 3] = (P[:3, 3] + c).astype(f32)
    return out, np.asarray(x6, f32), True


def default_shift(J, tau):
    return f32(f32(2) * f32(J + 1)) * f32(tau)


def align(vol, size, tau, ps, ns, M0, J=3, cos_gate=0.5, max_iters=30, max_points=262144, min_points=256, eps_rot=1e-5,
          eps_trans_m=1e-5, max_rot=0.2, max_shift_m=None):
    """the whole call -> (M_out [4, 4] binary32, stats: status, iterations, n_points, stride, n_used, rms_m, x_last, sums_last,
    used: the mask of the last iteration over the subsampled points, index: their indices in ps)"""
    ps, ns = np.asarray(ps, f32).reshape(-1, 3), np.asarray(ns, f32).reshape(-1, 3)
    stride, idx = subsample(len(ps), max_points)
    ps, ns = ps[idx], ns[idx]
    eps_rot, eps_trans_m, max_rot = f64(f32(eps_rot)), f64(f32(eps_trans_m)), f64(f32(max_rot))
    max_shift = f64(default_shift(J, tau) if max_shift_m is None else f32(max_shift_m))
    M0 = np.asarray(M0, f32).reshape(4, 4).copy()
    M = M0.copy()
    centre = [f32(size[i]) * f32(0.5) for i in range(3)]
    st = {"status": MAX_ITERS, "iterations": 0, "n_points": len(ps), "stride": stride, "n_used": [], "rms_m": [],
          "x_last": np.zeros(6, f32), "sums_last": np.zeros(28, f64), "used": np.zeros(len(ps), bool), "index": idx}
    rot_sum = shift_sum = f64(0)
    for it in range(max_iters):
        s, n_used, used = iteration(vol, size, tau, ps, ns, M, J, cos_gate)
        st["iterations"], st["sums_last"], st["used"] = it + 1, s, used
        st["n_used"].append(n_used)
        st["rms_m"].append(f32(np.sqrt(f64(s[27]) / f64(n_used))) if n_used else f32(0))
        if n_used < min_points:
            st["status"] = FEW
            break
        Mn, x6, ok = step(s, M, centre)
        if not ok:
            st["status"] = DEGENERATE
            break
        M, st["x_last"] = Mn, x6
        rot, shift = f64(np.abs(x6[:3]).max()), f64(np.abs(x6[3:]).max())
        rot_sum, shift_sum = rot_sum + rot, shift_sum + shift
        if rot_sum > max_rot or shift_sum > max_shift:
            st["status"], M = DIVERGED, M0.copy()
            break
        if rot < eps_rot and shift < eps_trans_m:
            st["status"] = CONVERGED
            break
    st["rms_m"] = np.array(st["rms_m"], f32)
    return M, st


# ---- the analytic scene ---------------------------------------------------------------------------------------------------
ROOM = ((0.3, 0.35, 0.4), (2.7, 2.6, 2.65))
FURNITURE = ((0.8, 0.35, 1.0), (1.3, 1.1, 1.5))     # it stands on the room's y = 0.35 wall
DST_DIMS, DST_SIZE = (80, 64, 48), (3.0, 3.0, 3.0)
SRC_DIMS, SRC_SIZE = (64, 64, 64), (3.0, 3.0, 3.0)
CENTRE = (1.5, 1.5, 1.5)


def _box_sdf(p, box):
    lo, hi = np.asarray(box[0]), np.asarray(box[1])
    d = np.maximum(lo - p, p - hi)
    return np.linalg.norm(np.maximum(d, 0.0), axis=-1) + np.minimum(d.max(axis=-1), 0.0)


def scene_distance(p):
    """the distance to the nearest surface at the points p [.., 3] (binary64), positive in the room's free space"""
    return np.minimum(-_box_sdf(p, ROOM), _box_sdf(p, FURNITURE))


def scene_volume(dims, size, tau, M=None):
    """the scene as a volume: raw = trunc(clip(d / tau, +-1) 32767), weight 1 where d > -tau, else (0, 0); with M, the scene
    moved by M^-1 (the distance is evaluated at M p for the voxel centre p)"""
    X, Y, Z = dims
    z, y, x = np.meshgrid((np.arange(Z) + 0.5) * (size[2] / Z), (np.arange(Y) + 0.5) * (size[1] / Y), (np.arange(X) + 0.5) * (size[0] / X),
                          indexing="ij")
    p = np.stack([x, y, z], -1)
    if M is not None:
        M = np.asarray(M, f64).reshape(4, 4)
        p = p @ M[:3, :3].T + M[:3, 3]
    d = scene_distance(p)
    vol = np.zeros((Z, Y, X, 2), np.int16)
    seen = d > -float(tau)
    vol[..., 0] = np.where(seen, np.trunc(np.clip(d / float(tau), -1.0, 1.0) * 32767.0), 0).astype(np.int16)
    vol[..., 1] = seen
    return vol


def scene_points(step=0.05):
    """surface points of the scene with unit normals towards free space, on a grid of `step` metres (binary64)"""
    pts, nrm = [], []

    def face(box, axis, side, sign):
        o = [i for i in range(3) if i != axis]
        u = np.arange(box[0][o[0]] + step / 2, box[1][o[0]], step)
        v = np.arange(box[0][o[1]] + step / 2, box[1][o[1]], step)
        uu, vv = np.meshgrid(u, v, indexing="ij")
        p = np.empty(uu.shape + (3,))
        p[..., o[0]], p[..., o[1]], p[..., axis] = uu, vv, box[side][axis]
        n = np.zeros(3)
        n[axis] = sign
        return p.reshape(-1, 3), n

    for axis in range(3):
        for side in (0, 1):
            p, n = face(ROOM, axis, side, 1.0 if side == 0 else -1.0)           # inwards
            keep = _box_sdf(p, FURNITURE) > 1e-9                                  # (not under the furniture)
            pts.append(p[keep])
            nrm.append(np.broadcast_to(n, p[keep].shape))
            if axis == 1 and side == 0:
                continue                                                          # (the furniture's face on the floor)
            p, n = face(FURNITURE, axis, side, -1.0 if side == 0 else 1.0)      # outwards
            pts.append(p)
            nrm.append(np.broadcast_to(n, p.shape))
    return np.concatenate(pts), np.concatenate(nrm)


def rigid(deg, shift_mm, axis=(1.0, 2.0, 3.0), centre=CENTRE):
    """the rotation by `deg` about `axis` through `centre`, then the shift in millimetres (binary64 4 x 4)"""
    k = np.asarray(axis, f64)
    k = k / np.linalg.norm(k)
    a = np.radians(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    c = np.asarray(centre, f64)
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = c - R @ c + np.asarray(shift_mm, f64) * 1e-3
    return m


def source_cloud(M_true, step=0.05):
    """the scene's points and normals in the coordinates of a source that M_true maps onto the scene (binary32)"""
    p, n = scene_points(step)
    inv = np.linalg.inv(np.asarray(M_true, f64))
    return (p @ inv[:3, :3].T + inv[:3, 3]).astype(f32), (n @ inv[:3, :3].T).astype(f32)


def point_error(M_out, M_true, ps):
    """the largest |M_out p - M_true p| over the points ps (binary64)"""
    a, b = np.asarray(M_out, f64), np.asarray(M_true, f64)
    p = np.asarray(ps, f64)
    return float(np.linalg.norm((p @ a[:3, :3].T + a[:3, 3]) - (p @ b[:3, :3].T + b[:3, 3]), axis=1).max()) if len(p) else 0.0
