"""The scene split in numpy: the rule hsk_split_scene, hsk_download_split, hsk_split_at and hsk_remove_objects follow,
restated with none of the kernels' machinery -- whole-array arithmetic in int64, the three binary64 products of the ALIGNED test,
scipy's labelling renumbered to the smallest lin, a literal search of a point's neighbourhood, a literal Chebyshev dilation.  A
volume is the host layout [z, y, x, 2] int16: (tsdf, weight); a colour volume [z, y, x, 4] uint8."""
import numpy as np
from scipy import ndimage

import clearance_twin as CT
from diff_twin import default_min_voxels, dilate

NONE_CLS, FLOOR, CEILING, WALL, OTHER, OBJECT, MINOR = range(7)
ERASE, RESTORE = 0, 1
NO_PLANE = 0xFF
NONE = 0xFFFFFFFF
COS30 = np.float32(0.8660254)


def cells_of(size_m, dims):
    """the context's binary32 cells"""
    return [np.float32(size_m[i]) / np.float32(dims[i]) for i in range(3)]


def effective_tau(size_m, dims, trunc_dist_m=0.03):
    """hsk_create's tau: trunc_dist_m, but at least 2.1 times the largest cell, in binary32"""
    lo = np.float32(2.1) * max(cells_of(size_m, dims))
    return max(np.float32(trunc_dist_m), np.float32(lo))


def default_params(size_m, dims, tau=None):
    tau = effective_tau(size_m, dims) if tau is None else np.float32(tau)
    return dict(dist_m=np.float32(0.04), back_m=np.float32(tau + np.float32(0.04)), cos_min=COS30, min_voxels=default_min_voxels(size_m, dims, tau))


def default_halo(size_m, dims, tau=None):
    tau = effective_tau(size_m, dims) if tau is None else np.float32(tau)
    return int(min(8.0, max(1.0, np.ceil(np.float64(tau) / np.float64(min(cells_of(size_m, dims)))) + 1.0)))


def plane_kinds(abcd, up, level_cos=np.cos(np.radians(15.0)), wall_sin=np.sin(np.radians(15.0))):
    """hsk_split_plane_kinds, in binary64 from the binary32 inputs"""
    a = np.asarray(abcd, np.float32).reshape(-1, 4)[:, :3].astype(np.float64)
    u = np.asarray(up, np.float32).astype(np.float64)
    level_cos, wall_sin = np.float64(np.float32(level_cos)), np.float64(np.float32(wall_sin))
    la = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    lu = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    t = ((a[:, 0] * u[0] + a[:, 1] * u[1]) + a[:, 2] * u[2]) / (la * lu)
    return np.where(t >= level_cos, FLOOR, np.where(t <= -level_cos, CEILING, np.where(np.abs(t) <= wall_sin, WALL, OTHER))).astype(np.int32)


def quantise(abcd, kinds, size_m, dims, tau, dist_m, back_m, cos_min):
    """the host's conversion, once, in binary64 from the binary32 inputs, with rint -> the rule's integers"""
    a = np.asarray(abcd, np.float32).reshape(-1, 4).astype(np.float64)
    c = np.array(cells_of(size_m, dims), np.float64)
    r = {"Q": np.rint((a[:, :3] * c[None, :]) * 2.0 ** 29).astype(np.int64), "Qd": np.rint(a[:, 3] * 2.0 ** 30).astype(np.int64),
         "N": np.rint(a[:, :3] * 4096.0).astype(np.int64), "kind": np.asarray(kinds, np.int64).reshape(-1),
         "front": int(np.rint(np.float64(np.float32(dist_m)) * 2.0 ** 30)), "back": int(np.rint(np.float64(np.float32(back_m)) * 2.0 ** 30)),
         "tauq": int(np.rint(np.float64(np.float32(tau)) * 2.0 ** 30)), "cos2": np.float64(np.float32(cos_min)) * np.float64(np.float32(cos_min)),
         "w": np.rint((4096.0 * c.min()) / c).astype(np.int64)}
    floors = np.flatnonzero(r["kind"] == FLOOR)
    r["floor"] = int(floors[0]) if len(floors) else -1
    return r


def inside(vol):
    return (vol[..., 1] != 0) & (vol[..., 0] < 0)


def gradient(vol):
    """g [3] (x, y, z), each [z, y, x] int64: central differences of r = max(raw, -32767) where both neighbours are observed, twice
    the one-sided difference where one is, 0 where neither; outside the grid counts as unobserved"""
    r, ob = np.maximum(vol[..., 0].astype(np.int64), -32767), vol[..., 1] != 0
    out = []
    for ax in (2, 1, 0):
        pad = [(0, 0)] * 3
        pad[ax] = (1, 1)
        rp, op = np.pad(r, pad), np.pad(ob, pad)
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -2), slice(2, None)
        lo, hi = tuple(lo), tuple(hi)
        g = np.where(op[lo] & op[hi], rp[hi] - rp[lo], np.where(op[hi], 2 * (rp[hi] - r), np.where(op[lo], 2 * (r - rp[lo]), 0)))
        out.append(g)
    return out


def distance(rule, k, shape):
    """s_k of every voxel, int64, in units of 2^-30 m"""
    Z, Y, X = shape
    z, y, x = np.meshgrid(2 * np.arange(Z, dtype=np.int64) + 1, 2 * np.arange(Y, dtype=np.int64) + 1, 2 * np.arange(X, dtype=np.int64) + 1, indexing="ij")
    Q = rule["Q"][k]
    return Q[0] * x + Q[1] * y + Q[2] * z + rule["Qd"][k]


def classify(vol, rule):
    """the class and the plane of every voxel before the MINOR step -> (cls, plane [z, y, x] uint8, n_edge, n_no_normal)"""
    ins = inside(vol)
    g = gradient(vol)
    G = [g[j] * rule["w"][j] for j in range(3)]
    G2 = G[0] * G[0] + G[1] * G[1] + G[2] * G[2]
    big = np.int64(1) << 62
    q_abs, m_abs = np.full(vol.shape[:3], big), np.full(vol.shape[:3], big)
    q_k, m_k, m = np.full(vol.shape[:3], -1), np.full(vol.shape[:3], -1), np.zeros(vol.shape[:3], np.int64)
    for k in range(len(rule["Q"])):
        s = distance(rule, k, vol.shape[:3])
        N = rule["N"][k]
        near = (s >= -rule["back"]) & (s <= rule["front"])
        dot = G[0] * N[0] + G[1] * N[1] + G[2] * N[2]
        N2 = np.float64(N[0] * N[0] + N[1] * N[1] + N[2] * N[2])
        d = dot.astype(np.float64)
        aligned = (G2 == 0) | ((dot > 0) & (d * d >= rule["cos2"] * (G2.astype(np.float64) * N2)))
        a = np.abs(s)
        m += near
        take = near & (a < m_abs)                       # (ascending k, strictly below: of equal |s| the lower index stays)
        m_abs, m_k = np.where(take, a, m_abs), np.where(take, k, m_k)
        take = near & aligned & (a < q_abs)
        q_abs, q_k = np.where(take, a, q_abs), np.where(take, k, q_k)
    edge = ins & (q_k < 0) & (m >= 2)
    pk = np.where(q_k >= 0, q_k, np.where(m >= 2, m_k, -1))
    kinds = np.concatenate([rule["kind"], [OBJECT]])        # (index -1: no plane)
    cls = np.where(ins, kinds[pk], NONE_CLS).astype(np.uint8)
    plane = np.where(ins & (pk >= 0), pk, NO_PLANE).astype(np.uint8)
    return cls, plane, int(edge.sum()), int((ins & (G2 == 0)).sum())


def neighbours(a, fill):
    """the six face neighbours' values of every voxel, `fill` outside the grid"""
    p = np.pad(a, 1, constant_values=fill)
    Z, Y, X = a.shape
    return [p[1:-1, 1:-1, 0:X], p[1:-1, 1:-1, 2:X + 2], p[1:-1, 0:Y, 1:-1], p[1:-1, 2:Y + 2, 1:-1], p[0:Z, 1:-1, 1:-1], p[2:Z + 2, 1:-1, 1:-1]]


def objects(cls, plane, rule, min_voxels):
    """the 6-connected components of OBJECT -> (final classes, labels [z, y, x] uint32, records, n_minor_objects): a record is a
    dict -- root (x, y, z), n_voxels, sum, lo, hi (exclusive), contact [4], plane_mask, height_lo, height_hi --, the records of the
    kept objects ordered by n_voxels descending, ties to the smaller root"""
    Z, Y, X = cls.shape
    obj = cls == OBJECT
    lab, n = ndimage.label(obj)                           # (the default structure: face neighbours only)
    out, label, recs = cls.copy(), np.full(cls.shape, NONE, np.uint32), []
    if n == 0:
        return out, label, recs, 0
    lin = np.arange(cls.size, dtype=np.int64).reshape(cls.shape)
    roots = ndimage.minimum(lin, lab, np.arange(1, n + 1)).astype(np.int64)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    boxes = ndimage.find_objects(lab)
    kept = sizes >= min_voxels
    kept_of = np.concatenate([[False], kept])[lab]
    out[obj & ~kept_of] = MINOR
    label[kept_of] = roots[lab[kept_of] - 1].astype(np.uint32)
    ncls, npl = neighbours(cls, NONE_CLS), neighbours(plane, NO_PLANE)
    touch = [np.zeros(cls.shape, bool) for _ in range(4)]
    mask = np.zeros(cls.shape, np.uint64)
    for c, p in zip(ncls, npl):
        for kind in range(1, 5):
            touch[kind - 1] |= c == kind
        struct = (c >= FLOOR) & (c <= OTHER)
        mask |= np.where(struct, np.uint64(1) << (p & 63).astype(np.uint64), np.uint64(0))
    height = (distance(rule, rule["floor"], cls.shape) >> 14) if rule["floor"] >= 0 else np.zeros(cls.shape, np.int64)
    for i in np.flatnonzero(kept):
        r, (sz, sy, sx) = int(roots[i]), boxes[i]
        me = lab == i + 1
        z, y, x = np.nonzero(me)
        recs.append({"root": (r % X, r // X % Y, r // (X * Y)), "n_voxels": int(sizes[i]), "sum": (int(x.sum()), int(y.sum()), int(z.sum())),
                     "lo": (sx.start, sy.start, sz.start), "hi": (sx.stop, sy.stop, sz.stop), "contact": tuple(int((t & me).sum()) for t in touch),
                     "plane_mask": int(np.bitwise_or.reduce(mask[me])), "height_lo": int(height[me].min()), "height_hi": int(height[me].max())})
    recs.sort(key=lambda c: (-c["n_voxels"], (c["root"][2] * Y + c["root"][1]) * X + c["root"][0]))
    return out, label, recs, int((~kept).sum())


def split(vol, rule, min_voxels):
    """hsk_split_scene -> (cls, plane, object, records, stats)"""
    cls, plane, n_edge, n_flat = classify(vol, rule)
    cls, label, recs, n_minor = objects(cls, plane, rule, min_voxels)
    stats = {"n_class": [int((cls == c).sum()) for c in range(7)], "n_objects": len(recs), "n_minor_objects": n_minor,
             "largest": recs[0]["n_voxels"] if recs else 0, "n_edge": n_edge, "n_no_normal": n_flat}
    return cls, plane, label, recs, stats


def split_at(cls, plane, label, size_m, xyz, radius):
    """hsk_split_at -> (cls [n] uint8, plane [n] uint8, object [n] uint32): among the voxels within Chebyshev `radius` of the point's
    voxel whose class is not NONE the one with the smallest (dx^2 + dy^2 + dz^2, lin); with none, or outside the grid: NONE, 0xff,
    NONE"""
    Z, Y, X = cls.shape
    pts = np.asarray(xyz, np.float32).reshape(-1, 3)
    g = [CT.vox_of(pts[:, i], np.float32(size_m[i]) / np.float32(n)) for i, n in enumerate((X, Y, Z))]
    out_c, out_p, out_o = np.full(len(pts), NONE_CLS, np.uint8), np.full(len(pts), NO_PLANE, np.uint8), np.full(len(pts), NONE, np.uint32)
    for e in range(len(pts)):
        x, y, z = int(g[0][e]), int(g[1][e]), int(g[2][e])
        if not (0 <= x < X and 0 <= y < Y and 0 <= z < Z):
            continue
        z0, z1, y0, y1, x0, x1 = max(z - radius, 0), min(z + radius + 1, Z), max(y - radius, 0), min(y + radius + 1, Y), max(x - radius, 0), min(x + radius + 1, X)
        cz, cy, cx = np.nonzero(cls[z0:z1, y0:y1, x0:x1] != NONE_CLS)
        if len(cz) == 0:
            continue
        cz, cy, cx = cz + z0, cy + y0, cx + x0
        key = ((cx - x) ** 2 + (cy - y) ** 2 + (cz - z) ** 2).astype(np.int64) * (1 << 32) + (cz * Y + cy) * X + cx
        i = int(np.argmin(key))
        out_c[e], out_p[e], out_o[e] = cls[cz[i], cy[i], cx[i]], plane[cz[i], cy[i], cx[i]], label[cz[i], cy[i], cx[i]]
    return out_c, out_p, out_o


def remove(vol, label, recs, rule, roots=None, mode=RESTORE, halo=3, fill_weight=1, color=None):
    """hsk_remove_objects for the kept objects' labels and records -> (the new volume, the new colour volume or None, stats)"""
    Z, Y, X = vol.shape[:3]
    by_root = {(c["root"][2] * Y + c["root"][1]) * X + c["root"][0]: c for c in recs}
    chosen = list(by_root) if roots is None else list(dict.fromkeys(int(r) for r in roots))
    T = np.isin(label, np.array(chosen, np.uint32)) if chosen else np.zeros(label.shape, bool)
    H = dilate(T, halo) if chosen else T
    in_box, A = np.zeros(label.shape, bool), np.zeros(label.shape, np.uint64)
    for r in chosen:
        c = by_root[r]
        box = tuple(slice(max(c["lo"][a] - halo, 0), min(c["hi"][a] + halo, (X, Y, Z)[a])) for a in (2, 1, 0))
        in_box[box] = True
        A[box] |= np.uint64(c["plane_mask"])
    big = np.int64(1) << 62
    s = np.full(label.shape, big)
    for k in range(len(rule["Q"])):
        has = ((A >> np.uint64(k)) & np.uint64(1)) != 0
        if has.any():
            s = np.where(has, np.minimum(s, distance(rule, k, label.shape)), s)
    tq = rule["tauq"]
    raw = (65534 * np.minimum(s, tq) + tq) // (2 * tq)       # (floor division)
    observed = vol[..., 1] != 0
    rule1 = (mode == RESTORE) & (A != 0) & in_box & (H | ~observed)
    rule2 = ~rule1 & (T | (H & observed & ~inside(vol)))
    filled = rule1 & (s >= -tq)
    out = vol.copy()
    out[rule1 | rule2] = 0
    out[..., 0][filled] = raw[filled].astype(np.int16)
    out[..., 1][filled] = fill_weight
    written = rule1 | rule2
    col = None
    if color is not None:
        col = color.copy()
        col[written] = 0
    n = int(written.sum())
    return out, col, {"n_objects": len(chosen), "n_targets": int(T.sum()), "n_written": n, "n_restored": int(filled.sum()), "n_colored": n if color is not None else 0}


def room_planes(wall_x=50.4, floor_z=6.3, cell=0.05):
    """the analytic room's floor (solid below z = floor_z, up is +z) and wall (solid beyond x = wall_x), exactly, for a cubic cell:
    ([2, 4] float32, kinds)"""
    return np.array([[0.0, 0.0, 1.0, -floor_z * cell], [-1.0, 0.0, 0.0, wall_x * cell]], np.float32), np.array([FLOOR, WALL], np.int32)
