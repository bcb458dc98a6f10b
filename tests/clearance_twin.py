"""The clearance field's rule in numpy: the obstacle predicate, the default parameters, the separable capped form
the kernels run -- one windowed minimum per axis, every intermediate above max_d2 replaced by "far" -- and, for tiny volumes, the
literal minimum over all obstacles and border terms; the floor map; the point lookup.  All integers (int64 inside, uint32 out).
A volume is the host layout [z, y, x, 2] int16: (tsdf, weight)."""
import numpy as np

f32 = np.float32
UNKNOWN = 1
FAR = 0xFFFFFFFF
OUTSIDE = 0xFFFFFFFE
MAX_REACH = 255
INF = 1 << 40        # "far" between the passes


def obstacles(vol, flags):
    """[z, y, x] bool: SOLID (weight != 0 and tsdf <= 0); with UNKNOWN also UNSEEN (weight == 0)"""
    solid = (vol[..., 1] != 0) & (vol[..., 0] <= 0)
    return solid | (vol[..., 1] == 0) if flags & UNKNOWN else solid


def reach(max_d2, w):
    """floor(sqrt(max_d2 / w)) in binary64 -- and the largest r with w r^2 <= max_d2, in integers: the two agree"""
    r = int(np.floor(np.sqrt(np.float64(max_d2) / np.float64(w))))
    assert w * r * r <= max_d2 < w * (r + 1) * (r + 1)
    return r


def default_params(size_m, dims):
    """hsk_default_clearance_params for a volume of size_m metres and dims voxels -> dict: weight, max_d2, flags, unit_m"""
    cell = [f32(size_m[i]) / f32(dims[i]) for i in range(3)]
    cmin = min(cell)
    if cell[0] == cell[1] == cell[2]:
        weight, unit = (1, 1, 1), f32(cmin)
    else:
        weight = tuple(int(min(1024.0, np.rint(16.0 * (np.float64(c) / np.float64(cmin)) ** 2))) for c in cell)
        unit = f32(np.float64(cmin) / 4.0)
    inv = 1.0 / np.float64(unit)
    max_d2 = int(min(np.ceil(inv * inv), 255.0 * 255.0 * min(weight)))
    return {"weight": weight, "max_d2": max_d2, "flags": UNKNOWN, "unit_m": unit}


def d2_of_metres(unit_m, metres):
    q = np.float64(f32(metres)) / np.float64(f32(unit_m))
    return int(min(np.ceil(q * q), float(FAR))) if metres > 0 else 0


def _pass(g, axis, w, max_d2, flags):
    """one capped windowed pass along `axis` of the int64 array g (values <= max_d2 or INF)"""
    n = g.shape[axis]
    R = reach(max_d2, w)
    out = g.copy()
    for j in range(1, min(R, n - 1) + 1):
        lo, hi = [slice(None)] * g.ndim, [slice(None)] * g.ndim
        lo[axis], hi[axis] = slice(0, n - j), slice(j, n)
        lo, hi = tuple(lo), tuple(hi)
        out[hi] = np.minimum(out[hi], g[lo] + w * j * j)
        out[lo] = np.minimum(out[lo], g[hi] + w * j * j)
    if flags & UNKNOWN:
        i = np.arange(n, dtype=np.int64)
        e = np.minimum(i + 1, n - i)
        shape = [1] * g.ndim
        shape[axis] = n
        out = np.minimum(out, (w * e * e).reshape(shape))
    return np.where(out <= max_d2, out, INF)


def transform(obst, weights, max_d2, flags, axes):
    """the separable capped form over the given axes of a bool array, weights in the axes' order -> uint32, FAR above max_d2"""
    g = np.where(obst, np.int64(0), np.int64(INF))
    for axis, w in zip(axes, weights):
        g = _pass(g, axis, int(w), int(max_d2), flags)
    return np.where(g <= max_d2, g, FAR).astype(np.uint32)


def field(vol, weight, max_d2, flags):
    """the field [z, y, x] uint32 of a volume: x, then y, then z, as the kernels run it"""
    return transform(obstacles(vol, flags), weight, max_d2, flags, (2, 1, 0))


def literal(obst, weights, max_d2, flags, axes=(2, 1, 0)):
    """the literal minimum over all obstacles and, with UNKNOWN, the border terms (tiny arrays only) -> uint32"""
    idx = np.indices(obst.shape).astype(np.int64)
    best = np.full(obst.shape, INF, np.int64)
    for o in np.argwhere(obst):
        d = np.zeros(obst.shape, np.int64)
        for axis, w in zip(axes, weights):
            d += int(w) * (idx[axis] - o[axis]) ** 2
        best = np.minimum(best, d)
    if flags & UNKNOWN:
        for axis, w in zip(axes, weights):
            n = obst.shape[axis]
            e = np.minimum(idx[axis] + 1, n - idx[axis])
            best = np.minimum(best, int(w) * e * e)
    return np.where(best <= max_d2, best, FAR).astype(np.uint32)


def stats(vol, fld, flags):
    near = fld[fld != FAR]
    return {"n_obstacle": int(obstacles(vol, flags).sum()), "n_far": int((fld == FAR).sum()), "max_d2_seen": int(near.max()) if near.size else 0}


def floor_map(vol, weight, max_d2, flags, axis, lo, hi):
    """the floor map [v, u] uint32 for the up axis (0 x, 1 y, 2 z) and its planes lo <= p < hi; u: the lower-numbered remaining axis"""
    np_axis = 2 - axis                        # the array's axis of the up axis
    band = [slice(None)] * 3
    band[np_axis] = slice(lo, hi)
    col = obstacles(vol, flags)[tuple(band)].any(axis=np_axis)      # [v, u]: the remaining axes keep their order, the higher first
    au, av = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    return transform(col, (weight[au], weight[av]), max_d2, flags, (1, 0))


def floor_stats(fmap):
    near = fmap[fmap != FAR]
    return {"n_obstacle": int((fmap == 0).sum()), "n_far": int((fmap == FAR).sum()), "max_d2_seen": int(near.max()) if near.size else 0}


def vox_of(p, cell):
    """hsk_vox_of_q(hsk_div_by_const(p, 1 / cell)): the binary32 quotient's floor, -1 below 0 and for a NaN, 1000000 above 1e6"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((np.asarray(p, f32) / f32(cell)).astype(f32))
    out = np.full(q.shape, -1, np.int64)
    ok = q >= 0
    out[ok] = np.where(q[ok] > 1.0e6, 1000000, np.minimum(q[ok], 1.0e6)).astype(np.int64)
    return out


def lookup(fld, size_m, xyz):
    """hsk_clearance_at: the field at the voxels of the points, OUTSIDE where the unclamped voxel is not in the grid"""
    Z, Y, X = fld.shape
    pts = np.asarray(xyz, f32).reshape(-1, 3)
    g = [vox_of(pts[:, i], f32(size_m[i]) / f32(n)) for i, n in enumerate((X, Y, Z))]
    inside = (g[0] >= 0) & (g[0] < X) & (g[1] >= 0) & (g[1] < Y) & (g[2] >= 0) & (g[2] < Z)
    c = [np.clip(g[i], 0, n - 1) for i, n in enumerate((X, Y, Z))]
    return np.where(inside, fld[c[2], c[1], c[0]], np.uint32(OUTSIDE)).astype(np.uint32)


def rank_views_clear(scores, eye_d2, min_d2):
    """hsk_rank_views_clear: larger gain first, ties to the larger n_frontier, then the lower index; behind all others, in the same
    order, the poses with eye_state != 0, eye_d2 < min_d2 or eye_d2 == OUTSIDE"""
    d = np.asarray(eye_d2, np.uint64)
    behind = (scores["eye_state"] != 0) | (d < min_d2) | (d == OUTSIDE)
    return np.array(sorted(range(len(scores)), key=lambda i: (bool(behind[i]), -int(scores["gain"][i]), -int(scores["n_frontier"][i]), i)), np.uint32)
