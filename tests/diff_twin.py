"""Volume differencing in numpy: the rule hsk_diff_volume, hsk_download_diff, hsk_diff_at and hsk_adopt_diff
follow, restated with none of the kernels' machinery -- whole-array comparisons, scipy's labelling renumbered to the smallest lin,
a literal search of a point's neighbourhood, a literal Chebyshev dilation.  All integers.  A volume is the host layout
[z, y, x, 2] int16: (tsdf, weight); a colour volume [z, y, x, 4] uint8."""
import numpy as np
from scipy import ndimage

import clearance_twin as CT

UNSEEN, ONLY_REF, ONLY_CUR, SAME, APPEARED, VANISHED, MINOR = range(7)
ADOPT_APPEARED, ADOPT_VANISHED = 1, 2
NONE = 0xFFFFFFFF
DEFAULT_THRESH = 16384


def value(vol):
    """a word's value: its raw TSDF, -32768 counting as -32767"""
    return np.maximum(vol[..., 0].astype(np.int32), -32767)


def classify(ref, cur, thresh=DEFAULT_THRESH, min_weight=1):
    """the class of every voxel before the MINOR step -> [z, y, x] uint8"""
    oa, ob = ref[..., 1] >= min_weight, cur[..., 1] >= min_weight
    d = value(cur) - value(ref)
    cls = np.full(ref.shape[:3], UNSEEN, np.uint8)
    cls[oa & ~ob] = ONLY_REF
    cls[~oa & ob] = ONLY_CUR
    cls[oa & ob] = SAME
    cls[oa & ob & (d <= -thresh)] = APPEARED
    cls[oa & ob & (d >= thresh)] = VANISHED
    return cls


def regions(cls, min_voxels):
    """the 6-connected components of CHANGED -> (final classes, labels [z, y, x] uint32, records, n_minor_regions): the label of a
    kept region's voxel is the region's smallest lin, NONE everywhere else; a record is a dict -- root (x, y, z), n_voxels,
    n_appeared, n_vanished, lo, hi (x, y, z; hi exclusive) --, the records ordered by n_voxels descending, ties to the smaller root"""
    Z, Y, X = cls.shape
    changed = (cls == APPEARED) | (cls == VANISHED)
    lab, n = ndimage.label(changed)                       # (the default structure: face neighbours only)
    out, region, recs, n_minor = cls.copy(), np.full(cls.shape, NONE, np.uint32), [], 0
    if n == 0:
        return out, region, recs, n_minor
    lin = np.arange(cls.size, dtype=np.int64).reshape(cls.shape)
    ids = np.arange(1, n + 1)
    roots = ndimage.minimum(lin, lab, ids).astype(np.int64)
    sizes = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    n_app = np.bincount(lab[cls == APPEARED], minlength=n + 1)[1:]
    boxes = ndimage.find_objects(lab)
    kept = sizes >= min_voxels
    kept_of = np.concatenate([[False], kept])[lab]
    out[changed & ~kept_of] = MINOR
    region[kept_of] = roots[lab[kept_of] - 1].astype(np.uint32)
    for i in np.flatnonzero(kept):
        r, (sz, sy, sx) = int(roots[i]), boxes[i]
        recs.append({"root": (r % X, r // X % Y, r // (X * Y)), "n_voxels": int(sizes[i]), "n_appeared": int(n_app[i]),
                     "n_vanished": int(sizes[i] - n_app[i]), "lo": (sx.start, sy.start, sz.start), "hi": (sx.stop, sy.stop, sz.stop)})
    recs.sort(key=lambda c: (-c["n_voxels"], (c["root"][2] * Y + c["root"][1]) * X + c["root"][0]))
    return out, region, recs, int((~kept).sum())


def default_min_voxels(size_m, dims, tau):
    """hsk_default_prune_params' min_voxels: the voxels of a cube of edge 4 tau, in binary64 from the binary32 fields"""
    cell = [np.float64(np.float32(size_m[i]) / np.float32(dims[i])) for i in range(3)]
    e = 4.0 * np.float64(np.float32(tau))
    return int(np.ceil(((e * e) * e) / ((cell[0] * cell[1]) * cell[2])))


def diff(ref, cur, thresh=DEFAULT_THRESH, min_weight=1, min_voxels=1):
    """hsk_diff_volume -> (cls, region, records, stats): stats = n_class (7, of the final classes), n_regions, n_minor_regions,
    largest"""
    cls, region, recs, n_minor = regions(classify(ref, cur, thresh, min_weight), min_voxels)
    stats = {"n_class": [int((cls == c).sum()) for c in range(7)], "n_regions": len(recs), "n_minor_regions": n_minor,
             "largest": recs[0]["n_voxels"] if recs else 0}
    return cls, region, recs, stats


def diff_at(cls, region, size_m, xyz, radius):
    """hsk_diff_at -> (cls [n] uint8, region [n] uint32): among the voxels within Chebyshev `radius` of the point's voxel whose
    class is APPEARED or VANISHED the one with the smallest (dx^2 + dy^2 + dz^2, lin); with none, the own voxel's class and NONE;
    a point outside the grid: UNSEEN and NONE"""
    Z, Y, X = cls.shape
    pts = np.asarray(xyz, np.float32).reshape(-1, 3)
    g = [CT.vox_of(pts[:, i], np.float32(size_m[i]) / np.float32(n)) for i, n in enumerate((X, Y, Z))]
    out_c, out_r = np.full(len(pts), UNSEEN, np.uint8), np.full(len(pts), NONE, np.uint32)
    for e in range(len(pts)):
        x, y, z = int(g[0][e]), int(g[1][e]), int(g[2][e])
        if not (0 <= x < X and 0 <= y < Y and 0 <= z < Z):
            continue
        out_c[e] = cls[z, y, x]
        z0, z1, y0, y1, x0, x1 = max(z - radius, 0), min(z + radius + 1, Z), max(y - radius, 0), min(y + radius + 1, Y), max(x - radius, 0), min(x + radius + 1, X)
        sub = cls[z0:z1, y0:y1, x0:x1]
        cz, cy, cx = np.nonzero((sub == APPEARED) | (sub == VANISHED))
        if len(cz) == 0:
            continue
        cz, cy, cx = cz + z0, cy + y0, cx + x0
        key = ((cx - x) ** 2 + (cy - y) ** 2 + (cz - z) ** 2).astype(np.int64) * (1 << 32) + (cz * Y + cy) * X + cx
        i = int(np.argmin(key))
        out_c[e], out_r[e] = cls[cz[i], cy[i], cx[i]], region[cz[i], cy[i], cx[i]]
    return out_c, out_r


def dilate(mask, r):
    """every voxel within Chebyshev distance r of a set voxel, clipped at the grid"""
    out = np.zeros_like(mask)
    Z, Y, X = mask.shape
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                src = mask[max(-dz, 0):Z - max(dz, 0), max(-dy, 0):Y - max(dy, 0), max(-dx, 0):X - max(dx, 0)]
                out[max(dz, 0):Z - max(-dz, 0), max(dy, 0):Y - max(-dy, 0), max(dx, 0):X - max(-dx, 0)] |= src
    return out


def adopt(ref, cur, cls, which=ADOPT_APPEARED | ADOPT_VANISHED, halo=2, ref_color=None, cur_color=None):
    """hsk_adopt_diff for the final classes `cls` -> (ref's new volume, ref's new colour volume or None, stats): the adopt set is
    every voxel with a non-zero weight in cur within Chebyshev `halo` of a target"""
    target = np.zeros(cls.shape, bool)
    if which & ADOPT_APPEARED:
        target |= cls == APPEARED
    if which & ADOPT_VANISHED:
        target |= cls == VANISHED
    S = dilate(target, halo) & (cur[..., 1] != 0)
    out = ref.copy()
    out[S] = cur[S]
    col = None
    if ref_color is not None:
        col = ref_color.copy()
        col[S] = cur_color[S] if cur_color is not None else 0
    n = int(S.sum())
    return out, col, {"n_targets": int(target.sum()), "n_adopted": n, "n_colored": n if ref_color is not None and cur_color is not None else 0}


# ---- the analytic room ---------------------------------------------------------------------------------------------------------------
ROOM_DIMS = (64, 48, 40)
ROOM_TAU = 2.1
ROOM_BOX = ((20.3, 14.2, 6.3), (33.7, 30.6, 19.4))


def box_sdf(p, lo, hi):
    """the signed distance of the points p [..., 3] to the box lo..hi: positive outside"""
    c, h = (np.asarray(lo) + np.asarray(hi)) / 2.0, (np.asarray(hi) - np.asarray(lo)) / 2.0
    q = np.abs(p - c) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)


def room(box=None, wall_x=50.4, floor_z=6.3, dims=ROOM_DIMS, tau=ROOM_TAU, weight=5):
    """a floor (solid below z = floor_z) and a wall (solid beyond x = wall_x) with, box = (lo, hi) in voxels, a box object; a
    voxel's centre lies at its index + 0.5; observed where sdf >= -tau, with `weight`; raw = rint(clip(sdf / tau, -1, 1) 32767)"""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z) + 0.5, np.arange(Y) + 0.5, np.arange(X) + 0.5, indexing="ij")
    sdf = np.minimum(z - floor_z, wall_x - x)
    if box is not None:
        sdf = np.minimum(sdf, box_sdf(np.stack([x, y, z], axis=-1), *box))
    vol = np.zeros((Z, Y, X, 2), np.int16)
    seen = sdf >= -tau
    vol[..., 0] = np.where(seen, np.rint(np.clip(sdf / tau, -1.0, 1.0) * 32767), 0).astype(np.int16)
    vol[..., 1] = np.where(seen, weight, 0)
    return vol


def crossings(vol):
    """the zero crossings in the cloud read-out's sense, as three boolean arrays (one an axis): two face-adjacent observed voxels,
    neither at 32767, one value > 0 and the other < 0"""
    v, ok = vol[..., 0].astype(np.int32), (vol[..., 1] != 0) & (vol[..., 0] != 32767)
    out = []
    for ax in range(3):
        a, b = [slice(None)] * 3, [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        out.append(ok[a] & ok[b] & (((v[a] > 0) & (v[b] < 0)) | ((v[a] < 0) & (v[b] > 0))))
    return out
