"""The room partition's rule in numpy: the cores -- the 6-connected components of the voxels whose clearance is at
least core_d2, labelled by their smallest lin --, the dropping of small ones, the spreading of the kept cores' labels as the least
fixpoint of K(v) = min(K(v), K(u) + (c << 32)) on the 64-bit keys K = G << 32 | L -- by a frontier relaxation that only ever lowers
keys, and, for small grids, by whole-grid Jacobi sweeps --, the room and door records, the merge, the point lookup and the floor
form.  The moves, the box rule and the costs are reach_twin's.  All integers.  A clearance field is [z, y, x] uint32."""
import numpy as np

import clearance_twin as CL
import reach_twin as RE

f32 = np.float32
UNASSIGNED, OUTSIDE, BLOCKED, NONE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
MAX_ROOMS = 1024
MAX_RADIUS = 4
KEY_UNASSIGNED = np.uint64(0xFFFFFFFFFFFFFFFF)
KEY_BLOCKED = np.uint64(0xFFFFFFFDFFFFFFFF)
NO_LABEL = 0xFFFFFFFF
ROOM_DTYPE = np.dtype([("n_voxels", "<u8"), ("n_core_voxels", "<u8"), ("sum", "<u8", 3), ("root", "<u4", 3), ("lo", "<u4", 3), ("hi", "<u4", 3),
                       ("max_d2", "<u4"), ("max_g", "<u4"), ("pad", "<u4")])
DOOR_DTYPE = np.dtype([("sum2", "<u8", 3), ("a", "<u4"), ("b", "<u4"), ("n_faces", "<u4", 3), ("lo", "<u4", 3), ("hi", "<u4", 3), ("max_d2", "<u4")])
_BIG = np.int64(1) << 40


class TooManyRooms(Exception):
    """more than MAX_ROOMS cores are kept: hsk_build_partition's HSK_ERR_ARG; args = (n_cores, n_kept)"""


def core_labels(d2, core_d2):
    """[z, y, x] uint32: for a core voxel (d2 >= core_d2; FAR passes) the smallest lin of its 6-connected component, NO_LABEL
    elsewhere.  Sweeps of neighbour minima, each followed by pointer jumping (a label is the lin of a voxel of the same component,
    whose own label is no larger), until nothing falls"""
    core = np.asarray(d2, np.uint32) >= np.uint32(core_d2)
    Z, Y, X = core.shape
    lab = np.where(core, np.arange(Z * Y * X, dtype=np.int64).reshape(Z, Y, X), _BIG)
    members = np.flatnonzero(core.reshape(-1))
    while True:
        new = lab.copy()
        for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            new = np.minimum(new, RE._shifted(lab, dx, dy, dz, _BIG))
        new = np.where(core, new, _BIG)
        flat = new.reshape(-1)
        while True:
            nxt = flat[flat[members]]
            if np.array_equal(nxt, flat[members]):
                break
            flat[members] = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(core, lab, NO_LABEL).astype(np.uint32)


def kept_roots(labels, min_core_voxels):
    """-> (the roots of the cores with at least min_core_voxels voxels, ascending, the number of cores before dropping)"""
    lab = labels[labels != NO_LABEL]
    roots, counts = np.unique(lab, return_counts=True)
    return roots[counts >= min_core_voxels].astype(np.uint32), int(roots.size)


def _finish(key, pas):
    out = np.where(key < (np.uint64(RE.MAX_COST + 1) << np.uint64(32)), key, KEY_UNASSIGNED)
    out[~pas.reshape(out.shape)] = KEY_BLOCKED
    return out


def field(d2, weight, core_d2, min_d2, min_core_voxels, max_cost):
    """-> (K [z, y, x] uint64, the kept roots ascending, n_cores): raises TooManyRooms when more than MAX_ROOMS cores are kept"""
    assert 1 <= min_d2 <= core_d2
    labels = core_labels(d2, core_d2)
    roots, n_cores = kept_roots(labels, min_core_voxels)
    if roots.size > MAX_ROOMS:
        raise TooManyRooms(n_cores, int(roots.size))
    pas = RE.passable(d2, min_d2)
    Z, Y, X = pas.shape
    ok = RE.allowed(pas).reshape(27, -1)
    c = [np.uint64(v) << np.uint64(32) for v in RE.costs(weight)]
    off = [dx + X * (dy + Y * dz) for dx, dy, dz in RE.MOVES]
    limit = (np.uint64(max_cost) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
    key = np.full(Z * Y * X, KEY_UNASSIGNED, np.uint64)
    flat = labels.reshape(-1)
    front = np.flatnonzero(np.isin(flat, roots) & (flat != NO_LABEL)).astype(np.int64)
    key[front] = flat[front].astype(np.uint64)                # (0, label)
    while front.size:                                        # (only ever lowers keys; stops when none can be lowered)
        fell = []
        for m in range(27):
            if m == 13:
                continue
            src = front[ok[m][front]]
            dst, cand = src + off[m], key[src] + c[m]         # (G <= MAX_COST, a cost <= 887: no carry out of 64 bits)
            keep = (cand <= limit) & (cand < key[dst])
            dst, cand = dst[keep], cand[keep]
            if dst.size:
                np.minimum.at(key, dst, cand)
                fell.append(dst)
        front = np.unique(np.concatenate(fell)) if fell else np.zeros(0, np.int64)
    return _finish(key, pas).reshape(Z, Y, X), roots, n_cores


def field_jacobi(d2, weight, core_d2, min_d2, min_core_voxels, max_cost):
    """the same keys by whole-grid sweeps (small grids): K <- min(K, shifted K + (c << 32)) over the allowed moves until nothing falls"""
    labels = core_labels(d2, core_d2)
    roots, _ = kept_roots(labels, min_core_voxels)
    pas = RE.passable(d2, min_d2)
    ok = RE.allowed(pas)
    cost = RE.costs(weight)
    limit = (np.uint64(max_cost) << np.uint64(32)) | np.uint64(0xFFFFFFFF)
    seeded = np.isin(labels, roots) & (labels != NO_LABEL)
    key = np.where(seeded, labels.astype(np.uint64), KEY_UNASSIGNED)
    value_top = np.uint64(RE.MAX_COST + 1) << np.uint64(32)
    while True:
        new = key.copy()
        for m, (dx, dy, dz) in enumerate(RE.MOVES):
            if m == 13:
                continue
            nb = RE._shifted(key, dx, dy, dz, KEY_UNASSIGNED)
            cand = np.where(nb < value_top, nb, np.uint64(0)) + (np.uint64(cost[m]) << np.uint64(32))
            new = np.where(ok[m] & (nb < value_top) & (cand <= limit) & (cand < new), cand, new)
        if np.array_equal(new, key):
            break
        key = new
    return _finish(key, pas)


def cost_of(key):
    """G alone: the reach field seeded at every kept core voxel, with reach_twin's UNREACHED and BLOCKED"""
    return (key >> np.uint64(32)).astype(np.uint32)


def rooms(key, d2, roots):
    """-> (the records, ROOM_DTYPE, ordered by n_voxels descending with ties to the smaller root; rank [len(roots)]: the id of
    roots[i])"""
    Z, Y, X = key.shape
    n = len(roots)
    held = key < (np.uint64(RE.MAX_COST + 1) << np.uint64(32))
    at = np.searchsorted(roots, (key[held] & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    g = cost_of(key)[held].astype(np.int64)
    zz, yy, xx = (c[held].astype(np.int64) for c in np.indices(key.shape))
    recs = np.zeros(n, ROOM_DTYPE)
    recs["n_voxels"] = np.bincount(at, minlength=n)
    recs["n_core_voxels"] = np.bincount(at[g == 0], minlength=n)
    recs["root"] = np.stack([roots % X, (roots // X) % Y, roots // (X * Y)], axis=1)
    for i, c in enumerate((xx, yy, zz)):
        total, lo, hi = np.zeros(n, np.int64), np.full(n, _BIG, np.int64), np.zeros(n, np.int64)
        np.add.at(total, at, c)
        np.minimum.at(lo, at, c)
        np.maximum.at(hi, at, c + 1)
        recs["sum"][:, i], recs["lo"][:, i], recs["hi"][:, i] = total, lo, hi
    for name, val in (("max_d2", d2[held].astype(np.int64)), ("max_g", g)):
        top = np.zeros(n, np.int64)
        np.maximum.at(top, at, val)
        recs[name] = top
    order = sorted(range(n), key=lambda i: (-int(recs["n_voxels"][i]), int(roots[i])))
    rank = np.zeros(n, np.uint32)
    rank[order] = np.arange(n, dtype=np.uint32)
    return recs[order], rank


def ids(key, roots, rank):
    """[z, y, x] uint32: the room id a voxel reports -- its room's rank, UNASSIGNED or BLOCKED"""
    held = key < (np.uint64(RE.MAX_COST + 1) << np.uint64(32))
    lab = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out = np.where(key == KEY_BLOCKED, np.uint32(BLOCKED), np.uint32(UNASSIGNED)).astype(np.uint32)
    if len(roots):
        at = np.searchsorted(roots, lab[held])
        out[held] = rank[at]
    return out


def doors(idmap, d2):
    """-> the door records, DOOR_DTYPE, ordered by (a, b): one per pair of rooms that share a face"""
    held = idmap < NONE
    n_rooms = int(idmap[held].max()) + 1 if held.any() else 0
    zz, yy, xx = np.indices(idmap.shape)
    parts = []
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[2 - axis], hi[2 - axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        u, v = idmap[lo].astype(np.int64), idmap[hi].astype(np.int64)
        face = (u < n_rooms) & (v < n_rooms) & (u != v)
        pair = (np.minimum(u, v) * max(n_rooms, 1) + np.maximum(u, v))[face]
        parts.append((pair, np.full(pair.size, axis), xx[lo][face], yy[lo][face], zz[lo][face], np.minimum(d2[lo], d2[hi])[face].astype(np.int64)))
    pair, axis, x, y, z, w = (np.concatenate([p[i] for p in parts]).astype(np.int64) for i in range(6))
    pairs, at = np.unique(pair, return_inverse=True)
    n = len(pairs)
    out = np.zeros(n, DOOR_DTYPE)
    out["a"], out["b"] = pairs // max(n_rooms, 1), pairs % max(n_rooms, 1)
    for i, c in enumerate((x, y, z)):
        total, lo, hi = np.zeros(n, np.int64), np.full(n, _BIG, np.int64), np.zeros(n, np.int64)
        np.add.at(total, at, 2 * c + (axis == i))
        np.minimum.at(lo, at, c)
        np.maximum.at(hi, at, c + 1)
        out["sum2"][:, i], out["lo"][:, i], out["hi"][:, i] = total, lo, hi
        out["n_faces"][:, i] = np.bincount(at[axis == i], minlength=n)
    top = np.zeros(n, np.int64)
    np.maximum.at(top, at, w)
    out["max_d2"] = top
    return out


def partition(d2, weight, core_d2, min_d2, min_core_voxels, max_cost):
    """everything hsk_build_partition reports -> dict: key, ids, cost, rooms, doors, stats"""
    key, roots, n_cores = field(d2, weight, core_d2, min_d2, min_core_voxels, max_cost)
    recs, rank = rooms(key, d2, roots)
    idmap = ids(key, roots, rank)
    drs = doors(idmap, d2)
    st = {"n_cores": n_cores, "n_rooms": len(roots), "n_dropped": n_cores - len(roots), "n_passable": int((key != KEY_BLOCKED).sum()),
          "n_assigned": int((idmap < NONE).sum()), "n_doors": len(drs)}
    return {"key": key, "ids": idmap, "cost": cost_of(key), "rooms": recs, "doors": drs, "stats": st}


def merge(drs, n_rooms, merge_d2):
    """hsk_merge_rooms: per room the smallest id of its class under the union of all pairs whose door has max_d2 >= merge_d2"""
    cls = list(range(n_rooms))
    for d in drs:
        if d["max_d2"] >= merge_d2:
            a, b = cls[int(d["a"])], cls[int(d["b"])]
            if a != b:
                cls = [min(a, b) if c in (a, b) else c for c in cls]
    return np.array(cls, np.uint32)


def lookup(idmap, weight, size_m, xyz, radius):
    """hsk_partition_at: the voxel of a point as clearance_twin.lookup finds it; among the voxels within radius of it on every axis
    that hold a room, the one minimising (weighted squared distance, lin); OUTSIDE / NONE"""
    Z, Y, X = idmap.shape
    pts = np.asarray(xyz, f32).reshape(-1, 3)
    g = [CL.vox_of(pts[:, i], f32(size_m[i]) / f32(n)) for i, n in enumerate((X, Y, Z))]
    out = np.full(len(pts), OUTSIDE, np.uint32)
    for i in range(len(pts)):
        x, y, z = int(g[0][i]), int(g[1][i]), int(g[2][i])
        if not (0 <= x < X and 0 <= y < Y and 0 <= z < Z):
            continue
        best, out[i] = None, NONE
        for dz in range(-radius, radius + 1):
            for dy in range(-radius, radius + 1):
                for dx in range(-radius, radius + 1):
                    a, b, c = x + dx, y + dy, z + dz
                    if 0 <= a < X and 0 <= b < Y and 0 <= c < Z and idmap[c, b, a] < NONE:
                        rank = (weight[0] * dx * dx + weight[1] * dy * dy + weight[2] * dz * dz, (c * Y + b) * X + a)
                        if best is None or rank < best:
                            best, out[i] = rank, idmap[c, b, a]
    return out


def floor(vol, weight, max_d2, flags, axis, lo, hi, core_d2, min_d2, min_core_voxels, max_cost):
    """hsk_partition_floor: the rule on clearance_twin.floor_map, one plane deep, with the weights of the two remaining axes -> the
    dict of `partition`, its arrays with a leading axis of one plane"""
    fmap = CL.floor_map(vol, weight, max_d2, flags, axis, lo, hi)
    au, av = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    return partition(fmap[None], (weight[au], weight[av], weight[axis]), core_d2, min_d2, min_core_voxels, max_cost)


def default_params(cpar, size_m, dims):
    """hsk_default_partition_params for clearance parameters as clearance_twin.default_params gives them"""
    cell = [np.float64(f32(size_m[i]) / f32(dims[i])) for i in range(3)]
    e = np.float64(0.25)
    return {"core_d2": max(1, min(CL.d2_of_metres(cpar["unit_m"], 0.5), cpar["max_d2"])), "min_d2": 1,
            "min_core_voxels": int(np.ceil(((e * e) * e) / ((cell[0] * cell[1]) * cell[2]))), "max_cost": RE.MAX_COST}
