"""The reach field's rule in numpy: which voxels are passable, which of the 26 moves the box rule allows, the seven
costs, the field as the least fixpoint of G(v) = min(G(v), G(u) + c) -- by a frontier relaxation that only ever lowers values and
stops when none can be lowered, and, for small grids, by whole-grid Jacobi sweeps --, the seeds, the path rule, the floor form, the
point lookup and the ranking.  All integers (int64 inside, uint32 out).  A clearance field is [z, y, x] uint32 (clearance_twin)."""
import numpy as np

import clearance_twin as CL

f32 = np.float32
UNREACHED, OUTSIDE, BLOCKED = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
MAX_COST = 0xF0000000
MAX_SEEDS = 4096
INF = 1 << 40
MOVES = [(m % 3 - 1, (m // 3) % 3 - 1, m // 9 - 1) for m in range(27)]          # (dx, dy, dz) of move index m; m = 13 is no move


def costs(weight):
    """c(d) = rint(16 sqrt(w_x dx^2 + w_y dy^2 + w_z dz^2)) in binary64, over the move index"""
    w = [np.float64(v) for v in weight]
    return [int(np.rint(16.0 * np.sqrt(w[0] * dx * dx + w[1] * dy * dy + w[2] * dz * dz))) for dx, dy, dz in MOVES]


def passable(d2, min_d2):
    return np.asarray(d2, np.uint32) >= np.uint32(min_d2)


def _shifted(a, dx, dy, dz, fill):
    """b[z, y, x] = a[z + dz, y + dy, x + dx], `fill` where that lies outside"""
    Z, Y, X = a.shape
    out = np.full(a.shape, fill, a.dtype)
    zs, zd = (slice(dz, Z), slice(0, Z - dz)) if dz >= 0 else (slice(0, Z + dz), slice(-dz, Z))
    ys, yd = (slice(dy, Y), slice(0, Y - dy)) if dy >= 0 else (slice(0, Y + dy), slice(-dy, Y))
    xs, xd = (slice(dx, X), slice(0, X - dx)) if dx >= 0 else (slice(0, X + dx), slice(-dx, X))
    out[zd, yd, xd] = a[zs, ys, xs]
    return out


def allowed(pas):
    """[27, z, y, x] bool: the move m from a voxel is allowed when every voxel of the box spanned by it and its neighbour lies in
    the grid and is passable"""
    out = np.zeros((27,) + pas.shape, bool)
    for m, (dx, dy, dz) in enumerate(MOVES):
        if m == 13:
            continue
        ok = np.ones(pas.shape, bool)
        for ez in ({0, dz}):
            for ey in ({0, dy}):
                for ex in ({0, dx}):
                    ok &= _shifted(pas, ex, ey, ez, False)
        out[m] = ok
    return out


def seed_voxels(size_m, dims, pts):
    """the voxels (x, y, z) of the seed points that lie inside the grid, in order (a NaN lies outside)"""
    X, Y, Z = dims
    p = np.asarray(pts, f32).reshape(-1, 3)
    g = [CL.vox_of(p[:, i], f32(size_m[i]) / f32(n)) for i, n in enumerate(dims)]
    inside = (g[0] >= 0) & (g[0] < X) & (g[1] >= 0) & (g[1] < Y) & (g[2] >= 0) & (g[2] < Z)
    return [(int(g[0][i]), int(g[1][i]), int(g[2][i])) for i in np.flatnonzero(inside)]


def field(d2, weight, min_d2, max_cost, seeds):
    """-> (G [z, y, x] uint32, n_seeds_used): seeds = voxels (x, y, z) inside the grid; one on a voxel that is not passable is ignored"""
    pas = passable(d2, min_d2)
    Z, Y, X = pas.shape
    ok = allowed(pas).reshape(27, -1)
    c = costs(weight)
    off = [dx + X * (dy + Y * dz) for dx, dy, dz in MOVES]
    g = np.full(Z * Y * X, INF, np.int64)
    used = [s for s in seeds if pas[s[2], s[1], s[0]]]
    front = np.unique(np.array([x + X * (y + Y * z) for x, y, z in used], np.int64))
    g[front] = 0
    while front.size:                                  # (only ever lowers values; stops when none can be lowered)
        fell = []
        for m in range(27):
            if m == 13:
                continue
            src = front[ok[m][front]]
            dst, cand = src + off[m], g[src] + c[m]
            keep = (cand <= max_cost) & (cand < g[dst])
            dst, cand = dst[keep], cand[keep]
            if dst.size:
                np.minimum.at(g, dst, cand)
                fell.append(dst)
        front = np.unique(np.concatenate(fell)) if fell else np.zeros(0, np.int64)
    out = np.where(g < INF, g, UNREACHED)
    out[~pas.reshape(-1)] = BLOCKED
    return out.astype(np.uint32).reshape(Z, Y, X), len(used)


def field_jacobi(d2, weight, min_d2, max_cost, seeds):
    """the same field by whole-grid sweeps (small grids): G <- min(G, shifted G + c) over the allowed moves until nothing falls"""
    pas = passable(d2, min_d2)
    ok = allowed(pas)
    c = costs(weight)
    g = np.full(pas.shape, INF, np.int64)
    for x, y, z in seeds:
        if pas[z, y, x]:
            g[z, y, x] = 0
    while True:
        new = g.copy()
        for m, (dx, dy, dz) in enumerate(MOVES):
            if m == 13:
                continue
            cand = _shifted(g, dx, dy, dz, INF) + c[m]
            new = np.where(ok[m] & (cand <= max_cost) & (cand < new), cand, new)
        if np.array_equal(new, g):
            break
        g = new
    out = np.where(g < INF, g, UNREACHED)
    out[~pas] = BLOCKED
    return out.astype(np.uint32)


def stats(g):
    val = g[g <= MAX_COST]
    return {"n_passable": int((g != BLOCKED).sum()), "n_reached": int(val.size), "max_cost_seen": int(val.max()) if val.size else 0}


def lookup(g, size_m, xyz):
    """hsk_reach_at: the field at the voxels of the points, OUTSIDE where the unclamped voxel is not in the grid"""
    return CL.lookup(g, size_m, xyz)


def path(g, weight, goal):
    """the path rule from the voxel goal = (x, y, z) -> [n, 3] int32 from the seed to the goal; n = 0 when the goal holds no value"""
    Z, Y, X = g.shape
    c = costs(weight)
    x, y, z = goal
    if not (0 <= x < X and 0 <= y < Y and 0 <= z < Z) or g[z, y, x] > MAX_COST:
        return np.zeros((0, 3), np.int32)

    def open_at(a, b, cc):
        return 0 <= a < X and 0 <= b < Y and 0 <= cc < Z and g[cc, b, a] != BLOCKED

    out = [(x, y, z)]
    while g[z, y, x] != 0:
        for m, (dx, dy, dz) in enumerate(MOVES):
            if m == 13:
                continue
            if all(open_at(x + ex, y + ey, z + ez) for ez in {0, dz} for ey in {0, dy} for ex in {0, dx}):
                n = int(g[z + dz, y + dy, x + dx])
                if n <= MAX_COST and n + c[m] == int(g[z, y, x]):
                    x, y, z = x + dx, y + dy, z + dz
                    break
        else:
            raise AssertionError(f"no move of the path rule at {(x, y, z)}: the field is no fixpoint")
        out.append((x, y, z))
    return np.array(out[::-1], np.int32)


def floor(vol, weight, max_d2, flags, axis, lo, hi, min_d2, max_cost, size_m, pts):
    """hsk_reach_floor -> (map [v, u] uint32, n_seeds_used): the rule on clearance_twin.floor_map, one plane deep, with the weights
    of the two remaining axes; the seeds projected by dropping the up axis (that coordinate does not count)"""
    Z, Y, X = vol.shape[:3]
    dims = (X, Y, Z)
    d2 = CL.floor_map(vol, weight, max_d2, flags, axis, lo, hi)
    au, av = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    p = np.array(np.asarray(pts, f32).reshape(-1, 3))
    p[:, axis] = 0.0
    seeds = [(s[au], s[av], 0) for s in seed_voxels(size_m, dims, p)]
    g, used = field(d2[None], (weight[au], weight[av], weight[axis]), min_d2, max_cost, seeds)
    return g[0], used


def default_params(cpar):
    """hsk_default_reach_params for clearance parameters as clearance_twin.default_params gives them"""
    return {"min_d2": max(1, min(CL.d2_of_metres(cpar["unit_m"], 0.3), cpar["max_d2"])), "max_cost": MAX_COST}


def metres(unit_m, g):
    return np.float32(np.nan) if g > MAX_COST else np.float32(np.float64(g) * np.float64(f32(unit_m)) / 16.0)


def rank_views_reach(scores, eye_g, max_g):
    """hsk_rank_views_reach: hsk_rank_views' order (free eyes first, larger gain, larger n_frontier, lower index); behind all others,
    in the same order, the poses whose eye_g is a marker or above max_g"""
    d = np.asarray(eye_g, np.uint64)
    behind = (d > MAX_COST) | (d > max_g)
    return np.array(sorted(range(len(scores)), key=lambda i: (bool(behind[i]), scores["eye_state"][i] != 0, -int(scores["gain"][i]),
                                                              -int(scores["n_frontier"][i]), i)), np.uint32)
