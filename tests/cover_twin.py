"""numpy restatement of scan coverage (include/hskinfu.h "Scan coverage"), written from the rule's text: binary32
unless said, one rounding per written operator; every count is an integer.

A volume is the host array of hsk_download_tsdf: [Z, Y, X, 2] int16 (tsdf, weight).  A probe is a dict with the fields of
hsk_probe: width, height, fx, fy, cx, cy, near_m, far_m, step_m."""
import numpy as np

import align_twin as AT

f32 = np.float32
f64 = np.float64
FREE, UNSEEN, SOLID, NOWHERE = 0, 1, 2, 3                      # a voxel's state; eye_state adds 3: outside the grid
HIT, FRONTIER, OPEN, BLIND, OUTSIDE = 0, 1, 2, 3, 4            # a ray's class, in the order of hsk_view_score's counts
CLASSES = ("n_hit", "n_frontier", "n_open", "n_blind", "n_outside")
VIEW_SCORE_DTYPE = np.dtype([(c, "<u4") for c in CLASSES] + [("eye_state", "<u4"), ("gain", "<u8")])     # hsk_view_score
MAX_SAMPLES = 4096


def probe(width, height, fx, fy, cx, cy, near_m, far_m, step_m):
    return dict(width=int(width), height=int(height), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), near_m=f32(near_m), far_m=f32(far_m),
                step_m=f32(step_m))


def states(vol):
    """[Z, Y, X]: UNSEEN where the weight is 0, else FREE where raw > 0, else SOLID"""
    r, w = vol[..., 0], vol[..., 1]
    return np.where(w == 0, UNSEEN, np.where(r > 0, FREE, SOLID)).astype(np.uint8)


def census(vol, box=None):
    """hsk_coverage_census over the voxels lo <= (x, y, z) < hi of box = (lo, hi) (None: all) -> dict: n_unseen, n_free, n_solid,
    n_frontier and faces [6] (-x, +x, -y, +y, -z, +z).  A neighbour outside the grid is not UNSEEN; one outside the box counts."""
    S = states(vol)
    Z, Y, X = S.shape
    lo, hi = ((0, 0, 0), (X, Y, Z)) if box is None else box
    U = S == UNSEEN
    pad = np.zeros((Z + 2, Y + 2, X + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = U
    # the neighbour's UNSEEN bit at every voxel, by direction (arrays are [z, y, x])
    nb = [pad[1:-1, 1:-1, :-2], pad[1:-1, 1:-1, 2:], pad[1:-1, :-2, 1:-1], pad[1:-1, 2:, 1:-1], pad[:-2, 1:-1, 1:-1], pad[2:, 1:-1, 1:-1]]
    sl = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
    F = (S == FREE)[sl]
    faces = np.array([int((F & n[sl]).sum()) for n in nb], np.uint64)
    return {"n_unseen": int((S[sl] == UNSEEN).sum()), "n_free": int(F.sum()), "n_solid": int((S[sl] == SOLID).sum()),
            "n_frontier": int((F & np.logical_or.reduce([n[sl] for n in nb])).sum()), "faces": faces}


def n_samples(pr):
    """min(4096, floor((far - near) / step) + 1) in binary64 from the binary32 fields"""
    return int(min(f64(MAX_SAMPLES), np.floor((f64(pr["far_m"]) - f64(pr["near_m"])) / f64(pr["step_m"])) + 1.0))


def _voxels(vol, size, p):
    """the voxel of the points p = (px, py, pz), unclamped -> (inside, state where inside else UNSEEN, (gx, gy, gz))"""
    Z, Y, X, _ = vol.shape
    dims = (X, Y, Z)
    cell = AT.cells(dims, size)
    g = [AT._vox_of(p[i], cell[i]) for i in range(3)]
    inside = np.ones(np.shape(p[0]), bool)
    for i in range(3):
        inside &= (g[i] >= 0) & (g[i] < dims[i])
    c = [np.clip(g[i], 0, dims[i] - 1) for i in range(3)]
    v = vol[c[2], c[1], c[0]]
    s = np.where(v[..., 1] == 0, UNSEEN, np.where(v[..., 0] > 0, FREE, SOLID))
    return inside, s, g


def ray_walk(vol, size, pr, poses):
    """every ray of the probe from each of the poses [m, 4, 4] (one pose [4, 4]: m = 1 and the leading axis dropped) -> dict of
    [m, h, w] arrays: cls, depth_mm, gain, voxel [m, h, w, 3]: the voxel (x, y, z) of each ray's deciding sample (-1 where it
    has none), and walked: the samples the ray took before it ended, the one that ended it included (what a kernel has to read
    of it at the least; no part of the rule)"""
    M = np.asarray(poses, f32)
    single = M.ndim == 2
    M = M.reshape(-1, 4, 4)
    R, t = M[:, :3, :3, None, None], M[:, :3, 3, None, None]
    w, h, m = pr["width"], pr["height"], len(M)
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(all="ignore"):
        dx = ((u.astype(f32) - pr["cx"]).astype(f32) / pr["fx"]).astype(f32)[None]
        dy = ((v.astype(f32) - pr["cy"]).astype(f32) / pr["fy"]).astype(f32)[None]
    alive = np.ones((m, h, w), bool)          # the ray has not ended
    entered = np.zeros((m, h, w), bool)       # a sample was inside
    frontier = np.zeros((m, h, w), bool)      # decided by an UNSEEN sample (and, while alive, still counting)
    cls = np.full((m, h, w), OUTSIDE, np.uint8)
    gain = np.zeros((m, h, w), np.int64)
    depth = np.zeros((m, h, w), np.int64)
    dvox = np.full((m, h, w, 3), -1, np.int64)
    walked = np.zeros((m, h, w), np.int64)
    for i in range(n_samples(pr)):
        if not alive.any():
            break
        with np.errstate(all="ignore"):
            z = f32(pr["near_m"] + f32(f32(i) * pr["step_m"]))
            x, y = (dx * z).astype(f32), (dy * z).astype(f32)
            p = [(((R[:, k, 0] * x + R[:, k, 1] * y).astype(f32) + R[:, k, 2] * z).astype(f32) + t[:, k]).astype(f32) for k in range(3)]
            inside, s, g = _voxels(vol, size, p)
            mm = np.rint(f32(z * f32(1000)))
        mm = int(mm) if 1 <= mm <= 65535 else 0
        walked += alive
        # an outside sample behind an inside one ends the ray (OPEN, or a FRONTIER ray's count)
        alive &= ~(~inside & entered)
        ins = alive & inside
        # the first inside sample: not FREE -> BLIND
        blind = ins & ~entered & (s != FREE)
        cls[blind] = BLIND
        alive &= ~blind
        entered |= ins
        ins &= ~blind
        # a FRONTIER ray goes on: it counts its UNSEEN samples up to the first SOLID one
        on = ins & frontier
        gain[on & (s == UNSEEN)] += 1
        alive &= ~(on & (s == SOLID))
        # an undecided ray: FREE so far
        und = ins & ~frontier
        cls[und & (s == FREE)] = OPEN
        hit = und & (s == SOLID)
        cls[hit] = HIT
        alive &= ~hit
        new = und & (s == UNSEEN)
        cls[new] = FRONTIER
        frontier |= new
        gain[new] += 1
        for sel in (hit, new):
            depth[sel] = mm
            for k in range(3):
                dvox[..., k][sel] = g[k][sel]
    out = {"cls": cls, "depth_mm": depth.astype(np.uint16), "gain": gain, "voxel": dvox, "walked": walked}
    return {k: a[0] for k, a in out.items()} if single else out


def ray_classes(vol, size, pr, pose):
    """one pose -> per pixel (class [h, w] uint8, depth_mm [h, w] uint16, gain [h, w] int64)"""
    r = ray_walk(vol, size, pr, np.asarray(pose, f32).reshape(4, 4))
    return r["cls"], r["depth_mm"], r["gain"]


def eye_states(vol, size, poses):
    t = np.asarray(poses, f32).reshape(-1, 4, 4)[:, :3, 3]
    with np.errstate(all="ignore"):
        inside, s, _ = _voxels(vol, size, [np.ascontiguousarray(t[:, k]) for k in range(3)])
    return np.where(inside, s, NOWHERE)


def eye_state(vol, size, pose):
    return int(eye_states(vol, size, pose)[0])


def score(vol, size, pr, poses, batch=64):
    """hsk_score_views -> a VIEW_SCORE_DTYPE array, one record per pose"""
    poses = np.asarray(poses, f32).reshape(-1, 4, 4)
    out = np.zeros(len(poses), VIEW_SCORE_DTYPE)
    for j in range(0, len(poses), batch):
        r = ray_walk(vol, size, pr, poses[j:j + batch])
        for c, name in enumerate(CLASSES):
            out[name][j:j + batch] = (r["cls"] == c).sum(axis=(1, 2))
        out["gain"][j:j + batch] = r["gain"].sum(axis=(1, 2))
    out["eye_state"] = eye_states(vol, size, poses)
    return out


def rank(scores):
    """hsk_rank_views: larger gain first; ties to the larger n_frontier, then the lower index; eye_state != 0 behind all others"""
    s = np.asarray(scores)
    return np.array(sorted(range(len(s)), key=lambda i: (int(s["eye_state"][i]) != 0, -int(s["gain"][i]), -int(s["n_frontier"][i]), i)), np.uint32)
