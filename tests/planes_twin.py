"""numpy restatement of oriented plane detection (include/hskinfu.h "Oriented plane detection"), written from the
rule's text: binary32 unless said, one rounding per written operator, every accumulated sum an integer (Python ints where 64
bits would not do).  Also what the tests of the rule need: the analytic scene's cloud with normals, and the thin wall."""
import math

import numpy as np

import align_twin as AT
import mesh_twin as MT
import np_twin as T

f32 = np.float32
f64 = np.float64
DEFAULTS = dict(dist_m=0.02, cos_min=0.8660254037844387, min_fraction=0.03, max_planes=12, n_hypotheses=512, refits=2, seed=0x9E3779B97F4A7C15)
RECORD_DTYPE = np.dtype([("abcd", "<f4", (4,)), ("n_inliers", "<u4"), ("pad", "<u4"), ("sum_abs", "<u8")])     # hsk_plane_record


class Lcg:
    """the host detector's generator: a 64-bit LCG, the upper 31 bits of the state"""

    def __init__(self, seed):
        self.s = int(seed) & (2 ** 64 - 1)

    def next(self):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return self.s >> 33


def _cols(a):
    a = np.asarray(a, f32).reshape(-1, 3)
    return [np.ascontiguousarray(a[:, i]) for i in range(3)]


def valid(ps, ns):
    """all six numbers finite and |x|, |y|, |z| <= 64"""
    ps, ns = np.asarray(ps, f32).reshape(-1, 3), np.asarray(ns, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.isfinite(ps).all(axis=1) & np.isfinite(ns).all(axis=1) & (np.abs(ps) <= f32(64)).all(axis=1)


def dot3(a, b, c, x, y, z):
    return ((a * x).astype(f32) + (b * y).astype(f32)).astype(f32) + (c * z).astype(f32)


def inliers(planes, ps, ns, open_, dist_m, cos_min):
    """the inlier test of the planes [m, 4] on the points -> (inlier [m, n] bool, |s| [m, n] binary32); open_: valid and unlabelled"""
    P = np.asarray(planes, f32).reshape(-1, 4)
    a, b, c, d = (P[:, i, None] for i in range(4))
    x, y, z = (v[None, :] for v in _cols(ps))
    nx, ny, nz = (v[None, :] for v in _cols(ns))
    with np.errstate(all="ignore"):
        s = (dot3(a, b, c, x, y, z) + d).astype(f32)
        g = dot3(a, b, c, nx, ny, nz).astype(f32)
        a_s = np.abs(s)
        return np.asarray(open_, bool)[None, :] & (a_s <= f32(dist_m)) & (g >= f32(cos_min)), a_s


def score(ps, ns, planes, dist_m, cos_min, labels=None, batch=64):
    """hsk_score_planes -> counts [m] uint32"""
    P = np.asarray(planes, f32).reshape(-1, 4)
    ps, ns = np.asarray(ps, f32).reshape(-1, 3), np.asarray(ns, f32).reshape(-1, 3)
    open_ = valid(ps, ns) if labels is None else valid(ps, ns) & (np.asarray(labels) < 0)
    keep = np.flatnonzero(open_)          # (a point that is not open is no plane's inlier)
    out = np.zeros(len(P), np.uint32)
    for j in range(0, len(P), batch):
        out[j:j + batch] = inliers(P[j:j + batch], ps[keep], ns[keep], np.ones(len(keep), bool), dist_m, cos_min)[0].sum(axis=1)
    return out


def abs_q(a_s):
    """what an inlier adds to sum_abs: rint(|s| 65536)"""
    return np.rint(np.asarray(a_s, f32) * f32(65536)).astype(np.int64)


def moments(ps):
    """the ten sums of step 3 over the points ps (the inliers): m, the sums of q, of q_a q_b (xx xy xz yy yz zz), as Python ints"""
    q = np.rint(np.asarray(ps, f32).reshape(-1, 3) * f32(4096)).astype(np.int64)
    s = [len(q)] + [int(q[:, i].sum()) for i in range(3)]
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        s.append(int((q[:, a] * q[:, b]).sum()))
    return s


def smallest_eigvec(A):
    """the host detector's cyclic Jacobi, operation for operation, in binary64 (Python floats)"""
    A = [[float(v) for v in row] for row in A]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(32):
        off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2]
        if off < 1e-30:
            break
        for p in range(3):
            for q in range(p + 1, 3):
                if abs(A[p][q]) < 1e-300:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    m = 0
    if A[1][1] < A[m][m]:
        m = 1
    if A[2][2] < A[m][m]:
        m = 2
    return [V[k][m] for k in range(3)]


def refit(sums10, prev_abcd):
    """hsk_plane_refit -> (abcd [4] binary32, ok)"""
    s = [int(v) for v in sums10]
    prev = np.asarray(prev_abcd, f32).reshape(4)
    m, S, SS = s[0], s[1:4], s[4:10]
    if m < 3:
        return prev.copy(), False
    at = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
    mm = float(m) * float(m)
    Cm = [[float(m * SS[at[a][b]] - S[a] * S[b]) / mm for b in range(3)] for a in range(3)]      # (float(int): rounded once)
    n = smallest_eigvec(Cm)
    length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    if length < 1e-12:
        return prev.copy(), False
    n = [v / length for v in n]
    if (n[0] * float(prev[0]) + n[1] * float(prev[1])) + n[2] * float(prev[2]) < 0.0:
        n = [-v for v in n]
    mean = [(float(S[a]) / float(m)) / 4096.0 for a in range(3)]
    d = -((n[0] * mean[0] + n[1] * mean[1]) + n[2] * mean[2])
    return np.array([n[0], n[1], n[2], d], f64).astype(f32), True


def min_inliers(min_fraction, n):
    return max(3, math.floor(float(f32(min_fraction)) * float(n)))


def detect(ps, ns, dist_m=0.02, cos_min=0.8660254037844387, min_fraction=0.03, max_planes=12, n_hypotheses=512, refits=2,
           seed=0x9E3779B97F4A7C15, batch=64):
    """hsk_detect_planes_oriented -> (records [k] RECORD_DTYPE, labels [n] int32, the number of invalid points)"""
    ps, ns = np.asarray(ps, f32).reshape(-1, 3), np.asarray(ns, f32).reshape(-1, 3)
    n = len(ps)
    ok = valid(ps, ns)
    labels = np.full(n, -1, np.int32)
    recs = []
    if n == 0:
        return np.zeros(0, RECORD_DTYPE), labels, 0
    rng = Lcg(seed)
    least = min_inliers(min_fraction, n)
    while len(recs) < max_planes:
        open_ = ok & (labels < 0)
        keep = np.flatnonzero(open_)
        seeds = np.array([rng.next() % n for _ in range(n_hypotheses)], np.int64)
        void = ~open_[seeds]
        with np.errstate(all="ignore"):
            hyp = np.concatenate([ns[seeds], -dot3(*(ns[seeds, i] for i in range(3)), *(ps[seeds, i] for i in range(3)))[:, None]], axis=1).astype(f32)
        counts = np.zeros(n_hypotheses, np.int64)
        for j in range(0, n_hypotheses, batch):
            counts[j:j + batch] = inliers(hyp[j:j + batch], ps[keep], ns[keep], np.ones(len(keep), bool), dist_m, cos_min)[0].sum(axis=1)
        counts[void] = 0
        best = int(np.argmax(counts))            # (the first of equal counts)
        if counts[best] < least:
            break
        plane = hyp[best].copy()
        for _ in range(refits):
            inl = inliers(plane[None], ps, ns, open_, dist_m, cos_min)[0][0]
            if inl.sum() < 3:
                break
            plane2, good = refit(moments(ps[inl]), plane)
            if not good:
                break
            plane = plane2
        inl, a_s = inliers(plane[None], ps, ns, open_, dist_m, cos_min)
        inl, a_s = inl[0], a_s[0]
        if inl.sum() < least:
            break
        labels[inl] = len(recs)
        recs.append((plane, int(inl.sum()), 0, int(abs_q(a_s[inl]).sum())))
    out = np.zeros(len(recs), RECORD_DTYPE)
    for i, r in enumerate(recs):
        out[i] = r
    return out, labels, int((~ok).sum())


# ---- the clouds of the tests -----------------------------------------------------------------------------------------
SCENE_DIMS, SCENE_SIZE = AT.DST_DIMS, AT.DST_SIZE      # 80 x 64 x 48 over 3 m: three different cells


def scene_volume():
    return AT.scene_volume(SCENE_DIMS, SCENE_SIZE, T.tau_of(SCENE_SIZE, SCENE_DIMS, 0.03))


def scene_cloud(vol):
    """the analytic scene's crossing points and the raycast's normals at them (what hsk_extract_cloud_attrs gives)"""
    xyz = T.extract_cloud(vol, SCENE_SIZE)
    with np.errstate(all="ignore"):
        nrm = MT.normal_at(T._Grid(vol, SCENE_SIZE, SCENE_DIMS[2], 0), xyz, SCENE_DIMS)
    return xyz, nrm


def room_faces():
    """the six faces of align_twin.ROOM as (a, b, c, d) with the normal into the room"""
    lo, hi = AT.ROOM
    out = []
    for axis in range(3):
        for side, at in ((1.0, lo[axis]), (-1.0, hi[axis])):
            n = [0.0, 0.0, 0.0]
            n[axis] = side
            out.append(n + [-side * at])
    return np.array(out, f64)


def thin_wall(side=150, gap=0.03, step=0.01):
    """two parallel faces `gap` apart with opposite normals -- the two sides of one wall at x = 1 and x = 1 + gap, side x side
    points each -- and a floor at y = 0 beside them -> (points, normals, face [n]: 0, 1 the wall's faces, 2 the floor)"""
    u, v = np.meshgrid(np.arange(side) * step + 0.2, np.arange(side) * step + 0.1, indexing="ij")
    u, v = u.reshape(-1), v.reshape(-1)
    one = np.ones_like(u)
    left = np.stack([1.0 * one, v, u], axis=1)
    right = np.stack([(1.0 + gap) * one, v, u], axis=1)
    floor = np.stack([u + 1.5, 0.0 * one, v + 0.1], axis=1)
    ps = np.concatenate([left, right, floor]).astype(f32)
    ns = np.concatenate([np.tile([-1.0, 0.0, 0.0], (len(left), 1)), np.tile([1.0, 0.0, 0.0], (len(right), 1)), np.tile([0.0, 1.0, 0.0], (len(floor), 1))])
    face = np.repeat(np.arange(3), len(left))
    return ps, ns.astype(f32), face
