"""numpy restatement of the upright-frame estimate (include/hskinfu.h "Upright frame"), written from the rule's
text: the per-point quantities in binary32 with one rounding per written operator, everything accumulated an integer, the host
steps in binary64 (Python floats) with +, -, x, / and sqrt only, in the written order.  Also what the tests of the rule need: the
tilted analytic scenes and the cloud of edge cases."""
import math

import numpy as np

import align_twin as AT
import mesh_twin as MT
import np_twin as T

f32 = np.float32
f64 = np.float64
N_SCALE, P_SCALE, A_SCALE = 16384, 1024, 4096
FACE, HIST_BINS = 16, 6 * 16 * 16
H_BINS, H_SHIFT, H_ZERO = 16384, 16, 8192
YAW_SHIFT = 19
UNIT = float(1 << 22)                                 # t = P . R counts 2^-22 m
UP, YAW, FLOOR, CEILING = 1, 2, 4, 8
NO_YAW = 1
DEFAULTS = dict(up_hint=(0.0, -1.0, 0.0), max_tilt_cos=0.7071067811865476, cone_cos=0.984807753012208, wall_sin=0.25881904510252074,
                min_fraction=0.02, refits=3, flags=0)


# ---- the work on one point -------------------------------------------------------------------------------------------------
def cell_weights(dims, size):
    c = AT.cells(dims, size)
    return np.array([f32(min(c)) / f32(c[k]) for k in range(3)], f32)


def quantise(ps, ns, w=None):
    """-> (valid [n] bool, N [n, 3] int64, P [n, 3] int64); the integers of an invalid point are zero"""
    ps, ns = np.asarray(ps, f32).reshape(-1, 3), np.asarray(ns, f32).reshape(-1, 3)
    w = np.ones(3, f32) if w is None else np.asarray(w, f32)
    with np.errstate(all="ignore"):
        ok = np.isfinite(ps).all(axis=1) & np.isfinite(ns).all(axis=1) & (np.abs(ps) <= f32(64)).all(axis=1) & (np.abs(ns) <= f32(2)).all(axis=1)
        n0, p0 = np.where(ok[:, None], ns, f32(0)), np.where(ok[:, None], ps, f32(0))
        N = np.rint(((n0 * w[None, :]).astype(f32) * f32(N_SCALE)).astype(f32)).astype(np.int64)
        P = np.rint((p0 * f32(P_SCALE)).astype(f32)).astype(np.int64)
    ok &= (N != 0).any(axis=1)
    N[~ok], P[~ok] = 0, 0
    return ok, N, P


def hist_bins(N):
    """the cube-map bin of every (valid) integer normal"""
    a = np.abs(N)
    m = np.argmax(a, axis=1)                          # (the first of equal magnitudes)
    r = np.arange(len(N))
    nm = a[r, m]
    f = 2 * m + (N[r, m] < 0)
    den = np.maximum(2 * nm, 1)
    i = np.minimum((N[r, (m + 1) % 3] * FACE + nm * FACE) // den, FACE - 1)
    j = np.minimum((N[r, (m + 2) % 3] * FACE + nm * FACE) // den, FACE - 1)
    return (f * FACE + j) * FACE + i


def histogram(ok, N):
    return np.bincount(hist_bins(N[ok]), minlength=HIST_BINS).astype(np.uint32)


def cone(N, A, c2, inside):
    """the two cone tests against the integer axis A: (double)(dot^2) >= c2 (double)(|N|^2 |A|^2), or <= for inside = False"""
    A = np.asarray(A, np.int64)
    dot = N @ A
    lhs = (dot * dot).astype(f64)
    rhs = f64(c2) * ((N * N).sum(axis=1) * int((A * A).sum())).astype(f64)
    return (lhs >= rhs if inside else lhs <= rhs), dot


def axis_sums(ok, N, A, cone_cos):
    """-> [count, Sx, Sy, Sz] of the supporters of A, each normal sign-aligned with A"""
    c = float(f32(cone_cos))
    sup, dot = cone(N, A, c * c, True)
    sup &= ok
    sgn = np.where(dot < 0, -1, 1)[sup]
    S = (N[sup] * sgn[:, None]).sum(axis=0)
    return [int(sup.sum())] + [int(v) for v in S]


def wall_sums(ok, N, A, E1, E2, wall_sin):
    """-> [count, re, im] over the wall points of the up axis A"""
    s = float(f32(wall_sin))
    wall, _ = cone(N, A, s * s, False)
    wall &= ok
    U = ((N[wall] @ np.asarray(E1, np.int64)) + (1 << (YAW_SHIFT - 1))) >> YAW_SHIFT
    V = ((N[wall] @ np.asarray(E2, np.int64)) + (1 << (YAW_SHIFT - 1))) >> YAW_SHIFT
    U2, V2 = U * U, V * V
    return [int(wall.sum()), int((U2 * U2 - 6 * U2 * V2 + V2 * V2).sum()), int((4 * U * V * (U2 - V2)).sum())]


def extents(ok, N, P, R, cone_cos, classes=True):
    """-> (box [6]: min then max of t_k, counts [2, H_BINS] uint32, sums [2, H_BINS] int64)"""
    R = np.asarray(R, np.int64).reshape(3, 3)
    t = P[ok] @ R.T
    box = [int(v) for v in t.min(axis=0)] + [int(v) for v in t.max(axis=0)] if ok.any() else [0] * 6
    cnt, sm = np.zeros((2, H_BINS), np.uint32), np.zeros((2, H_BINS), np.int64)
    if classes and ok.any():
        c = float(f32(cone_cos))
        sup, dot = cone(N[ok], R[1], c * c, True)
        for cls, pick in ((0, sup & (dot < 0)), (1, sup & (dot > 0))):
            t1 = t[pick, 1]
            b = (t1 >> H_SHIFT) + H_ZERO
            cnt[cls] = np.bincount(b, minlength=H_BINS)
            np.add.at(sm[cls], b, t1)
    return box, cnt, sm


# ---- the host steps (binary64) ----------------------------------------------------------------------------------------------
def _norm(v):
    l = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return ([v[0] / l, v[1] / l, v[2] / l], True) if l > 0.0 and math.isfinite(l) else ([0.0, 0.0, 0.0], False)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _proj(v, d):
    s = _dot(v, d)
    return [v[0] - s * d[0], v[1] - s * d[1], v[2] - s * d[2]]


def quantise_axis(a):
    return [int(round(v * A_SCALE)) for v in a]       # (round(): half to even, as rint)


def least_count(min_fraction, n):
    return max(3, math.floor(float(f32(min_fraction)) * float(n)))


def hint_of(up_hint):
    return _norm([float(f32(v)) for v in up_hint])[0]


def solve_seed(hist, hint, max_tilt_cos, least):
    """-> (axis, support, found): the 2 x 2 block of bins, with its antipodes, of the largest count among those whose shared corner
    lies within the hint's cone; the first of equals"""
    tilt = float(f32(max_tilt_cos))
    best, best_d = -1, None
    for f in range(6):
        m = f // 2
        for j in range(FACE - 1):
            for i in range(FACE - 1):
                d = [0.0, 0.0, 0.0]
                d[m] = -1.0 if f & 1 else 1.0
                d[(m + 1) % 3] = (2 * (i + 1) - FACE) / 16.0
                d[(m + 2) % 3] = (2 * (j + 1) - FACE) / 16.0
                d = _norm(d)[0]
                if not _dot(d, hint) >= tilt:
                    continue
                sup = 0
                for jj in (j, j + 1):
                    for ii in (i, i + 1):
                        sup += int(hist[(f * FACE + jj) * FACE + ii]) + int(hist[(((f ^ 1) * FACE) + (FACE - 1 - jj)) * FACE + (FACE - 1 - ii)])
                if sup > best:
                    best, best_d = sup, d
    if best_d is None or best < least:
        return [0.0, 0.0, 0.0], max(best, 0), False
    return best_d, best, True


def solve_axis(s4, hint):
    """the axis of a count and three signed sums, in the hint's hemisphere -> (axis, ok)"""
    a, ok = _norm([float(s4[1]), float(s4[2]), float(s4[3])])
    if ok and _dot(a, hint) < 0.0:
        a = [-a[0], -a[1], -a[2]]
    return a, ok


def basis(a):
    """e1, e2 with (e1, e2, a) right-handed: e1 from the volume axis of the smallest |a_k|"""
    k = 0
    for c in (1, 2):
        if abs(a[c]) < abs(a[k]):
            k = c
    e = [0.0, 0.0, 0.0]
    e[k] = 1.0
    e1 = _norm(_proj(e, a))[0]
    return e1, _cross(a, e1)


def plain_x(a):
    """without a yaw: the volume's +X, or +Z where +X is degenerate, projected off a"""
    e = [0.0, 0.0, 1.0] if a[0] * a[0] > 0.5 else [1.0, 0.0, 0.0]
    return _norm(_proj(e, a))[0]


def solve_yaw(w3, least, a):
    """-> (x, found)"""
    cnt, re, im = int(w3[0]), float(w3[1]), float(w3[2])
    r = math.sqrt(re * re + im * im)
    if cnt < least or not r > 0.0:
        return plain_x(a), False
    c, s = re / r, im / r
    for _ in range(2):
        c, s = math.sqrt((1.0 + c) / 2.0), math.copysign(math.sqrt((1.0 - c) / 2.0), s)
    e1, e2 = basis(a)
    x = [c * e1[k] + s * e2[k] for k in range(3)]
    q = _cross(a, x)
    best = x
    for cand in (q, [-v for v in x], [-v for v in q]):
        if cand[0] > best[0]:
            best = cand
    return _norm(_proj(best, a))[0], True


def frame_rows(a, x):
    d = [-a[0], -a[1], -a[2]]
    return [x, d, _cross(x, d)]


def solve_frame(s12, least, hint, a, x, yaw):
    """one refit of the frame from the three axes' counts and sums -> (a, x)"""
    if s12[4] >= least:
        a2, ok = solve_axis(s12[4:8], hint)
        if ok:
            a = a2
    d = [-a[0], -a[1], -a[2]]
    v = [0.0, 0.0, 0.0]
    if yaw:
        if s12[0] >= least:
            v = _proj([float(s12[1]), float(s12[2]), float(s12[3])], d)
        if s12[8] >= least:
            u = _cross(d, _proj([float(s12[9]), float(s12[10]), float(s12[11])], d))
            v = [v[0] + u[0], v[1] + u[1], v[2] + u[2]]
    x2, ok = _norm(v)
    if not ok:
        x2 = _norm(_proj(x, d))[0]
    return a, x2


def solve_heights(cnt, sm, least):
    """-> (floor_m, ceiling_m, found bits)"""
    out, bits = [0.0, 0.0], 0
    for cls in (0, 1):
        c = cnt[cls].astype(np.int64)
        if int(c.sum()) < least or int(c.sum()) == 0:
            continue
        peak = int(c.max())
        at = np.flatnonzero(2 * c >= peak)
        b = int(at[-1] if cls == 0 else at[0])
        lo, hi = max(b - 1, 0), min(b + 1, H_BINS - 1)
        out[cls] = (float(int(sm[cls, lo:hi + 1].sum())) / float(int(c[lo:hi + 1].sum()))) / UNIT
        bits |= FLOOR if cls == 0 else CEILING
    return out[0], out[1], bits


# ---- the whole estimate ------------------------------------------------------------------------------------------------------
def estimate(ps, ns, w=None, up_hint=(0.0, -1.0, 0.0), max_tilt_cos=DEFAULTS["max_tilt_cos"], cone_cos=DEFAULTS["cone_cos"],
             wall_sin=DEFAULTS["wall_sin"], min_fraction=0.02, refits=3, flags=0):
    """hsk_estimate_upright_oriented -> a dict of hsk_upright's fields, plus `trace`: every device answer in the order asked"""
    ok, N, P = quantise(ps, ns, w)
    n = len(ok)
    out = dict(level=np.eye(4, dtype=f32), floor_m=f32(0), ceiling_m=f32(0), box_lo=np.zeros(3, f32), box_hi=np.zeros(3, f32), n_points=n,
               n_invalid=int((~ok).sum()), n_axis=[0, 0, 0], n_walls=0, found=0, trace=[])
    if n == 0:
        return out
    hint = hint_of(up_hint)
    least = least_count(min_fraction, n)
    hist = histogram(ok, N)
    out["trace"].append(("hist", hist))
    a, support, found_up = solve_seed(hist, hint, max_tilt_cos, least)
    yaw = False
    if found_up:
        out["found"] |= UP
        out["n_axis"][1] = support
        for _ in range(refits):
            s4 = axis_sums(ok, N, quantise_axis(a), cone_cos)
            out["trace"].append(("axis", s4))
            if s4[0] < least:
                break
            a2, good = solve_axis(s4, hint)
            if not good:
                break
            a = a2
        x = plain_x(a)
        if not flags & NO_YAW:
            e1, e2 = basis(a)
            w3 = wall_sums(ok, N, quantise_axis(a), quantise_axis(e1), quantise_axis(e2), wall_sin)
            out["trace"].append(("walls", w3))
            out["n_walls"] = w3[0]
            x, yaw = solve_yaw(w3, least, a)
            if yaw:
                out["found"] |= YAW
        for _ in range(refits):
            rows = frame_rows(a, x)
            s12 = []
            for k in range(3):
                s12 += axis_sums(ok, N, quantise_axis(rows[k]), cone_cos)
            out["trace"].append(("frame", s12))
            out["n_axis"] = [s12[0], s12[4], s12[8]]
            a, x = solve_frame(s12, least, hint, a, x, yaw)
        out["level"][:3, :3] = np.array(frame_rows(a, x), f64).astype(f32)
    R = [quantise_axis([float(v) for v in out["level"][k, :3]]) for k in range(3)]
    box, cnt, sm = extents(ok, N, P, R, cone_cos, classes=found_up)
    out["trace"].append(("extents", box, cnt, sm))
    if ok.any():
        out["box_lo"] = np.array([box[k] / UNIT for k in range(3)], f64).astype(f32)
        out["box_hi"] = np.array([box[3 + k] / UNIT for k in range(3)], f64).astype(f32)
    if found_up:
        fl, ce, bits = solve_heights(cnt, sm, least)
        out["floor_m"], out["ceiling_m"] = f32(fl), f32(ce)
        out["found"] |= bits
    return out


# ---- hsk_level_config ----------------------------------------------------------------------------------------------------------
def level_config(dims, size, trunc, up, margin_m=None):
    """-> (dst dims, dst size [3] binary32, dst trunc binary32, M [4, 4] binary32)"""
    c = max(AT.cells(dims, size))
    tau = T.tau_of(size, dims, trunc)
    margin = f32(tau + f32(2) * c) if margin_m is None or margin_m < 0 else f32(margin_m)
    lo = [float(up["box_lo"][k]) - float(margin) for k in range(3)]
    hi = [float(up["box_hi"][k]) + float(margin) for k in range(3)]
    out_dims, out_size = [], []
    for k in range(3):
        d = max(8, 8 * math.ceil((hi[k] - lo[k]) / float(c) / 8.0))
        while True:
            s = f32(f32(d) * c)
            while f32(s / f32(d)) > c:
                s = np.nextafter(s, f32(0))
            if float(s) >= hi[k] - lo[k]:
                break
            d += 8
        out_dims.append(d)
        out_size.append(s)
    M = np.array(up["level"], f64)
    M[:3, 3] = [-v for v in lo]
    return tuple(out_dims), np.array(out_size, f32), f32(tau), M.astype(f32)


# ---- the clouds of the tests ---------------------------------------------------------------------------------------------------
def rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def about_centre(R):
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.array(AT.CENTRE) - R @ np.array(AT.CENTRE)
    return M


TILTS = {"a": rot(0, 11.0) @ rot(2, 6.0) @ rot(1, 9.0), "b": rot(0, -20.0) @ rot(2, 3.0) @ rot(1, 40.0), "level": np.eye(3)}
SCENES = {"80x64x48": ((80, 64, 48), (3.0, 3.0, 3.0)), "64": ((64, 64, 64), (3.0, 3.0, 3.0))}


def scene(dims, size, R, trunc=0.03):
    """(volume, points, normals) of the analytic scene turned by R^T about the centre: a scene direction d lies along R^T d"""
    tau = T.tau_of(size, dims, trunc)
    vol = AT.scene_volume(dims, size, tau, about_centre(R))
    xyz = T.extract_cloud(vol, size)
    with np.errstate(all="ignore"):
        nrm = MT.normal_at(T._Grid(vol, size, dims[2], 0), xyz, dims)
    return vol, xyz, nrm


def edge_cloud():
    """the hand-made cloud of edge cases: NaN and zero normals, |n_k| > 2, ties of the largest component, normals exactly on bin
    edges, an antipodal pair, dot = 0 against the axes the tests use, points at +-64 m and just beyond"""
    above = np.nextafter(f32(64), f32(np.inf))
    ns = [(np.nan, 0, 1), (0, 0, 0), (1e-9, 0, 0), (2.5, 0, 0), (0, -2.0, 0), (0, np.inf, 0), (1, 1, 0), (1, -1, 1), (-1, -1, -1), (0.5, 0.5, -0.5),
          (1, 0.125, 0), (1, -0.125, 0.25), (1, 1, 1), (0, 1, 0.875), (0.6, -0.8, 0), (-0.6, 0.8, 0), (0, -1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1),
          (0, 0, -1), (-1, 0, 0), (0.8, 0, 0.6), (0.6, 0, -0.8), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, -1, 0), (0, 1, 0), (3e-5, -3e-5, 0)]
    ps = [(0.5, 0.5, 0.5)] * len(ns)
    ps = np.array(ps, f32)
    ps[24], ps[25], ps[26], ps[27], ps[28] = (64, -64, 64), (-64, 64, -64), (above, 0, 0), (0, np.nan, 0), (0, 0, -above)
    return ps, np.array(ns, f32)
