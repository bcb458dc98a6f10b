"""numpy restatement of pose scoring and relocalisation (include/hskinfu.h "Loss hold and relocalisation"), written
from the rule's text: binary32 unless said, one rounding per written operator; every sum is an integer.  The sample is
align_twin.probe's (the raycast's trilinear sample), the refinement align_twin.align.  Also what the tests of the rule need: a
look-at camera, the candidate lattice in binary64, and frames of align_twin's analytic scene traced ray by ray.

A volume is the host array of hsk_download_tsdf: [Z, Y, X, 2] int16 (tsdf, weight)."""
import numpy as np

import align_twin as AT

f32 = np.float32
f64 = np.float64
FOUND, NONE, EMPTY = 0, 1, 2
STATUS = ("found", "none", "empty")
CLASSES = ("n_near", "n_free", "n_behind", "n_unseen", "n_outside", "n_skipped")
SCORE_DTYPE = np.dtype([(c, "<u4") for c in CLASSES] + [("sum_abs", "<u8")])     # hsk_pose_score


def classes(vol, size, ps, poses):
    """the rule for the points ps [n, 3] under the poses [m, 4, 4] -> (class [m, n] in 0..5, q [m, n]: what a near point adds to
    sum_abs)"""
    M = np.asarray(poses, f32).reshape(-1, 4, 4)
    R, t = M[:, :3, :3, None], M[:, :3, 3, None]
    x, y, z = (np.ascontiguousarray(ps[:, i], f32)[None, :] for i in range(3))
    with np.errstate(all="ignore"):
        p = [(((R[:, i, 0] * x + R[:, i, 1] * y).astype(f32) + R[:, i, 2] * z).astype(f32) + t[:, i]).astype(f32) for i in range(3)]
        inside, F, Ws, _ = AT.probe(vol, size, p)
        aF = np.abs(F)
        cls = np.where(F > 0, 1, 2)
        cls = np.where(aF < 1, 0, cls)
        cls = np.where(Ws > 0, cls, 3)
        cls = np.where(inside, cls, 4)
        cls = np.where(np.isnan(x) | np.isnan(y) | np.isnan(z), 5, cls)
        q = np.rint(np.where(cls == 0, aF, f32(0)).astype(f64) * 65536.0).astype(np.int64)
    return cls, q


def score(vol, size, ps, poses, batch=64):
    """hsk_score_cloud -> a SCORE_DTYPE array, one record per pose"""
    ps = np.asarray(ps, f32).reshape(-1, 3)
    poses = np.asarray(poses, f32).reshape(-1, 4, 4)
    out = np.zeros(len(poses), SCORE_DTYPE)
    if len(ps) == 0:
        return out
    for j in range(0, len(poses), batch):
        cls, q = classes(vol, size, ps, poses[j:j + batch])
        for c, name in enumerate(CLASSES):
            out[name][j:j + batch] = (cls == c).sum(axis=1)
        out["sum_abs"][j:j + batch] = q.sum(axis=1)
    return out


def rank(scores):
    """hsk_rank_scores: key = n_near - n_free - n_behind (signed), larger first; ties to the smaller sum_abs, then the lower index"""
    s = np.asarray(scores)
    key = s["n_near"].astype(np.int64) - s["n_free"].astype(np.int64) - s["n_behind"].astype(np.int64)
    return np.array(sorted(range(len(s)), key=lambda i: (-int(key[i]), int(s["sum_abs"][i]), i)), np.uint32)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], f64)


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], f64)


def shift(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def displaced(pose, t, yaw_deg, pitch_deg):
    """pose . T(t) . Ry(yaw) . Rx(pitch): a camera moved in its own frame (binary64)"""
    return np.asarray(pose, f64) @ shift(*t) @ rot_y(np.radians(yaw_deg)) @ rot_x(np.radians(pitch_deg))


def lattice(centre, step_m, n_trans, step_rad, n_rot):
    """hsk_pose_lattice in binary64, rounded once -> [n, 4, 4] binary32; i slowest, then j, k, a, and b fastest"""
    c = np.asarray(centre, f32).reshape(4, 4).astype(f64)
    step_m, step_rad = f64(f32(step_m)), f64(f32(step_rad))
    T, A = range(-n_trans, n_trans + 1), range(-n_rot, n_rot + 1)
    out = [c @ shift(i * step_m, j * step_m, k * step_m) @ rot_y(a * step_rad) @ rot_x(b * step_rad) for i in T for j in T for k in T for a in A for b in A]
    return np.array(out).astype(f32)


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """the camera at `eye` looking at `target` (z forward, x right, y down in the image, `up` upwards in it) -> [4, 4] binary64"""
    eye, target, up = (np.asarray(v, f64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def trace(pose, w, h, fx, fy, cx, cy):
    """align_twin's scene (a room seen from inside, a box on its floor) seen from the camera `pose`, ray by ray, analytically
    -> (points [h w, 3] in camera coordinates, unit normals [h w, 3] in camera coordinates facing the camera), binary32,
    row-major; the camera must stand in the room's free space"""
    pose = np.asarray(pose, f64)
    R, e = pose[:3, :3], pose[:3, 3]
    v, u = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones(u.shape)], -1).reshape(-1, 3)
    d = d_cam @ R.T
    with np.errstate(all="ignore"):
        def slabs(box):
            lo, hi = (np.asarray(box[0]) - e) / d, (np.asarray(box[1]) - e) / d
            return np.minimum(lo, hi), np.maximum(lo, hi)
        # the room from inside: where the ray leaves it
        _, far = slabs(AT.ROOM)
        t, axis = far.min(axis=1), far.argmin(axis=1)
        # the furniture from outside: where the ray enters it, if it does
        near, far = slabs(AT.FURNITURE)
        tn, tf = near.max(axis=1), far.min(axis=1)
        hit = (tn <= tf) & (tn > 0) & (tn < t)
    t, axis = np.where(hit, tn, t), np.where(hit, near.argmax(axis=1), axis)
    n_world = np.zeros_like(d)
    n_world[np.arange(len(d)), axis] = -np.sign(d[np.arange(len(d)), axis])
    return (d_cam * t[:, None]).astype(f32), (n_world @ R).astype(f32)


def relocalize(vol, size, tau, ps, ns, poses, n_refine=4, accept_fraction=0.5, accept_rms_m=None, **align):
    """hsk_relocalize behind the preprocessing: the cloud ps with normals ns (NaN rows: invalid pixels) -> (M [4, 4] binary32,
    stats: status, n_valid, n_candidates, best, scores, order, candidate, refined: align_twin.align's result per refined candidate)"""
    ps, ns = np.asarray(ps, f32).reshape(-1, 3), np.asarray(ns, f32).reshape(-1, 3)
    poses = np.asarray(poses, f32).reshape(-1, 4, 4)
    st = {"status": EMPTY, "n_valid": 0, "n_candidates": len(poses), "best": -1, "candidate": [], "refined": []}
    if len(poses) == 0 or len(ps) == 0:
        return np.eye(4, dtype=f32), st
    sc = score(vol, size, ps, poses)
    st["scores"], st["n_valid"] = sc, len(ps) - int(sc["n_skipped"][0])
    if st["n_valid"] == 0:
        return np.eye(4, dtype=f32), st
    order = rank(sc)
    st["order"] = order
    rms_bar = f32(tau) / f32(4) if accept_rms_m is None else f32(accept_rms_m)
    need = f64(f32(accept_fraction)) * f64(st["n_valid"])
    st["status"], st["best"], out, win = NONE, int(order[0]), poses[order[0]].copy(), None
    for r in range(min(n_refine, len(poses))):
        M, a = AT.align(vol, size, tau, ps, ns, poses[order[r]], **align)
        st["candidate"].append(int(order[r]))
        st["refined"].append((M, a))
        used, rms = a["n_used"][-1], a["rms_m"][-1]
        if a["status"] == AT.CONVERGED and f64(used) >= need and rms <= rms_bar and (win is None or used > win[0] or (used == win[0] and rms < win[1])):
            win, out = (used, rms), M
            st["status"], st["best"] = FOUND, int(order[r])
    return out, st
