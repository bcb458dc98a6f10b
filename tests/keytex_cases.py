"""The small cases of keyframe textures, shared by tests/test_keytex_host.py (the kernel's text on the CPU) and
tests/test_gpu_keytex.py (the kernel): the analytic wall of tests/texture_cases.py with hand-made keyframes of 50 x 38 pixels
(neither a multiple of 4; fx = fy = 40), the box case with three keyframes rendered on the CPU by tests/view_twin.py, and 70
keyframes of 16 x 12 pixels around the wall -- one more than any staging by 32 or 64 would take at a time.  The twin's results are
made once and left unchanged.

The wall is the plane x = WALL_PLANE_M with its normal along +x; a camera "in front" stands on the +x side and looks along -x."""
import numpy as np

import keytex_twin as KT
import simplify_twin as ST
import texture_cases as TC
import view_twin as VT
from simplify_cases import BOX_DIMS, twin_of

f32 = np.float32


def differing(got, tw):
    """the differing bytes of a keyframe bake against the twin's: every output, the charts and both infos"""
    n = 0
    for name in ("rgb", "normal_rgb", "mask", "source"):
        assert got[name].shape == tw[name].shape, (name, got[name].shape, tw[name].shape)
        n += int((got[name] != tw[name]).sum())
    n += int((np.ascontiguousarray(got["uv"]).view(np.uint32) != tw["uv"].view(np.uint32)).sum())
    n += int((np.asarray(got["charts"]).view(np.int32).reshape(-1, 4) != tw["charts"].view(np.int32).reshape(-1, 4)).sum())
    n += sum(a != b for a, b in zip(TC.info_list(got["info"]), TC.info_list(tw["info"])))
    n += sum(a != b for a, b in zip(kinfo_list(got["kinfo"]), kinfo_list(tw["kinfo"])))
    return n


_CACHE = {}
KW, KH, KF = 50, 38, 40.0
INTR = np.array([KF, KF, (KW - 1) / 2.0, (KH - 1) / 2.0], f32)
WALL_PLANE_M = (TC.WALL_X + 0.5) * TC.WALL_CELL
WALL_MID_M = (15 + 0.5) * TC.WALL_CELL           # the middle of wall_mesh's square, in y and in z
FRONT_M = 1.8                                    # the frontal camera's distance: a pixel is 45 mm there, two are less than a 93.75 mm voxel
NEAR_DEPTH_MM, HOLE = 1300, (slice(10, 16), slice(30, 37))     # the edited depth image: an occluder 0.5 m nearer, a block of D = 0
LEFT_COLS = 17                                   # its columns 0 .. 16 are the occluder's: columns 16 and 17 are where the two depths meet


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world pose (4 x 4 float32) of a camera at `eye` whose z axis points at `target` (x right, y down)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m.astype(f32)


def frontal_pose(distance=FRONT_M, side=1.0):
    return look_at((WALL_PLANE_M + side * distance, WALL_MID_M, WALL_MID_M), (WALL_PLANE_M, WALL_MID_M, WALL_MID_M))


def plane_depth(pose, intr, w, h):
    """the exact depth image of the wall's plane from a camera, in millimetres (0 where the ray does not reach it in front)"""
    fx, fy, cx, cy = (float(v) for v in intr)
    R, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    d = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones((h, w))], axis=-1) @ R.T       # the rays at z_c = 1, in world coordinates
    with np.errstate(all="ignore"):
        z = (WALL_PLANE_M - t[0]) / d[..., 0]
    return np.where(np.isfinite(z) & (z > 0) & (z < 60), np.rint(z * 1000.0), 0).astype(np.uint16)


def stripes(w=KW, h=KH):
    """two-pixel stripes of two levels 128 apart: red along x, green along y, blue a checker of both"""
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.stack([64 + 128 * ((i // 2) & 1), 64 + 128 * ((j // 2) & 1), 64 + 128 * (((i // 2) + (j // 2)) & 1)], axis=-1).astype(np.uint8)


def noise(seed, w=KW, h=KH):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def frontal(rgb=None):
    pose = frontal_pose()
    return KT.keyframe(plane_depth(pose, INTR, KW, KH), stripes() if rgb is None else rgb, pose, INTR)


def frontal_edited():
    kf = frontal()
    d = kf["depth"].copy()
    d[:, :LEFT_COLS] = NEAR_DEPTH_MM
    d[HOLE] = 0
    return dict(kf, depth=d)


def competing():
    """0 frontal; 1 oblique and farther, seeing the whole mesh; 2 = 0 again (the tie goes to 0); 3 behind the wall (the view angle
    fails); 4 so near that z_min_m cuts it; 5 frontal at 1 m, whose image border cuts the mesh"""
    def cam(pose, seed):
        return KT.keyframe(plane_depth(pose, INTR, KW, KH), noise(seed), pose, INTR)
    oblique = look_at((WALL_PLANE_M + 2.6, WALL_MID_M, WALL_MID_M + 0.8), (WALL_PLANE_M, WALL_MID_M, WALL_MID_M))
    return [frontal(), cam(oblique, 1), frontal(), cam(frontal_pose(1.0, -1.0), 3), cam(frontal_pose(0.2), 4), cam(frontal_pose(1.0), 5)]


def ring70():
    """70 keyframes of 16 x 12 pixels on an arc in front of the wall, all looking at its middle"""
    intr = np.array([12.0, 12.0, 7.5, 5.5], f32)
    out = []
    for k in range(70):
        a = np.radians(-50.0 + 100.0 * k / 69.0)
        r = 1.6 + 0.01 * k
        pose = look_at((WALL_PLANE_M + r * np.cos(a), WALL_MID_M + r * np.sin(a), WALL_MID_M + 0.3 * np.sin(3 * a)), (WALL_PLANE_M, WALL_MID_M, WALL_MID_M))
        out.append(KT.keyframe(plane_depth(pose, intr, 16, 12), noise(100 + k, 16, 12), pose, intr))
    return out


def box_keyframes(oracle):
    """three views of the box room's inside, 40 x 30 pixels: depth and colour rendered by the view twin from the box case's volumes"""
    if "boxkf" not in _CACHE:
        vol, col, size = TC.box_case()
        intr = np.array([30.0, 30.0, 19.5, 14.5], f32)
        cfg = VT.view_config(oracle, BOX_DIMS, 40, 30, *[float(v) for v in intr], size=size)
        out = []
        for eye, target in (((0.6, 0.8, 0.6), (2.5, 0.8, 0.6)), ((2.0, 0.5, 0.45), (0.3, 1.2, 0.7)), ((1.35, 0.35, 0.8), (1.35, 1.5, 0.3))):
            pose = look_at(eye, target)
            vm, nm = VT.geometry(oracle, cfg, vol, pose)
            sh = VT.shade(vm, nm, pose, mode=VT.COLOR, color=col, size=size)
            out.append(KT.keyframe(sh["depth"], sh["rgb"], pose, intr))
        assert all((k["depth"] > 0).mean() > 0.5 for k in out)
        _CACHE["boxkf"] = out
    return _CACHE["boxkf"]


def wall_cases():
    """{name: (vol, col, size, vertices, faces, keyframes, keytex params, texture params)} on the analytic wall"""
    vol, col = TC.wall_volume(), TC.wall_colour()
    v, f = TC.wall_mesh(0.3)
    tex = dict(atlas_width=128)
    return {
        "frontal": (vol, None, TC.WALL_SIZE, v, f, [frontal()], {}, tex),
        "edited depth": (vol, None, TC.WALL_SIZE, v, f, [frontal_edited()], {}, tex),
        "edited depth, fallback": (vol, col, TC.WALL_SIZE, v, f, [frontal_edited()], {}, tex),
        "competing": (vol, col, TC.WALL_SIZE, v, f, competing(), dict(fallback_volume=0), tex),
        "ring of 70": (vol, None, TC.WALL_SIZE, v, f, ring70(), dict(border_px=1.0, cos_min=0.1, blend_floor=0.25), tex),
        "empty store": (vol, col, TC.WALL_SIZE, v, f, [], {}, tex),
    }


def box_cases(oracle):
    vol, col, size = TC.box_case()
    tw = twin_of(oracle, "box with colour", 8, ST.QUADRIC)
    kfs = box_keyframes(oracle)
    return {
        "box": (vol, col, size, tw["vertices"], tw["faces"], kfs, {}, dict(atlas_width=64)),
        "box, no colour, loose": (vol, None, size, tw["vertices"], tw["faces"], kfs, dict(border_px=0.0, cos_min=0.0, z_min_m=0.0, blend_floor=0.0),
                                  dict(atlas_width=256)),
    }


def all_cases(oracle):
    return dict(wall_cases(), **box_cases(oracle))


def twin_bake(key, mode, vol, col, size, v, f, kfs, keytex, tex):
    """the twin's bake of a named case in a mode, made once and left unchanged"""
    if (key, mode) not in _CACHE:
        _CACHE[(key, mode)] = KT.bake(vol, col, size, v, f, kfs, dict(keytex, mode=mode), **tex)
    return _CACHE[(key, mode)]


def kinfo_list(kinfo):
    return [kinfo[n] for n in KT.KINFO_FIELDS]


def project64(kf, points):
    """the pixel (u, v) of world points [m, 3] in a keyframe, and z_c, in binary64"""
    R, t = kf["pose"][:3, :3].astype(np.float64), kf["pose"][:3, 3].astype(np.float64)
    fx, fy, cx, cy = (float(x) for x in kf["intr"])
    c = (points.astype(np.float64) - t) @ R
    return fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy, c[:, 2]
