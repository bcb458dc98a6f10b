"""numpy restatement of a scene view's shading (include/hskinfu.h "Scene views"), written from the
rule's text: binary32 throughout, one rounding per written operator, rint ties-to-even, correctly rounded / and sqrt.  The
geometry (step 1) is the CPU oracle's raycast, called with a config that carries the view's size and intrinsics."""
import numpy as np

f32 = np.float32
LAMBERT, NORMALS, COLOR, COLOR_LIT = 0, 1, 2, 3


def geometry(oracle, view_cfg, vol, pose, omp=True):
    """step 1: (vmap, nmap), each (3, H, W) float32, NaN = no hit / no normal -- oracle.raycast for the view's camera"""
    vm, nm, _, _ = oracle.raycast(view_cfg, np.ascontiguousarray(vol), np.asarray(pose, f32), omp=omp)
    return vm, nm


def view_config(oracle, dims, W, H, fx, fy, cx, cy, size=(3.0, 3.0, 3.0)):
    """an oracle config for a volume of dims = (X, Y, Z) voxels seen by the view's camera"""
    return oracle.default_config(int(dims[0]), vol=dims, size=size, W=int(W), H=int(H), fx=fx, fy=fy, cx=cx, cy=cy)


def brightness(vm, nm, pose, light, light_in_camera):
    """step 4 for every pixel (int32; meaningful on hits): 50 + trunc(205 w), at most 255"""
    R = np.asarray(pose, f32)[:3, :3]
    t = np.asarray(pose, f32)[:3, 3]
    l = [f32(x) for x in light]
    if light_in_camera:
        l = [f32(f32(f32(R[i, 0] * l[0]) + f32(R[i, 1] * l[1])) + f32(R[i, 2] * l[2])) + t[i] for i in range(3)]
        l = [f32(x) for x in l]
    with np.errstate(all="ignore"):
        L = [(l[i] - vm[i]).astype(f32) for i in range(3)]
        s = ((L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]).astype(f32)
        dot = ((L[0] * nm[0] + L[1] * nm[1]) + L[2] * nm[2]).astype(f32)
        w = (dot * (f32(1) / np.sqrt(s))).astype(f32)
        w = np.where(w > 0, w, f32(0)).astype(f32)            # max(w, 0); NaN -> 0
        w = np.where((s == 0) | np.isnan(nm[0]), f32(0), w).astype(f32)
        br = 50 + (f32(205) * w).astype(f32).astype(np.int32)   # (w >= 0: the conversion truncates)
    return np.minimum(255, br)


def shade(vm, nm, pose, mode=LAMBERT, light=(0.0, 0.0, 0.0), light_in_camera=True, background=(0, 0, 0), color=None,
          size=(3.0, 3.0, 3.0)):
    """steps 2-5 -> dict(rgb (H, W, 3) uint8, depth (H, W) uint16, n_hit, n_uncolored).  color: the colour volume
    [Z, Y, X, 4] uint8 of (r, g, b, w), needed by the two colour modes"""
    pose = np.asarray(pose, f32).reshape(4, 4)
    R, t = pose[:3, :3], pose[:3, 3]
    H, W = vm.shape[1:]
    hit = ~np.isnan(vm[0])
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:] = np.asarray(background, np.uint8)
    with np.errstate(all="ignore"):
        # step 3
        zc = ((R[0, 2] * (vm[0] - t[0]) + R[1, 2] * (vm[1] - t[1])) + R[2, 2] * (vm[2] - t[2])).astype(f32)
        d = np.rint((zc * f32(1000)).astype(f32))
        depth = np.where(hit & (d >= 1) & (d <= 65535), d, 0).astype(np.uint16)
        n_unc = 0
        if mode in (LAMBERT, COLOR_LIT):
            br = brightness(vm, nm, pose, light, light_in_camera)
        if mode == LAMBERT:
            rgb[hit] = br[hit][:, None].astype(np.uint8)
        elif mode == NORMALS:
            has_n = hit & ~np.isnan(nm[0])
            for i in range(3):
                c = np.rint(((nm[i] * f32(0.5) + f32(0.5)).astype(f32) * f32(255)).astype(f32))
                rgb[..., i][has_n] = c[has_n].astype(np.int32).astype(np.uint8)
        else:
            Z, Y, X, _ = color.shape
            g = []
            for i, dim in enumerate((X, Y, Z)):
                cell = f32(size[i]) / f32(dim)
                q = np.floor((vm[i] / cell).astype(f32))
                g.append(np.clip(np.where(hit, q, 0), 0, dim - 1).astype(np.int64))
            cw = color[g[2], g[1], g[0]]                      # (H, W, 4)
            unc = hit & (cw[..., 3] == 0)
            n_unc = int(unc.sum())
            c = np.where(unc[..., None], 0, cw[..., :3]).astype(np.int64)
            if mode == COLOR_LIT:
                c = (c * br[..., None].astype(np.int64) + 127) // 255
            rgb[hit] = c[hit].astype(np.uint8)
    return {"rgb": rgb, "depth": depth, "n_hit": int(hit.sum()), "n_uncolored": n_unc}


def plane_volume(n=64, cells_in_front=3.5, size=3.0, trunc=0.03):
    """a volume nobody scanned: TSDF = the clipped signed distance (in units of the truncation distance) to the plane
    `cells_in_front` cells before the far z face, every weight 1.  Rays reach that plane inside the two outer cell layers,
    where the raycast gives a vertex but no normal."""
    cell = size / n
    tau = max(trunc, 2.1 * cell)
    zc = (np.arange(n) + 0.5) * cell
    sd = np.clip(((size - cells_in_front * cell) - zc) / tau, -1.0, 1.0)
    vol = np.empty((n, n, n, 2), np.int16)
    vol[..., 0] = np.rint(sd * 32767).astype(np.int16)[:, None, None]
    vol[..., 1] = 1
    return vol
