"""The colour twin (tests/color_twin.py) pinned without a GPU: against the rule written out voxel by voxel in scalar float32
steps, against the integrate's twin (every voxel coloured is one the integrate has just updated), and the band's three
regimes."""
import numpy as np
import pytest

import color_cases as CC
import color_twin as CT
from np_twin import integrate_full, scale_depth, tau_of

f32 = np.float32


def scalar_color(col, size3, scaled, rgb, fx, fy, cx, cy, pose, band, max_w):
    """the rule of housescan_amd/csrc/color.hip's header and DESIGN.md "Colour", a voxel at a time, every operator on float32
    scalars and rounding once: project with the integrate's arithmetic; take the pixel's colour iff the pixel is in the image,
    D_s != 0 and -band < sdf < band; c' = (c w + p + ((w + 1) >> 1)) // (w + 1), w' = min(w + 1, max_w)"""
    Z, Y, X, _ = col.shape
    H, W = scaled.shape
    cell = [f32(size3[0]) / f32(X), f32(size3[1]) / f32(Y), f32(size3[2]) / f32(Z)]
    R = [[f32(pose[i][j]) for j in range(3)] for i in range(3)]
    t = [f32(pose[i][3]) for i in range(3)]
    fx, fy, cx, cy, band = f32(fx), f32(fy), f32(cx), f32(cy), f32(band)
    tiny, lim = f32(1.17549435e-38), f32(1e6)
    n = 0
    with np.errstate(all="ignore"):
        for z in range(Z):
            gz = (f32(z) + f32(0.5)) * cell[2] - t[2]
            for y in range(Y):
                gy = (f32(y) + f32(0.5)) * cell[1] - t[1]
                for x in range(X):
                    gx = (f32(x) + f32(0.5)) * cell[0] - t[0]
                    # camera = R^T g
                    c0 = (R[0][0] * gx + R[1][0] * gy) + R[2][0] * gz
                    c1 = (R[0][1] * gx + R[1][1] * gy) + R[2][1] * gz
                    c2 = (R[0][2] * gx + R[1][2] * gy) + R[2][2] * gz
                    if not c2 >= tiny:
                        continue
                    inv_z = f32(1) / c2
                    fu = (c0 * fx) * inv_z + cx
                    fv = (c1 * fy) * inv_z + cy
                    if not (-lim < fu < lim and -lim < fv < lim):
                        continue
                    u, v = int(np.rint(fu)), int(np.rint(fv))
                    if u < 0 or v < 0 or u >= W or v >= H:
                        continue
                    Ds = f32(scaled[v, u])
                    if Ds == 0:
                        continue
                    sdf = Ds - np.sqrt(gz * gz + (gx * gx + gy * gy))
                    if not (-band < sdf < band):
                        continue
                    w = int(col[z, y, x, 3])
                    for ch in range(3):
                        col[z, y, x, ch] = (int(col[z, y, x, ch]) * w + int(rgb[v, u, ch]) + ((w + 1) >> 1)) // (w + 1)
                    col[z, y, x, 3] = min(w + 1, max_w)
                    n += 1
    return n


def _rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _pose(R, t):
    P = np.eye(4, dtype=f32)
    P[:3, :3] = np.asarray(R, np.float64).astype(f32)
    P[:3, 3] = np.asarray(t, f32)
    return P


@pytest.mark.parametrize("max_w", [1, 255])
def test_twin_equals_the_scalar_rule(max_w):
    dims, size = (16, 8, 12), (0.8, 0.5, 0.48)
    W, H, fx, fy, cx, cy = 20, 12, 17.0, 15.5, 10.25, 5.0
    rng = np.random.default_rng(max_w)
    poses = [_pose(_rot(1, 25.0) @ _rot(0, -15.0), (0.37, 0.21, 0.2)),      # inside the volume, voxels all round it
             _pose(np.eye(3), (0.4, 0.25, -0.3)),                           # axis-aligned, in front of the z = 0 face
             _pose(_rot(0, 90.0), (0.425, 0.6, 0.22)),                      # axis-aligned about x: looks along -y from above
             _pose(_rot(2, 40.0) @ _rot(1, 160.0), (0.3, 0.2, 0.6))]        # looks back through the volume, part of it behind
    col = CC.random_color(rng, dims, max_w)
    col[..., 3][rng.random(col.shape[:3]) < 0.3] = 0
    assert (col[..., 3] == 0).any() and (col[..., 3] == max_w).any()
    assert max_w == 1 or ((col[..., 3] > 0) & (col[..., 3] < max_w)).any()
    ref = col.copy()
    band = CT.band_of(dims, size, 0.0, 0.03)
    behind = 0
    for k, pose in enumerate(poses):
        depth = rng.integers(150, 700, size=(H, W)).astype(np.uint16)
        depth[rng.random((H, W)) < 0.1] = 0
        rgb = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        scaled = scale_depth(depth, fx, fy, cx, cy)
        b = band if k != 2 else f32(0.02)   # (one frame with a band thinner than a cell)
        n = CT.integrate_color(col, size, scaled, rgb, fx, fy, cx, cy, pose, b, max_w)
        assert scalar_color(ref, size, scaled, rgb, fx, fy, cx, cy, pose, b, max_w) == n > 0, k
        assert np.array_equal(col, ref), f"pose {k}: {(col != ref).any(axis=3).sum()} voxels differ"
        corners = np.array([[x, y, z] for x in (0, size[0]) for y in (0, size[1]) for z in (0, size[2])])
        behind += ((corners - pose[:3, 3]) @ pose[:3, 2] < 0).any()
    assert CC.inside(poses[0], size) and behind >= 2


@pytest.mark.parametrize("camera", list(CC.CAMERAS))
def test_colored_voxels_are_the_ones_the_integrate_updates(camera):
    """band = tau on a zero TSDF and a zero colour volume, one frame: every voxel the integrate left with weight 1 and
    |tsdf| < 32767 is coloured, and every coloured voxel has weight 1 -- on the ragged volume, with either camera"""
    checked = 0
    for seed in CC.SEEDS:
        _, dims, size, cam, _, frames = CC.fuzz_case("ragged", camera, seed)
        tau = tau_of(size, dims, CC.TRUNC)
        for pose, depth, rgb, _, _ in frames:
            scaled = scale_depth(depth, *cam[2:])
            vol = np.zeros((dims[2], dims[1], dims[0], 2), np.int16)
            col = np.zeros((dims[2], dims[1], dims[0], 4), np.uint8)
            integrate_full(vol, size, CC.TRUNC, scaled, *cam[2:], pose)
            n = CT.integrate_color(col, size, scaled, rgb, *cam[2:], pose, tau, 64)
            colored = col[..., 3] != 0
            assert n == colored.sum()
            near = (vol[..., 1] == 1) & (np.abs(vol[..., 0].astype(np.int32)) < 32767)
            assert not (near & ~colored).any(), "a voxel the integrate put inside the truncation band stayed uncoloured"
            assert (vol[..., 1][colored] == 1).all(), "a coloured voxel the integrate did not update"
            checked += int(n)
    assert checked > 10000


def test_band_of_three_regimes():
    dims, size = (72, 40, 50), (2.7, 1.8, 1.5)     # cells 37.5 / 45 / 30 mm: the largest is y's, not x's
    cell = [f32(size[i]) / f32(dims[i]) for i in range(3)]
    assert max(cell) == cell[1] != cell[0]
    tau = tau_of(size, dims, 0.03)
    assert tau == f32(2.1) * cell[1]               # (2.1 cells is more than the 30 mm asked for)
    assert CT.band_of(dims, size, 0.0, 0.03) == f32(2.0) * cell[1] < tau          # default: two of the largest cells
    assert CT.band_of(dims, size, -1.0, 0.03) == f32(2.0) * cell[1]
    assert CT.band_of(dims, size, 0.004, 0.03) == f32(0.004)                      # explicit, thinner than a cell
    assert CT.band_of(dims, size, 1.0, 0.03) == tau                               # capped at tau
    assert CT.band_of(dims, size, 0.0, 0.2) == f32(2.0) * cell[1]                 # a long truncation distance leaves the default
    assert CT.band_of(dims, size, 0.15, 0.2) == f32(0.15) and CT.band_of(dims, size, 0.25, 0.2) == f32(0.2)
    assert CT.band_of((64, 64, 64), (3.0,) * 3, 0.0, 0.03) == f32(2.0) * (f32(3.0) / f32(64))
