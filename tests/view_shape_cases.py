"""The shapes, fillings and cameras of the image kernels' shape tests (tests/test_view_shapes_host.py, tests/test_gpu_view_shapes.py),
and the brick tests' shape table, scene filling and poses (tests/test_gpu_bricks.py), which those tests share.

Volumes: non-cubic, a cell per axis, filled with align_twin's room (scene_fill) and, where named, a random colour volume with 45 %
of its weights and one whole z plane of them 0.  Cameras: fitted to each volume's box -- section cameras (a)-(f) and the two view
cameras (g).  References: section_twin.render, computed once per (volume, camera) and handed out read-only.  The comparisons
(assert_section, assert_view, check_camera) stand here too, so that no test imports another."""
import numpy as np

import align_twin as AT
import section_twin as ST
import view_twin as VT
from kit import same_bits_nan
from np_twin import tau_of
from view_cases import RAGGED

f32 = np.float32
EYE = np.eye(3, dtype=np.float32)
CYC = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float32)    # volume x <- world z, volume y <- world x, volume z <- world y
TAU_SCENE = 0.1                                                   # the truncation of the uploaded scene, in the scene's own units
TRUNC = 0.03                                                      # the contexts' truncation distance (metres), given to both sides
MODES = (VT.LAMBERT, VT.NORMALS, VT.COLOR, VT.COLOR_LIT)
ODD = dict(width=240, height=200, fx=190.0, fy=190.0, cx=119.5, cy=99.5)   # 25 rows of 8 x 8 tiles (RAGGED: 28, the last ragged)


def look(eye, at, down=(0.0, 0.0, 1.0)):
    """camera-to-volume pose: at `eye` (metres), its z axis towards `at`, its y axis (image rows downwards) as near `down` as
    that allows"""
    eye, at = np.asarray(eye, np.float64), np.asarray(at, np.float64)
    z = (at - eye) / np.linalg.norm(at - eye)
    d = np.asarray(down, np.float64)
    if abs(d @ z) > 0.95:
        d = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(d, z)
    x /= np.linalg.norm(x)
    P = np.eye(4, dtype=np.float32)
    P[:3, :3] = np.stack([x, np.cross(z, x), z], axis=1).astype(np.float32)
    P[:3, 3] = eye.astype(np.float32)
    return P


def along_x(eye):
    """a camera that looks exactly along +x (its central rays run the length of a brick row); image rows downwards = +z"""
    return look(eye, np.asarray(eye, np.float64) + [1.0, 0.0, 0.0])


# dims (X, Y, Z) and size in metres (the three cells within a factor of three of one another);
# scene: the uploaded filling -- align_twin's room with a box in it, evaluated at shift + scale * 3 * (p / size) per axis;
# world: the integrated filling -- the synthetic stream's frames, the volume placed in its world by a rotation and an origin;
# poses: three raycasts per filling (outside looking in, inside, along +x), in the volume's metres.
BRICK_CASES = {
    # 41 bricks a row: the rows whose first bit is bit 24..31 of a word take their last bricks from a third word
    "328x40x44": dict(
        dims=(328, 40, 44), size=(3.0, 1.08, 1.18), omp=False, full=True,
        scene=dict(scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.5)),
        world=dict(rot=CYC, origin=(0.7, 1.2, 0.0), frames=(0, 10, 20)),
        poses=dict(upload=[look((1.5, 0.54, -0.4), (1.5, 0.54, 1.0), (0, 1, 0)), look((0.6, 0.4, 0.2), (2.4, 0.7, 0.7)), along_x((0.5, 0.54, 0.4))],
                   integrate=[look((2.2, -0.25, 0.59), (2.8, 0.45, 0.59)), look((2.1, 0.5, 0.6), (2.8, 0.6, 0.5)), along_x((1.0, 0.54, 0.59))])),
    # exactly 64 bricks a row: the mask is used untrimmed, brick 63 is its top bit
    "512x64x52": dict(
        dims=(512, 64, 52), size=(3.0, 1.1, 0.9), omp=False, full=True,
        scene=dict(scale=(1.0, 1.0, 1.0), shift=(-0.28, 0.0, 0.5)),
        world=dict(rot=CYC, origin=(0.7, 1.3, -0.17), frames=(0, 10, 20)),
        poses=dict(upload=[look((1.5, 0.55, -0.4), (1.5, 0.55, 1.0), (0, 1, 0)), look((0.9, 0.4, 0.2), (2.6, 0.7, 0.5)), along_x((0.8, 0.55, 0.3))],
                   integrate=[look((2.4, -0.3, 0.45), (2.97, 0.5, 0.45)), look((2.2, 0.5, 0.45), (2.97, 0.6, 0.4)), along_x((1.2, 0.55, 0.45))])),
    # 66 bricks a row: no row mask, every segment is swept
    "528x16x20": dict(
        dims=(528, 16, 20), size=(3.0, 0.27, 0.34), omp=False, full=True,
        scene=dict(scale=(1.0, 1.0, 1.0), shift=(-0.25, 0.0, 0.5)),
        world=dict(rot=EYE, origin=(-0.15, 0.9, 2.6), frames=(0, 10, 20)),
        poses=dict(upload=[look((1.5, 0.135, -0.3), (1.5, 0.135, 0.3), (0, 1, 0)), look((1.0, 0.1, 0.05), (1.5, 0.16, 0.2)), along_x((0.9, 0.135, 0.12))],
                   integrate=[look((1.5, 0.135, -0.6), (1.5, 0.135, 0.2), (0, 1, 0)), look((1.0, 0.135, 0.03), (1.6, 0.135, 0.2)), along_x((0.4, 0.135, 0.16))])),
    # 1156 words: the march stages more than four quads a lane, the super-brick words start behind word 1024
    "264x264x264": dict(
        dims=(264, 264, 264), size=(3.0, 3.0, 3.0), omp=True, full=False,
        scene=dict(scale=(1.0, 1.0, 0.7653), shift=(0.0, 0.0, 0.5148)),
        world=dict(rot=EYE, origin=(0.0, 0.0, 0.0), frames=(0, 10)),
        poses=dict(upload=[look((1.5, 1.5, -0.4), (1.5, 1.5, 1.5), (0, 1, 0)), look((0.6, 1.6, 0.5), (2.4, 1.4, 2.6), (0, 1, 0)), along_x((0.5, 1.5, 1.5))],
                   integrate=[look((1.5, 1.5, -0.3), (1.5, 1.5, 1.5), (0, 1, 0)), look((1.2, 1.2, 1.0), (2.0, 2.2, 2.8), (0, 1, 0)), along_x((0.5, 1.9, 1.8))])),
    # 1089 super-bricks: more than the 1024 super bits, so no super bit is written and the march never crosses wave-wide
    "1048x1048x12": dict(
        dims=(1048, 1048, 12), size=(3.0, 3.0, 0.103), omp=True, full=False,
        scene=dict(scale=(1.0, 1.0, 0.1), shift=(0.0, -0.3, 2.5)),
        world=dict(rot=EYE, origin=(0.0, -0.2, 2.75), frames=(0, 10)),
        poses=dict(upload=[look((1.5, 1.6, -0.5), (1.5, 1.6, 0.05), (0, 1, 0)), look((1.0, 1.2, 0.01), (1.6, 1.5, 0.0515), (0, 0, 1)), along_x((1.0, 2.0, 0.02))],
                   integrate=[look((1.4, 1.4, -0.5), (1.4, 1.4, 0.05), (0, 1, 0)), look((0.9, 1.0, 0.01), (1.5, 1.3, 0.05), (0, 0, 1)), along_x((0.6, 1.3, 0.02))])),
}


def scene_fill(dims, size, scale, shift):
    """align_twin.scene_volume's quantisation of align_twin's scene, stretched and shifted per axis, a few planes at a time"""
    X, Y, Z = dims
    ax = [shift[k] + scale[k] * 3.0 * (np.arange(dims[k]) + 0.5) / dims[k] for k in range(3)]
    vol = np.zeros((Z, Y, X, 2), np.int16)
    step = max(1, 1500000 // (X * Y))
    for z0 in range(0, Z, step):
        zz, yy, xx = np.meshgrid(ax[2][z0:z0 + step], ax[1], ax[0], indexing="ij")
        d = AT.scene_distance(np.stack([xx, yy, zz], -1))
        seen = d > -TAU_SCENE
        vol[z0:z0 + step, ..., 0] = np.where(seen, np.trunc(np.clip(d / TAU_SCENE, -1.0, 1.0) * 32767.0), 0).astype(np.int16)
        vol[z0:z0 + step, ..., 1] = seen
    return vol


# ---- the volumes of the image kernels' shape tests ---------------------------------------------------------------------------------
# color: "all" -- every colour mode is rendered; "one" -- one colour mode; None -- geometry only (no colour volume is made).
# side: the longest image side of the section cameras; e_axis: the axis the (e) cameras look along (default y); a_need: the top-down
# camera's condition (default "shares"); doll: the dollhouse camera's place, from the centre, in units of the longest side.  The
# brick shapes keep the sizes, scales and shifts of BRICK_CASES.
# 136 x 72 x 46: three cells (22.1, 23.6, 23.9 mm); x spans three 64-voxel rows, the last an eighth full; 46 planes: the last plane
# group is half padding.  Its filling puts the far x wall's surface at voxel 132 and the far z wall's at voxel 42.4, so that the last
# row of x and the last plane group hold negative voxels (the negative band is 0.1 scene units: 4.5 voxels of x, 3.1 of z), and leaves
# the z = 0 face open to the room, as the brick shapes do.
VOLUMES = {
    "136x72x46": dict(dims=(136, 72, 46), size=(3.0, 1.7, 1.1), scene=dict(scale=(1.0, 1.0, 0.5), shift=(-0.2118, 0.0, 1.2674)),
                      color="all", side=200, seed=46,
                      views=[look((1.5, 0.85, -3.0), (1.5, 0.85, 0.8), (0, 1, 0)), look((0.7, 0.6, 0.15), (2.5, 1.1, 0.9))]),
    "328x40x44": dict(color="all", side=200, seed=44),
    "512x64x52": dict(color="all", side=200, seed=52),
    "528x16x20": dict(color=None, side=200, seed=20, e_axis=2, a_need="cut", doll=(0.0, -0.3, -1.0)),
    "264x264x264": dict(color="one", side=160, seed=264),
    "1048x1048x12": dict(color=None, side=128, seed=12),
}
# views: (g)'s two poses, from outside looking in and from inside -- the brick tests' own where the picture they give holds 2 %
# of background, else the same camera further back (outside) or turned towards the open z = 0 face (inside)
for _name, _v in VOLUMES.items():
    if _name in BRICK_CASES:
        _v.update(dims=BRICK_CASES[_name]["dims"], size=BRICK_CASES[_name]["size"], scene=BRICK_CASES[_name]["scene"],
                  views=BRICK_CASES[_name]["poses"]["upload"][:2])
VOLUMES["512x64x52"]["views"] = [look((1.5, 0.55, -1.2), (1.5, 0.55, 1.0), (0, 1, 0)), VOLUMES["512x64x52"]["views"][1]]
VOLUMES["264x264x264"]["views"] = [look((1.5, 1.5, -2.2), (1.5, 1.5, 1.5), (0, 1, 0)), look((1.6, 1.5, 1.2), (0.5, 1.3, -0.6), (0, 1, 0))]
VOLUMES["1048x1048x12"]["views"] = [look((1.5, 1.6, -3.2), (1.5, 1.6, 0.05), (0, 1, 0)), None]

SMALL_BRICKS = ("328x40x44", "512x64x52", "528x16x20", "264x264x264")

_FILLED = {}


def volume(name):
    """(tsdf [Z, Y, X, 2] int16, colour [Z, Y, X, 4] uint8 or None) of a volume, made once, read-only"""
    if name not in _FILLED:
        v = VOLUMES[name]
        X, Y, Z = v["dims"]
        vol = scene_fill(v["dims"], v["size"], **v["scene"])
        vol.setflags(write=False)
        col = None
        if v["color"]:
            rng = np.random.default_rng(v["seed"])
            col = rng.integers(0, 256, size=(Z, Y, X, 4), dtype=np.uint8)
            col[..., 3] = rng.integers(1, 256, size=(Z, Y, X))
            col[..., 3][rng.random((Z, Y, X), dtype=np.float32) < 0.45] = 0
            col[Z // 3, :, :, 3] = 0
            col.setflags(write=False)
        _FILLED[name] = (vol, col)
    return _FILLED[name]


def cells(name):
    v = VOLUMES[name]
    return [v["size"][k] / v["dims"][k] for k in range(3)]


def wall_voxel(name, axis):
    """where the room's far wall along `axis` has its surface, in voxels of that axis (the room's box ends at AT.ROOM[1])"""
    v = VOLUMES[name]
    return (AT.ROOM[1][axis] - v["scene"]["shift"][axis]) / (3.0 * v["scene"]["scale"][axis]) * v["dims"][axis]


def march_step(name):
    """the march's step in metres: 0.8 of the effective truncation distance"""
    v = VOLUMES[name]
    return 0.8 * float(tau_of(v["size"], v["dims"], TRUNC))


def before_wall(name, axis, steps):
    """a coordinate (metres) in free space before the room's far wall along `axis`, such that a march that starts there along
    +axis puts its sample number `steps` on the centre of the first voxel behind the wall's surface.  (The scene's negative band is
    0.1 scene units -- in the thin shapes one voxel or less -- and the march decides by the voxels that hold its samples: a start
    chosen without regard to the step can walk over the band.)"""
    w = wall_voxel(name, axis)
    centre = np.floor(w) + 0.5
    if centre <= w:
        centre += 1.0
    return centre * cells(name)[axis] - steps * march_step(name)


def last_row_start(name):
    """the first voxel of the last 64-voxel row of x"""
    return 64 * ((VOLUMES[name]["dims"][0] - 1) // 64)


def last_group_start(name):
    """the first plane of the last plane group: the padded one where Z is no multiple of 4"""
    Z = VOLUMES[name]["dims"][2]
    return 4 * (Z // 4) if Z % 4 else Z - 4


# ---- cameras -----------------------------------------------------------------------------------------------------------------------
MARGIN = 1.15


def ortho_fit(name, axis, long_side, wh=None, margin=MARGIN):
    """an orthographic camera outside the volume, looking exactly along +axis at the volume's box, the image `margin` times the box
    in both directions: its longer side `long_side` pixels and the pixels square to within the rounding of its sides, or, with
    wh = (W, H), that size and the pixels as they come"""
    sz = VOLUMES[name]["size"]
    mid = [0.5 * s for s in sz]
    eye, at = list(mid), list(mid)
    eye[axis], at[axis] = -0.5, 1.0
    pose = look(eye, at, {0: (0, 0, 1), 1: (0, 0, 1), 2: (0, 1, 0)}[axis])
    R = pose[:3, :3]
    su = sum(abs(float(R[k, 0])) * sz[k] for k in range(3)) * margin      # the box's extent along the image's u and v
    sv = sum(abs(float(R[k, 1])) * sz[k] for k in range(3)) * margin
    if wh is None:
        ppm = long_side / max(su, sv)
        wh = max(8, int(round(su * ppm))), max(8, int(round(sv * ppm)))
    W, H = wh
    return dict(width=W, height=H, fx=W / su, fy=H / sv, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0, pose=pose, projection=ST.ORTHO)


def pinhole_fit(name, eye, W, H, down, y_from, margin=1.08):
    """a pinhole camera at `eye` looking at the volume's centre, its intrinsics chosen so that the corners of the box's part
    with y >= y_from (what a plane leaves of it) fill the image"""
    sz = VOLUMES[name]["size"]
    pose = look(eye, [0.5 * s for s in sz], down)
    R, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    corners = np.array([[x, y, z] for x in (0, sz[0]) for y in (y_from, sz[1]) for z in (0, sz[2])], np.float64)
    c = (corners - t) @ R
    assert (c[:, 2] > 0.1).all(), "the dollhouse camera must stand clear of the box"
    u, v = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
    fx, fy = W / (margin * (u.max() - u.min())), H / (margin * (v.max() - v.min()))
    return dict(width=W, height=H, fx=fx, fy=fy, cx=(W - 1) / 2.0 - fx * 0.5 * (u.max() + u.min()),
                cy=(H - 1) / 2.0 - fy * 0.5 * (v.max() + v.min()), pose=pose, projection=ST.PINHOLE)


def faces_cam(name):
    """(f): top-down, the pixel pitch exactly half a cell of x along u and half a cell of z along v, the camera's centre on a voxel
    corner and cx, cy whole numbers: every second ray lies on a voxel face of x and of z, to within rounding.  At most 333 x 217:
    where that does not span the volume's x, the image is placed over the far x wall"""
    v = VOLUMES[name]
    X, Y, Z = v["dims"]
    sz = v["size"]
    W, H = min(333, 2 * X + 16), min(217, 2 * Z + 16)
    kx = X // 2 if W == 2 * X + 16 else int(round(wall_voxel(name, 0))) - 60
    kz = Z // 2
    pose = look((kx * sz[0] / X, -0.5, kz * sz[2] / Z), (kx * sz[0] / X, 1.0, kz * sz[2] / Z), (0, 0, 1))
    return dict(width=W, height=H, fx=2.0 * X / sz[0], fy=2.0 * Z / sz[2], cx=float(W // 2), cy=float(H // 2), pose=pose,
                projection=ST.ORTHO)


SHARES = (0.20, 0.02, 0.02)    # (hit, cut, background) of the twin's image, cameras (a)-(d)


def cameras(name):
    """name -> dict(fields: section_twin.section's, need: "shares" | "both" | "cut", kind: "a".."f" or "b-last")
    need "shares": hit >= 0.20, cut >= 0.02, background >= 0.02 of the twin's image; "both": n_hit > 0 and n_cut > 0;
    "cut": n_cut > 0 (the plane inside the last plane group, behind which nothing can be hit, and 528 x 16 x 20 from above, whose
    floor no ray along +y finds: tests/test_view_shapes_host.py asserts both facts)"""
    v = VOLUMES[name]
    X, Y, Z = v["dims"]
    sx, sy, sz = v["size"]
    cl = cells(name)
    side = v["side"]
    colour = v["color"] == "all"
    lit, flat = (VT.COLOR_LIT, VT.COLOR) if colour else (VT.LAMBERT, VT.NORMALS)
    sun = dict(light=(0.3, -1.0, 0.2), light_in_camera=False, light_directional=True)
    head = dict(light=(0.1, 0.2, -1.0), light_in_camera=True, light_directional=True)
    lamp = dict(light=(0.5 * sx, 0.3 * sy, 0.4 * sz), light_in_camera=False, light_directional=False)
    torch = dict(light=(0.0, 0.0, 0.0), light_in_camera=True, light_directional=False)
    zb = before_wall(name, 2, 2)                                           # free space, two march steps before the far z wall
    xc = before_wall(name, 0, 2)                                           # ... before the far x wall:
    wx = wall_voxel(name, 0)
    if wx >= last_row_start(name) and xc / cl[0] < max(last_row_start(name), 8 * int(wx // 8)):
        xc = before_wall(name, 0, 1)                                       # inside the last row of x, and inside the wall's own brick
    yb = before_wall(name, 1, 3)
    e_axis = v.get("e_axis", 1)
    along_z = ortho_fit(name, 2, side, wh=(333, 217) if name == "136x72x46" else None)
    if name == "1048x1048x12":   # one orthographic section
        return {"along z": dict(fields=dict(along_z, clip=[(0, 0, 1, -zb)], mode=VT.LAMBERT, **sun), need="shares", kind="b")}
    top = ortho_fit(name, 1, side)
    far = max(sx, sy, sz)
    doll = v.get("doll", (-0.2, -1.2, -0.4))                               # from above, through the plane that takes the ceiling off
    box = top if e_axis == 1 else along_z
    first = (0, 1, 0, -0.5 * sy) if e_axis == 1 else (0, 0, 1, -zb)
    four = [(0, 1, 0, -yb), (1, 0, 0, -0.3 * sx), (-1, 0, 0, 0.96 * sx), (0, 0, 1, -0.2 * sz)] if e_axis == 1 else \
        [(0, 0, 1, -zb), (1, 0, 0, -0.1 * sx), (-1, 0, 0, 0.96 * sx), (0, 1, 0, -0.05 * sy)]
    cams = {
        "top-down": dict(fields=dict(top, clip=[(0, 1, 0, -0.5 * sy)], mode=VT.COLOR_LIT if v["color"] else VT.LAMBERT, **sun,
                                     background=(20, 30, 40)), need=v.get("a_need", "shares"), kind="a"),
        "along z": dict(fields=dict(along_z, clip=[(0, 0, 1, -zb)], mode=VT.LAMBERT, **head), need="shares", kind="b"),
        "along x": dict(fields=dict(ortho_fit(name, 0, side), clip=[(1, 0, 0, -xc)], mode=flat, cut_rgb=(1, 2, 3)),
                        need="shares", kind="c"),
        "dollhouse": dict(fields=dict(pinhole_fit(name, [0.5 * v["size"][k] + far * doll[k] for k in range(3)], side, (3 * side) // 4 + 1,
                                                  (0, 0, 1) if abs(doll[1]) > abs(doll[2]) else (0, 1, 0), 0.4 * sy),
                                      clip=[(0, 1, 0, -0.4 * sy)], mode=lit, **torch), need="shares", kind="d"),
        "two planes": dict(fields=dict(box, clip=[first, (1, 0, 0, -0.5 * sx)], mode=VT.LAMBERT, **lamp), need="both", kind="e"),
        "box of four": dict(fields=dict(box, clip=four, mode=VT.NORMALS, background=(255, 255, 255)), need="both", kind="e"),
    }
    if name == "136x72x46":      # the one shape whose last plane group is padded, filled so that the group holds negative voxels
        zl = (last_group_start(name) + 0.5) * cl[2]
        cams["along z, last group"] = dict(fields=dict(along_z, clip=[(0, 0, 1, -zl)], mode=VT.NORMALS, cut_rgb=(9, 8, 7)), need="cut", kind="b-last")
    if name in ("136x72x46", "328x40x44"):
        cams["on the faces"] = dict(fields=dict(faces_cam(name), clip=[(0, 1, 0, -0.5 * sy)], mode=VT.COLOR, background=(0, 0, 64)),
                                    need="both", kind="f")
    return cams


def view_cameras(name):
    """(g): [(what, camera, pose)] -- from outside looking in and from inside"""
    outside, inside = VOLUMES[name]["views"]
    if name == "1048x1048x12":   # one pinhole view, at most 128 x 128
        return [("outside, 128x120", dict(width=128, height=120, fx=100.0, fy=100.0, cx=63.5, cy=59.5), outside)]
    return [("outside, 333x217", RAGGED, outside), ("inside, 240x200", ODD, inside)]


_REF = {}


def reference(name, cam):
    """section_twin.render of a named camera, computed once -> (section, its image)"""
    if (name, cam) not in _REF:
        vol, col = volume(name)
        sec = ST.section(**cameras(name)[cam]["fields"])
        _REF[name, cam] = (sec, ST.render(vol, VOLUMES[name]["size"], TRUNC, sec, color=col))
    return _REF[name, cam]


def shares(ref):
    return tuple(float((ref["cls"] == c).mean()) for c in (ST.HIT, ST.CUT, ST.BACKGROUND))


def start_points(name, sec):
    """steps 1-3 of a section: the rays' origins o, and per pixel the voxel that step 6 gathers (where the ray starts, clamped
    into the grid) and whether the ray marches"""
    v = VOLUMES[name]
    o, d = ST.rays(sec)
    t_box, t_exit = ST.box(o, d, v["size"])
    t_start, t_exit, alive = ST.clip_rays(o, d, t_box, t_exit, sec["clip"])
    with np.errstate(all="ignore"):
        marching = alive & (t_start < t_exit)
    ts = np.where(marching & (t_start > t_box), t_start, f32(0)).astype(f32)
    cl = [f32(v["size"][k]) / f32(v["dims"][k]) for k in range(3)]
    vox = [np.clip(np.floor(((o[k] + d[k] * ts).astype(f32) / cl[k]).astype(f32)), 0, v["dims"][k] - 1).astype(np.int64) for k in range(3)]
    return o, vox, marching


def hit_voxels(name, ref):
    """the voxels (x, y, z) that hold the hit pixels' vertices"""
    v = VOLUMES[name]
    hit = ref["cls"] == ST.HIT
    cl = [f32(v["size"][k]) / f32(v["dims"][k]) for k in range(3)]
    return [np.clip(np.floor(ref["vmap"][k][hit] / cl[k]), 0, v["dims"][k] - 1).astype(np.int64) for k in range(3)]


def check_conditions(name, cam, ref):
    """the condition of a named camera on the twin's own image -- before any comparison with the device counts"""
    c = cameras(name)[cam]
    sh = shares(ref)
    if c["need"] == "shares":
        assert all(s >= m for s, m in zip(sh, SHARES)), f"{name} {cam}: shares (hit, cut, background) {sh} below {SHARES}"
    elif c["need"] == "both":
        assert ref["n_hit"] > 0 and ref["n_cut"] > 0, f"{name} {cam}: {ref['n_hit']} hits, {ref['n_cut']} cut pixels"
    else:
        assert ref["n_cut"] > 0, f"{name} {cam}: no cut pixel"
    if c["fields"]["mode"] in (VT.COLOR, VT.COLOR_LIT):
        colored = ref["n_hit"] - ref["n_uncolored"]
        assert ref["n_uncolored"] >= 500 and colored >= 500, f"{name} {cam}: {ref['n_uncolored']} uncoloured and {colored} coloured hits"
    return sh


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def assert_section(got, ref, what):
    """every pixel of every output and the three counts, zero differences"""
    for key in ("n_hit", "n_cut", "n_uncolored"):
        assert got[key] == ref[key], f"{what}: {key} {got[key]} != {ref[key]}"
    assert same_bits_nan(got["vmap"], ref["vmap"]), f"{what}: vmap ({(np.isnan(got['vmap'][0]) != np.isnan(ref['vmap'][0])).sum()} hit pixels differ)"
    assert same_bits_nan(got["nmap"], ref["nmap"]), f"{what}: nmap"
    bad = np.argwhere(got["depth"] != ref["depth"])
    assert len(bad) == 0, f"{what}: {len(bad)} depth pixels differ, first {bad[:4].tolist()}"
    bad = np.argwhere((got["rgb"] != ref["rgb"]).any(axis=2))
    assert len(bad) == 0, (f"{what}: {len(bad)} rgb pixels differ, first {bad[:4].tolist()}: "
                           f"{got['rgb'][tuple(bad[0])].tolist()} != {ref['rgb'][tuple(bad[0])].tolist()}")


def assert_view(got, vm, nm, ref, what):
    """every pixel of every output, zero differences"""
    assert got["n_hit"] == ref["n_hit"], f"{what}: n_hit {got['n_hit']} != {ref['n_hit']}"
    assert got["n_uncolored"] == ref["n_uncolored"], f"{what}: n_uncolored {got['n_uncolored']} != {ref['n_uncolored']}"
    if "vmap" in got:
        assert same_bits_nan(got["vmap"], vm), f"{what}: vmap"
    if "nmap" in got:
        assert same_bits_nan(got["nmap"], nm), f"{what}: nmap"
    bad = np.argwhere(got["depth"] != ref["depth"])
    assert len(bad) == 0, f"{what}: {len(bad)} depth pixels differ, first {bad[:4].tolist()}"
    bad = np.argwhere((got["rgb"] != ref["rgb"]).any(axis=2))
    assert len(bad) == 0, (f"{what}: {len(bad)} rgb pixels differ, first {bad[:4].tolist()}: "
                           f"{got['rgb'][tuple(bad[0])].tolist()} != {ref['rgb'][tuple(bad[0])].tolist()}")


def check_camera(trk, oracle, dims, tsdf, color, cam, pose, what, degenerate=False, modes=MODES, size=(3.0, 3.0, 3.0), uncolored="share"):
    """one camera: the geometry once (with the first mode), then every mode with the light in camera and in world coordinates.
    uncolored: the condition on a colour mode's reference -- "share": at most 5 % of the hits without colour (a scanned volume);
    "both": at least 500 hits without and at least 500 with colour (a random colour volume)"""
    cfg = VT.view_config(oracle, dims, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], size=size)
    vm, nm = VT.geometry(oracle, cfg, tsdf, pose)
    hit = ~np.isnan(vm[0])
    if not degenerate:   # the condition on the inputs: a test cannot pass on an empty (or a full) picture
        assert hit.mean() >= 0.20, f"{what}: the reference has only {hit.mean():.3f} hit pixels"
        assert (~hit).mean() >= 0.02, f"{what}: the reference has only {(~hit).mean():.3f} background pixels"
    first = True
    for mode in modes:
        if mode in (VT.COLOR, VT.COLOR_LIT) and color is None:
            continue
        for light, in_cam in (((0.1, -0.2, 0.05), True), ((1.4, 0.3, 0.2), False)):
            bg = (10 + mode, 200, 33)
            ref = VT.shade(vm, nm, pose, mode, light, in_cam, bg, color=color, size=size)
            if mode in (VT.COLOR, VT.COLOR_LIT) and not degenerate:
                if uncolored == "share":
                    assert ref["n_uncolored"] <= 0.05 * ref["n_hit"], f"{what}: {ref['n_uncolored']} of {ref['n_hit']} hits uncoloured"
                else:
                    assert ref["n_uncolored"] >= 500 and ref["n_hit"] - ref["n_uncolored"] >= 500, \
                        f"{what}: {ref['n_uncolored']} uncoloured and {ref['n_hit'] - ref['n_uncolored']} coloured hits"
            got = trk.render_view(pose=pose, mode=mode, light=light, light_in_camera=int(in_cam), background=bg, vmap=first,
                                  nmap=first, **cam)
            assert_view(got, vm, nm, ref, f"{what} mode {mode} light_in_camera {in_cam}")
            first = False
            if mode in (VT.NORMALS, VT.COLOR):
                break   # (no light in these modes)
    return hit
