"""The cases of the colour path's shape tests, shared by the host tests (tests/test_color_twin_host.py) and the GPU tests
(tests/test_gpu_color_shapes.py): volumes, cameras and the fuzz's frames -- the integrate's fuzz recipe
(tests/test_gpu_parity.py) for any image size, with a colour image of independent random bytes."""
import numpy as np

from parity_cases import _lookat_pose, _random_pose

TRUNC = 0.03
# (X, Y, Z) voxels over metres
VOLUMES = {
    "cube": ((64, 64, 64), (3.0, 3.0, 3.0)),       # the control
    "ragged": ((72, 40, 50), (2.7, 1.8, 1.5)),     # cells 37.5 / 45 / 30 mm; no axis a multiple of a chunk's 16
    "flat": ((64, 160, 24), (1.6, 3.2, 0.9)),      # one and a half chunk layers
}
# (W, H, fx, fy, cx, cy)
CAMERAS = {
    "vga": (640, 480, 525.0, 525.0, 319.5, 239.5),
    "small": (68, 52, 58.0, 54.1, 36.75, 23.0),    # 5 x 4 tiles of 16 px, the last column and row clipped; off-centre
}
SEEDS = (1, 2, 3)
# (max_w, band_m): the default band; a band thinner than a cell; a band capped at tau.  A seed starts with its own and takes the
# next with every frame (hsk_enable_color again, between frames): a band of 4 mm alone colours some 80 voxels a frame at
# these sizes, too few to say that a seed's frames exercised the sweep
COLOR_PARAMS = ((64, 0.0), (1, 0.004), (255, 1.0))


def tracker_config(hsk, dims, size, cam, **over):
    W, H, fx, fy, cx, cy = cam
    return hsk.default_config(dims[0], vol_x=dims[0], vol_y=dims[1], vol_z=dims[2], own_z1=dims[2], vol_size_m=size, width=W, height=H,
                              fx=fx, fy=fy, cx=cx, cy=cy, **over)


def random_depth(rng, h, w):
    """blocky random depth in millimetres: patches of 1..48 px with independent values of 300..2500 mm (surfaces inside these
    volumes), holes -- one rectangular, an eighth of the image each way --, per-pixel noise on half the pixels, and a few
    extreme values (1 mm, 65535 mm)"""
    by, bx = int(rng.integers(1, 49)), int(rng.integers(1, 49))
    coarse = rng.integers(300, 2500, size=(h // by + 2, w // bx + 2))
    d = np.kron(coarse, np.ones((by, bx), np.int64))[:h, :w]
    d = d + rng.integers(-20, 21, size=(h, w)) * (rng.random((h, w)) < 0.5)
    d[rng.random((h, w)) < 0.1] = 0
    hh, hw = h // 8, w // 8
    hy, hx = rng.integers(0, h - hh), rng.integers(0, w - hw)
    d[hy:hy + hh, hx:hx + hw] = 0
    ex = rng.random((h, w))
    d[ex < 0.001] = 1
    d[ex > 0.999] = 65535
    return np.clip(d, 0, 65535).astype(np.uint16)


def random_color(rng, dims, max_w):
    """a colour volume [Z, Y, X, 4] of random bytes with weights 0 .. max_w, a tenth of them already capped"""
    shape = (dims[2], dims[1], dims[0])
    col = rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)
    col[..., 3] = rng.integers(0, max_w + 1, size=shape)
    col[..., 3][rng.random(shape) < 0.1] = max_w
    return col


def fuzz_case(volume, camera, seed, frames=8):
    """-> (rng, dims, size, cam, max_w0, [(pose, depth, rgb, max_w, band_m)]): poses alternately anywhere and looking at the
    middle, within 0.4 and 0.9 of the extent of the volume's centre (inside and outside); max_w0 is the first frame's, for
    the weights of the volume the run starts from"""
    dims, size = VOLUMES[volume]
    cam = CAMERAS[camera]
    W, H = cam[:2]
    rng = np.random.default_rng([seed, sorted(VOLUMES).index(volume), sorted(CAMERAS).index(camera)])
    ext = np.array(size)
    out = []
    for k in range(frames):
        pose = (_lookat_pose if k % 2 else _random_pose)(rng, ext / 2, ext * (0.9 if k % 4 >= 2 else 0.4))
        out.append((pose, random_depth(rng, H, W), rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)) + COLOR_PARAMS[(seed + k) % 3])
    return rng, dims, size, cam, COLOR_PARAMS[seed % 3][0], out


def inside(pose, size):
    t = pose[:3, 3]
    return bool(all(0.0 < t[i] < size[i] for i in range(3)))


def frame_of(hsk, src, k):
    """(pose, depth, rgb) of frame k of the scripted stream ("synth") or of room 0's scan ("room")"""
    if src == "synth":
        pose = hsk.synth_pose(k)
        return pose, hsk.synth_depth(pose), hsk.synth_rgb(pose)
    pose = hsk.synth_room_pose(0, k, 720)
    return pose, hsk.synth_room_depth(0, pose), hsk.synth_rgb(pose, 0)


def run_tracker(hsk, n, frames, color=True, use_graph=0, mode="sync", profile=False):
    trk = hsk.KinfuTracker(n=n, use_graph=use_graph)
    if color:
        trk.enable_color()
    if profile:
        trk.set_profiling(1)
    out = []
    if mode == "sync":
        for pose, depth, rgb in frames:
            out.append(trk.process_frame_rgbd(depth, rgb) if color else trk.process_frame(depth))
    else:
        for i, (pose, depth, rgb) in enumerate(frames):
            trk.submit_frame_rgbd(depth, rgb) if color else trk.submit_frame(depth)
            if i >= 2:
                out.append(trk.wait_frame())
        while len(out) < len(frames):
            out.append(trk.wait_frame())
    return trk, out


def read_pcd_xyzrgbnormal(path):
    """numpy parse of the binary PCD: header lines, then 32-B records -> (header dict, xyz, rgb bits, normals, curvature)"""
    raw = open(path, "rb").read()
    head, pos = {}, 0
    while True:
        end = raw.index(b"\n", pos)
        line = raw[pos:end].decode()
        pos = end + 1
        if line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        head[key] = val
        if key == "DATA":
            break
    n = int(head["POINTS"])
    rec = np.frombuffer(raw[pos:], dtype=np.uint32)
    assert rec.size == 8 * n, (rec.size, n)
    rec = rec.reshape(n, 8)
    xyz = rec[:, 0:3].copy().view(np.float32)
    nrm = rec[:, 4:7].copy().view(np.float32)
    return head, xyz, rec[:, 3].copy(), nrm, rec[:, 7].copy().view(np.float32)
