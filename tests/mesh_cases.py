"""The mesh tests' volumes (a sphere, random signs, planted zeros) and the reader of the indexed PLY files."""
import numpy as np

f32 = np.float32


def sphere_volume(n, size, centre, radius, tau, observed=None):
    """int16 (tsdf, weight) pairs of a solid sphere: negative inside, weight 1 where `observed`"""
    cell = size / n
    g = (np.arange(n) + 0.5) * cell
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    f = np.clip(d / tau, -1, 1)
    vol = np.zeros((n, n, n, 2), np.int16)
    vol[..., 0] = np.rint(f * 32767).astype(np.int16)
    vol[..., 1] = 1 if observed is None else observed.astype(np.int16)
    return vol


def random_sign_volume(n, seed=11):
    """test_mesh's volume of random signs and weights in which every one of the 256 cases occurs (no exact zeros)"""
    rng = np.random.default_rng(seed)
    noise = np.zeros((n, n, n, 2), np.int16)
    noise[..., 0] = rng.integers(1, 32767, (n, n, n)) * rng.choice([-1, 1], (n, n, n))
    noise[..., 1] = (rng.random((n, n, n)) > 0.02) * rng.integers(1, 100, (n, n, n))
    return noise


def planted_zeros_volume(n, seed=5):
    """a sphere with exact zeros, 32767s and zero weights planted on and near its surface"""
    rng = np.random.default_rng(seed)
    v = sphere_volume(n, 3.0, np.array([1.45, 1.52, 1.57]), 0.8, 0.15)
    near = np.argwhere(np.abs(v[..., 0]) < 6000)
    for val, cnt in ((0, 400), (32767, 100)):
        pick = near[rng.choice(len(near), cnt, replace=False)]
        v[pick[:, 0], pick[:, 1], pick[:, 2], 0] = val
    pick = near[rng.choice(len(near), 60, replace=False)]
    v[pick[:, 0], pick[:, 1], pick[:, 2], 1] = 0
    return v


def read_ply_indexed(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[2])
    props = [l.split()[2] for l in lines if l.startswith("property ") and not l.startswith("property list")]
    dt = np.dtype([(p, "<f4" if p in ("x", "y", "z", "nx", "ny", "nz") else "u1") for p in props])
    rec = np.frombuffer(body[:nv * dt.itemsize], dt)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    fr = np.frombuffer(body[nv * dt.itemsize:], fdt)
    assert len(fr) == nf and (fr["n"] == 3).all()
    v = np.stack([rec["x"], rec["y"], rec["z"]], axis=1) if nv else np.zeros((0, 3), f32)
    n = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1) if "nx" in props else None
    c = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1) if "red" in props else None
    return head + b"end_header\n", v, fr["i"].astype(np.int32), n, c
