"""The volumes the split tests share (tests/test_split_host.py on the host, tests/test_gpu_split.py on the device), each with its
planes, the parameters it is split with and the removals made of it, and the twin's result of each, computed once."""
import numpy as np

import diff_twin as DT
import split_twin as ST
from diff_cases import sl
from fill_cases import RANDOM_DIMS, random_volume

FIELDS = ("root", "n_voxels", "sum", "lo", "hi", "contact", "plane_mask", "height_lo", "height_hi")


def records_as_dicts(recs):
    return [{n: (int(c[n]) if np.ndim(c[n]) == 0 else tuple(int(v) for v in c[n])) for n in FIELDS} for c in recs]


_CACHE = {}
CELL = 0.05                       # the hand-built grids' cell; the truncation distance is then 2.1 cells
RANDOM_CELL = 0.0375
RANDOM_PLANES = (0, 1, 7, 64)
ANISO_DIMS = (72, 56, 40)
ANISO_SIZE = (2.7, 2.8, 1.6)      # cells 0.0375, 0.05, 0.04: w = 4096, 3072, 3840
SHAPE_DIMS = (32, 24, 20)         # 20 planes: a plane group of its own for the last four
ALL = None


def size_of(dims, cell=CELL):
    return tuple(cell * d for d in dims)


def lin_of(c, dims):
    return (c["root"][2] * dims[1] + c["root"][1]) * dims[0] + c["root"][0]


def random_planes(n, size, seed):
    """n planes through points inside the volume: unit normals, a few scaled to a length of 0.5 .. 2; every kind"""
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= np.where(rng.random(n) < 0.25, rng.uniform(0.55, 1.9, n), 1.0)[:, None]
    pts = rng.uniform(0.1, 0.9, (n, 3)) * np.asarray(size)
    abcd = np.concatenate([nrm, -(nrm * pts).sum(axis=1, keepdims=True)], axis=1).astype(np.float32)
    return abcd, rng.integers(1, 5, n).astype(np.int32)


def make_case(vol, size, abcd, kinds, params=None, removes=(), color=False, box=None):
    dims = (vol.shape[2], vol.shape[1], vol.shape[0])
    p = ST.default_params(size, dims)
    p.update(params or {})
    return dict(vol=vol, size=size, dims=dims, abcd=np.asarray(abcd, np.float32).reshape(-1, 4), kinds=np.asarray(kinds, np.int32).reshape(-1), params=p,
                removes=list(removes), color=color, box=box)


def random_case(dims, n_planes, size=None):
    key = ("random", dims, n_planes, size)
    if key not in _CACHE:
        sz = size or size_of(dims, RANDOM_CELL)
        abcd, kinds = random_planes(n_planes, sz, 100 * dims[2] + n_planes)
        _CACHE[key] = make_case(random_volume(dims), sz, abcd, kinds, dict(min_voxels=8),
                                removes=[(ALL, ST.RESTORE, 2, 3), ("largest", ST.ERASE, 1, 1)] if n_planes in (7, 64) else [(ALL, ST.RESTORE, 1, 1)], color=n_planes == 7)
    return _CACHE[key]


def room_params(size, dims):
    tau = ST.effective_tau(size, dims)
    return dict(dist_m=np.float32(0.5 * CELL), back_m=np.float32(np.float64(tau) + 0.5 * CELL), min_voxels=64)


def room_case(name):
    """the analytic room (diff_twin.room, 64 x 48 x 40, cell 0.05) with the floor and the wall given exactly: dist 0.5 cell, back
    tau + 0.5 cell"""
    boxes = {"the empty room": None, "a box on the floor": DT.ROOM_BOX, "a box against the wall": ((36.7, 14.2, 6.3), (50.4, 30.6, 19.4)),
             "a box lifted off the floor": ((20.3, 14.2, 12.3), (33.7, 30.6, 25.4))}
    key = ("room", name)
    if key not in _CACHE:
        dims, size = DT.ROOM_DIMS, size_of(DT.ROOM_DIMS)
        abcd, kinds = ST.room_planes()
        if name == "two boxes":
            # one on the floor, one against the wall, six voxels apart: with a halo of 3 or more their grown boxes overlap, and
            # their plane masks differ
            vol = np.minimum(DT.room(((20.3, 14.2, 6.3), (30.7, 30.6, 19.4)))[..., 0], DT.room(((36.7, 14.2, 6.3), (50.4, 30.6, 15.4)))[..., 0])
            seen = DT.room(((20.3, 14.2, 6.3), (30.7, 30.6, 19.4)))[..., 1] & DT.room(((36.7, 14.2, 6.3), (50.4, 30.6, 15.4)))[..., 1]
            vol = np.stack([np.where(seen != 0, vol, 0), seen], axis=-1).astype(np.int16)
            removes = [(ALL, ST.RESTORE, 4, 1), ("largest", ST.RESTORE, 3, 2), ("second", ST.RESTORE, 8, 1), (ALL, ST.ERASE, 2, 1), (ALL, ST.RESTORE, 0, 1)]
            _CACHE[key] = make_case(vol, size, abcd, kinds, room_params(size, dims), removes, color=True)
        else:
            removes = [] if boxes[name] is None else [(ALL, ST.RESTORE, 3, 1), (ALL, ST.ERASE, 3, 1)]
            _CACHE[key] = make_case(DT.room(boxes[name]), size, abcd, kinds, room_params(size, dims), removes, box=((17, 11, 5), (37, 34, 22)))
    return _CACHE[key]


ROOM_NAMES = ("the empty room", "a box on the floor", "a box against the wall", "a box lifted off the floor", "two boxes")


def small_room():
    """the room at 32 x 24 x 20: the floor at z = 4.3, the wall at x = 26.4"""
    return DT.room(None, wall_x=26.4, floor_z=4.3, dims=SHAPE_DIMS)


def shapes():
    if "shapes" in _CACHE:
        return _CACHE["shapes"]
    out = {}
    size = size_of(SHAPE_DIMS)
    abcd, kinds = ST.room_planes(26.4, 4.3)
    base = room_params(size, SHAPE_DIMS)
    # objects painted into the small room's free space
    vol = small_room()
    for at, word in ((sl((6, 11), (14, 19), (14, 19)), (-9000, 3)),          # across the tile faces x = 16, y = 16 and z = 8
                     (sl((17, 20), (0, 3), (0, 3)), (-5000, 1)),             # in the grid's corner x = y = 0, z = Z - 1
                     (sl((10, 13), (8, 11), (20, 23)), (-32768, 2)),         # raw -32768 counts as -32767
                     (sl((14, 16), (4, 6), (5, 8)), (-700, 1)),              # exactly min_voxels = 12 ...
                     (sl((14, 16), (9, 11), (5, 8)), (-700, 1)), (sl(15, 10, 7), (900, 1))):   # ... and one less
        vol[at] = word
    for z, y, x in ((12, 5, 10), (4, 20, 8)):                                # isolated INSIDE voxels: G = 0; the second lies NEAR the floor
        vol[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2] = (0, 0)
        vol[z, y, x] = (-100, 1)
    out["objects in the small room"] = make_case(vol, size, abcd, kinds, dict(base, min_voxels=12),
                                                 [(ALL, ST.RESTORE, 2, 1), ("largest", ST.ERASE, 0, 1), (ALL, ST.RESTORE, 8, 128)], color=True)
    # everything INSIDE with random values and a plane just inside each grid face: one-sided gradients on all six faces
    rng = np.random.default_rng(5)
    Z, Y, X = SHAPE_DIMS[2], SHAPE_DIMS[1], SHAPE_DIMS[0]
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[..., 0] = rng.integers(-30000, -1000, (Z, Y, X))
    vol[..., 1] = 2
    e = 0.4 * CELL
    faces = np.array([[1, 0, 0, -e], [-1, 0, 0, size[0] - e], [0, 1, 0, -e], [0, -1, 0, size[1] - e], [0, 0, 1, -e], [0, 0, -1, size[2] - e]], np.float32)
    out["a plane inside each grid face"] = make_case(vol, size, faces, [ST.WALL, ST.WALL, ST.OTHER, ST.OTHER, ST.FLOOR, ST.CEILING], dict(base, min_voxels=1, cos_min=0.3),
                                                     [(ALL, ST.RESTORE, 1, 1)])
    # the room's planes each given twice, the copies with other kinds: of equal |s| the lower index wins; and a block whose values
    # rise along y alone at the floor-wall edge: NEAR both planes, ALIGNED with neither
    vol = small_room()
    y = np.arange(8, 16)
    vol[4:7, 8:16, 24:28, 0] = (-3000 - 2500 * (y - 8))[None, :, None]
    vol[4:7, 8:16, 24:28, 1] = 2
    out["twice the planes and a block at the edge"] = make_case(vol, size, np.concatenate([abcd, abcd]), [ST.FLOOR, ST.WALL, ST.OTHER, ST.CEILING], dict(base, min_voxels=4))
    # no plane at all: every INSIDE voxel is OBJECT
    out["no planes"] = make_case(small_room(), size, np.zeros((0, 4), np.float32), [], dict(base, min_voxels=100), [(ALL, ST.RESTORE, 2, 1)])
    _CACHE["shapes"] = out
    return out


def case_of(key):
    kind = key[0]
    return random_case(*key[1:]) if kind == "random" else (room_case(key[1]) if kind == "room" else shapes()[key[1]])


def all_keys():
    keys = [("random", dims, n) for dims in RANDOM_DIMS for n in RANDOM_PLANES] + [("random", ANISO_DIMS, 7, ANISO_SIZE)]
    return keys + [("room", n) for n in ROOM_NAMES] + [("shape", n) for n in shapes()]


def rule_of(c):
    p = c["params"]
    return ST.quantise(c["abcd"], c["kinds"], c["size"], c["dims"], ST.effective_tau(c["size"], c["dims"]), p["dist_m"], p["back_m"], p["cos_min"])


def twin_of(key):
    """the twin's (cls, plane, object, records, stats), computed once per key; nobody writes into the arrays"""
    if ("twin", key) not in _CACHE:
        c = case_of(key)
        _CACHE[("twin", key)] = ST.split(c["vol"], rule_of(c), c["params"]["min_voxels"])
    return _CACHE[("twin", key)]


def color_of(key):
    c = case_of(key)
    if not c["color"]:
        return None
    if ("color", key) not in _CACHE:
        Z, Y, X = c["vol"].shape[:3]
        _CACHE[("color", key)] = np.random.default_rng(len(str(key))).integers(0, 256, (Z, Y, X, 4), dtype=np.uint8)
    return _CACHE[("color", key)]


def roots_of(key, which):
    """a removal's selection as labels: ALL -> None; "largest", "second" -> that record's root"""
    if which is ALL:
        return None
    recs, dims = twin_of(key)[3], case_of(key)["dims"]
    i = {"largest": 0, "second": 1}[which]
    return [lin_of(recs[i], dims)] if i < len(recs) else []


def remove_twin(key, which, mode, halo, fill_weight):
    k = ("remove", key, which, mode, halo, fill_weight)
    if k not in _CACHE:
        c = case_of(key)
        _, _, label, recs, _ = twin_of(key)
        _CACHE[k] = ST.remove(c["vol"], label, recs, rule_of(c), roots_of(key, which), mode, halo, fill_weight, color_of(key))
    return _CACHE[k]


def query_points(dims, size, seed=3, n=300):
    """points for hsk_split_at: voxel centres, points on cell faces (an integer number of cells), points outside the grid"""
    rng = np.random.default_rng(seed)
    cell = np.array([np.float32(size[i]) / np.float32(dims[i]) for i in range(3)], np.float32)
    idx = rng.integers(0, np.array(dims), (n, 3))
    centres = ((idx + 0.5) * cell).astype(np.float32)
    faces = (idx * cell).astype(np.float32)
    outside = np.array([[-0.01, 0.5, 0.5], [0.5, -1.0, 0.5], [0.5, 0.5, size[2] + 0.01], [size[0], 0.2, 0.2], [np.nan, 0.1, 0.1], [1e9, 0.1, 0.1]], np.float32)
    return np.concatenate([centres, faces, outside])
