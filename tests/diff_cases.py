"""The volume pairs the diff tests share (tests/test_diff_host.py on the host, tests/test_gpu_diff.py on the device), each with the
parameters it is diffed and adopted with, and the twin's result of each, computed once."""
import numpy as np

import diff_twin as DT
from fill_cases import RANDOM_DIMS, random_volume


def words_of(raw, n, offset):
    w = np.frombuffer(raw, np.uint32, n, offset)
    return np.stack([(w & 0xffff).astype(np.uint16).view(np.int16), (w >> 16).astype(np.uint16).view(np.int16)], axis=-1)


def records_as_dicts(recs):
    return [{"root": tuple(map(int, c["root"])), "n_voxels": int(c["n_voxels"]), "n_appeared": int(c["n_appeared"]), "n_vanished": int(c["n_vanished"]),
             "lo": tuple(map(int, c["lo"])), "hi": tuple(map(int, c["hi"]))} for c in recs]


_CACHE = {}
RANDOM_MIN_VOXELS = 8
BOTH = DT.ADOPT_APPEARED | DT.ADOPT_VANISHED


def random_pair(dims):
    """ref = the random volume of these dims; cur = a copy with boxes replaced by rolled content of the same volume -- one across
    the tile faces x = 16, y = 16 and z = 8 together, one on the last planes, small ones -- and a few weights zeroed"""
    key = ("pair", dims)
    if key not in _CACHE:
        X, Y, Z = dims
        ref = random_volume(dims)
        cur = ref.copy()
        rolled = np.roll(ref, 4, axis=0)
        for z, y, x in ((slice(2, 16), slice(6, 28), slice(6, 28)), (slice(Z - 9, Z), slice(30, 44), slice(40, 60)), (slice(20, 30), slice(0, 9), slice(X - 10, X)),
                        (slice(16, 19), slice(40, 43), slice(4, 8)), (slice(25, 27), slice(50, 52), slice(30, 32))):
            cur[z, y, x] = rolled[z, y, x]
        rng = np.random.default_rng(X * 1000 + Z)
        for _ in range(40):
            z, y, x = rng.integers(0, Z - 2), rng.integers(0, Y - 2), rng.integers(0, X - 2)
            cur[z:z + 2, y:y + 2, x:x + 2, 1] = 0
        _CACHE[key] = (ref, np.ascontiguousarray(cur))
    return _CACHE[key]


def random_colors(dims):
    key = ("colors", dims)
    if key not in _CACHE:
        X, Y, Z = dims
        rng = np.random.default_rng(7 + Z)
        _CACHE[key] = tuple(rng.integers(0, 256, (Z, Y, X, 4), dtype=np.uint8) for _ in range(2))
    return _CACHE[key]


def flat(shape, raw=0, weight=2):
    Z, Y, X = shape
    vol = np.zeros((Z, Y, X, 2), np.int16)
    vol[..., 0] = raw
    vol[..., 1] = weight
    return vol


def painted(ref, blocks):
    """a copy of ref with blocks = [((z, y, x) slices, (raw, weight) or raw)] painted in"""
    cur = ref.copy()
    for at, word in blocks:
        if isinstance(word, tuple):
            cur[at] = word
        else:
            cur[at + (0,)] = word
    return cur


def sl(z, y, x):
    return tuple(slice(*v) if isinstance(v, tuple) else slice(v, v + 1) for v in (z, y, x))


APP, VAN = -20000, 20000          # cur's raw over a ref of raw 0: d = -20000 <= -16384, d = 20000 >= 16384
SHAPE = (20, 24, 32)              # 20 planes: a plane group of its own for the last four


def shapes():
    """name -> dict: ref, cur, params (diff; min_voxels 1 unless the case says otherwise), box (for the download; None: a default one), adopts = [(which, halo)], color =
    None | "both" | "ref" """
    if "shapes" in _CACHE:
        return _CACHE["shapes"]
    out = {}

    def case(name, ref, cur, params=None, adopts=(), box=None, color=None):
        out[name] = dict(ref=ref, cur=cur, params=dict(dict(min_voxels=1), **(params or {})), adopts=list(adopts), box=box, color=color)

    lo, hi = DT.ROOM_BOX
    empty, boxed = DT.room(), DT.room(DT.ROOM_BOX)
    moved = DT.room(((lo[0] + 6, lo[1], lo[2]), (hi[0] + 6, hi[1], hi[2])))
    room_p = dict(min_voxels=64)
    case("the box appears", empty, boxed, room_p, [(BOTH, 0), (BOTH, 1), (BOTH, 2), (DT.ADOPT_VANISHED, 2)], box=((17, 11, 5), (37, 34, 22)))
    case("the box vanishes", boxed, empty, room_p, [(BOTH, 2), (DT.ADOPT_APPEARED, 2), (DT.ADOPT_VANISHED, 1)], color="both")
    case("the box moves", boxed, moved, room_p, [(BOTH, 2), (DT.ADOPT_APPEARED, 2), (DT.ADOPT_VANISHED, 2), (BOTH, 8)], color="ref")
    case("the wall shifted by 0.5", empty, DT.room(wall_x=50.9), room_p, [(BOTH, 2)])
    case("the wall shifted by 1.0", empty, DT.room(wall_x=51.4), room_p)
    # d exactly at the threshold and one inside it, on either side, at the default thresh and at thresh 1 and 65534
    ref = flat(SHAPE)
    for t in (16384, 1, 65534):
        base = flat(SHAPE, raw=0 if t < 40000 else -32767)
        at = [sl(3, 5, 6), sl(3, 5, 9), sl(9, 13, 17), sl(9, 13, 20)]
        if t < 40000:
            vals = [t, t - 1, -t, -(t - 1)]
            case(f"d at thresh {t}", base, painted(base, list(zip(at, vals))), dict(thresh=t))
        else:
            # ref -32767, cur 32767: d = 65534 = thresh, VANISHED; cur 32766: 65533, SAME; and the mirror from a ref of 32767
            up = painted(base, [(at[2], 32767), (at[3], 32767)])
            case(f"d at thresh {t}", up, painted(base, [(at[0], 32767), (at[1], 32766), (at[2], -32767), (at[3], -32766)]), dict(thresh=t))
    # W exactly min_weight and one below, on either side: ref observed for x < 16 (W = 3; beyond, W = 2), cur for y < 12
    ref = painted(flat(SHAPE, weight=3), [(sl((0, 20), (0, 24), (16, 32)), (0, 2))])
    cur = painted(flat(SHAPE, weight=3), [(sl((4, 9), (6, 18), (10, 22)), (VAN, 3)), (sl((0, 20), (12, 24), (0, 32)), (0, 2)), (sl((4, 9), (12, 18), (10, 22)), (VAN, 2))])
    case("W at min_weight 3", ref, cur, dict(min_weight=3), [(BOTH, 1)])
    case("min_weight 128", painted(flat(SHAPE, weight=128), [(sl((0, 20), (0, 24), (0, 7)), (0, 127))]),
         painted(flat(SHAPE, raw=APP, weight=128), [(sl((0, 20), (10, 24), (0, 32)), (APP, 127)), (sl(19, 3, 30), (APP, 129))]), dict(min_weight=128))
    # a raw of -32768 on either side counts as -32767: with thresh 65534 the pairs (-32768, 32766) and (32766, -32768) give
    # |d| = 65533, SAME; taken literally they would give 65534
    ref = painted(flat(SHAPE), [(sl(4, 4, (4, 8)), -32768), (sl(6, 4, (4, 8)), 32766), (sl(8, 4, (4, 8)), -32768), (sl(10, 4, (4, 8)), 32767)])
    cur = painted(flat(SHAPE), [(sl(4, 4, (4, 8)), 32766), (sl(6, 4, (4, 8)), -32768), (sl(8, 4, (4, 8)), 32767), (sl(10, 4, (4, 8)), -32768)])
    case("raw -32768 on either side", ref, cur, dict(thresh=65534), [(BOTH, 1)])
    ref = flat(SHAPE)
    case("a face joins APPEARED and VANISHED", ref, painted(ref, [(sl((5, 9), (6, 10), (4, 8)), APP), (sl((5, 9), (6, 10), (8, 12)), VAN)]), adopts=[(DT.ADOPT_APPEARED, 1)])
    case("an edge does not join", ref, painted(ref, [(sl((5, 9), (6, 10), (4, 8)), APP), (sl((5, 9), (10, 14), (8, 12)), VAN)]))
    # regions of 12 and 11 voxels with min_voxels 12; two kept regions of 18 voxels each: the tie goes to the smaller root
    case("min_voxels and one less", ref, painted(ref, [(sl((2, 4), (2, 4), (2, 5)), APP), (sl((2, 4), (8, 10), (2, 5)), VAN), (sl(3, 9, 4), 0),
                                                     (sl((12, 14), (3, 6), (20, 23)), VAN), (sl((6, 8), (15, 18), (9, 12)), APP)]), dict(min_voxels=12), [(BOTH, 2)])
    case("a region on each grid face", ref, painted(ref, [(sl((6, 12), (8, 16), (0, 3)), APP), (sl((6, 12), (8, 16), (29, 32)), VAN), (sl((6, 12), (0, 3), (10, 22)), APP),
                                                         (sl((6, 12), (21, 24), (10, 22)), VAN), (sl((0, 2), (8, 16), (10, 22)), APP), (sl((18, 20), (8, 16), (10, 22)), VAN)]),
         dict(min_voxels=20), [(BOTH, 8), (BOTH, 2)], color="both")
    case("identical volumes", boxed, boxed.copy(), room_p, [(BOTH, 2)])
    case("everything changed", flat((9, 24, 24)), flat((9, 24, 24), raw=APP), adopts=[(BOTH, 0)])
    # the widest halo from two opposite corners of a grid with X = 24 (no multiple of 16) and Z = 9 (one ragged plane group): the x
    # window runs past both row ends, the y and z windows past both faces
    small = flat((9, 24, 24))
    case("halo 8 from two corners", small, painted(small, [(sl(0, 0, 0), APP), (sl(8, 23, 23), VAN)]), adopts=[(BOTH, 8)], color="both")
    # cur has never-observed voxels inside the halo: they are not adopted
    cur = painted(ref, [(sl((5, 9), (6, 10), (4, 8)), APP), (sl((3, 6), (4, 12), (8, 11)), (123, 0)), (sl(9, (5, 11), (3, 9)), (0, 0))])
    case("cur unobserved inside the halo", ref, cur, adopts=[(BOTH, 2), (BOTH, 1)], color="both")
    _CACHE["shapes"] = out
    return out


def colors_of(name):
    """(ref's colour volume or None, cur's or None) of a shape"""
    c = shapes()[name]
    if c["color"] is None:
        return None, None
    Z, Y, X = c["ref"].shape[:3]
    key = ("shape colors", name)
    if key not in _CACHE:
        rng = np.random.default_rng(len(name))
        _CACHE[key] = tuple(rng.integers(0, 256, (Z, Y, X, 4), dtype=np.uint8) for _ in range(2))
    a, b = _CACHE[key]
    return a, (b if c["color"] == "both" else None)


def twin_of(key, ref, cur, params):
    """the twin's (cls, region, records, stats), computed once per key; nobody writes into the arrays"""
    if ("twin", key) not in _CACHE:
        _CACHE[("twin", key)] = DT.diff(ref, cur, **params)
    return _CACHE[("twin", key)]


def shape_twin(name):
    c = shapes()[name]
    return twin_of(("shape", name), c["ref"], c["cur"], c["params"])


def random_twin(dims):
    ref, cur = random_pair(dims)
    return twin_of(("random", dims), ref, cur, dict(min_voxels=RANDOM_MIN_VOXELS))


def adopt_twin(key, ref, cur, cls, which, halo, ref_color=None, cur_color=None):
    k = ("adopt", key, which, halo, ref_color is not None, cur_color is not None)
    if k not in _CACHE:
        _CACHE[k] = DT.adopt(ref, cur, cls, which, halo, ref_color, cur_color)
    return _CACHE[k]


def query_points(dims, size_m, seed=3, n=400):
    """points for hsk_diff_at: voxel centres, points on cell faces (an integer number of cells), points outside the grid"""
    rng = np.random.default_rng(seed)
    cell = np.array([np.float32(size_m[i]) / np.float32(dims[i]) for i in range(3)], np.float32)
    idx = rng.integers(0, np.array(dims), (n, 3))
    centres = ((idx + 0.5) * cell).astype(np.float32)
    faces = (idx * cell).astype(np.float32)
    outside = np.array([[-0.01, 0.5, 0.5], [0.5, -1.0, 0.5], [0.5, 0.5, size_m[2] + 0.01], [size_m[0], 0.2, 0.2], [np.nan, 0.1, 0.1], [1e9, 0.1, 0.1]], np.float32)
    return np.concatenate([centres, faces, outside])
