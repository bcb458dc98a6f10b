"""The fusion tests' plane and general cases on the host, the room scans the device tests share, the device-against-twin
assertions, and the shape cases (tests/test_fuse_shapes_host.py, tests/test_gpu_fuse_shapes.py): ragged volumes, unequal cells,
lone observed cells, a footprint of more chunks than the sweep has waves -- with their twin results, made once, and a binary64
restatement of the bricks a destination chunk can reach, by which the host test shows that each case reaches what it is for."""
from collections import namedtuple

import numpy as np
import pytest

import fuse_twin as FT
import level_twin as LT
from level_cases import tilted, twin_of as level_twin_of
from section_cases import SCAN_FRAMES
from view_twin import plane_volume

f32 = np.float32


def general(n_cells_shift=0.37, size=3.0, n=32):
    """a general rotation about the volume's centre (no axis of it is a grid axis) with a sub-cell shift"""
    c = size / 2
    m = FT.rot_about("y", 25.0, (c, c, c)) @ FT.rot_about("x", -13.0, (c, c, c)) @ FT.rot_about("z", 8.0, (c, c, c))
    m = m.astype(np.float64)
    m[:3, 3] += n_cells_shift * size / n * np.array([1.0, -0.6, 0.3])
    return m.astype(f32)


PLANE_N, PLANE_TAU = 64, 0.3


def plane_case():
    """(source volume, source -> destination matrix, the moved plane as (unit normal, offset): n . p = d)"""
    src = plane_volume(PLANE_N, cells_in_front=3.5, size=3.0, trunc=PLANE_TAU)
    cell = 3.0 / PLANE_N
    m = FT.rot_about("y", 30.0, (1.5, 1.5, 1.5), (0.31 * cell, -0.23 * cell, 0.17 * cell))
    M = m.astype(np.float64)
    nrm = M[:3, :3] @ np.array([0.0, 0.0, 1.0])
    d = (3.0 - 3.5 * cell) + nrm @ M[:3, 3]
    return src, m, nrm, d


N = 128
SIZE = (3.0, 3.0, 3.0)
HOUSE_DIMS, HOUSE_SIZE = (256, 128, 128), (6.0, 3.0, 3.0)

SCAN_STEP = 3    # every third frame of the scripted three-turn scan: 240 frames per room

_SCANS = {}


def scan_room(hsk, variant, lo=0, hi=SCAN_FRAMES, step=SCAN_STEP):
    """a room's RGB-D scan at 128^3: depth and colour of the scripted trajectory's frames, fused at the script's own poses
    through the stage-level calls (at 47 mm of truncation the TRACKER loses this trajectory near frame 190; what is under test
    here is what happens to a scanned volume, not how its poses were found)"""
    trk = hsk.KinfuTracker(n=N, init_pose=hsk.synth_room_pose(variant, 0, SCAN_FRAMES))
    trk.enable_color()
    for at in range(lo, hi, 48 * step):
        ks = list(range(at, min(at + 48 * step, hi), step))
        for k, (d, c) in zip(ks, room_frames_at(hsk, variant, ks)):
            pose = hsk.synth_room_pose(variant, k, SCAN_FRAMES)
            trk.integrate(d, pose)
            trk.integrate_color(d, c, pose)
    return trk


def room_frames_at(hsk, variant, ks):
    from concurrent.futures import ThreadPoolExecutor
    poses = [hsk.synth_room_pose(variant, k, SCAN_FRAMES) for k in ks]
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda p: (hsk.synth_room_depth(variant, p), hsk.synth_rgb(p, variant)), poses))


def room_scan(hsk, variant):
    """(tracker, tsdf, colour volume) of a room's RGB-D scan at 128^3, made once per module"""
    if variant not in _SCANS:
        trk = scan_room(hsk, variant)
        _SCANS[variant] = (trk, trk.download_tsdf(), trk.download_color())
    return _SCANS[variant]


@pytest.fixture(scope="module", autouse=True)
def _close_scans():
    yield
    for trk, _, _ in _SCANS.values():
        trk.close()
    _SCANS.clear()


def make_ctx(hsk, dims=(N, N, N), size=SIZE, color=True, **over):
    cfg = hsk.default_config(dims[2], vol_x=dims[0], vol_y=dims[1], vol_z=dims[2], vol_size_m=size, **over)
    trk = hsk.KinfuTracker(cfg)
    if color:
        trk.enable_color()
    return trk


# ---- the device against the twin ---------------------------------------------------------------------------------------------------
def empty_like_ctx(dims, color=True):
    tsdf = np.zeros((dims[2], dims[1], dims[0], 2), np.int16)
    return tsdf, (np.zeros((dims[2], dims[1], dims[0], 4), np.uint8) if color else None)


def assert_fused(dst, stats, ref_tsdf, ref_color, ref_stats, box, what):
    """the device against the twin, zero differences"""
    assert stats["box"] == box, f"{what}: box {stats['box']} != {box}"
    assert stats["n_fused"] == ref_stats["n_fused"], f"{what}: n_fused {stats['n_fused']} != {ref_stats['n_fused']}"
    assert stats["n_colored"] == ref_stats["n_colored"], f"{what}: n_colored {stats['n_colored']} != {ref_stats['n_colored']}"
    got = dst.download_tsdf()
    bad = np.argwhere((got != ref_tsdf).any(axis=-1))
    assert len(bad) == 0, (f"{what}: {len(bad)} TSDF pairs differ, first (z, y, x) {bad[:4].tolist()}: "
                           f"{got[tuple(bad[0])].tolist()} != {ref_tsdf[tuple(bad[0])].tolist()}")
    if ref_color is not None:
        gc = dst.download_color()
        bad = np.argwhere((gc != ref_color).any(axis=-1))
        assert len(bad) == 0, (f"{what}: {len(bad)} colour voxels differ, first {bad[:4].tolist()}: "
                               f"{gc[tuple(bad[0])].tolist()} != {ref_color[tuple(bad[0])].tolist()}")
    assert FT.box_contains(box, ref_stats["box"]), f"{what}: the footprint {box} misses fused voxels {ref_stats['box']}"
    assert stats["chunks_swept"] <= stats["chunks_total"]
    assert stats["n_fused"] == 0 or stats["chunks_swept"] > 0, what


def assert_nontrivial(ref_tsdf, ref_stats, src_tsdf, what, share=0.05):
    """the twin's own result: it fused at least 5 % of the source's observed voxels and holds both signs"""
    observed = int((src_tsdf[..., 1] > 0).sum())
    assert ref_stats["n_fused"] >= share * observed, f"{what}: the twin fused {ref_stats['n_fused']} of {observed} observed voxels"
    f = ref_tsdf[..., 0][ref_stats["fused"]]
    assert (f < 0).any() and (f > 0).any(), f"{what}: the fused TSDF has one sign only"


# ---- crafted volumes ------------------------------------------------------------------------------------------------------------
def crafted(dims, seed, hole=0.03):
    """a [Z, Y, X, 2] int16 volume of noise: raw values uniform in -32767 .. 32767, weights in 1 .. 5, and a `hole` share of the
    voxels at weight 0 (their raw values stay: a rule that read them would show), so that Ws == 0 leaves voxels alone in the
    middle of the swept region"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vol = np.empty((Z, Y, X, 2), np.int16)
    vol[..., 0] = rng.integers(-32767, 32768, (Z, Y, X))
    vol[..., 1] = rng.integers(1, 6, (Z, Y, X))
    vol[rng.random((Z, Y, X)) < hole, 1] = 0
    return vol


def crafted_colour(dims, seed, none=0.10):
    """the [Z, Y, X, 4] uint8 companion of crafted(): random colours, weights in 1 .. 40, about 10 % of the voxels at weight 0"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    col = rng.integers(0, 256, (Z, Y, X, 4), dtype=np.uint8)
    col[..., 3] = np.where(rng.random((Z, Y, X)) < none, 0, rng.integers(1, 41, (Z, Y, X)))
    return col


def lone_cells(dims, corners, seed):
    """an empty volume in which each lower corner (x, y, z) of `corners` gets a 2 x 2 x 2 cube of observed voxels (noise, weights
    in 1 .. 5): the eight taps of exactly one sample cell"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vol = np.zeros((Z, Y, X, 2), np.int16)
    for x, y, z in corners:
        assert 1 <= x <= X - 3 and 1 <= y <= Y - 3 and 1 <= z <= Z - 3, (x, y, z)
        vol[z:z + 2, y:y + 2, x:x + 2, 0] = rng.integers(-32767, 32768, (2, 2, 2))
        vol[z:z + 2, y:y + 2, x:x + 2, 1] = rng.integers(1, 6, (2, 2, 2))
    return vol


def block_volume(dims, lo, hi, seed):
    """an empty volume whose voxels lo .. hi - 1 on every axis are observed (noise, weights in 1 .. 5)"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vol = np.zeros((Z, Y, X, 2), np.int16)
    n = hi - lo
    vol[lo:hi, lo:hi, lo:hi, 0] = rng.integers(-32767, 32768, (n, n, n))
    vol[lo:hi, lo:hi, lo:hi, 1] = rng.integers(1, 6, (n, n, n))
    return vol


# ---- what a destination chunk can reach -----------------------------------------------------------------------------------------------
CHUNK = 16        # fuse.hip: HSK_FCHUNK
Reach = namedtuple("Reach", "chunk lo n nb observed")


def chunk_grid(box):
    """the footprint in chunks as the sweep counts them: (first voxel per axis, a multiple of 16; chunks per axis)"""
    c0 = [box[2 * i] // CHUNK * CHUNK for i in range(3)]
    return c0, [(box[2 * i + 1] - c0[i] + CHUNK - 1) // CHUNK for i in range(3)]


def chunk_index(box, x, y, z):
    """the sweep's chunk number of destination voxel (x, y, z) of the footprint"""
    c0, cn = chunk_grid(box)
    return (x - c0[0]) // CHUNK + cn[0] * ((y - c0[1]) // CHUNK + cn[1] * ((z - c0[2]) // CHUNK))


def chunk_bricks(src_dims, src_size, dst_dims, dst_size, m, box, src=None):
    """In plain binary64, what the chunks of the footprint `box` can reach of the source: per chunk, in the sweep's order, a
    Reach(chunk (cx, cy, cz), lo, n, nb, observed) -- the box of 8^3 source bricks `lo .. lo + n - 1` per axis that the taps of the
    chunk's voxels lie in (the images of the chunk's eight corner centres, their voxels' range ga .. gb, the taps max(ga, 1) - 1 ..
    min(gb, dims - 2) + 1, each >> 3: as k_fuse_sweep pads it, without the float slack), nb = n_x n_y n_z, and, when the source
    volume is given, the in-box indices x + n_x (y + n_y z) of the bricks that hold an observed voxel, ascending.  A chunk whose
    range misses the source's interior has nb = 0.  Only ever asked whether a case reaches what it is for; never compared with the
    device (the slack may give the device a larger box)."""
    inv = FT.invert_rigid(m).astype(np.float64)
    A, b = inv[:3, :3], inv[:3, 3]
    cs = [np.float64(c) for c in FT.cells(src_dims, src_size)]
    cd = [np.float64(c) for c in FT.cells(dst_dims, dst_size)]
    table = None
    if src is not None:
        Z, Y, X, _ = src.shape
        pad = np.zeros((-(-Z // 8) * 8, -(-Y // 8) * 8, -(-X // 8) * 8), bool)
        pad[:Z, :Y, :X] = src[..., 1] != 0
        table = pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8, pad.shape[2] // 8, 8).any(axis=(1, 3, 5))     # [bz, by, bx]
    c0, cn = chunk_grid(box)
    out = []
    for cz in range(cn[2]):
        for cy in range(cn[1]):
            for cx in range(cn[0]):
                a = [c0[0] + cx * CHUNK, c0[1] + cy * CHUNK, c0[2] + cz * CHUNK]
                e = [min(a[i] + CHUNK - 1, dst_dims[i] - 1) for i in range(3)]
                corners = np.array([[((e[i] if (c >> i) & 1 else a[i]) + 0.5) * cd[i] for i in range(3)] for c in range(8)])
                ps = corners @ A.T + b
                lo, n, miss = [], [], False
                for i in range(3):
                    ga = int(min(max(np.floor(ps[:, i].min() / cs[i]), -2.0), src_dims[i] + 1))
                    gb = int(min(max(np.floor(ps[:, i].max() / cs[i]), -2.0), src_dims[i] + 1))
                    miss |= gb < 1 or ga > src_dims[i] - 2
                    ta, tb = max(ga, 1) - 1, min(gb, src_dims[i] - 2) + 1
                    lo.append(ta >> 3)
                    n.append((tb >> 3) - (ta >> 3) + 1)
                if miss:
                    out.append(Reach((cx, cy, cz), None, None, 0, [] if table is not None else None))
                    continue
                obs = None
                if table is not None:
                    z, y, x = np.nonzero(table[lo[2]:lo[2] + n[2], lo[1]:lo[1] + n[1], lo[0]:lo[0] + n[0]])
                    obs = sorted(int(v) for v in x + n[0] * (y + n[1] * z))
                out.append(Reach((cx, cy, cz), tuple(lo), tuple(n), n[0] * n[1] * n[2], obs))
    return out


# ---- the shape cases ----------------------------------------------------------------------------------------------------------------
# (source dims (X, Y, Z), size, destination dims, size, source -> destination matrix, colour or not, trunc_dist_m of every context of
# the case: hsk_fuse_volume refuses contexts whose effective truncation distances differ, and that distance is
# max(trunc_dist_m, 2.1 x the largest cell), so one value at or above 2.1 x the largest cell of either volume serves both)
Case = namedtuple("Case", "sdims ssize ddims dsize m colour trunc")

RAG_SRC = ((72, 40, 50), (2.7, 1.5, 1.875))     # 13 plane groups: an odd count, one group in the last brick layer; X crosses one 64-voxel row
RAG_DST = ((56, 72, 41), (2.4, 2.7, 1.9))       # X, Y no multiples of 16, Z ends on the first plane of a group; cells 42.9, 37.5, 46.3 mm
COARSE_SRC = ((128, 128, 128), (3.0, 3.0, 3.0))
COARSE_DST = ((40, 40, 40), (3.0, 3.0, 3.0))    # cells of 75 mm against 23.4 mm: a chunk reaches 7 x 7 x 7 bricks and more
SLAB_DST = ((1448, 1456, 4), (3.0, 3.0, 4 * 3.0 / 128))   # 91 x 91 x 1 = 8281 chunks, the last one in x half filled
SWEEP_WAVES = 4 * 2048                          # fuse.hip, launch_fuse_sweep: at most 2048 workgroups of four waves
LONE_DST = ((152, 88, 100), (2.85, 1.65, 1.875))          # cells half the source's: every turned source cell holds a centre
# lower corners (x, y, z) of the lone cells: the first and the last interior cell; cells that straddle a brick boundary (voxels
# 8k - 1 | 8k) on one axis, on two and on all three; a few that lie inside one brick
LONE_CORNERS = ((1, 1, 1), (69, 37, 47),
                (7, 12, 20), (18, 15, 4), (28, 3, 39), (63, 20, 12),
                (23, 7, 28), (36, 31, 15), (47, 26, 23), (12, 23, 47),
                (39, 23, 31), (55, 15, 39), (15, 31, 7), (31, 7, 47),
                (50, 4, 44),(60, 33, 34), (4, 34, 36), (44, 18, 2))
LONE_SEEDS = (11, 12, 13)
LEVEL_SCENE, LEVEL_TILT, LEVEL_TRUNC = "80x64x48", "a", 0.03

DEFER_N, DEFER_FRAMES = 64, 4                   # case F: a tracked 64^3 source whose free-space weights are still deferred


def deferred_case():
    """case F's geometry: the 64^3 tracker's volume under a general matrix into the ragged destination (its source is grown on
    the device, so it has no twin result here)"""
    return Case((DEFER_N,) * 3, (3.0, 3.0, 3.0), *RAG_DST, general(n=DEFER_N), False, PLANE_TAU)


SHAPE_NAMES = ("A ragged both", "A again", "B brick 285", "B last lane", "B dense, turned", "C slab",
               "D lone 0", "D lone 1", "D lone 2", "E levelled")
PREVIOUS = {"A again": "A ragged both"}         # the destination a case starts from, when it is not empty
_SHAPES = {}


def turned(centre, degrees, shift):
    """rotations about y, x and z through `centre` (no axis of the result is a grid axis), then the translation `shift`"""
    m = FT.rot_about("y", degrees[0], centre) @ FT.rot_about("x", degrees[1], centre) @ FT.rot_about("z", degrees[2], centre)
    m = m.astype(np.float64)
    m[:3, 3] += np.asarray(shift, np.float64)
    return m.astype(f32)


def lone_matrix(seed):
    """a seeded rigid matrix: rotations within +-40 degrees about the source's centre, which goes to the destination's centre, and
    a shift below one destination cell"""
    rng = np.random.default_rng(seed)
    sc, dc = np.array(RAG_SRC[1]) / 2, np.array(LONE_DST[1]) / 2
    return turned(tuple(sc), rng.uniform(-40, 40, 3), dc - sc + rng.uniform(-0.5, 0.5, 3) * 0.01875)


def case_of(name):
    if name not in _SHAPES:
        sc = tuple(s / 2 for s in RAG_SRC[1])
        cell = 0.0375
        if name == "A ragged both":
            c = Case(*RAG_SRC, *RAG_DST, turned(sc, (25.0, -13.0, 8.0), (0.37 * cell, -0.22 * cell, 0.11 * cell)), True, PLANE_TAU)
        elif name == "A again":        # the source once more, from the other side and up the destination's y, into what the first fuse left
            c = Case(*RAG_SRC, *RAG_DST, turned(sc, (-9.0, 17.0, -21.0), (-0.2 + 0.41 * cell, 1.2 + 0.13 * cell, 0.06 - 0.29 * cell)), True, PLANE_TAU)
        elif name in ("B brick 285", "B last lane"):
            c = Case(*COARSE_SRC, *COARSE_DST, np.eye(4, dtype=f32), False, PLANE_TAU)
        elif name == "B dense, turned":
            c = Case(*COARSE_SRC, *COARSE_DST, general(n=128), False, PLANE_TAU)
        elif name == "C slab":
            # the slab's four planes lie in the source's planes 59 .. 63, a third of a cell off the grid.  Along z alone the
            # footprint would end at x = 1438, the image of the source's last interior cell: 90 x 91 = 8190 chunks, two short of
            # the waves; 0.4 source cells along x take it to 1442 and into the last, half-filled chunk column: 91 x 91
            c = Case(*COARSE_SRC, *SLAB_DST, FT.translation((0.4 * 3.0 / 128, 0.0, -(59 + 0.37) * 3.0 / 128)), False, PLANE_TAU)
        elif name.startswith("D lone"):
            c = Case(*RAG_SRC, *LONE_DST, lone_matrix(LONE_SEEDS[int(name[-1])]), False, PLANE_TAU)
        elif name == "E levelled":     # the product's own use: destination, truncation and matrix are hsk_level_config's, on the twin
            dims, size = LT.SCENES[LEVEL_SCENE]
            d_dims, d_size, d_trunc, M = LT.level_config(dims, size, LEVEL_TRUNC, level_twin_of(LEVEL_SCENE, LEVEL_TILT))
            c = Case(dims, size, d_dims, tuple(float(v) for v in d_size), M, False, float(d_trunc))
        else:
            raise KeyError(name)
        _SHAPES[name] = c
    return _SHAPES[name]


def source_of(name):
    """(volume, colour volume or None) of a case's source, made once and left unchanged"""
    key = ("source", "A ragged both" if name == "A again" else "D" if name.startswith("D lone") else name)
    if key not in _SHAPES:
        c = case_of(name)
        if name.startswith("A "):
            src = crafted(c.sdims, 21), crafted_colour(c.sdims, 22)
        elif name == "B brick 285":
            src = block_volume(c.sdims, 40, 48, 23), None
        elif name == "B last lane":
            src = block_volume(c.sdims, 48, 52, 24), None
        elif name in ("B dense, turned", "C slab"):
            src = crafted(c.sdims, 25), None
        elif name.startswith("D lone"):
            src = lone_cells(c.sdims, LONE_CORNERS, 26), None
        else:
            src = tilted(LEVEL_SCENE, LEVEL_TILT, LEVEL_TRUNC)[0], None
        for a in src:
            if a is not None:
                a.setflags(write=False)
        _SHAPES[key] = src
    return _SHAPES[key]


def before_of(name):
    """(volume, colour volume or None) of a case's destination before the fuse: empty, or what the case before it left"""
    if name in PREVIOUS:
        return twin_of(PREVIOUS[name])[:2]
    c = case_of(name)
    return empty_like_ctx(c.ddims, c.colour)


def twin_of(name):
    """FT.fuse of a case -> (volume, colour volume or None, stats), made once and left unchanged"""
    key = ("twin", name)
    if key not in _SHAPES:
        c = case_of(name)
        d_t, d_c = before_of(name)
        s_t, s_c = source_of(name)
        ref = FT.fuse(d_t, c.dsize, s_t, c.ssize, c.m, d_c, s_c, planes=2 if name == "C slab" else 16)    # (the slab: 2 planes keep the twin's arrays small)
        for a in ref[:2]:
            if a is not None:
                a.setflags(write=False)
        _SHAPES[key] = ref
    return _SHAPES[key]


def footprint_of(name):
    c = case_of(name)
    return FT.footprint(c.sdims, c.ssize, c.ddims, c.dsize, c.m)


def reach_of(name):
    """chunk_bricks of a case, made once"""
    key = ("reach", name)
    if key not in _SHAPES:
        c = case_of(name)
        _SHAPES[key] = chunk_bricks(c.sdims, c.ssize, c.ddims, c.dsize, c.m, footprint_of(name), source_of(name)[0])
    return _SHAPES[key]


def lone_cell_counts(name):
    """per lone cell of a case D: (inside: all eight corners of the cell's cube of sample points map into the destination's interior,
    the centres 1 .. dims - 2 and half a cell around them; fused: the destination voxels of the twin that took their sample from it)"""
    c = case_of(name)
    cs = [float(v) for v in FT.cells(c.sdims, c.ssize)]
    cd = [float(v) for v in FT.cells(c.ddims, c.dsize)]
    M = c.m.astype(np.float64)
    inv = FT.invert_rigid(c.m).astype(np.float64)
    fused = twin_of(name)[2]["fused"]
    z, y, x = np.nonzero(fused)
    pd = np.stack([(x + 0.5) * cd[0], (y + 0.5) * cd[1], (z + 0.5) * cd[2]], -1)
    ps = pd @ inv[:3, :3].T + inv[:3, 3]
    out = []
    for corner in LONE_CORNERS:
        lo = np.array([(corner[i] + 0.5) * cs[i] for i in range(3)])
        hi = np.array([(corner[i] + 1.5) * cs[i] for i in range(3)])
        cube = np.array([[hi[i] if (k >> i) & 1 else lo[i] for i in range(3)] for k in range(8)]) @ M[:3, :3].T + M[:3, 3]
        inside = all((cube[:, i] >= cd[i]).all() and (cube[:, i] <= (c.ddims[i] - 1) * cd[i]).all() for i in range(3))
        eps = 1e-6
        mine = ((ps >= lo - eps) & (ps <= hi + eps)).all(axis=1)
        out.append((inside, int(mine.sum())))
    assert sum(n for _, n in out) == len(x), "a fused voxel belongs to no lone cell, or to two"
    return out
