"""The cases of the simplified mesh's shape tests, shared by the host test (tests/test_simplify_shapes_host.py) and the GPU test
(tests/test_gpu_simplify_shapes.py): volumes wide enough to leave the first 64-cluster segment of a cluster row and tall enough
to leave the first 1024-row scan block, their twins (tests/simplify_twin.py), made once, and the census of a twin result that says
which of the kernels' bookkeeping an input reaches -- asserted by the host test on every case, so that the GPU test cannot pass
on an input that misses the code it is there for."""
import numpy as np

import simplify_twin as ST
from kit import same_bits
from mesh_twin import mesh_indexed, same_normals

CLUSTERS = (2, 4, 8, 16)
MODES = (ST.QUADRIC, ST.MEAN)
BOX_DIMS, BOX_SIZE = (72, 40, 24), (2.7, 1.6, 1.2)      # X crosses the indexed mesh's 64-voxel segment; no dim a multiple of 16
SMALL_DIMS, SMALL_SIZE = (32, 24, 12), (3.0, 3.0, 3.0)  # (anisotropic cells)
_CACHE = {}


def grid(dims):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    return x.astype(np.float64), y.astype(np.float64), z.astype(np.float64)


def volume_of(dist_voxels, tau=3.0, weight=3):
    """a signed distance in voxels (positive: free space) -> [Z, Y, X, 2] int16 (tsdf, weight), every weight non-zero"""
    t = np.clip(np.rint(dist_voxels / tau * 32767.0), -32767, 32767).astype(np.int16)
    return np.stack([t, np.full(t.shape, weight, np.int16)], axis=-1)


def box_distance(dims, lo, hi):
    """the free inside of an axis-aligned box room: the distance to the nearest wall, negative in the walls"""
    x, y, z = grid(dims)
    return np.minimum.reduce([x - lo[0], hi[0] - x, y - lo[1], hi[1] - y, z - lo[2], hi[2] - z])


def box_volume():
    return volume_of(box_distance(BOX_DIMS, (5.3, 4.7, 3.4), (66.6, 35.2, 20.3)))


def sphere_volume():
    x, y, z = grid((32, 32, 32))
    return volume_of(np.sqrt((x - 15.3) ** 2 + (y - 16.1) ** 2 + (z - 15.7) ** 2) - 9.4)


def two_walls_volume():
    """free space, one plane of solid voxels at x = 11, free space again: two parallel surfaces one voxel apart"""
    x, y, z = grid(SMALL_DIMS)
    t = np.where(x == 11, -6000.0 - 41.0 * y - 13.0 * z, 8000.0 + 37.0 * y + 11.0 * z)
    return np.stack([t.astype(np.int16), np.full(t.shape, 2, np.int16)], axis=-1)


def holes_volume():
    v = box_volume()
    rng = np.random.default_rng(1905)
    v[rng.random(v.shape[:3]) < 0.1, 1] = 0
    return v


def exact_zeros_volume():
    """stored TSDF exactly 0 on the grid planes x = 12 and x = 20: edges with the ratio exactly 1 (-4000 -> 0) and exactly 0 (0 -> -4000)"""
    x, _, _ = grid(SMALL_DIMS)
    t = np.minimum(x - 12.0, 20.0 - x) * 4000.0
    v = np.stack([t.astype(np.int16), np.full(t.shape, 1, np.int16)], axis=-1)
    assert (v[..., 0] == 0).sum() == 2 * 24 * 12
    return v


def six_faces_volume():
    """a tilted plane that meets all six faces of the volume"""
    x, y, z = grid(SMALL_DIMS)
    return volume_of((x / 31.0 + y / 23.0 + z / 11.0 - 1.5) * 9.0)


def blob_volume():
    """one solid voxel at (5, 5, 5): the lower corners of its six cut edges are 4 or 5 on every axis -- one cluster at every size"""
    v = volume_of(np.full(SMALL_DIMS[::-1], 2.0))
    v[5, 5, 5, 0] = -9000
    return v


def empty_volume():
    return np.zeros(SMALL_DIMS[::-1] + (2,), np.int16)


def box_colour():
    rng = np.random.default_rng(77)
    X, Y, Z = BOX_DIMS
    col = rng.integers(0, 256, (Z, Y, X, 4), dtype=np.uint8)
    col[..., 3] = np.where(rng.random((Z, Y, X)) < 0.45, 0, 5)
    col[:, :, :14, 3] = 0                                  # (no colour at all near the wall x = 5.3: uncoloured clusters)
    return col


def small_cases():
    """{name: (volume, dims, size, colour or None)}: the GPU list's uploaded volumes"""
    if "cases" not in _CACHE:
        _CACHE["cases"] = {
            "box": (box_volume(), BOX_DIMS, BOX_SIZE, None),
            "sphere": (sphere_volume(), (32, 32, 32), (3.0, 3.0, 3.0), None),
            "two walls": (two_walls_volume(), SMALL_DIMS, SMALL_SIZE, None),
            "holes": (holes_volume(), BOX_DIMS, BOX_SIZE, None),
            "exact zeros": (exact_zeros_volume(), SMALL_DIMS, SMALL_SIZE, None),
            "six faces": (six_faces_volume(), SMALL_DIMS, SMALL_SIZE, None),
            "blob": (blob_volume(), SMALL_DIMS, SMALL_SIZE, None),
            "empty": (empty_volume(), SMALL_DIMS, SMALL_SIZE, None),
            "box with colour": (box_volume(), BOX_DIMS, BOX_SIZE, box_colour()),
        }
    return _CACHE["cases"]


def case_of(name):
    """a small case or a shape case by its name (the two lists share no name)"""
    return small_cases()[name] if name in small_cases() else shape_cases()[name]


def mesh_of(oracle, name):
    """the indexed mesh of a case, made once"""
    if ("mesh", name) not in _CACHE:
        vol, _, size, col = case_of(name)
        _CACHE[("mesh", name)] = mesh_indexed(vol, *oracle.mc_table(), size=size, col=col, normals=False)
    return _CACHE[("mesh", name)]


def twin_of(oracle, name, c, mode):
    """the twin's result for a case, made once and left unchanged"""
    key = ("twin", name, c, mode)
    if key not in _CACHE:
        vol, _, size, col = case_of(name)
        _CACHE[key] = ST.simplify(vol, *oracle.mc_table(), c=c, mode=mode, size=size, col=col, mesh=mesh_of(oracle, name))
    return _CACHE[key]


def directed_edge_balance(faces):
    """the largest |count(a, b) - count(b, a)| over the directed edges of a face list (0: closed)"""
    f = np.asarray(faces, np.int64)
    if not len(f):
        return 0
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(f.max()) + 1
    fwd, nf = np.unique(a * n + b, return_counts=True)
    bwd, nb = np.unique(b * n + a, return_counts=True)
    return 0 if (np.array_equal(fwd, bwd) and np.array_equal(nf, nb)) else 1 + int(np.setxor1d(fwd, bwd).size)


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def stats_list(st):
    return [st["n_in_vertices"], st["n_in_faces"], st["n_clusters"], st["n_out_vertices"], st["n_out_faces"], st["n_faces_collapsed"]] + st["n_rank"] + \
        [st["n_clamped"], st["n_uncolored"]]


HALL_DIMS, HALL_SIZE = (1032, 24, 21), (6.45, 0.3, 0.21)      # CX = 516, 258, 129, 65 at c = 2, 4, 8, 16: 9, 5, 3, 2 segments
TALL_DIMS, TALL_SIZE = (24, 72, 61), (0.6, 1.2, 1.5)          # 36 x 31 = 1116 cluster rows at c = 2: a second scan block
# the scanned case.  CX = 160 and 80 at c = 2 and 4.  (At 264 voxels over the same 3 m the scene's surfaces end at x = 246 of 264:
# in clusters of 4 voxels nothing is referenced from cx = 64 on, whatever the number of frames -- 4 or 8 frames of the oracle gave
# 835 and 841 output clusters, all in segment 0.  At 320 they end at x = 298, and 137 of the 994 output clusters lie in segment 1.)
WIDE_DIMS, WIDE_SIZE = (320, 48, 40), (3.0, 3.0, 3.0)
WIDE_FRAMES = 4
# x from, x to: the walls across the hall, each for y in [8.3, 14.6] and every z.  In clusters of 2, 4 and 8 voxels the first
# three straddle cx = 63 | 64 (x = 127 | 128, 255 | 256, 511 | 512); in clusters of 16 the end wall (x = 1026.6) and the floor do
HALL_WALLS = ((126.4, 130.7), (253.5, 258.2), (509.3, 515.6), (700.2, 703.9))
HALL_FLIP = (10, 11, 126)                                     # (z, y, x): the free voxel 0.4 in front of the first wall


def room_distance(dims):
    """a room open at the top: the walls at x = 5.3 and X - 5.4, y = 4.7 and Y - 4.8 and the floor at z = 3.4; the walls meet the
    volume's last plane"""
    X, Y, _ = dims
    x, y, z = grid(dims)
    return np.minimum.reduce([x - 5.3, (X - 5.4) - x, y - 4.7, (Y - 4.8) - y, z - 3.4])


def with_holes(vol):
    rng = np.random.default_rng(2024)
    vol[rng.random(vol.shape[:3]) < 0.03, 1] = 0
    return vol


def hall_volume():
    x, y, _ = grid(HALL_DIMS)
    d = room_distance(HALL_DIMS)
    for a, b in HALL_WALLS:
        d = np.minimum(d, np.maximum.reduce([a - x, x - b, 8.3 - y, y - 14.6]))
    return with_holes(volume_of(d))


def hall_colour():
    """tests/test_simplify_host.py's box_colour() at the hall's size"""
    rng = np.random.default_rng(77)
    X, Y, Z = HALL_DIMS
    col = rng.integers(0, 256, (Z, Y, X, 4), dtype=np.uint8)
    col[..., 3] = np.where(rng.random((Z, Y, X)) < 0.45, 0, 5)
    col[:, :, :14, 3] = 0
    return col


def hall_flipped():
    """the hall with one further voxel's sign flipped: a bulge of the first wall, next to the segment edge at c = 2, that adds an
    output cluster and two faces there (the counts of the hall no longer fit)"""
    vol = shape_cases()["hall"][0].copy()
    z, y, x = HALL_FLIP
    assert vol[z, y, x, 0] > 0 and vol[z, y, x, 1] != 0
    vol[z, y, x, 0] = -vol[z, y, x, 0]
    return vol


def tall_volume():
    return with_holes(volume_of(room_distance(TALL_DIMS)))


def shape_cases():
    """{name: (volume, dims, size, colour or None)}: the uploaded volumes, made once"""
    if "shapes" not in _CACHE:
        _CACHE["shapes"] = {
            "hall": (hall_volume(), HALL_DIMS, HALL_SIZE, hall_colour()),
            "tall": (tall_volume(), TALL_DIMS, TALL_SIZE, None),
        }
        _CACHE["shapes"]["hall flipped"] = (hall_flipped(), HALL_DIMS, HALL_SIZE, _CACHE["shapes"]["hall"][3])
        for vol, _, _, _ in _CACHE["shapes"].values():
            vol.setflags(write=False)
    return _CACHE["shapes"]


def wide_frames(synth_frames):
    """the scanned case's input: the first frames of the scripted stream with their ground-truth poses, [(pose, depth)]"""
    return [synth_frames(k) for k in range(WIDE_FRAMES)]


def wide_oracle_volume(oracle, synth_frames):
    """the scanned case on the CPU: the oracle's integrate of the same frames at the same poses, made once"""
    if "wide" not in _CACHE:
        X, Y, Z = WIDE_DIMS
        cfg = oracle.default_config(X, vol=WIDE_DIMS, size=WIDE_SIZE)
        vol = np.zeros((Z, Y, X, 2), np.int16)
        for pose, depth in wide_frames(synth_frames):
            oracle.integrate(cfg, vol, oracle.scale_depth(cfg, depth), pose)
        vol.setflags(write=False)
        _CACHE["wide"] = vol
    return _CACHE["wide"]


# ---- the census ---------------------------------------------------------------------------------------------------------------------
def face_cubes(edges, faces):
    """the cube (x, y, z) of every face of an indexed mesh, from the edges (z, y, x, axis) of its three corners: an edge with
    lower corner g along axis k lies on the cubes whose origin o has o_k = g_k and o_j = g_j - 1 or g_j on the other axes; the
    three edges of a table triangle share exactly one cube (asserted: no triangle lies in a face of its cube), the one at the
    smallest lower corner on every axis"""
    e = np.asarray(edges, np.int64)[np.asarray(faces, np.int64)]          # [m, 3, 4]
    g = e[:, :, 2::-1]                                                    # (x, y, z) of the three lower corners
    on_axis = e[:, :, 3:4] == np.arange(3)[None, None, :]
    lo = np.where(on_axis, g, g - 1).max(axis=1)
    hi = g.min(axis=1)
    assert (lo == hi).all()
    return hi


def census(vol, mesh, tw, c):
    """what a twin result says about the bookkeeping of the kernels (housescan_amd/csrc/simplify.hip) on this input, as a dict:
    cx, crows, cseg     the cluster grid's width, its rows (CY CZ) and the 64-cluster segments of a row
    rows_full           cluster rows with a segment whose 64 clusters are all referenced (an all-ones ballot, rank 63)
    rows_gap            cluster rows with a segment without a referenced cluster between two that have some
    segments_used       the distinct segment numbers that hold a referenced cluster
    at_63, at_64        referenced clusters at cx % 64 == 63, and at cx % 64 == 0 with cx >= 64
    in_last             referenced clusters in the row's last segment
    top_layer           referenced clusters in the top cell layer; top_partial: that layer is cut by the volume's last plane
    rows_1024           referenced clusters in cluster rows >= 1024; rows_below: in the rows before
    faces_across        surviving faces whose three clusters do not all have the same segment number cx >> 6
    trip_rows           cube rows whose surviving faces lie in three or more distinct 64-cube trips of k_simp_faces with a trip
                        between two of them that holds no surviving face; trip_rows_skipped: ... and no edge bit on the cube
                        row's four grid rows either, so that the kernel's `any == 0` test skips it"""
    Z, Y, X, _ = vol.shape
    s = ST.SHIFT[c]
    CX, CY, CZ = (X + c - 1) >> s, (Y + c - 1) >> s, (Z + c - 1) >> s
    cseg = (CX + 63) // 64
    cl = np.asarray(tw["clusters"], np.int64)
    cx, crow = cl % CX, cl // CX
    per = np.zeros((CY * CZ, cseg), np.int64)
    np.add.at(per, (crow, cx >> 6), 1)
    used = per > 0
    before = np.cumsum(used, axis=1) - used > 0                           # (a used segment to the left)
    after = np.cumsum(used[:, ::-1], axis=1)[:, ::-1] - used > 0
    out = dict(cx=CX, crows=CY * CZ, cseg=cseg, n_out=len(cl), n_faces=len(tw["faces"]),
               rows_full=int((per == 64).any(axis=1).sum()), rows_gap=int((~used & before & after).any(axis=1).sum()),
               segments_used=sorted(int(v) for v in np.unique(cx >> 6)),
               at_63=int((cx % 64 == 63).sum()), at_64=int(((cx % 64 == 0) & (cx >= 64)).sum()), in_last=int(((cx >> 6) == cseg - 1).sum()),
               top_layer=int((crow // CY == CZ - 1).sum()), top_partial=Z % c != 0,
               rows_1024=int((crow >= 1024).sum()), rows_below=int((crow < 1024).sum()))
    f = np.asarray(tw["faces"], np.int64)
    seg = (cx >> 6)[f] if len(f) else np.zeros((0, 3), np.int64)
    out["faces_across"] = int(((seg[:, 0] != seg[:, 1]) | (seg[:, 0] != seg[:, 2])).sum())
    # the trips of the cube rows: the surviving input faces by (cube row, trip), the edge bits by (grid row, trip)
    edges, faces_in = np.asarray(mesh["edges"], np.int64), np.asarray(mesh["faces"], np.int64)
    trips = (X - 1 + 63) // 64
    g = edges[:, 2::-1] >> s
    vcl = (g[:, 2] * CY + g[:, 1]) * CX + g[:, 0]
    fc = vcl[faces_in] if len(faces_in) else np.zeros((0, 3), np.int64)
    survive = (fc[:, 0] != fc[:, 1]) & (fc[:, 0] != fc[:, 2]) & (fc[:, 1] != fc[:, 2])
    assert int(survive.sum()) == len(f)
    cube = face_cubes(edges, faces_in[survive]) if survive.any() else np.zeros((0, 3), np.int64)
    held = np.zeros(((Y - 1) * (Z - 1), trips), bool)
    held[cube[:, 2] * (Y - 1) + cube[:, 1], cube[:, 0] >> 6] = True
    bits = np.zeros((Z, Y, trips), bool)
    bits[edges[:, 0], edges[:, 1], edges[:, 2] >> 6] = True
    clear = ~(bits[:-1, :-1] | bits[:-1, 1:] | bits[1:, :-1] | bits[1:, 1:]).reshape((Y - 1) * (Z - 1), trips)
    left = np.cumsum(held, axis=1) - held > 0
    right = np.cumsum(held[:, ::-1], axis=1)[:, ::-1] - held > 0
    three = held.sum(axis=1) >= 3
    out["trip_rows"] = int((three & (~held & left & right).any(axis=1)).sum())
    out["trip_rows_skipped"] = int((three & (~held & clear & left & right).any(axis=1)).sum())
    return out


def check(trk, tw, c, mode, rgb=False, tag=""):
    """one call of the context against a twin result: every array and every statistic"""
    v, f, nrm, col, st = trk.extract_mesh_simplified(cluster_voxels=c, mode=mode, normals=True, rgb=rgb)
    tag = (tag, c, mode)
    assert same_bits(v, tw["vertices"]), (tag, len(v), len(tw["vertices"]))
    assert same_normals(nrm, tw["normals"]), tag
    assert f.shape == tw["faces"].shape and np.array_equal(f, tw["faces"]), tag
    want = dict(tw["stats"])
    if rgb:
        assert np.array_equal(col, tw["rgb"]), tag
    else:
        assert col is None
        want["n_uncolored"] = 0
    assert stats_list(st) == stats_list(want), (tag, st, want)
    return v, f, st
