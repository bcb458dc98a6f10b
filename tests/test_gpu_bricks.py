"""The brick skip structure ("this brick has held a negative TSDF", one bit per brick and one per super-brick of 4^3 bricks) at
the shapes whose index arithmetic no cube reaches: a row of bricks that spans three flag words, exactly 64 and more than 64
bricks along x, fields longer than 1024 words, more super-bricks than super bits, slabs whose stored planes are no multiple of
a brick.  A wrong bit or a wrong index faults nothing -- a piece of surface is just not there -- so every comparison is bit for
bit against the oracle, which visits every voxel, and every case proves with the twin (tests/brick_twin.py) on the oracle's
volume that it reaches the path it is there for.  Also hsk_create's refusal of a field that does not fit the LDS."""
import numpy as np
import pytest

import brick_twin as BT
import mesh_twin as MT
from kit import assert_same_bits
from np_twin import _Grid
from view_shape_cases import BRICK_CASES as CASES, along_x, look, scene_fill

pytestmark = pytest.mark.gpu


def configs(hsk, oracle, dims, size, omp=False, **over):
    X, Y, Z = dims
    cfg_h = hsk.default_config(X, vol_y=Y, vol_z=Z, own_z1=Z, vol_size_m=size, **over)
    cfg_o = oracle.default_config(X, omp=omp, vol=dims, size=size)
    return cfg_h, cfg_o


def world_pose(world, pose):
    """the stream's camera in the volume's coordinates: p_volume = rot (p_world - origin)"""
    P = np.eye(4, dtype=np.float32)
    P[:3, :3] = world["rot"] @ pose[:3, :3]
    P[:3, 3] = world["rot"] @ (pose[:3, 3] - np.asarray(world["origin"], np.float32))
    return P


_INTEGRATED = {}


def integrated(oracle, synth_frames, case, frames=None):
    """the oracle's volume after the case's frames (computed once, then handed out read-only) -> (vol, [(depth, pose, n_upd)])"""
    c = CASES[case]
    frames = tuple(c["world"]["frames"] if frames is None else frames)
    if (case, frames) not in _INTEGRATED:
        X, Y, Z = c["dims"]
        cfg_o = oracle.default_config(X, omp=c["omp"], vol=c["dims"], size=c["size"])
        if len(frames) > 1 and (case, frames[:-1]) in _INTEGRATED:
            vol, fed = _INTEGRATED[case, frames[:-1]]
            vol, fed, todo = vol.copy(), list(fed), frames[-1:]
        else:
            vol, fed, todo = np.zeros((Z, Y, X, 2), np.int16), [], frames
        for k in todo:
            pose, depth = synth_frames(k)
            pose = world_pose(c["world"], pose)
            fed.append((depth, pose, oracle.integrate(cfg_o, vol, oracle.scale_depth(cfg_o, depth), pose, omp=c["omp"])))
        vol.setflags(write=False)
        _INTEGRATED[case, frames] = (vol, fed)
    return _INTEGRATED[case, frames]


def assert_reaches_its_path(case, vol):
    """the design of the case, on the oracle's volume alone"""
    X, Y, Z = CASES[case]["dims"]
    L = BT.layout(X, Y, Z)
    assert L["bshift"] == 3
    b = BT.brick_bits(vol, 3)
    if case == "328x40x44":
        assert len(BT.third_word_bricks(b)) > 0, "no set brick bit comes from a row's third word"
    if case == "512x64x52":
        assert L["bxn"] == 64 and b[:, :, 63].any(), "brick 63 of no row is set"
    if case in ("528x16x20", "1048x1048x12"):
        assert L["bxn"] > 64 and (vol[:, :, 512:, 0] < 0).any(), "no negative voxel at x >= 512"
    if case in ("264x264x264", "1048x1048x12"):
        assert L["words"] > 1024 and BT.set_bits_beyond_word(b, 1024) > 0, "no set brick bit beyond word 1024"
    if case == "264x264x264":
        assert L["super_ok"] and BT.field(vol)[L["words"]:].any(), "no super bit set"
    if case == "1048x1048x12":
        assert not L["super_ok"]


def reference(oracle, cfg_o, vol, case, poses, full=None, omp=None):
    """the oracle's products of `vol`, with the conditions that make the comparison worth something (on the oracle alone)"""
    c = CASES[case]
    full = c["full"] if full is None else full
    omp = c["omp"] if omp is None else omp
    X, Y, Z = c["dims"]
    ref = dict(full=full, poses=poses)
    ref["cloud"] = oracle.extract_cloud(cfg_o, vol)
    assert ref["cloud"][1] > 1000, ref["cloud"][1]
    ref["cubes"] = oracle.extract_mesh(cfg_o, vol, cubes=True)
    assert ref["cubes"][1] > 1000, ref["cubes"][1]
    if full:
        ref["tets"] = oracle.extract_mesh(cfg_o, vol)
        assert ref["tets"][1] > 1000
        ref["indexed"] = MT.mesh_indexed(vol, *oracle.mc_table(), size=c["size"], normals=False)
        with np.errstate(all="ignore"):
            ref["normals"] = MT.normal_at(_Grid(vol, c["size"], Z, 0), ref["cloud"][0], (X, Y, Z))
        assert (~np.isnan(ref["normals"][:, 0])).sum() > 500
    ref["rays"] = []
    for i, pose in enumerate(poses):
        vm, nm, keys, _ = oracle.raycast(cfg_o, vol, pose, omp=omp)
        hit = float((~np.isnan(vm[0])).mean())
        assert hit > 0.2, f"{case} pose {i}: only {hit:.3f} of the pixels hit"
        ref["rays"].append((vm, nm, keys))
    return ref


def compare(trk, ref, what):
    pts, total = trk.extract_cloud()
    assert total == ref["cloud"][1], f"{what}: cloud total {total} vs {ref['cloud'][1]}"
    assert_same_bits(pts, ref["cloud"][0], f"{what}: cloud")
    tri, nt = trk.extract_mesh(cubes=True)
    assert nt == ref["cubes"][1], f"{what}: cubes total {nt} vs {ref['cubes'][1]}"
    assert_same_bits(tri, ref["cubes"][0], f"{what}: cubes mesh")
    if ref["full"]:
        tri, nt = trk.extract_mesh()
        assert nt == ref["tets"][1], f"{what}: tetrahedra total {nt} vs {ref['tets'][1]}"
        assert_same_bits(tri, ref["tets"][0], f"{what}: tetrahedra mesh")
        v, f, _, _, _ = trk.extract_mesh_indexed(normals=False, rgb=False)
        assert_same_bits(v, ref["indexed"]["vertices"], f"{what}: indexed vertices")
        assert np.array_equal(f, ref["indexed"]["faces"]), f"{what}: indexed faces"
        xyz, nrm, _, n_attr, _ = trk.extract_cloud_attrs(rgb=False)
        assert n_attr == ref["cloud"][1]
        assert_same_bits(xyz, ref["cloud"][0], f"{what}: attribute pass points")
        assert_same_bits(nrm, ref["normals"], f"{what}: normals")
    for i, (pose, (ovm, onm, okeys)) in enumerate(zip(ref["poses"], ref["rays"])):
        vm, nm, keys = trk.raycast(pose, want_keys=True)
        assert np.array_equal(keys, okeys), f"{what} pose {i}: step keys differ at {int((keys != okeys).sum())} pixels"
        assert_same_bits(vm, ovm, f"{what} pose {i}: vmap")
        assert_same_bits(nm, onm, f"{what} pose {i}: nmap")


# ---- A: the shape matrix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["upload", "integrate"])
@pytest.mark.parametrize("case", list(CASES))
def test_shape_matrix(hsk, oracle, synth_frames, case, fill):
    """the flags from k_rebuild_flags (an uploaded scene) and from integrate's pass B (frames of the synthetic stream): cloud,
    both meshes, indexed mesh, normals and three raycasts with their step keys are the oracle's (the two large shapes: cloud,
    cubes mesh and raycasts, OpenMP oracle)"""
    c = CASES[case]
    cfg_h, cfg_o = configs(hsk, oracle, c["dims"], c["size"], c["omp"])
    trk = hsk.KinfuTracker(cfg_h)
    if fill == "upload":
        vol = scene_fill(c["dims"], c["size"], **c["scene"])
        trk.upload_tsdf(vol)
    else:
        vol, fed = integrated(oracle, synth_frames, case)
        for depth, pose, n_upd in fed:
            assert trk.count_updates(depth, pose) == n_upd
            trk.integrate(depth, pose)
        assert_same_bits(trk.download_tsdf(), vol, f"{case}: tsdf")
    assert_reaches_its_path(case, vol)
    compare(trk, reference(oracle, cfg_o, vol, case, c["poses"][fill]), f"{case} {fill}")
    trk.close()


# ---- B: lone negative voxels ----------------------------------------------------------------------------------------------------
# (z, y, x) of single voxels with F = -0.5 in a volume of F = +0.5: the corners (0, 0, 0) and (7, 7, 7) of bricks at the edges of
# the index arithmetic, and two voxels in the top plane
LONE = {
    (328, 40, 44): dict(size=(3.0, 1.08, 1.18), inner=[
        (15, 15, 63), (24, 24, 64),        # either side of the 64-cell segment edge
        (7, 23, 31), (16, 8, 32),          # either side of a super-brick edge
        (8, 24, 320),                      # the last brick of a row
        (40, 16, 80),                      # plane Z - 4: the first of the last, short brick layer
        (15, 23, 7), (8, 16, 8),           # row (1, 2) starts at bit 287: bit 31 of word 8, then bit 0 of word 9
        (8, 16, 288), (15, 23, 303),       # the same row's bricks 36 and 37: their bits come from the row's third word
        (40, 24, 304),                     # row (5, 3), first bit 28 of its word: brick 38 from the third word, in plane Z - 4
    ], top=[(43, 12, 100), (43, 28, 200)]),
    (96, 96, 52): dict(size=(3.0, 3.0, 1.625), inner=[
        (15, 15, 63), (24, 24, 64),
        (7, 23, 31), (16, 8, 32),
        (8, 24, 88),                       # the last brick of a row
        (48, 16, 40),                      # plane Z - 4
        (8, 48, 56), (15, 55, 71),         # row (1, 6) starts at bit 216: its brick 7 is bit 31 of word 6, brick 8 bit 0 of word 7
    ], top=[(51, 60, 20), (51, 30, 70)]),
}


def lone_volume(dims):
    X, Y, Z = dims
    spec = LONE[dims]
    vol = np.empty((Z, Y, X, 2), np.int16)
    vol[..., 0], vol[..., 1] = 16384, 1
    pts = np.array(spec["inner"] + spec["top"])
    vol[pts[:, 0], pts[:, 1], pts[:, 2], 0] = -16384
    return vol, pts


@pytest.mark.parametrize("dims", list(LONE))
def test_lone_negative_voxels(hsk, oracle, dims):
    """three of a lone voxel's six crossings and seven of the eight cubes round it belong to cells of neighbouring bricks that
    are clear: a sweep that consulted only a cell's own brick would lose them.  The totals are known without the oracle: six
    crossings and eight one-triangle cubes per interior voxel, five and four for a voxel in the top plane."""
    X, Y, Z = dims
    spec = LONE[dims]
    vol, pts = lone_volume(dims)
    inner, top = spec["inner"], spec["top"]
    # the design: where the voxels sit
    assert Z % 8 != 0 and all(z == Z - 1 for z, _, _ in top)
    assert all(0 < z < Z - 1 and 0 < y < Y - 1 and 0 < x < X - 1 for z, y, x in inner) and all(0 < y < Y - 1 and 0 < x < X - 1 for _, y, x in top)
    assert all(p[0] % 8 == p[1] % 8 == p[2] % 8 and p[0] % 8 in (0, 7) for p in inner)
    d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)
    assert d[~np.eye(len(pts), dtype=bool)].min() >= 3
    xs = {p[2] for p in inner}
    assert {63, 64, 31, 32} <= xs and any(p[2] >> 3 == (X >> 3) - 1 for p in inner) and any(p[0] == Z - 4 for p in inner)
    L = BT.layout(X, Y, Z)
    bit = [((z >> 3) * L["byn"] + (y >> 3)) * L["bxn"] + (x >> 3) for z, y, x in inner]
    assert any(b & 31 == 31 for b in bit) and any(b & 31 == 0 for b in bit)
    b = BT.brick_bits(vol, 3)
    assert b.sum() == len(pts)                         # a brick each
    if X == 328:
        assert len(BT.third_word_bricks(b)) >= 2
    cfg_h, cfg_o = configs(hsk, oracle, dims, spec["size"])
    trk = hsk.KinfuTracker(cfg_h)
    trk.upload_tsdf(vol)
    cell = np.array(spec["size"]) / np.array(dims)
    target = (np.array(inner[1][::-1]) + 0.5) * cell    # (x, y, z) metres of a voxel: seen straight on from 0.5 m
    poses = [look(target - [0, 0, 0.5], target, (0, 1, 0)), look(np.array(spec["size"]) * [0.1, 0.3, 0.2], (np.array(inner[-1][::-1]) + 0.5) * cell),
             along_x((0.05, (inner[0][1] + 0.5) * cell[1], (inner[0][0] + 0.5) * cell[2]))]
    opts, ototal = oracle.extract_cloud(cfg_o, vol)
    assert ototal == 6 * len(inner) + 5 * len(top)
    pts_g, total = trk.extract_cloud()
    assert total == 6 * len(inner) + 5 * len(top)
    assert_same_bits(pts_g, opts, "lone voxels: cloud")
    for cubes in (True, False):
        otri, ont = oracle.extract_mesh(cfg_o, vol, cubes=cubes)
        tri, nt = trk.extract_mesh(cubes=cubes)
        assert nt == ont and (not cubes or nt == 8 * len(inner) + 4 * len(top)), (cubes, nt, ont)
        assert_same_bits(tri, otri, f"lone voxels: mesh (cubes={cubes})")
    tw = MT.mesh_indexed(vol, *oracle.mc_table(), size=spec["size"], normals=False)
    v, f, _, _, _ = trk.extract_mesh_indexed(normals=False, rgb=False)
    assert len(f) == 8 * len(inner) + 4 * len(top) and len(v) == 6 * len(inner) + 5 * len(top)
    assert_same_bits(v, tw["vertices"], "lone voxels: indexed vertices")
    assert np.array_equal(f, tw["faces"])
    for i, pose in enumerate(poses):
        vm, nm, keys = trk.raycast(pose, want_keys=True)
        ovm, onm, okeys, _ = oracle.raycast(cfg_o, vol, pose)
        assert np.array_equal(keys, okeys), f"lone voxels pose {i}: keys differ at {int((keys != okeys).sum())} pixels"
        assert_same_bits(vm, ovm, f"lone voxels pose {i}: vmap")
        assert_same_bits(nm, onm, f"lone voxels pose {i}: nmap")
    trk.close()


# ---- C: grown flags against rebuilt flags --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["328x40x44", "1048x1048x12"])
def test_grown_flags_against_rebuilt_flags(hsk, oracle, synth_frames, case):
    """a context that integrated four frames holds every brick that EVER held a negative voxel; a fresh context handed its volume
    rebuilds the bricks that hold one now -- a subset.  Their products are each other's and the oracle's; and again after one
    more frame in both, marked on top of the grown and of the rebuilt field."""
    c = CASES[case]
    base = tuple(c["world"]["frames"])
    five = (base + (30, 40, 50))[:5]
    cfg_h, cfg_o = configs(hsk, oracle, c["dims"], c["size"], c["omp"])
    poses = c["poses"]["integrate"][:2]
    a, b = hsk.KinfuTracker(cfg_h), hsk.KinfuTracker(cfg_h)
    for n in range(len(base), 5):          # (the shape matrix's volume, then a frame at a time)
        vol, fed = integrated(oracle, synth_frames, case, five[:n])
    assert len(fed) == 4
    for depth, pose, _ in fed:
        a.integrate(depth, pose)
    got = a.download_tsdf()
    assert_same_bits(got, vol, f"{case}: tsdf after four frames")
    b.upload_tsdf(got)
    ref = reference(oracle, cfg_o, vol, case, poses, full=False)
    compare(a, ref, f"{case} grown")
    compare(b, ref, f"{case} rebuilt")
    vol, fed = integrated(oracle, synth_frames, case, five)
    depth, pose, _ = fed[-1]
    a.integrate(depth, pose)
    b.integrate(depth, pose)
    assert_same_bits(a.download_tsdf(), vol, f"{case}: tsdf after five frames")
    assert_same_bits(b.download_tsdf(), vol, f"{case}: tsdf after upload and a fifth frame")
    ref = reference(oracle, cfg_o, vol, case, poses, full=False)
    compare(a, ref, f"{case} grown, one more frame")
    compare(b, ref, f"{case} rebuilt, one more frame")
    a.close()
    b.close()


# ---- D: the LDS bound -----------------------------------------------------------------------------------------------------------
def test_create_refuses_a_field_that_does_not_fit_the_lds(hsk):
    """648^3 (1.0 GiB) stays at 8^3 bricks -- 648 is 8 mod 16 -- and its staged field is 66560 B: refused before anything is
    allocated, with the remedy; so is 888^3, beyond what a block of any device here gets.  328 x 40 x 44 (288 B) is created.  No
    kernel is launched at a refused shape."""
    for n in (648, 888):
        assert BT.bshift_of(n, n, n) == 3 and BT.flag_words_total(n, n, n, 3) * 4 > 64 * 1024
        with pytest.raises(hsk.KinfuError, match=r"brick bitfield.*multiples of 16, or the next power of two"):
            hsk.KinfuTracker(n=n)
    trk = hsk.KinfuTracker(hsk.default_config(328, vol_y=40, vol_z=44, own_z1=44, vol_size_m=(3.0, 1.08, 1.18)))
    assert trk.stored_nz == 44
    trk.close()


# ---- E: slabs ---------------------------------------------------------------------------------------------------------------------
def test_slabs_whose_planes_are_no_multiple_of_a_brick(hsk, synth_frames):
    """a two-slab group at 328 x 40 x 44 fed case A's integrated frames: the second slab's stored planes start off zero, and
    neither slab stores a multiple of 8 planes.  The slabs' clouds and cubes meshes, one behind the other, are the single
    context's."""
    c = CASES["328x40x44"]
    frames = [synth_frames(k) for k in c["world"]["frames"]]
    start = world_pose(c["world"], frames[0][0])
    X, Y, Z = c["dims"]
    kw = dict(vol_y=Y, vol_z=Z, own_z1=Z, vol_size_m=c["size"], init_pose=start)
    grp = hsk.KinfuGroup(hsk.default_config(X, **kw), device_ids=[0, 0])
    ref = hsk.KinfuTracker(hsk.default_config(X, **kw))
    for _, depth in frames:
        pg, okg = grp.process_frame(depth)
        pr, okr = ref.process_frame(depth)
        assert okg == okr
        assert_same_bits(pg, pr, "group pose")
    slabs = [grp.slab(i) for i in range(grp.n_slabs())]
    assert len(slabs) == 2 and slabs[1].stored_z0 > 0 and slabs[1].stored_z0 % 8 != 0
    assert all(s.stored_nz % 8 != 0 and s.stored_nz < Z for s in slabs)
    cloud, total = ref.extract_cloud()
    tri, nt = ref.extract_mesh(cubes=True)
    assert total > 1000 and nt > 1000
    parts = [s.extract_cloud() for s in slabs]
    assert sum(p[1] for p in parts) == total
    assert_same_bits(np.concatenate([p[0] for p in parts]), cloud, "slab clouds")
    parts = [s.extract_mesh(cubes=True) for s in slabs]
    assert sum(p[1] for p in parts) == nt
    assert_same_bits(np.concatenate([p[0] for p in parts]), tri, "slab cubes meshes")
    grp.close()
    ref.close()
