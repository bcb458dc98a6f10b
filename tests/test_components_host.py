"""Surface components without a GPU: the numpy twin (tests/components_twin.py) pinned by hand-written cases (and cross-checked with
scipy.ndimage.label where that happens to import); the kernels' shared text (housescan_amd/csrc/hsk_comp_point.h) compiled for the
host with the sanitizers, labelling sequentially, against the twin -- labels and records, zero differences; the twin's prune rule;
the default min_voxels arithmetic; ties in the record order; keep_largest with equal sizes at the cut; the C layout of the new
structs and their Python mirror; the argument errors that need no device.  The volumes built here are the GPU tests' too."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import components_twin as KT
import kit
import np_twin as T
from align_cases import TAU
from components_cases import BLOBS, IN, empty, fill, injected_volume, shapes, speckled, twin_of
from cover_cases import carved_volume
from kit import blocked

f32 = np.float32


def host_cases():
    cases = {name: v for name, (v, _) in shapes().items()}
    cases["injected"] = injected_volume()[0]
    cases["speckled 46 planes"] = speckled(carved_volume(), 46)[:46]
    sp = speckled(carved_volume(), 40)
    cases["speckled 72 x 56 x 40"] = np.ascontiguousarray(sp[:40, :56, :72])
    return cases


# ---- 1. the twin itself --------------------------------------------------------------------------------------------------------
def test_the_twin_on_hand_written_cases():
    v = empty((8, 8, 4))
    fill(v, 1, 2, slice(1, 4))                 # a bar of three: lin 81, 82, 83 (X = 8, Y = 8: lin = (z 8 + y) 8 + x)
    fill(v, 2, 2, 3)                           # ... and the voxel above its end: lin 147
    fill(v, 0, 0, 0)                           # a single voxel at the origin
    fill(v, 3, 7, 7), fill(v, 3, 6, 6)         # two voxels in diagonal contact: two components
    fill(v, 1, 5, 5, (0, 9)), fill(v, 1, 5, 6, (-7, 0)), fill(v, 1, 5, 4, (5, 9))   # tsdf 0, weight 0, positive: no members
    lab = KT.labels(v)
    assert lab.dtype == np.uint32 and lab.shape == (4, 8, 8)
    want = np.full((4, 8, 8), KT.NONE, np.uint32)
    want[1, 2, 1:4] = 81
    want[2, 2, 3] = 81
    want[0, 0, 0] = 0
    want[3, 7, 7] = 255
    want[3, 6, 6] = 246
    assert np.array_equal(lab, want)
    rec = KT.records(v)
    assert rec["n_voxels"].tolist() == [4, 1, 1, 1] and rec["root"].tolist() == [[1, 2, 1], [0, 0, 0], [6, 6, 3], [7, 7, 3]]
    assert rec["lo"][0].tolist() == [1, 2, 1] and rec["hi"][0].tolist() == [4, 3, 3]
    assert KT.stats(rec) == {"n_components": 4, "n_inside": 7, "largest": 4}
    for name, (vol, n) in shapes().items():
        lab, rec = twin_of(name, vol)
        assert len(rec) == n, name
        m = KT.inside(vol)
        assert ((lab != KT.NONE) == m).all() and int(rec["n_voxels"].sum()) == int(m.sum())
        if n:
            assert np.array_equal(np.unique(lab[m]), np.sort(KT.root_lin(rec, vol.shape[2::-1]).astype(np.uint32)))
    assert twin_of("snake", None)[1]["n_voxels"][0] == 4 * (32 * 62 + 31) + 3 * 7 and twin_of("every voxel", None)[1]["n_voxels"][0] == 32 * 24 * 12


def test_the_twin_against_scipy_where_it_imports():
    try:
        from scipy import ndimage
    except ImportError:
        return
    for name, vol in host_cases().items():
        lab = twin_of(name, vol)[0]
        ref, n = ndimage.label(KT.inside(vol), structure=ndimage.generate_binary_structure(3, 1))
        assert n == len(twin_of(name, vol)[1]), name
        lin = np.arange(lab.size).reshape(lab.shape)
        if n:
            smallest = ndimage.minimum(lin, ref, np.arange(1, n + 1)).astype(np.uint32)
            assert np.array_equal(lab[ref > 0], smallest[ref[ref > 0] - 1]), name
        assert (lab[ref == 0] == KT.NONE).all()


# ---- 2. the kernels' shared text on the host ------------------------------------------------------------------------------------
def test_the_kernels_find_and_unite_equal_the_twin_on_the_host(tmp_path):
    """hsk_comp_point.h built for the host with the address and undefined-behaviour sanitizers (their runtime linked into the
    program), labelling sequentially with the plain minimum: labels and records against the twin, zero differences"""
    exe = kit.build_harness("comp_point", tmp_path)
    for name, vol in host_cases().items():
        Z, Y, X = vol.shape[:3]
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(src, "wb") as f:
            f.write(np.array([X, Y, Z], np.int32).tobytes())
            f.write(blocked(vol).tobytes())
        kit.run_harness(exe, src, dst)
        raw = open(dst, "rb").read()
        lab = np.frombuffer(raw, np.uint32, X * Y * Z).reshape(Z, Y, X)
        n = int(np.frombuffer(raw, np.uint32, 1, X * Y * Z * 4)[0])
        rec = np.frombuffer(raw, KT.COMPONENT_DTYPE, n, X * Y * Z * 4 + 4)
        ref_lab, ref_rec = twin_of(name, vol)
        print(f"{name}: {n} components, the largest {int(rec['n_voxels'][0]) if n else 0}")
        assert int((lab != ref_lab).sum()) == 0, name
        assert n == len(ref_rec) and np.array_equal(rec, ref_rec), name
    assert len(twin_of("speckled 46 planes", None)[1]) > 2000


# ---- 3. the prune rule, the order of the records ---------------------------------------------------------------------------------
def blocks_volume():
    """four blocks of 8, 8, 12 and 27 voxels and a single voxel, far apart; the two of 8 tie, the smaller root first"""
    v = empty((16, 16, 8))
    fill(v, slice(0, 2), slice(0, 2), slice(0, 2))            # 8, root lin 0
    fill(v, slice(0, 2), slice(8, 10), slice(8, 10))          # 8, root (8, 8, 0)
    fill(v, slice(4, 6), slice(0, 2), slice(8, 11))           # 12
    fill(v, slice(4, 7), slice(8, 11), slice(0, 3))           # 27
    fill(v, 7, 15, 15, (-1, 1))                               # 1
    return v


def test_ties_in_the_record_order_and_keep_largest_at_the_cut():
    v = blocks_volume()
    rec = KT.records(v)
    assert rec["n_voxels"].tolist() == [27, 12, 8, 8, 1] and rec["root"][2:4].tolist() == [[0, 0, 0], [8, 8, 0]]
    assert KT.pruned_mask(rec, 9, 0).tolist() == [False, False, True, True, True]
    assert KT.pruned_mask(rec, 8, 0).tolist() == [False, False, False, False, True]          # n_voxels < min_voxels, strictly
    assert KT.pruned_mask(rec, 0, 3).tolist() == [False, False, False, True, True]           # equal sizes at the cut: the smaller root stays
    assert KT.pruned_mask(rec, 10, 4).tolist() == [False, False, True, True, True]
    assert not KT.pruned_mask(rec, 0, 0).any()
    colour = np.full(v.shape[:3] + (4,), 9, np.uint8)
    out, col, st = KT.prune(v, colour, min_voxels=0, keep_largest=3)
    assert st == {"n_components": 5, "n_pruned": 2, "n_pruned_voxels": 9, "n_kept_voxels": 47}
    gone = np.zeros(v.shape[:3], bool)
    gone[0:2, 8:10, 8:10] = True
    gone[7, 15, 15] = True
    assert (out[gone] == 0).all() and np.array_equal(out[~gone], v[~gone]) and (col[gone] == 0).all() and (col[~gone] == 9).all()
    free, _, st2 = KT.prune(v, None, min_voxels=9, keep_largest=0, fill=KT.FREE)
    assert st2["n_pruned"] == 3 and (free[7, 15, 15] == (32767, 1)).all() and (free[0, 0, 0] == (32767, 3)).all() and (free[4, 0, 8] == IN).all()
    same, _, st3 = KT.prune(v, None)
    assert st3["n_pruned"] == 0 and np.array_equal(same, v)


def test_the_injected_blobs_are_below_the_default_min_voxels_and_the_walls_above():
    """the condition of the GPU prune tests' input, on the twin; and what pruning is for: the cloud of the pruned volume is the
    cloud of the room that never had the blobs (np_twin.extract_cloud: a crossing needs a negative, observed partner)"""
    vol, cores = injected_volume()
    lab, rec = twin_of("injected", vol)
    base_rec = KT.records(carved_volume())
    mv = KT.default_min_voxels(AT.DST_SIZE, AT.DST_DIMS, TAU)
    assert mv == 1318               # ceil(0.525^3 / (0.0375 * 0.046875 * 0.0625)) = ceil(1317.12)
    assert len(rec) == len(base_rec) + len(BLOBS)
    sizes = []
    for core in cores:
        roots = np.unique(lab[core])
        assert len(roots) == 1 and int((lab == roots[0]).sum()) == int(core.sum()), "a blob is one component of its own"
        sizes.append(int(core.sum()))
    print(f"blobs {sizes}, walls {base_rec['n_voxels'].tolist()}, min_voxels {mv}")
    assert all(30 <= s <= 400 for s in sizes) and (base_rec["n_voxels"] > mv).all()
    out, _, st = KT.prune(vol, None, min_voxels=mv)
    assert st["n_pruned"] == len(BLOBS) and st["n_pruned_voxels"] == sum(sizes)
    assert np.array_equal(T.extract_cloud(out, AT.DST_SIZE), T.extract_cloud(carved_volume(), AT.DST_SIZE))
    assert len(T.extract_cloud(vol, AT.DST_SIZE)) > len(T.extract_cloud(out, AT.DST_SIZE))


# ---- 4. the default min_voxels, header, C layout, Python mirror, errors without a device ----------------------------------------
def test_default_prune_params_without_a_context(hsk):
    cfg = hsk.default_config(256)
    p = hsk.default_prune_params()
    tau = T.tau_of(tuple(cfg.vol_size_m), (cfg.vol_x, cfg.vol_y, cfg.vol_z), cfg.trunc_dist_m)
    assert p.min_voxels == KT.default_min_voxels(tuple(cfg.vol_size_m), (cfg.vol_x, cfg.vol_y, cfg.vol_z), tau) == 1074
    assert (p.keep_largest, p.fill) == (0, hsk._lib.HSK_PRUNE_UNSEEN)
    assert KT.default_min_voxels((3.0, 3.0, 3.0), (512, 512, 512), 0.03) == int(np.ceil((4.0 * float(f32(0.03))) ** 3 / float(f32(3.0) / f32(512)) ** 3))
    q = hsk.default_prune_params(min_voxels=5, keep_largest=2, fill=1)
    assert (q.min_voxels, q.keep_largest, q.fill) == (5, 2, 1)
    with pytest.raises(TypeError, match="no field"):
        hsk.default_prune_params(size=3)
    hsk._lib.load().hsk_default_prune_params(None, None)


def test_component_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    K, S, P, R = _lib.HskComponent, _lib.HskComponentStats, _lib.HskPruneParams, _lib.HskPruneStats
    assert C.sizeof(K) == 48 and hsk.kinfu.COMPONENT_DTYPE.itemsize == 48 and KT.COMPONENT_DTYPE == hsk.kinfu.COMPONENT_DTYPE
    assert (KT.NONE, KT.UNSEEN, KT.FREE) == (_lib.HSK_COMPONENT_NONE, _lib.HSK_PRUNE_UNSEEN, _lib.HSK_PRUNE_FREE) == (hsk.kinfu.COMPONENT_NONE, hsk.kinfu.PRUNE_UNSEEN, hsk.kinfu.PRUNE_FREE)
    assert tuple(n for n, _ in P._fields_) == hsk.kinfu.PRUNE_FIELDS


def test_null_contexts_are_refused(hsk):
    lib, L = hsk._lib.load(), hsk._lib
    n = C.c_size_t(77)
    st = L.HskComponentStats(n_inside=77)
    rec = np.full(2, 7, KT.COMPONENT_DTYPE)
    assert lib.hsk_label_components(None, rec.ctypes.data_as(C.POINTER(L.HskComponent)), 2, C.byref(n), C.byref(st)) == -1
    assert n.value == 77 and st.n_inside == 77 and (rec == np.full(1, 7, KT.COMPONENT_DTYPE)[0]).all()
    lab = np.full(4, 9, np.uint32)
    assert lib.hsk_download_components(None, lab.ctypes.data) == -1 and (lab == 9).all()
    ps = L.HskPruneStats(n_pruned=77)
    assert lib.hsk_prune_components(None, None, C.byref(ps)) == -1 and ps.n_pruned == 77
    for name in ("label_components", "download_components", "prune_components", "default_prune_params"):
        assert callable(getattr(hsk.KinfuTracker, name))
