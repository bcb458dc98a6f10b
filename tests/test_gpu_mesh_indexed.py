"""hsk_extract_mesh_indexed on the GPU: geometry, normals and colour bit-exact against the numpy restatement
(tests/mesh_twin.py), the triangle soup recovered from the indexed form, the call protocol, the deferred weights, group slabs,
and a room scanned at 512^3 written as a coloured .ply."""
import numpy as np
import pytest

from color_cases import frame_of, run_tracker
from kit import same_bits
from mesh_cases import planted_zeros_volume, random_sign_volume, read_ply_indexed, sphere_volume
from mesh_twin import mesh_indexed, same_normals

pytestmark = pytest.mark.gpu


def edge_census(faces):
    """(directed edges' counts, undirected edges' counts) of a face list"""
    f = faces.astype(np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    n = int(f.max()) + 1 if len(f) else 1
    _, directed = np.unique(a * n + b, return_counts=True)
    _, undirected = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)
    return directed, undirected


def check_geometry(trk, vol, oracle, closed=False):
    ntri, codes = oracle.mc_table()
    v, f, nrm, col, unc = trk.extract_mesh_indexed(normals=False, rgb=False)
    assert nrm is None and col is None and unc == 0
    tw = mesh_indexed(vol, ntri, codes, normals=False)
    assert same_bits(v, tw["vertices"]), (len(v), len(tw["vertices"]))
    assert np.array_equal(f, tw["faces"])
    soup, total = trk.extract_mesh(cubes=True)
    assert len(f) == total and same_bits(v[f], soup)
    if closed:
        directed, undirected = edge_census(f)
        assert directed.max() == 1 and (undirected == 2).all()  # every edge in two faces, in opposite directions
    return v, f


@pytest.mark.parametrize("n", [96, 128])
def test_geometry_of_a_tracked_scan(oracle, hsk, synth_frames, n):
    trk = hsk.KinfuTracker(n=n)
    for k in range(6):
        trk.process_frame(synth_frames(k)[1])
    v, f = check_geometry(trk, trk.download_tsdf(), oracle)
    assert len(f) > 5000 and len(v) < 0.6 * len(f)
    trk.close()


def test_geometry_of_uploaded_volumes(oracle, hsk):
    """an analytic sphere (a closed oriented manifold), the 256-case random volume (over a million triangles), and planted
    exact zeros, 32767s and zero weights (coincident vertices stay apart)"""
    n = 96
    trk = hsk.KinfuTracker(n=n)
    sv = sphere_volume(n, 3.0, np.array([1.4, 1.6, 1.5]), 0.7, 0.12)
    sv[..., 0][sv[..., 0] == 0] = 1
    trk.upload_tsdf(sv)
    check_geometry(trk, sv, oracle, closed=True)
    noise = random_sign_volume(n)
    trk.upload_tsdf(noise)
    _, f = check_geometry(trk, noise, oracle)
    assert len(f) > 1000000
    pz = planted_zeros_volume(n)
    assert (pz[..., 0] == 0).any() and (pz[..., 0] == 32767).any() and (pz[..., 1] == 0).any()
    trk.upload_tsdf(pz)
    v, _ = check_geometry(trk, pz, oracle)
    assert len(np.unique(v.view(np.uint32).reshape(-1, 3), axis=0)) < len(v)
    trk.close()


def test_attributes_of_an_rgbd_scan(oracle, hsk):
    n = 128
    frames = [frame_of(hsk, "synth", k) for k in range(15)]
    trk, _ = run_tracker(hsk, n, frames)
    v, f, nrm, col, unc = trk.extract_mesh_indexed()
    tsdf, rgbw = trk.download_tsdf(), trk.download_color()
    ntri, codes = oracle.mc_table()
    tw = mesh_indexed(tsdf, ntri, codes, col=rgbw)
    assert same_bits(v, tw["vertices"]) and np.array_equal(f, tw["faces"])
    assert same_normals(nrm, tw["normals"]) and (~np.isnan(nrm[:, 0])).sum() > 0.9 * len(v)
    assert np.array_equal(col, tw["rgb"]) and unc == tw["n_uncolored"]
    assert (col != 0).any(axis=1).sum() > 0.9 * len(v)
    # without colour: rgb is refused, normals alone work and match
    plain, _ = run_tracker(hsk, n, frames, color=False)
    with pytest.raises(hsk.KinfuError):
        plain.extract_mesh_indexed()
    pv, pf, pn, pc, pu = plain.extract_mesh_indexed(rgb=False)
    assert pc is None and pu == 0
    assert same_bits(pv, v) and np.array_equal(pf, f) and same_normals(pn, nrm)
    trk.close()
    plain.close()


def test_call_protocol(oracle, hsk, synth_frames):
    import ctypes as C
    n = 96
    trk = hsk.KinfuTracker(n=n)
    for k in range(6):
        trk.process_frame(synth_frames(k)[1])
    lib, h = trk.lib, trk.h
    nv, nf, nu = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.hsk_extract_mesh_indexed(h, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), C.byref(nu)) == 0
    v, f, nrm, _, _ = trk.extract_mesh_indexed(rgb=False)
    assert (nv.value, nf.value) == (len(v), len(f)) and nu.value == 0
    # a short cap: an error, the counts set, the caller's buffers untouched -- for either array
    vb = np.full((len(v), 3), 7.0, np.float32)
    fb = np.full((len(f), 3), -5, np.int32)
    for cv, cf in ((len(v) - 1, len(f)), (len(v), len(f) - 1)):
        nv.value = nf.value = 0
        rc = lib.hsk_extract_mesh_indexed(h, vb.ctypes.data, None, None, cv, C.byref(nv), fb.ctypes.data, cf, C.byref(nf), None)
        assert rc == -1 and (nv.value, nf.value) == (len(v), len(f))
        assert (vb == 7.0).all() and (fb == -5).all()
    # any subset: faces alone, normals alone
    assert lib.hsk_extract_mesh_indexed(h, None, None, None, 0, C.byref(nv), fb.ctypes.data, len(fb), C.byref(nf), None) == 0
    assert np.array_equal(fb, f)
    nb = np.empty_like(nrm)
    assert lib.hsk_extract_mesh_indexed(h, None, nb.ctypes.data, None, len(nb), C.byref(nv), None, 0, C.byref(nf), None) == 0
    assert same_normals(nb, nrm)
    # repeated calls give identical output; interleaved with the other products and a further frame
    for _ in range(2):
        v2, f2, n2, _, _ = trk.extract_mesh_indexed(rgb=False)
        assert same_bits(v2, v) and np.array_equal(f2, f) and same_normals(n2, nrm)
    trk.extract_cloud()
    v3, f3, _, _, _ = trk.extract_mesh_indexed(normals=False, rgb=False)
    assert same_bits(v3, v) and np.array_equal(f3, f)
    soup, _ = trk.extract_mesh(cubes=True)
    v4, f4, _, _, _ = trk.extract_mesh_indexed(normals=False, rgb=False)
    assert same_bits(v4, v) and np.array_equal(f4, f) and same_bits(v4[f4], soup)
    trk.process_frame(synth_frames(6)[1])
    v5, f5, _, _, _ = trk.extract_mesh_indexed(normals=False, rgb=False)
    tw = mesh_indexed(trk.download_tsdf(), *oracle.mc_table(), normals=False)
    assert same_bits(v5, tw["vertices"]) and np.array_equal(f5, tw["faces"])
    trk.close()


@pytest.mark.parametrize("stream", ["scripted", "holes"])
def test_no_flush_of_the_deferred_weights(hsk, synth_frames, stream):
    n = 128 if stream == "scripted" else 256
    frames = [synth_frames(k)[1] for k in range(12)] if stream == "scripted" else hsk.synth_sensor_frames(12, absorbing=True)[1]
    trk = hsk.KinfuTracker(n=n)
    for d in frames:
        trk.process_frame(d)
    before = trk.extract_mesh_indexed(rgb=False)
    vol = trk.download_tsdf()  # (flushes)
    assert int((vol[..., 1] > 1).sum()) > 100000
    trk.upload_tsdf(vol)       # (a new volume epoch: the count pass runs again on the flushed weights)
    after = trk.extract_mesh_indexed(rgb=False)
    assert same_bits(before[0], after[0]) and np.array_equal(before[1], after[1]) and same_normals(before[2], after[2])
    assert len(before[1]) > 10000
    trk.close()


def test_group_slabs(hsk, synth_frames):
    """a 2-slab group on one device: each slab's indexed mesh expands to that slab's soup; together they hold the whole
    context's faces, and the vertices of the shared plane appear in both"""
    n = 96
    grp = hsk.KinfuGroup(hsk.default_config(n), device_ids=[0, 0])
    ref = hsk.KinfuTracker(n=n)
    for k in range(6):
        grp.process_frame(synth_frames(k)[1])
        ref.process_frame(synth_frames(k)[1])
    faces, keys = 0, []
    for i in range(grp.n_slabs()):
        s = grp.slab(i)
        with pytest.raises(hsk.KinfuError):
            s.extract_mesh_indexed()
        v, f, nrm, _, _ = s.extract_mesh_indexed(rgb=False)
        soup, total = s.extract_mesh(cubes=True)
        assert len(f) == total > 1000 and same_bits(v[f], soup) and len(nrm) == len(v)
        faces += len(f)
        keys.append({tuple(p) for p in v.view(np.uint32).tolist()})
    assert faces == ref.extract_mesh(cubes=True)[1]
    rv, _, _, _, _ = ref.extract_mesh_indexed(normals=False, rgb=False)
    whole = {tuple(p) for p in rv.view(np.uint32).tolist()}
    assert keys[0] | keys[1] == whole and len(keys[0] & keys[1]) > 10
    grp.close()
    ref.close()


def test_room_at_512_as_a_sensor_sees_it(hsk, tmp_path):
    n, scan, count = 512, 720, 120
    poses, frames = hsk.synth_sensor_frames(count, room=0, scan=scan)
    trk = hsk.KinfuTracker(n=n, init_pose=poses[0])
    trk.enable_color()
    trk.submit_frame_rgbd(frames[0], hsk.synth_rgb(poses[0], 0))
    tracked = []
    for k in range(1, count):
        trk.submit_frame_rgbd(frames[k], hsk.synth_rgb(poses[k], 0))
        tracked.append(trk.wait_frame()[1])
    tracked.append(trk.wait_frame()[1])
    assert all(tracked[1:])
    v, f, nrm, col, unc = trk.extract_mesh_indexed()
    assert len(f) > 200000 and len(v) < 0.7 * len(f)
    soup, total = trk.extract_mesh(cubes=True)
    assert total == len(f) and same_bits(v[f], soup)
    from housescan_amd import products
    path = str(tmp_path / "mesh.ply")
    products.write_ply_indexed(path, v, f, normals=nrm, rgb=col)
    _, gv, gf, gn, gc = read_ply_indexed(path)
    assert same_bits(gv, v) and np.array_equal(gf, f) and same_bits(gn, np.nan_to_num(nrm, nan=0.0)) and np.array_equal(gc, col)
    directed, undirected = edge_census(f)
    assert directed.max() == 1 and undirected.max() <= 2
    assert (col != 0).any(axis=1).sum() > 0.85 * len(v), unc
    trk.close()
