"""The indexed marching-cubes mesh on the CPU: the numpy restatement (tests/mesh_twin.py) pinned against the oracle's triangle
soup and the host weld, the indexed .ply writer, and hsk_transform_normals."""
import ctypes as C
import os

import numpy as np
import pytest

from housescan_amd import _lib, products

from kit import same_bits
from mesh_cases import planted_zeros_volume, random_sign_volume, read_ply_indexed, sphere_volume
from mesh_twin import mesh_indexed

f32 = np.float32


def rough_volume(m, seed=7):
    """a smoothed random field with every kind of ambiguous face, no exact zeros, closed off at the border"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((m, m, m))
    for _ in range(2):
        f = (f + np.roll(f, 1, 0) + np.roll(f, 1, 1) + np.roll(f, 1, 2)) / 4
    f = f / np.abs(f).max()
    f[[0, -1], :, :] = f[:, [0, -1], :] = f[:, :, [0, -1]] = 1.0
    vol = np.zeros((m, m, m, 2), np.int16)
    vol[..., 0] = np.where(f < 0, np.minimum(np.rint(f * 30000), -1), np.maximum(np.rint(f * 30000), 1)).astype(np.int16)
    vol[..., 1] = 3
    return vol


def no_zero_sphere(n):
    v = sphere_volume(n, 3.0, np.array([1.4, 1.6, 1.5]), 0.7, 0.12)
    v[..., 0][v[..., 0] == 0] = 1
    return v


def unique_rows(p):
    return np.unique(np.ascontiguousarray(p).view(np.uint32).reshape(-1, 3), axis=0)


@pytest.mark.parametrize("kind", ["sphere", "rough", "cases256"])
def test_twin_matches_the_oracle_soup_and_the_weld(oracle, hsk, kind):
    n = {"sphere": 96, "rough": 128, "cases256": 96}[kind]
    vol = {"sphere": lambda: no_zero_sphere(n), "rough": lambda: rough_volume(n), "cases256": lambda: random_sign_volume(n)}[kind]()
    assert not (vol[..., 0] == 0).any()
    ntri, codes = oracle.mc_table()
    cfg = oracle.default_config(n)
    soup, total = oracle.extract_mesh(cfg, vol, cubes=True)
    tw = mesh_indexed(vol, ntri, codes, normals=False)
    assert len(tw["faces"]) == total > 1000
    if kind == "cases256":
        assert total > 1000000
    assert same_bits(tw["vertices"][tw["faces"]], soup)
    # every vertex is used, and the vertex order is the edges' order (plane, row, x, axis)
    assert np.array_equal(np.unique(tw["faces"]), np.arange(len(tw["vertices"])))
    e = tw["edges"]
    key = ((e[:, 0] * n + e[:, 1]) * n + e[:, 2]) * 3 + e[:, 3]
    assert np.all(np.diff(key) > 0)
    # no exact zeros and cells of 96^3 / 128^3: no two edges share coordinates -- the host weld finds the same vertices
    wv, widx = products.weld_triangles(soup)
    assert len(wv) == len(tw["vertices"])
    assert np.array_equal(unique_rows(wv), unique_rows(tw["vertices"]))


def test_twin_with_planted_zeros_keeps_coincident_edges_apart(oracle, hsk):
    n = 64
    vol = planted_zeros_volume(n)
    ntri, codes = oracle.mc_table()
    soup, total = oracle.extract_mesh(oracle.default_config(n), vol, cubes=True)
    tw = mesh_indexed(vol, ntri, codes, normals=False)
    assert same_bits(tw["vertices"][tw["faces"]], soup)
    wv, _ = products.weld_triangles(soup)
    nv = len(tw["vertices"])
    assert nv > len(wv)                                         # the planted zeros do make edges meet on grid points
    u, cnt = np.unique(tw["vertices"].view(np.uint32).reshape(-1, 3), axis=0, return_counts=True)
    assert len(u) == len(wv) and np.array_equal(u, unique_rows(wv))
    # every surplus vertex shares its coordinates with another one, and they sit on grid points (a stored 0)
    assert nv - len(u) == int((cnt - 1).sum())
    shared = u[cnt > 1].view(f32)
    cell = f32(3.0) / f32(n)
    g = shared / cell - 0.5
    assert np.allclose(g, np.rint(g), atol=1e-3)


# ---- the .ply writer -----------------------------------------------------------------------------------------------
def small_mesh():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], f32)
    f = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 0]], np.int32)
    n = np.array([[0, 0, 1], [np.nan, np.nan, np.nan], [0, 0.6, 0.8], [1, 0, 0]], f32)
    c = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]], np.uint8)
    return v, f, n, c


@pytest.mark.parametrize("with_n,with_c", [(False, False), (True, False), (False, True), (True, True)])
def test_ply_indexed_layout_and_roundtrip(tmp_path, with_n, with_c):
    v, f, n, c = small_mesh()
    path = str(tmp_path / "m.ply")
    products.write_ply_indexed(path, v, f, normals=n if with_n else None, rgb=c if with_c else None)
    want_head = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                 + ("property float nx\nproperty float ny\nproperty float nz\n" if with_n else "")
                 + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if with_c else "")
                 + "element face 3\nproperty list uchar int vertex_indices\nend_header\n").encode()
    raw = open(path, "rb").read()
    assert raw.startswith(want_head)
    assert len(raw) == len(want_head) + 4 * (12 + (12 if with_n else 0) + (3 if with_c else 0)) + 13 * 3
    head, gv, gf, gn, gc = read_ply_indexed(path)
    assert head == want_head and same_bits(gv, v) and np.array_equal(gf, f)
    if with_n:
        assert same_bits(gn, np.nan_to_num(n, nan=0.0))               # NaN components written as 0
    else:
        assert gn is None
    if with_c:
        assert np.array_equal(gc, c)
    else:
        assert gc is None


def test_ply_indexed_errors_and_empty(tmp_path):
    lib = _lib.load()
    v, f, n, c = small_mesh()
    for bad in ([[0, 1, 4]], [[0, -1, 2]]):
        path = tmp_path / "bad.ply"
        fb = np.array(bad, np.int32)
        rc = lib.hsk_write_ply_indexed(os.fsencode(str(path)), v.ctypes.data, None, None, len(v), fb.ctypes.data, len(fb))
        assert rc == -1 and not path.exists()                           # HSK_ERR_ARG, no file
        with pytest.raises(RuntimeError):
            products.write_ply_indexed(str(path), v, fb)
        assert not path.exists()
    rc = lib.hsk_write_ply_indexed(os.fsencode(str(tmp_path / "nodir" / "m.ply")), v.ctypes.data, None, None, len(v), f.ctypes.data, len(f))
    assert rc == -3                                                     # HSK_ERR_STATE: the file cannot be created
    products.write_ply_indexed(str(tmp_path / "empty.ply"), np.zeros((0, 3), f32), np.zeros((0, 3), np.int32),
                               normals=np.zeros((0, 3), f32), rgb=np.zeros((0, 3), np.uint8))
    head, gv, gf, gn, gc = read_ply_indexed(str(tmp_path / "empty.ply"))
    assert b"element vertex 0\n" in head and b"element face 0\n" in head and len(gv) == len(gf) == len(gn) == len(gc) == 0
    assert os.path.getsize(tmp_path / "empty.ply") == len(head)
    # a null path, null arrays with non-zero counts
    assert lib.hsk_write_ply_indexed(None, v.ctypes.data, None, None, len(v), f.ctypes.data, len(f)) == -1
    assert lib.hsk_write_ply_indexed(os.fsencode(str(tmp_path / "x.ply")), None, None, None, 4, None, 0) == -1


def test_extract_mesh_indexed_rejects_null_arguments():
    lib = _lib.load()
    nv, nf = C.c_size_t(), C.c_size_t()
    assert lib.hsk_extract_mesh_indexed(None, None, None, None, 0, C.byref(nv), None, 0, C.byref(nf), None) == -1


# ---- hsk_transform_normals ------------------------------------------------------------------------------------------
def test_transform_normals_bitwise_and_in_place():
    rng = np.random.default_rng(3)
    nrm = rng.standard_normal((5000, 3)).astype(f32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[::97] = np.nan
    a = rng.standard_normal(3)
    c, s = np.cos(a), np.sin(a)
    R = (np.array([[c[0], -s[0], 0], [s[0], c[0], 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, c[1], -s[1]], [0, s[1], c[1]]])
         @ np.array([[c[2], 0, s[2]], [0, 1, 0], [-s[2], 0, c[2]]]))
    m = np.eye(4, dtype=f32)
    m[:3, :3] = R
    m[:3, 3] = [4.5, -2.0, 7.25]                                         # the translation is not applied
    x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    want = np.stack([(m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z for r in range(3)], axis=1).astype(f32)
    got = products.transform_normals(nrm, m)
    assert same_bits(got, want)
    assert np.isnan(got[::97]).all() and not np.isnan(np.delete(got, np.s_[::97], axis=0)).any()
    assert np.allclose(np.linalg.norm(np.delete(got, np.s_[::97], axis=0), axis=1), 1.0, atol=1e-5)
    # the positions' transform is the same matrix with the translation (hsk_transform_cloud)
    assert np.allclose(products.transform_cloud(np.nan_to_num(nrm), m) - m[:3, 3], products.transform_normals(np.nan_to_num(nrm), m), atol=1e-5)
    # in place (out aliases n)
    lib = _lib.load()
    buf = nrm.copy()
    mm = np.ascontiguousarray(m.reshape(16))
    assert lib.hsk_transform_normals(buf.ctypes.data, len(buf), mm.ctypes.data_as(C.POINTER(C.c_float)), buf.ctypes.data) == 0
    assert same_bits(buf, want)
    assert lib.hsk_transform_normals(None, 3, mm.ctypes.data_as(C.POINTER(C.c_float)), buf.ctypes.data) == -1
