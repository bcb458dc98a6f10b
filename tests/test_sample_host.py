"""The TSDF sample at a point without a GPU: housescan_amd/csrc/hsk_sample.h -- the text the raycast, the normals of the cloud and
the mesh, and alignment sample the volume with -- built for the host (tests/sample_harness.cpp) and compared bit for bit with the
three numpy twins that restate it: np_twin._Grid.trilinear (the raycast), fuse_twin.sample (fusion) and align_twin.probe
(alignment).  The volume is the alignment tests' scene, 80 x 64 x 48 over 3 m: three different cells, weights 0 present."""

import numpy as np
import pytest

import align_twin as AT
import fuse_twin as FT
import kit
import np_twin as T
from align_cases import M_TRUE, scene
from kit import blocked

f32 = np.float32
DIMS, SIZE = AT.DST_DIMS, AT.DST_SIZE
CELL = AT.cells(DIMS, SIZE)


def points():
    """the point set, [n, 3] binary32: every class the sample treats differently, on every axis"""
    rng = np.random.default_rng(7)
    vol, ps, ns = scene()
    M = M_TRUE
    surf = (ps.astype(np.float64) @ M[:3, :3].T + M[:3, 3])            # the scene's surfaces, in the volume's coordinates
    dims, cell = np.array(DIMS), np.array([float(c) for c in CELL])
    inner = lambda n: rng.uniform(1.5, dims - 1.5, (n, 3)) * cell      # noqa: E731  (well inside)
    out = [surf + rng.normal(0, 0.04, surf.shape), inner(2000)]
    for i in range(3):
        g = rng.integers(1, dims[i] - 1, 300)
        p = inner(300).astype(f32)
        p[:, i] = (g.astype(f32) + f32(0.5)) * CELL[i]                   # exact cell centres, as the sample forms them
        out.append(p)
        p = inner(300).astype(f32)
        p[:, i] = rng.integers(2, dims[i] - 2, 300).astype(f32) * CELL[i]  # exact cell faces
        out.append(p)
        p = inner(300)
        p[:, i] = (4 * rng.integers(0, dims[i] // 4 - 1, 300) + 3 + rng.uniform(0.55, 1.45, 300)) * cell[i]   # lower corner & 3 == 3
        out.append(p)
        for g in (0, 1, dims[i] - 2, dims[i] - 1):                       # both faces of the outer shell, and one cell inside them
            p = inner(100)
            p[:, i] = (g + rng.uniform(0.05, 0.95, 100)) * cell[i]
            out.append(p)
        for bad in (-0.3, SIZE[i] + 0.3, -1e9, 1e9, np.nan, np.inf, -np.inf):   # outside the box, and not a place at all
            p = inner(20)
            p[:, i] = bad
            out.append(p)
    centres = ((rng.integers(1, dims - 1, (300, 3)).astype(f32) + f32(0.5)) * np.array(CELL, f32)).astype(f32)
    out.append(centres)                                                  # a centre on all three axes: the voxel's own value
    return np.concatenate([np.asarray(p, f32) for p in out])


def equal_words(a, b):
    """binary32 arrays equal bit for bit, a NaN equal to any NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """(points, the harness's 15 words per point)"""
    tmp = tmp_path_factory.mktemp("sample")
    exe = kit.build_harness("sample", tmp)
    vol = scene()[0]
    p = points()
    with open(tmp / "in.bin", "wb") as f:
        for part in (np.array(DIMS, np.int32), np.array(SIZE, f32), np.uint32(len(p)), blocked(vol), np.ascontiguousarray(p.T)):
            f.write(part.tobytes())
    # (a tap outside the volume's array, or undefined behaviour, ends the program with a report and a non-zero status)
    kit.run_harness(exe, tmp / "in.bin", tmp / "out.bin")
    out = np.fromfile(tmp / "out.bin", np.int32).reshape(len(p), 15)
    return p, out


def test_the_point_set_holds_every_class(run):
    """counted with the twins' own arithmetic: the containing voxel is fuse_twin's floor, the lower corner follows from its
    clamped voxel and the centre test"""
    p, _ = run
    vol = scene()[0]
    ok, _, Ws, vox = FT.sample(vol, SIZE, [p[:, i] for i in range(3)])
    assert (ok & (Ws > 0)).sum() > 5000 and (ok & (Ws == 0)).sum() > 500
    for i in range(3):
        g = FT._vox_of(p[:, i], CELL[i])
        centre = ((vox[i].astype(f32) + f32(0.5)) * CELL[i]).astype(f32)
        with np.errstate(invalid="ignore"):
            low = vox[i] - (p[:, i] < centre)
            low_centre = ((low.astype(f32) + f32(0.5)) * CELL[i]).astype(f32)
            assert (ok & (p[:, i] == low_centre)).sum() >= 300, i                 # exact centres: the fraction is 0
            face = np.isfinite(p[:, i]) & (p[:, i] == (np.rint(p[:, i] / CELL[i]).astype(f32) * CELL[i]).astype(f32))
        assert (ok & face).sum() >= 250, i                                         # exact faces
        if i != 1:
            assert (ok & ((low & 3) == 3)).sum() >= 300, i                         # the +13 step (x), the plane-group step (z)
        for shell in (0, DIMS[i] - 1):
            assert ((g == shell) & ~ok).sum() >= 90 and not ((g == shell) & ok).any(), (i, shell)
        for inside in (1, DIMS[i] - 2):
            assert ((g == inside) & ok).sum() >= 90, (i, inside)
        assert ((g == -1) & np.isfinite(p[:, i])).sum() >= 40 and ((g >= DIMS[i]) & (g < 1000000)).sum() >= 20, i
        assert (g == 1000000).sum() >= 40 and np.isnan(p[:, i]).sum() == 20 and np.isinf(p[:, i]).sum() == 40, i


def test_the_sample_equals_the_raycast_twin(run):
    p, out = run
    vol = scene()[0]
    with np.errstate(all="ignore"):
        ref = T._Grid(vol, SIZE, DIMS[2], 0).trilinear([p[:, i] for i in range(3)])
    got = np.where(out[:, 0] != 0, out[:, 7].view(f32), f32(np.nan))
    assert np.isnan(ref).sum() > 1000 and (~np.isnan(ref)).sum() > 10000
    assert equal_words(got, ref).all(), np.flatnonzero(~equal_words(got, ref))[:10]
    assert np.array_equal(np.isnan(ref), out[:, 0] == 0)


def test_the_sample_equals_the_fusion_twin(run):
    p, out = run
    vol = scene()[0]
    ok, F, Ws, vox = FT.sample(vol, SIZE, [p[:, i] for i in range(3)])
    assert np.array_equal(ok, out[:, 0] != 0)
    assert equal_words(out[:, 7].view(f32), F).all()                      # (off the interior too: the clamped cell's blend)
    assert np.array_equal(out[:, 8], Ws)
    for i in range(3):
        assert np.array_equal(out[:, 1 + i], vox[i]), i
        # the lower corner, and the voxel that contains the point clamped into the grid (the views' colour look-up)
        centre = ((vox[i].astype(f32) + f32(0.5)) * CELL[i]).astype(f32)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(out[:, 4 + i], vox[i] - (p[:, i] < centre)), i
        assert np.array_equal(out[:, 12 + i], np.clip(FT._vox_of(p[:, i], CELL[i]), 0, DIMS[i] - 1)), i


def test_the_sample_equals_the_alignment_twin(run):
    p, out = run
    vol = scene()[0]
    ok, F, Ws, g = AT.probe(vol, SIZE, [p[:, i] for i in range(3)])
    assert np.array_equal(ok & (Ws > 0), (out[:, 0] != 0) & (out[:, 8] > 0))    # the probe's verdict
    assert np.array_equal(ok, out[:, 0] != 0) and np.array_equal(Ws, out[:, 8])
    assert equal_words(out[:, 7].view(f32), F).all()
    for i in range(3):
        assert equal_words(out[:, 9 + i].view(f32), g[i]).all(), i
        assert (np.abs(g[i][ok & (Ws > 0)]) > 0).sum() > 1000, i
