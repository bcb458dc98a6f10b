"""hsk_render_section and hsk_render_view on non-cubic volumes with a cell per axis (tests/view_shape_cases.py): 136 x 72 x 46 -- x
in three 64-voxel rows, the last an eighth full, a padded last plane group, three cells -- and the brick tests' shapes: 41, exactly
64 and more than 64 bricks a row, a field beyond 1024 words with super bits, more super-bricks than super bits.  Every section
camera against section_twin.render and every view camera against oracle.raycast + view_twin.shade with the volume's own size, every
output and every count, zero differences; the degenerate section against the view, byte for byte; and the volumes as they were
uploaded afterwards.  Each camera counts only after its condition holds on the reference's own image (check_conditions,
check_camera); that each reaches the path it is there for is shown without a GPU in tests/test_view_shapes_host.py."""
import numpy as np
import pytest

import section_twin as ST
import view_shape_cases as VS
import view_twin as VT
from kit import same_bits_nan, volume_ctx

pytestmark = pytest.mark.gpu
NAMES = list(VS.VOLUMES)


def context(hsk, name):
    """a context of the volume's shape and size holding its filling (and its colour volume)"""
    v = VS.VOLUMES[name]
    vol, col = VS.volume(name)
    trk = volume_ctx(hsk, v["dims"], v["size"], color=col is not None, trunc_dist_m=VS.TRUNC)
    trk.upload_tsdf(vol)
    if col is not None:
        trk.upload_color(col)
    return trk, vol, col


def assert_nothing_moved(trk, vol, col, name):
    assert np.array_equal(trk.download_tsdf(), vol), f"{name}: the TSDF volume changed"
    if col is not None:
        assert np.array_equal(trk.download_color(), col), f"{name}: the colour volume changed"


@pytest.mark.parametrize("name", NAMES)
def test_sections_against_twin(hsk, name):
    """every section camera of the volume: rgb, depth, vmap, nmap, n_hit, n_cut and n_uncolored are the twin's"""
    from housescan_amd import _lib
    trk, vol, col = context(hsk, name)
    for cam in VS.cameras(name):
        sec, ref = VS.reference(name, cam)
        sh = VS.check_conditions(name, cam, ref)   # on the twin's own image, before anything is compared
        print(f"{name} {cam}: twin hit {sh[0]:.4f} cut {sh[1]:.4f} background {sh[2]:.4f}")
        got = trk.render_section(ST.to_struct(sec, _lib), vmap=True, nmap=True)
        VS.assert_section(got, ref, f"{name} {cam}")
    assert_nothing_moved(trk, vol, col, name)
    trk.close()


@pytest.mark.parametrize("name", NAMES)
def test_views_against_oracle_and_twin(hsk, oracle, name):
    """the view cameras (g), from outside looking in and from inside (1048 x 1048 x 12: one view, the OpenMP oracle as everywhere):
    every mode the volume has, the light in camera and in world coordinates"""
    v = VS.VOLUMES[name]
    trk, vol, col = context(hsk, name)
    modes = {"all": VS.MODES, "one": (VT.LAMBERT, VT.NORMALS, VT.COLOR_LIT), None: (VT.LAMBERT, VT.NORMALS)}[v["color"]]
    for what, cam, pose in VS.view_cameras(name):
        hit = VS.check_camera(trk, oracle, v["dims"], vol, col, cam, pose, f"{name} {what}", modes=modes, size=v["size"], uncolored="both")
        print(f"{name} {what}: oracle hit {hit.mean():.4f}")
    assert_nothing_moved(trk, vol, col, name)
    trk.close()


@pytest.mark.parametrize("name", ["136x72x46", "328x40x44"])
def test_degenerate_section_is_render_view(hsk, name):
    """pinhole, no planes, a point light: rgb, depth_mm, vmap, nmap, n_hit and n_uncolored are hsk_render_view's, n_cut is 0, in
    every mode, from both view cameras"""
    trk, vol, col = context(hsk, name)
    checked = 0
    for what, cam, pose in VS.view_cameras(name):
        for mode in VS.MODES:
            kw = dict(mode=mode, light=(0.2, -0.1, 0.05), light_in_camera=int(mode != VT.COLOR_LIT), background=(9, 8, 7), vmap=True,
                      nmap=True, pose=pose, **cam)
            a = trk.render_view(**kw)
            b = trk.render_section(**kw)
            tag = f"{name} {what} mode {mode}"
            assert a["n_hit"] > 0.2 * cam["width"] * cam["height"], tag
            assert (b["n_hit"], b["n_uncolored"], b["n_cut"]) == (a["n_hit"], a["n_uncolored"], 0), tag
            for key in ("rgb", "depth", "vmap", "nmap"):
                assert same_bits_nan(a[key], b[key]), f"{tag}: {key}"
            checked += 1
    assert checked == 8
    assert_nothing_moved(trk, vol, col, name)
    trk.close()
