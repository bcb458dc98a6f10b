"""The image kernels' shape cases without a GPU (tests/view_shape_cases.py): section_twin pinned to the oracle on two non-cubes with
the per-axis size in use, and every named camera shown, on the twin's own image, to be worth rendering on the device -- its shares
of hits, cut outlines and background, its coloured and uncoloured hits, and the path it is there for: the padded plane group, the
last 64-voxel row of x, rays on voxel faces, the bricks whose bits no cube reaches.

What the shapes' fixed fillings cannot give is asserted as a fact about the filling, next to the condition it replaces:
- a ray that starts in the last plane group cannot hit: its first far sample lies 1.68 cells or more on (the step is 0.8 tau and tau
  at least 2.1 cells), in the volume's last plane, where no trilinear sample exists.  So camera (b) is two cameras: "along z", whose
  plane stands two march steps before the far z wall and which meets the shares, and, at 136 x 72 x 46, "along z, last group", whose
  plane is in the padded group and whose pixels are cut or background.  The brick shapes' fillings hold no negative voxel in their
  last four planes (and Z is a multiple of 4 there: no group is padded), so they have the first of the two only;
- 328 x 40 x 44 and 264^3 hold no negative voxel in their last, partial row of x: camera (c)'s plane is in the row that holds the far
  x wall; at 136 x 72 x 46, 512 x 64 x 52 and 528 x 16 x 20 it is in the last row (brick 63; x >= 512);
- 528 x 16 x 20 has 16 voxels of y over 3 scene units: the floor's negative band (0.1 units) is half a voxel and holds no voxel
  centre, so no ray along +y finds a surface.  Its top-down camera shows cut outlines and background only, and its (e) cameras look
  along +z."""
import time

import numpy as np
import pytest

import brick_twin as BT
import section_twin as ST
import view_shape_cases as VS
import view_twin as VT
from kit import same_bits_nan

f32 = np.float32
NAMES = list(VS.VOLUMES)
SMALL = [n for n in NAMES if n != "1048x1048x12"]


@pytest.mark.parametrize("name", ["136x72x46", "328x40x44"])
def test_twin_is_pinned_to_the_oracle_on_a_non_cube(oracle, name):
    """pinhole rays, no planes, a point light: section_twin.render's maps are oracle.raycast's under view_config(..., size=size) and
    its images view_twin.shade(..., size=size)'s, bit for bit, in every mode; and the colour image is NOT what the default 3 m size
    gives, so the size is in use"""
    v = VS.VOLUMES[name]
    dims, size = v["dims"], v["size"]
    vol, col = VS.volume(name)
    differs = 0
    for what, cam, pose in VS.view_cameras(name):
        cfg = VT.view_config(oracle, dims, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], size=size)
        vm, nm = VT.geometry(oracle, cfg, vol, pose, omp=False)
        hit = ~np.isnan(vm[0])
        print(f"{name} {what}: oracle hit {hit.mean():.3f}")
        assert hit.mean() >= 0.20 and (~hit).mean() >= 0.02, "the pin needs hits and background"
        vm3, _ = VT.geometry(oracle, VT.view_config(oracle, dims, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]),
                             vol, pose, omp=False)
        assert not same_bits_nan(vm3, vm), "the oracle's geometry must depend on the size"
        for mode in VS.MODES:
            light, in_cam, bg = (0.1, -0.2, 0.05), mode != VT.COLOR_LIT, (3, 4, 5)
            ref = VT.shade(vm, nm, pose, mode, light, in_cam, bg, color=col, size=size)
            sec = ST.section(**cam, pose=pose, projection=ST.PINHOLE, clip=(), mode=mode, light=light, light_in_camera=in_cam, background=bg)
            got = ST.render(vol, size, VS.TRUNC, sec, color=col)
            assert same_bits_nan(got["vmap"], vm) and same_bits_nan(got["nmap"], nm), f"{name} {what} mode {mode}"
            assert np.array_equal(got["rgb"], ref["rgb"]) and np.array_equal(got["depth"], ref["depth"]), f"{name} {what} mode {mode}"
            assert (got["n_hit"], got["n_cut"], got["n_uncolored"]) == (ref["n_hit"], 0, ref["n_uncolored"])
            if mode in (VT.COLOR, VT.COLOR_LIT):
                assert ref["n_uncolored"] >= 500 and ref["n_hit"] - ref["n_uncolored"] >= 500
                default = VT.shade(vm, nm, pose, mode, light, in_cam, bg, color=col)
                differs += int((default["rgb"] != ref["rgb"]).any(axis=2).sum())
                assert not np.array_equal(default["rgb"], ref["rgb"]), "the look-up with 3 m cells must pick other voxels"
    print(f"{name}: {differs} colour pixels differ from the default 3 m size")


@pytest.mark.parametrize("name", NAMES)
def test_every_camera_meets_its_condition(name):
    """(a)-(d): hit >= 0.20, cut >= 0.02, background >= 0.02 of the twin's image; (e), (f): hits and cut pixels; a colour mode: at
    least 500 hits with and 500 without colour; the exceptions of the module's docstring, each with the fact that makes it one"""
    vol, col = VS.volume(name)
    Z, Y, X, _ = vol.shape
    t0 = time.time()
    kinds = set()
    for cam, c in VS.cameras(name).items():
        sec, ref = VS.reference(name, cam)
        sh = VS.check_conditions(name, cam, ref)
        kinds.add(c["kind"])
        print(f"{name} {cam} ({c['kind']}, {sec['width']}x{sec['height']}, mode {sec['mode']}): twin hit {sh[0]:.3f} cut {sh[1]:.3f} "
              f"background {sh[2]:.3f}, uncoloured {ref['n_uncolored']} of {ref['n_hit']} hits")
        assert sec["width"] <= 333 and sec["height"] <= 217
    print(f"{name}: the twin's images took {time.time() - t0:.1f} s")
    cams = VS.cameras(name)
    if name == "1048x1048x12":
        assert kinds == {"b"} and max(cams["along z"]["fields"]["width"], cams["along z"]["fields"]["height"]) <= 128
        return
    assert kinds >= {"a", "b", "c", "d", "e"}
    needs = {cam: c["need"] for cam, c in cams.items() if c["kind"] in "abcd"}
    if name == "528x16x20":
        assert needs.pop("top-down") == "cut"
        t = vol[..., 0]
        assert not ((t[:, Y // 2:-1] > 0) & (t[:, Y // 2 + 1:] < 0)).any(), "from mid height on, no positive voxel has a negative one behind it along +y"
        assert not VS.reference(name, "top-down")[1]["raw_hit"].any()
    assert set(needs.values()) == {"shares"}, needs
    if name == "264x264x264":
        assert all(max(c["fields"]["width"], c["fields"]["height"]) <= 160 for c in cams.values())
    modes = {c["fields"]["mode"] for c in cams.values()}
    if VS.VOLUMES[name]["color"] == "all":
        assert modes == set(VS.MODES)
        lights = {(c["fields"]["light_in_camera"], c["fields"]["light_directional"]) for c in cams.values()
                  if c["fields"]["mode"] in (VT.LAMBERT, VT.COLOR_LIT)}
        assert lights == {(True, True), (True, False), (False, True), (False, False)}
    elif VS.VOLUMES[name]["color"] == "one":
        assert len(modes & {VT.COLOR, VT.COLOR_LIT}) == 1
    else:
        assert col is None and not modes & {VT.COLOR, VT.COLOR_LIT}


def test_the_plane_in_the_last_plane_group():
    """camera (b) at 136 x 72 x 46: 46 planes, the last group half padding.  "along z, last group" gathers at least 100 CUT pixels
    from planes >= 44; nothing is hit behind such a plane.  The brick shapes hold no negative voxel in their last four planes."""
    name = "136x72x46"
    z0 = VS.last_group_start(name)
    assert VS.VOLUMES[name]["dims"][2] % 4 == 2 and z0 == 44
    sec, ref = VS.reference(name, "along z, last group")
    _, vox, marching = VS.start_points(name, sec)
    cut = ref["cls"] == ST.CUT
    n = int((vox[2][cut] >= z0).sum())
    print(f"{name} along z, last group: {n} of {ref['n_cut']} CUT pixels gathered from planes >= {z0}; {int(ref['raw_hit'].sum())} march hits")
    assert n >= 100 and n == ref["n_cut"]
    assert marching.sum() > ref["n_cut"] and not ref["raw_hit"].any()
    # the other camera (b) gathers its cut pixels before the wall, and hits the wall
    sec, ref = VS.reference(name, "along z")
    _, vox, _ = VS.start_points(name, sec)
    assert (vox[2][ref["cls"] == ST.CUT] < z0).all() and ref["n_hit"] > 1000
    for other in VS.SMALL_BRICKS:
        vol, _ = VS.volume(other)
        assert vol.shape[0] % 4 == 0 and not (vol[-4:, ..., 0] < 0).any(), other


@pytest.mark.parametrize("name", SMALL)
def test_the_plane_in_the_last_row_of_x(name):
    """camera (c): at least 100 CUT pixels gathered from the last 64-voxel row of x -- at 512 x 64 x 52 from brick 63, at
    528 x 16 x 20 from x >= 512; where the filling leaves that row empty (328 x 40 x 44: voxels 320..327; 264^3: 256..263), from the
    row that holds the far x wall"""
    vol, _ = VS.volume(name)
    X = VS.VOLUMES[name]["dims"][0]
    x0 = VS.last_row_start(name)
    if name in ("328x40x44", "264x264x264"):
        assert not (vol[:, :, x0:, 0] < 0).any() and X - x0 == 8
        x0 = 64 * int(VS.wall_voxel(name, 0) // 64)
    elif name == "512x64x52":
        x0 = 8 * 63
    assert {"136x72x46": 128, "328x40x44": 256, "512x64x52": 504, "528x16x20": 512, "264x264x264": 192}[name] == x0
    sec, ref = VS.reference(name, "along x")
    _, vox, _ = VS.start_points(name, sec)
    cut = ref["cls"] == ST.CUT
    n = int((vox[0][cut] >= x0).sum())
    print(f"{name} along x: {n} of {ref['n_cut']} CUT pixels gathered from x >= {x0}")
    assert n >= 100 and n == ref["n_cut"]


@pytest.mark.parametrize("name", ["136x72x46", "328x40x44"])
def test_rays_on_voxel_faces(name):
    """camera (f): at least a quarter of the marching rays have o / cell within 2.5e-4 of an integer on both lateral axes (every
    second ray of x times every second of z), hits and cuts are present, and the pitch is half a cell"""
    v = VS.VOLUMES[name]
    sec, ref = VS.reference(name, "on the faces")
    o, _, marching = VS.start_points(name, sec)
    near = np.ones(marching.shape, bool)
    for k in (0, 2):
        q = o[k].astype(np.float64) / float(f32(v["size"][k]) / f32(v["dims"][k]))
        near &= np.abs(q - np.rint(q)) <= 2.5e-4
    share = float(near[marching].mean())
    print(f"{name} on the faces: {share:.3f} of {int(marching.sum())} marching rays lie on a face of x and of z; hits {ref['n_hit']}, cut {ref['n_cut']}")
    assert share >= 0.25 and ref["n_hit"] > 0 and ref["n_cut"] > 0
    for f, k in ((sec["fx"], 0), (sec["fy"], 2)):   # (binary32 intrinsics: half a cell to a part in 10^6)
        assert float(f) * v["size"][k] / v["dims"][k] == pytest.approx(2.0, rel=1e-6)
    hit_on = near & (ref["cls"] == ST.HIT)
    assert hit_on.sum() >= 1000, "hits among the rays on the faces"


@pytest.mark.parametrize("name", [n for n in NAMES if n in VS.BRICK_CASES])
def test_brick_shapes_reach_their_paths(name):
    """the design of each brick shape on the filling alone (as test_gpu_bricks.assert_reaches_its_path), and at least 1000 hit
    pixels of one section image with their vertex in a brick the named path covers"""
    vol, _ = VS.volume(name)
    X, Y, Z = VS.VOLUMES[name]["dims"]
    L = BT.layout(X, Y, Z)
    assert L["bshift"] == 3
    b = BT.brick_bits(vol, 3)
    covered = np.zeros(b.shape, bool)
    bit = np.arange(b.size).reshape(b.shape)
    if name == "328x40x44":
        third = BT.third_word_bricks(b)
        assert len(third) > 0
        covered[tuple(np.array(third).T)] = True
    if name == "512x64x52":
        assert L["bxn"] == 64 and b[:, :, 63].any()
        covered[:, :, 63] = True
    if name in ("528x16x20", "1048x1048x12"):
        assert L["bxn"] > 64 and (vol[:, :, 512:, 0] < 0).any()
        covered[:, :, 64:] = True
    if name in ("264x264x264", "1048x1048x12"):
        assert L["words"] > 1024 and BT.set_bits_beyond_word(b, 1024) > 0
        covered = covered | ((bit >> 5) >= 1024)
    if name == "264x264x264":
        assert L["super_ok"] and BT.field(vol)[L["words"]:].any()
    if name == "1048x1048x12":
        assert not L["super_ok"]
    best = ("", 0)
    for cam in VS.cameras(name):
        _, ref = VS.reference(name, cam)
        x, y, z = VS.hit_voxels(name, ref)
        n = int(covered[z >> 3, y >> 3, x >> 3].sum())
        print(f"{name} {cam}: {n} of {ref['n_hit']} hit pixels have their vertex in a brick of the path")
        best = max(best, (cam, n), key=lambda p: p[1])
    assert best[1] >= 1000, best
