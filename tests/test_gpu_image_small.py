"""The image kernels at the smallest image sizes at which they can go wrong, bit for bit against the CPU oracle.

68 x 52 is a multiple of 4 and of neither 8 nor 16: the raycast's fused pyramid is off, so every frame ends in k_resize_maps2;
the 16-pixel tiles of k_pyramid_maps are ragged on both axes; the levels are 34 x 26 and 17 x 13 (odd).  72 x 56 and 88 x 72 have
whole 8 x 8 tiles (fused pyramid on), 88 is no multiple of 16.  A group of two slabs at 68 x 52 ends its frames in
k_adopt_pyramid at the same odd level sizes."""
import functools

import numpy as np
import pytest

from kit import assert_same_bits

pytestmark = pytest.mark.gpu
N_FRAMES = 5


def _intr(w, h):
    s = w / 640.0
    return dict(fx=525.0 * s, fy=525.0 * s, cx=w / 2 - 0.5, cy=h / 2 - 0.5)


@functools.lru_cache(maxsize=None)
def _frames(w, h, ks=tuple(range(N_FRAMES))):
    import housescan_amd as hsk
    i = _intr(w, h)
    return [hsk.synth_depth(hsk.synth_pose(k), w, h, i["fx"], i["fy"], i["cx"], i["cy"]) for k in ks]


def test_preprocess_small_image(hsk, oracle):
    """k_bilateral_scale and k_pyramid_maps at 68 x 52: ragged 16-pixel tiles on both axes, odd upper levels"""
    w, h = 68, 52
    cfg_o = oracle.default_config(32, W=w, H=h, **_intr(w, h))
    trk = hsk.KinfuTracker(n=32, width=w, height=h, **_intr(w, h))
    rng = np.random.default_rng(7)
    for depth in _frames(w, h, (0, 30)):
        # the noise, the 2 % holes and the rectangular hole (scaled to the image) of test_preprocess_bit_exact
        d = (depth.astype(np.int32) + rng.integers(-8, 9, depth.shape)).clip(0, 65535).astype(np.uint16)
        d[rng.random(d.shape) < 0.02] = 0
        d[11:15, 21:28] = 0
        trk.preprocess(d)
        lv = [oracle.bilateral(cfg_o, d)]
        lv.append(oracle.pyrdown(lv[0]))
        lv.append(oracle.pyrdown(lv[1]))
        assert_same_bits(trk.download_scaled_depth(), oracle.scale_depth(cfg_o, d), "scaled depth")
        for l in range(3):
            assert lv[l].shape == (h >> l, w >> l)
            assert_same_bits(trk.download_depth_level(l), lv[l], f"depth level {l}")
            vm = oracle.vmap(cfg_o, lv[l], l)
            assert_same_bits(trk.download_map(0, l), vm, f"vmap level {l}")
            assert_same_bits(trk.download_map(1, l), oracle.nmap(vm), f"nmap level {l}")
    trk.close()


@pytest.mark.parametrize("w,h", [(68, 52), (72, 56), (88, 72)])
def test_model_pyramid_small_images(hsk, oracle, w, h):
    """the model maps of levels 0 to 2 behind tracked frames (k_resize_maps2 at 68 x 52, the raycast's fused pyramid at the
    other two), then a stage-level raycast, which always ends in k_resize_maps2"""
    n = 64
    ot = oracle.Tracker(oracle.default_config(n, W=w, H=h, **_intr(w, h)), omp=True)
    trk = hsk.KinfuTracker(n=n, width=w, height=h, **_intr(w, h))
    pose = None
    for k, depth in enumerate(_frames(w, h)):
        po, oko = ot.process(depth)
        pose, okh = trk.process_frame(depth)
        assert oko == okh == (k > 0), f"{w}x{h} frame {k}"
        assert_same_bits(pose, po, f"{w}x{h} pose frame {k}")
    for level in range(3):
        vm = ot.model_map(2, level)
        assert np.isnan(vm[0]).any() and not np.isnan(vm[0]).all(), "the NaN branch of the mean must be exercised"
        assert_same_bits(trk.download_map(2, level), vm, f"{w}x{h} model vmap {level}")
        assert_same_bits(trk.download_map(3, level), ot.model_map(3, level), f"{w}x{h} model nmap {level}")
    v, nm = trk.raycast(pose)
    for level in (1, 2):
        v, nm = oracle.resize_vmap(v), oracle.resize_nmap(nm)
        assert_same_bits(trk.download_map(2, level), v, f"{w}x{h} resized vmap {level}")
        assert_same_bits(trk.download_map(3, level), nm, f"{w}x{h} resized nmap {level}")
    trk.close()
    ot.close()


def test_two_slabs_small_image(hsk):
    """k_adopt_pyramid at odd level sizes: two slabs on one device at 68 x 52, synchronous and pipelined calls mixed, equal
    the single context: poses, the volume, the model maps of every slab"""
    w, h, n = 68, 52, 64
    frames = _frames(w, h)
    ref = hsk.KinfuTracker(n=n, width=w, height=h, **_intr(w, h))
    want = [ref.process_frame(d) for d in frames]
    grp = hsk.KinfuGroup(hsk.default_config(n, width=w, height=h, **_intr(w, h)), device_ids=[0, 0])
    assert grp.n_slabs() == 2
    got = [grp.process_frame(frames[0]), grp.process_frame(frames[1])]
    grp.submit_frame(frames[2])
    for d in frames[3:]:
        grp.submit_frame(d)
        got.append(grp.wait_frame())
    got.append(grp.wait_frame())
    assert len(got) == len(want) == N_FRAMES
    for k, ((p, ok), (pr, okr)) in enumerate(zip(got, want)):
        assert ok == okr == (k > 0), f"frame {k}"
        assert_same_bits(p, pr, f"group pose frame {k}")
    assert_same_bits(grp.download_tsdf(), ref.download_tsdf(), "group tsdf")
    for i in range(2):
        s = grp.slab(i)
        for level in range(3):
            assert_same_bits(s.download_map(2, level), ref.download_map(2, level), f"slab {i} model vmap {level}")
            assert_same_bits(s.download_map(3, level), ref.download_map(3, level), f"slab {i} model nmap {level}")
    grp.close()
    ref.close()
