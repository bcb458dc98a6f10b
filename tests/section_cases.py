"""The section tests' room frames and orthographic camera, shared with the fusion and pack tests."""
from concurrent.futures import ThreadPoolExecutor

import section_twin as ST

SCAN_FRAMES = 720
SIDE, SPAN = 200, 3.2                    # the named cameras: 200 x 200 pixels over 3.2 m (62.5 px/m), or a pinhole with f = 180


def room_frames(hsk, variant, lo, hi):
    """frames lo..hi-1 of the scripted scan inside room `variant` (the renderers release the GIL: eight at a time)"""
    poses = [hsk.synth_room_pose(variant, k, SCAN_FRAMES) for k in range(lo, hi)]
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda p: (hsk.synth_room_depth(variant, p), hsk.synth_rgb(p, variant)), poses))


def ortho_cam(pose, side=SIDE, span=SPAN, width=None, height=None):
    w, h = width or side, height or side
    ppm = side / span
    return dict(width=w, height=h, fx=ppm, fy=ppm, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, pose=pose, projection=ST.ORTHO)
