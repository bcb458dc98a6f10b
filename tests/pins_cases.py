"""The small camera, configuration and depth image of the oracle's pinned results."""
W, H, FX, CX, CY = 160, 120, 131.25, 79.75, 59.75


def small_cfg(O, n=32):
    return O.default_config(n, W=W, H=H, fx=FX, fy=FX, cx=CX, cy=CY)


def small_depth(hsk, k):
    return hsk.synth_depth(hsk.synth_pose(k), W, H, FX, FX, CX, CY)
