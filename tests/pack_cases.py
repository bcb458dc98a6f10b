"""The pack tests' comparison of two contexts, field by field and as images."""
import numpy as np

import pack_twin as PT

f32 = np.float32


def ctx_fields(hsk, trk):
    """the header fields a context contributes, computed here from its configuration (binary32 throughout, as hsk_create)"""
    cfg = trk.cfg
    dims = (cfg.vol_x, cfg.vol_y, cfg.vol_z)
    size = np.array(cfg.vol_size_m[:], f32)
    cell = size / np.array(dims, f32)
    tau = max(f32(cfg.trunc_dist_m), f32(2.1) * cell.max())
    color = trk.color_params if getattr(trk, "color_params", None) else None
    return PT.default_fields(dims, size_m=tuple(size), trunc_dist_m=f32(cfg.trunc_dist_m), trunc_eff_m=f32(tau), width=cfg.width,
                             height=cfg.height, fx=cfg.fx, fy=cfg.fy, cx=cfg.cx, cy=cfg.cy, pose=tuple(trk.get_pose().reshape(-1)),
                             frame=trk.lib.hsk_mgpu_frame_index(trk.h), color_max_weight=color[0] if color else 0,
                             color_band_m=f32(min(f32(2.0) * cell.max(), tau)) if color else f32(0.0))


def assert_same_image(got, want, what):
    if got == want:
        return
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    n = min(len(a), len(b))
    bad = np.flatnonzero(a[:n] != b[:n])
    f = PT.info(want)
    raise AssertionError(f"{what}: {len(got)} bytes against the twin's {len(want)}; {len(bad)} differ, first at {bad[:8].tolist()} "
                         f"(sections at {f['at']}); device header {PT.read_header(got) if len(got) >= 256 else None}")
