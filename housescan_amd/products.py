"""Products on the file seam between the KinFu core and HouseScan (host side).

`write_room_dir` produces exactly the directory `loadRoom` reads (/root/reference/housescan/Main.hs:1738-1762):
  cloud_downsampled.pcd   XYZ float PCD                               (Main.hs:1740, :1334-1345)
  planes.txt              "a b c d" per line, PCL form ax+by+cz+d=0   (Main.hs:1379-1389)
  cloud_plane_hull<k>.pcd polygon of plane k, vertices in drawing order (Main.hs:1395-1400)
plus cloud_bin.pcd, the full-resolution cloud HouseScan's printed pcl_transform_point_cloud commands act on
(Main.hs:2311-2313, :2436-2438).
"""
import ctypes as C
import os

import numpy as np

from . import _lib


def _ck(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def voxel_downsample(xyz, leaf):
    lib = _lib.load()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.empty_like(pts)
    n = C.c_size_t()
    _ck(lib.hsk_voxel_downsample(pts.ctypes.data, len(pts), C.c_float(leaf), out.ctypes.data, len(pts), C.byref(n)), "hsk_voxel_downsample")
    return out[:n.value].copy()


def write_pcd(path, xyz):
    lib = _lib.load()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    _ck(lib.hsk_write_pcd_xyz(os.fsencode(path), pts.ctypes.data, len(pts)), "hsk_write_pcd_xyz")


def write_pcd_xyzrgbnormal(path, xyz, rgb, normals=None):
    """binary PCD with x y z rgb normal_x normal_y normal_z curvature (32 B per point; rgb packed as 0x00RRGGBB; NaN normals
    kept; normals None: NaN)"""
    lib = _lib.load()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    col = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    if len(col) != len(pts):
        raise ValueError("write_pcd_xyzrgbnormal: rgb must have one row per point")
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(nrm) != len(pts):
            raise ValueError("write_pcd_xyzrgbnormal: normals must have one row per point")
    _ck(lib.hsk_write_pcd_xyzrgbnormal(os.fsencode(path), pts.ctypes.data, col.ctypes.data, None if nrm is None else nrm.ctypes.data, len(pts)),
        "hsk_write_pcd_xyzrgbnormal")


def voxel_downsample_attrs(xyz, leaf, rgb=None, normals=None):
    """voxel_downsample (the same xyz, bit for bit, in the same order) with the rounded mean colour and the renormalised mean
    of the non-NaN normals per leaf -> (xyz, rgb or None, normals or None)"""
    lib = _lib.load()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    col = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    for a in (col, nrm):
        if a is not None and len(a) != len(pts):
            raise ValueError("voxel_downsample_attrs: attributes must have one row per point")
    out = np.empty_like(pts)
    out_rgb = None if col is None else np.empty((len(pts), 3), np.uint8)
    out_nrm = None if nrm is None else np.empty((len(pts), 3), np.float32)
    n = C.c_size_t()
    _ck(lib.hsk_voxel_downsample_attrs(pts.ctypes.data, None if col is None else col.ctypes.data, None if nrm is None else nrm.ctypes.data,
                                       len(pts), C.c_float(leaf), out.ctypes.data, None if out_rgb is None else out_rgb.ctypes.data,
                                       None if out_nrm is None else out_nrm.ctypes.data, len(pts), C.byref(n)), "hsk_voxel_downsample_attrs")
    m = n.value
    return out[:m].copy(), None if out_rgb is None else out_rgb[:m].copy(), None if out_nrm is None else out_nrm[:m].copy()


def write_ply_mesh(path, triangles):
    """triangle soup [n, 3, 3] -> welded binary .ply mesh; returns (vertices, faces) written"""
    lib = _lib.load()
    tri = np.ascontiguousarray(triangles, np.float32).reshape(-1, 9)
    nv, nf = C.c_size_t(), C.c_size_t()
    _ck(lib.hsk_write_ply_mesh(os.fsencode(path), tri.ctypes.data, len(tri), C.byref(nv), C.byref(nf)), "hsk_write_ply_mesh")
    return nv.value, nf.value


def weld_triangles(triangles):
    """triangle soup [n, 3, 3] -> (vertices [v, 3] in order of first appearance, indices [n, 3])"""
    lib = _lib.load()
    tri = np.ascontiguousarray(triangles, np.float32).reshape(-1, 9)
    nv = C.c_size_t()
    verts = np.empty((max(1, 3 * len(tri)), 3), np.float32)
    idx = np.empty((len(tri), 3), np.int32)
    _ck(lib.hsk_weld_triangles(tri.ctypes.data, len(tri), verts.ctypes.data, len(verts), C.byref(nv), idx.ctypes.data), "hsk_weld_triangles")
    return verts[:nv.value].copy(), idx


def detect_planes(xyz, dist_thresh=0.02, min_fraction=0.03, max_planes=12, iterations=300):
    """-> (planes [k,4] as a,b,c,d of ax+by+cz+d=0 with unit normal, labels [n])"""
    lib = _lib.load()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    planes = np.zeros((max_planes, 4), np.float32)
    labels = np.empty(len(pts), np.int32)
    k = C.c_int()
    _ck(lib.hsk_detect_planes(pts.ctypes.data, len(pts), C.c_float(dist_thresh), C.c_float(min_fraction), max_planes, iterations,
                              planes.ctypes.data, labels.ctypes.data, C.byref(k)), "hsk_detect_planes")
    return planes[:k.value].copy(), labels


def plane_hull(xyz, labels, plane, abcd):
    lib = _lib.load()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    lab = np.ascontiguousarray(labels, np.int32)
    eq = np.ascontiguousarray(abcd, np.float32)
    cap = max(16, int((lab == plane).sum()))
    hull = np.empty((cap, 3), np.float32)
    n = C.c_size_t()
    _ck(lib.hsk_plane_hull(pts.ctypes.data, len(pts), lab.ctypes.data, int(plane), eq.ctypes.data_as(C.POINTER(C.c_float)),
                           hull.ctypes.data, cap, C.byref(n)), "hsk_plane_hull")
    return hull[:n.value].copy()


def write_room_dir(room_dir, cloud_xyz, leaf=0.03, *, cloud_rgb=None, cloud_normals=None, colored_downsampled=False, planes=None, **plane_args):
    """cloud (full resolution, KinFu frame) -> the files HouseScan's loadRoom expects. Returns (planes, n_downsampled).
    With cloud_rgb (and cloud_normals; KinfuTracker.extract_cloud_attrs) cloud_bin.pcd is written as XYZRGBNormal, the coloured
    form of HouseScan's cloud loader (Main.hs:1325-1345) -- NaN normals when cloud_normals is None; cloud_downsampled.pcd stays
    XYZ -- the form loadRoom tries first -- unless colored_downsampled.  Plane detection always runs on the same downsampled xyz.
    Normals without colour, or colored_downsampled without colour, are refused (ValueError): there is no XYZ + normal form.
    planes = (planes_abcd [k, 4], labels [m], xyz [m, 3]): planes found elsewhere (KinfuTracker.detect_planes on the device) with
    the points they were found on -- the RANSAC is skipped, planes.txt holds them and the hulls are hsk_plane_hull's of the
    labelled points; plane_args are then refused (ValueError)."""
    if cloud_rgb is None and (cloud_normals is not None or colored_downsampled):
        raise ValueError("write_room_dir: cloud_normals and colored_downsampled need cloud_rgb (the coloured file carries both)")
    lib = _lib.load()
    os.makedirs(room_dir, exist_ok=True)
    colored = cloud_rgb is not None
    if colored:
        write_pcd_xyzrgbnormal(os.path.join(room_dir, "cloud_bin.pcd"), cloud_xyz, cloud_rgb, cloud_normals)
    else:
        write_pcd(os.path.join(room_dir, "cloud_bin.pcd"), cloud_xyz)
    down = voxel_downsample(cloud_xyz, leaf)
    if colored and colored_downsampled:
        d_xyz, d_rgb, d_nrm = voxel_downsample_attrs(cloud_xyz, leaf, cloud_rgb, cloud_normals)
        write_pcd_xyzrgbnormal(os.path.join(room_dir, "cloud_downsampled.pcd"), d_xyz, d_rgb, d_nrm)
    else:
        write_pcd(os.path.join(room_dir, "cloud_downsampled.pcd"), down)
    hull_pts = down
    if planes is None:
        planes, labels = detect_planes(down, **plane_args)
    else:
        if plane_args:
            raise ValueError("write_room_dir: planes were given, so the detector's arguments have nothing to act on")
        planes, labels, hull_pts = planes
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
        labels = np.ascontiguousarray(labels, np.int32).reshape(-1)
        hull_pts = np.ascontiguousarray(hull_pts, np.float32).reshape(-1, 3)
        if len(labels) != len(hull_pts):
            raise ValueError(f"write_room_dir: {len(labels)} labels for {len(hull_pts)} points")
    _ck(lib.hsk_write_planes_txt(os.fsencode(os.path.join(room_dir, "planes.txt")), planes.ctypes.data, len(planes)),
        "hsk_write_planes_txt")
    for k, eq in enumerate(planes):
        write_pcd(os.path.join(room_dir, f"cloud_plane_hull{k}.pcd"), plane_hull(hull_pts, labels, k, eq))
    return planes, len(down)


def write_ply_indexed(path, vertices, faces, normals=None, rgb=None):
    """indexed mesh -> binary little-endian .ply: x y z [nx ny nz] [red green blue] per vertex (NaN normals written as 0),
    every face as given; an index outside [0, n) raises and writes no file"""
    lib = _lib.load()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    col = None if rgb is None else np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    for a in (nrm, col):
        if a is not None and len(a) != len(v):
            raise ValueError("write_ply_indexed: attributes must have one row per vertex")
    _ck(lib.hsk_write_ply_indexed(os.fsencode(path), v.ctypes.data, None if nrm is None else nrm.ctypes.data,
                                  None if col is None else col.ctypes.data, len(v), f.ctypes.data, len(f)), "hsk_write_ply_indexed")


def write_ply_textured(path, vertices, faces, uv, texture_file, normals=None):
    """indexed mesh with per-face texture coordinates -> binary little-endian .ply that names its atlas in a "comment TextureFile"
    line: x y z [nx ny nz] per vertex, per face the indices and six floats texcoord (KinfuTracker.bake_texture's uv)"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    t = np.ascontiguousarray(uv, np.float32).reshape(-1, 6)
    nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(t) != len(f) or (nrm is not None and len(nrm) != len(v)):
        raise ValueError("write_ply_textured: uv needs one row per face, normals one per vertex")
    _ck(_lib.load().hsk_write_ply_textured(os.fsencode(path), v.ctypes.data, None if nrm is None else nrm.ctypes.data, len(v), f.ctypes.data, len(f),
                                           t.ctypes.data, os.fsencode(texture_file)), "hsk_write_ply_textured")


def write_png_rgb(path, rgb):
    """(h, w, 3) uint8 image -> 8-bit RGB PNG with stored (uncompressed) deflate blocks: KinfuTracker.bake_texture's rgb"""
    a = np.ascontiguousarray(rgb, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_png_rgb: an (h, w, 3) uint8 array is needed")
    _ck(_lib.load().hsk_write_png_rgb(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]), "hsk_write_png_rgb")


def write_ppm(path, rgb):
    """(h, w, 3) uint8 image -> binary PPM (P6): KinfuTracker.render_view's rgb"""
    a = np.ascontiguousarray(rgb, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_ppm: an (h, w, 3) uint8 array is needed")
    _ck(_lib.load().hsk_write_ppm(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]), "hsk_write_ppm")


def write_pgm16(path, depth_mm):
    """(h, w) uint16 image -> binary PGM (P5, maxval 65535, big-endian samples): KinfuTracker.render_view's depth"""
    a = np.ascontiguousarray(depth_mm, np.uint16)
    if a.ndim != 2:
        raise ValueError("write_pgm16: an (h, w) uint16 array is needed")
    _ck(_lib.load().hsk_write_pgm16(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]), "hsk_write_pgm16")


def section_in_room(house, room_xf):
    """a section given in house coordinates (an `_lib.HskSection`, follow = 0) -> the same section in the frame of the room that
    the rigid 4x4 room -> house matrix `room_xf` (its .xf) places in the house (hsk_section_in_room)"""
    m = np.ascontiguousarray(room_xf, np.float32).reshape(16)
    room = _lib.HskSection()
    _ck(_lib.load().hsk_section_in_room(C.byref(house), m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(room)), "hsk_section_in_room")
    return room


def invert_rigid(m):
    """the inverse (R^T, -R^T t) of a rigid row-major 4x4 matrix, computed in binary64 and rounded once (hsk_invert_rigid)"""
    a = np.ascontiguousarray(m, np.float32).reshape(16)
    out = np.empty(16, np.float32)
    fp = C.POINTER(C.c_float)
    _ck(_lib.load().hsk_invert_rigid(a.ctypes.data_as(fp), out.ctypes.data_as(fp)), "hsk_invert_rigid")
    return out.reshape(4, 4)


def align_step(sums27, m, centre):
    """host only: one alignment iteration's solve and pose update about `centre` (hsk_align_step) -> (m_next [4, 4] float32,
    x6 float32, ok); a singular system: m_next = m, x6 zeros, ok False"""
    s = np.ascontiguousarray(sums27, np.float64).reshape(-1)[:27].copy()
    a = np.ascontiguousarray(m, np.float32).reshape(16)
    c = np.ascontiguousarray(centre, np.float32).reshape(3)
    out, x6, ok = np.empty(16, np.float32), np.empty(6, np.float32), C.c_int()
    fp = C.POINTER(C.c_float)
    _ck(_lib.load().hsk_align_step(s.ctypes.data_as(C.POINTER(C.c_double)), a.ctypes.data_as(fp), c.ctypes.data_as(fp),
                                   out.ctypes.data_as(fp), x6.ctypes.data_as(fp), C.byref(ok)), "hsk_align_step")
    return out.reshape(4, 4), x6, bool(ok.value)


def fuse_footprint(src_dims, src_size_m, dst_dims, dst_size_m, src_to_dst):
    """the half-open destination voxel box (x0, x1, y0, y1, z0, z1) that can receive a sample when a source volume of
    src_dims voxels over src_size_m metres is fused through `src_to_dst` (hsk_fuse_footprint); all zeros when empty"""
    sd = np.ascontiguousarray(src_dims, np.int32).reshape(3)
    dd = np.ascontiguousarray(dst_dims, np.int32).reshape(3)
    ss = np.ascontiguousarray(src_size_m, np.float32).reshape(3)
    ds = np.ascontiguousarray(dst_size_m, np.float32).reshape(3)
    m = np.ascontiguousarray(src_to_dst, np.float32).reshape(16)
    box = np.zeros(6, np.int32)
    ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
    _ck(_lib.load().hsk_fuse_footprint(sd.ctypes.data_as(ip), ss.ctypes.data_as(fp), dd.ctypes.data_as(ip), ds.ctypes.data_as(fp),
                                       m.ctypes.data_as(fp), box.ctypes.data_as(C.POINTER(C.c_int32))), "hsk_fuse_footprint")
    return tuple(int(x) for x in box)


def composite_views(rgbs, depths, background=(0, 0, 0), *, want_rgb=True):
    """images of one size, one per room (KinfuTracker.render_section's rgb and depth) -> (rgb, depth, index): per pixel the
    view with the smallest non-zero depth, the lowest index on a tie; background, 0 and -1 where no view has a depth
    (hsk_composite_views).  rgbs may be None with want_rgb=False (rgb is then None)"""
    deps = [np.ascontiguousarray(d, np.uint16) for d in depths]
    n = len(deps)
    if n < 1 or any(d.shape != deps[0].shape or d.ndim != 2 for d in deps):
        raise ValueError("composite_views: at least one (h, w) depth image, all of one size")
    h, w = deps[0].shape
    cols = None
    if want_rgb:
        cols = [np.ascontiguousarray(c, np.uint8) for c in rgbs]
        if len(cols) != n or any(c.shape != (h, w, 3) for c in cols):
            raise ValueError("composite_views: one (h, w, 3) rgb image per depth image")
    bg = np.asarray(background, np.uint8).reshape(3).copy()
    out_rgb = np.empty((h, w, 3), np.uint8) if want_rgb else None
    out_dep = np.empty((h, w), np.uint16)
    out_idx = np.empty((h, w), np.int32)
    dp = (C.c_void_p * n)(*[d.ctypes.data for d in deps])
    cp = (C.c_void_p * n)(*[c.ctypes.data for c in cols]) if want_rgb else None
    _ck(_lib.load().hsk_composite_views(n, cp, dp, w, h, bg.ctypes.data, None if out_rgb is None else out_rgb.ctypes.data,
                                        out_dep.ctypes.data, out_idx.ctypes.data), "hsk_composite_views")
    return out_rgb, out_dep, out_idx


def write_xf(path, m):
    lib = _lib.load()
    a = np.ascontiguousarray(m, np.float32).reshape(16)
    _ck(lib.hsk_write_xf(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_float))), "hsk_write_xf")


def read_xf(path):
    lib = _lib.load()
    a = np.empty(16, np.float32)
    _ck(lib.hsk_read_xf(os.fsencode(path), a.ctypes.data_as(C.POINTER(C.c_float))), "hsk_read_xf")
    return a.reshape(4, 4)


def transform_cloud(xyz, m):
    lib = _lib.load()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    a = np.ascontiguousarray(m, np.float32).reshape(16)
    out = np.empty_like(pts)
    _ck(lib.hsk_transform_cloud(pts.ctypes.data, len(pts), a.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data), "hsk_transform_cloud")
    return out


def transform_normals(normals, m):
    """normals by the rotation part of a row-major .xf matrix (no translation, no renormalisation; NaN stays NaN)"""
    lib = _lib.load()
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    a = np.ascontiguousarray(m, np.float32).reshape(16)
    out = np.empty_like(n)
    _ck(lib.hsk_transform_normals(n.ctypes.data, len(n), a.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data), "hsk_transform_normals")
    return out


class DepthStreamWriter:
    """HSKD raw depth recording (frames in the layout of HoniHelper.takeDepthSnapshot)."""

    def __init__(self, path, w=640, h=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5):
        self.lib = _lib.load()
        self.h = self.lib.hsk_stream_create(os.fsencode(path), w, h, fx, fy, cx, cy)
        if not self.h:
            raise RuntimeError(f"cannot create {path}")
        self.shape = (h, w)

    def write(self, depth):
        d = np.ascontiguousarray(depth, np.uint16)
        assert d.shape == self.shape
        _ck(self.lib.hsk_stream_write(self.h, d.ctypes.data), "hsk_stream_write")

    def close(self):
        if self.h:
            _ck(self.lib.hsk_stream_close(self.h), "hsk_stream_close")
            self.h = None


class DepthStreamReader:
    def __init__(self, path):
        self.lib = _lib.load()
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        intr = (C.c_float * 4)()
        self.h = self.lib.hsk_stream_open(os.fsencode(path), C.byref(w), C.byref(h), C.byref(n), intr)
        if not self.h:
            raise RuntimeError(f"{path} is not an HSKD stream")
        self.w, self.hgt, self.n, self.intr = w.value, h.value, n.value, tuple(intr)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        d = np.empty((self.hgt, self.w), np.uint16)
        rc = self.lib.hsk_stream_read(self.h, int(i), d.ctypes.data)
        if rc != 0:
            raise IndexError(i)
        return d

    def close(self):
        if self.h:
            self.lib.hsk_stream_close(self.h)
            self.h = None
