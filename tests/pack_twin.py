"""The "HSKV" version 1 sparse volume image restated in numpy, from the rule: what hsk_pack_volume's bytes are
compared against, bit for bit.

The volume is cut into bricks of 8 x 8 x 8 voxels of the stored planes, ordered (bz, by, bx) with bx fastest; inside a brick the
voxels run (z, y, x) with x fastest; voxels of the last brick layer beyond the stored planes count as word 0 when packing and are
dropped when unpacking.  A voxel's word is (uint16)tsdf | (uint16)weight << 16.

    header (256 B) | TSDF class table | TSDF payload | [colour class table | colour payload]

Class table: one byte per brick, zero-padded to a multiple of 8.  TSDF classes: 0 ZERO (every word 0), 1 UNIFORM (every word
equal, not 0: the word, 4 B), 2 SPLIT (every tsdf equal, every weight in 0..255, neither of the above: int16 tsdf, uint16 0,
512 weight bytes), 3 RAW (512 words).  Colour classes: 0 ZERO, 3 RAW (512 rgbw words).  The payload is the records of the
non-ZERO bricks in brick order, back to back.
"""
import struct

import numpy as np

HEADER_BYTES = 256
ZERO, UNIFORM, SPLIT, RAW = 0, 1, 2, 3
REC_BYTES = {ZERO: 0, UNIFORM: 4, SPLIT: 516, RAW: 2048}

# the header's fields: (name, byte offset, struct format); little-endian, zero elsewhere
FIELDS = [
    ("magic", 0, "4s"), ("version", 4, "I"), ("header_bytes", 8, "I"), ("flags", 12, "I"),
    ("dims", 16, "3i"), ("z0", 28, "i"), ("nz", 32, "i"), ("size_m", 36, "3f"),
    ("trunc_dist_m", 48, "f"), ("trunc_eff_m", 52, "f"),
    ("width", 56, "i"), ("height", 60, "i"), ("fx", 64, "f"), ("fy", 68, "f"), ("cx", 72, "f"), ("cy", 76, "f"),
    ("pose", 80, "16f"), ("frame", 144, "i"), ("color_max_weight", 148, "i"), ("color_band_m", 152, "f"),
    ("n_bricks", 160, "Q"), ("tsdf_bricks", 168, "4Q"), ("color_bricks", 200, "2Q"),
    ("tsdf_table_bytes", 216, "Q"), ("tsdf_payload_bytes", 224, "Q"),
    ("color_table_bytes", 232, "Q"), ("color_payload_bytes", 240, "Q"), ("total_bytes", 248, "Q"),
]


def default_fields(dims, **over):
    """header fields a test need not care about: a 3 m cube, the default camera, the identity pose"""
    f = dict(dims=tuple(int(d) for d in dims), z0=0, nz=int(dims[2]), size_m=(3.0, 3.0, 3.0), trunc_dist_m=0.03, trunc_eff_m=0.05,
             width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5, pose=tuple(np.eye(4, dtype=np.float32).reshape(-1)),
             frame=0, color_max_weight=0, color_band_m=0.0)
    f.update(over)
    return f


def words_of(tsdf):
    """[nz, Y, X, 2] int16 pairs -> [nz, Y, X] uint32 words"""
    t = np.ascontiguousarray(tsdf, np.int16).view(np.uint16).astype(np.uint32)
    return t[..., 0] | (t[..., 1] << 16)


def bricks_of(words):
    """[nz, Y, X] uint32 -> [n_bricks, 512] in brick order, voxels (z, y, x) inside; the last layer padded with 0"""
    nz, Y, X = words.shape
    assert Y % 8 == 0 and X % 8 == 0
    nbz = (nz + 7) // 8
    pad = np.zeros((nbz * 8, Y, X), np.uint32)
    pad[:nz] = words
    b = pad.reshape(nbz, 8, Y // 8, 8, X // 8, 8).transpose(0, 2, 4, 1, 3, 5)
    return np.ascontiguousarray(b).reshape(-1, 512)


def unbricks(bricks, nz, Y, X):
    nbz = (nz + 7) // 8
    b = bricks.reshape(nbz, Y // 8, X // 8, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5)
    return np.ascontiguousarray(b).reshape(nbz * 8, Y, X)[:nz]


def classify_tsdf(bricks):
    zero = (bricks == 0).all(axis=1)
    uniform = (bricks == bricks[:, :1]).all(axis=1) & ~zero
    t = bricks & 0xFFFF
    split = (t == t[:, :1]).all(axis=1) & ((bricks >> 16) <= 255).all(axis=1) & ~zero & ~uniform
    cls = np.full(len(bricks), RAW, np.uint8)
    cls[split] = SPLIT
    cls[uniform] = UNIFORM
    cls[zero] = ZERO
    return cls


def classify_color(bricks):
    return np.where((bricks == 0).all(axis=1), ZERO, RAW).astype(np.uint8)


def _table(cls):
    out = np.zeros((len(cls) + 7) // 8 * 8, np.uint8)
    out[:len(cls)] = cls
    return out.tobytes()


def _payload_tsdf(bricks, cls):
    parts = []
    for b, c in zip(bricks[cls != ZERO], cls[cls != ZERO]):
        if c == UNIFORM:
            parts.append(b[:1].astype("<u4").tobytes())
        elif c == SPLIT:
            parts.append(struct.pack("<HH", int(b[0] & 0xFFFF), 0) + (b >> 16).astype(np.uint8).tobytes())
        else:
            parts.append(b.astype("<u4").tobytes())
    return b"".join(parts)


def write_header(f):
    head = bytearray(HEADER_BYTES)
    for name, at, fmt in FIELDS:
        v = f[name]
        struct.pack_into("<" + fmt, head, at, *(tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else (v,)))
    return bytes(head)


def read_header(image):
    f = {}
    for name, at, fmt in FIELDS:
        v = struct.unpack_from("<" + fmt, image, at)
        f[name] = v[0] if len(v) == 1 else tuple(v)
    return f


def pack(tsdf, color, fields):
    """tsdf [nz, Y, X, 2] int16, color [nz, Y, X, 4] uint8 or None, fields: default_fields()'s keys -> the image's bytes"""
    nz, Y, X = tsdf.shape[:3]
    assert tuple(fields["dims"][:2]) == (X, Y) and fields["nz"] == nz
    tb = bricks_of(words_of(tsdf))
    tc = classify_tsdf(tb)
    sections = [_table(tc), _payload_tsdf(tb, tc)]
    f = dict(fields, magic=b"HSKV", version=1, header_bytes=HEADER_BYTES, flags=0 if color is None else 1, n_bricks=len(tb),
             tsdf_bricks=tuple(int((tc == c).sum()) for c in range(4)), color_bricks=(0, 0))
    f["pose"] = tuple(np.asarray(fields["pose"], np.float32).reshape(-1))
    if color is not None:
        cb = bricks_of(np.ascontiguousarray(color, np.uint8).view("<u4")[..., 0])
        cc = classify_color(cb)
        sections += [_table(cc), cb[cc == RAW].astype("<u4").tobytes()]
        f["color_bricks"] = (int((cc == ZERO).sum()), int((cc == RAW).sum()))
    else:
        sections += [b"", b""]
    (f["tsdf_table_bytes"], f["tsdf_payload_bytes"], f["color_table_bytes"], f["color_payload_bytes"]) = (len(s) for s in sections)
    f["total_bytes"] = HEADER_BYTES + sum(len(s) for s in sections)
    return write_header(f) + b"".join(sections)


def info(image):
    """the header's fields, and where the sections lie: "at" = (tsdf table, tsdf payload, colour table, colour payload, end)"""
    f = read_header(image)
    at = [HEADER_BYTES]
    for key in ("tsdf_table_bytes", "tsdf_payload_bytes", "color_table_bytes", "color_payload_bytes"):
        at.append(at[-1] + f[key])
    f["at"] = tuple(at)
    return f


def _unpack_records(image, at, cls, color):
    bricks = np.zeros((len(cls), 512), np.uint32)
    for i, c in enumerate(cls):
        if c == ZERO:
            continue
        if c == UNIFORM and not color:
            bricks[i] = np.frombuffer(image, "<u4", 1, at)[0]
        elif c == SPLIT and not color:
            t = struct.unpack_from("<H", image, at)[0]
            bricks[i] = t | (np.frombuffer(image, np.uint8, 512, at + 4).astype(np.uint32) << 16)
        else:
            assert c == RAW
            bricks[i] = np.frombuffer(image, "<u4", 512, at)
        at += REC_BYTES[int(c)]
    return bricks, at


def unpack(image):
    """-> (tsdf [nz, Y, X, 2] int16, color [nz, Y, X, 4] uint8 or None, header fields)"""
    f = info(image)
    assert f["magic"] == b"HSKV" and f["version"] == 1 and f["total_bytes"] == len(image)
    X, Y, _ = f["dims"]
    nz, n = f["nz"], f["n_bricks"]
    cls = np.frombuffer(image, np.uint8, n, f["at"][0])
    bricks, end = _unpack_records(image, f["at"][1], cls, False)
    assert end == f["at"][2]
    w = unbricks(bricks, nz, Y, X)
    tsdf = np.stack([(w & 0xFFFF).astype(np.uint16).view(np.int16), (w >> 16).astype(np.uint16).view(np.int16)], axis=-1)
    color = None
    if f["flags"] & 1:
        ccls = np.frombuffer(image, np.uint8, n, f["at"][2])
        cbricks, end = _unpack_records(image, f["at"][3], ccls, True)
        assert end == f["at"][4]
        color = np.ascontiguousarray(unbricks(cbricks, nz, Y, X).astype("<u4")).view(np.uint8).reshape(nz, Y, X, 4)
    return tsdf, color, f


def crafted_volume(dims, seed=0, color=True):
    """a random volume of dims (X, Y, Z) that holds every class: ZERO, UNIFORM, SPLIT (a tsdf != 0 under weight 0 among them),
    RAW, a brick that is RAW only because one weight is 256, and, with colour, ZERO and RAW colour bricks"""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    nb = (X // 8, Y // 8, (Z + 7) // 8)
    kind = rng.integers(0, 6, (nb[2], nb[1], nb[0]))
    kind.reshape(-1)[:6] = np.arange(6)            # every kind at least once
    tsdf = np.zeros((Z, Y, X, 2), np.int16)
    col = np.zeros((Z, Y, X, 4), np.uint8) if color else None
    for bz in range(nb[2]):
        for by in range(nb[1]):
            for bx in range(nb[0]):
                s = (slice(8 * bz, min(8 * bz + 8, Z)), slice(8 * by, 8 * by + 8), slice(8 * bx, 8 * bx + 8))
                shp = tsdf[s].shape[:3]
                k = kind[bz, by, bx]
                if k == 1:      # UNIFORM (in a last, partial layer the padding makes it SPLIT or RAW: a case of its own)
                    tsdf[s] = (int(rng.integers(-32767, 32768)), int(rng.integers(1, 129)))
                elif k == 2:    # SPLIT: free space, byte weights
                    tsdf[s + (0,)] = 32767
                    tsdf[s + (1,)] = rng.integers(0, 256, shp)
                elif k == 3:    # RAW
                    tsdf[s + (0,)] = rng.integers(-32767, 32768, shp)
                    tsdf[s + (1,)] = rng.integers(0, 129, shp)
                elif k == 4:    # one tsdf, but a weight of 256: RAW
                    tsdf[s + (0,)] = -5
                    tsdf[s + (1,)] = rng.integers(1, 256, shp)
                    tsdf[s][0, 3, 5, 1] = 256
                elif k == 5:    # a tsdf != 0 under weight 0 everywhere: UNIFORM by its word, not ZERO
                    tsdf[s + (0,)] = 77
                if color and k in (3, 4) and rng.random() < 0.7:
                    col[s] = rng.integers(0, 256, shp + (4,))
    if color:
        col[0:1, 0:8, 0:8] = 9      # a RAW colour brick for certain
    return tsdf, col
