"""Surface components, restated in numpy (include/hskinfu.h "Surface components"): the rule the kernels of
housescan_amd/csrc/components.hip implement, in the plainest form that is still fast enough for a test.  All integers.

A voxel of a volume [Z, Y, X, 2] (tsdf, weight; int16) is INSIDE iff weight != 0 and tsdf < 0.  Two INSIDE voxels are adjacent when
they differ by 1 on exactly one axis.  lin(x, y, z) = (z Y + y) X + x; an INSIDE voxel's label is the smallest lin of its component,
every other voxel's NONE.  Records: root (x, y, z), n_voxels, the box lo, hi (exclusive), ordered by n_voxels descending, ties to
the smaller root.  Prune: a component goes iff n_voxels < min_voxels or (keep_largest > 0 and rank >= keep_largest); its voxels
become (0, 0) (fill UNSEEN) or (32767, weight) (fill FREE), their colour words 0."""
import numpy as np

NONE = 0xFFFFFFFF
UNSEEN, FREE = 0, 1
COMPONENT_DTYPE = np.dtype([("root", "<i4", (3,)), ("pad", "<i4"), ("n_voxels", "<u8"), ("lo", "<i4", (3,)), ("hi", "<i4", (3,))])
f32 = np.float32


def inside(vol):
    return (vol[..., 1] != 0) & (vol[..., 0] < 0)


def labels(vol):
    """[Z, Y, X] uint32.  A union-find over the pairs of adjacent INSIDE voxels: every round hooks the larger of a pair's two roots
    to the smaller (a minimum, so the order of the pairs does not matter) and then shortens every path to its root; it ends when
    every pair has one root.  parent[v] <= v throughout, so a root is its component's smallest lin."""
    m = inside(vol)
    Z, Y, X = m.shape
    lin = np.arange(Z * Y * X, dtype=np.int64).reshape(Z, Y, X)
    a, b = [], []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        both = m[tuple(lo)] & m[tuple(hi)]
        a.append(lin[tuple(lo)][both])
        b.append(lin[tuple(hi)][both])
    a, b = np.concatenate(a), np.concatenate(b)
    parent = np.arange(Z * Y * X, dtype=np.int64)
    while True:
        while True:                                  # every entry -> its root
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        ra, rb = parent[a], parent[b]
        open_ = ra != rb
        if not open_.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[open_], np.minimum(ra, rb)[open_])
    out = np.where(m, parent.reshape(Z, Y, X), NONE).astype(np.uint32)
    return out


def records(vol, lab=None):
    """the components' records, in their order -> a structured array with COMPONENT_DTYPE"""
    lab = labels(vol) if lab is None else lab
    Z, Y, X = lab.shape
    z, y, x = np.nonzero(lab != NONE)
    roots, inv, counts = np.unique(lab[z, y, x], return_inverse=True, return_counts=True)
    rec = np.zeros(len(roots), COMPONENT_DTYPE)
    r = roots.astype(np.int64)
    rec["root"] = np.stack([r % X, (r // X) % Y, r // (X * Y)], -1)
    rec["n_voxels"] = counts
    for k, c in enumerate((x, y, z)):
        lo = np.full(len(roots), np.iinfo(np.int64).max)
        hi = np.full(len(roots), -1)
        np.minimum.at(lo, inv, c)
        np.maximum.at(hi, inv, c)
        rec["lo"][:, k] = lo
        rec["hi"][:, k] = hi + 1
    order = np.lexsort((r, -counts.astype(np.int64)))   # (the last key is the primary one)
    return rec[order]


def root_lin(rec, dims):
    """lin of the records' roots; dims = (X, Y, Z)"""
    r = rec["root"].astype(np.int64)
    return (r[:, 2] * dims[1] + r[:, 1]) * dims[0] + r[:, 0]


def stats(rec):
    return {"n_components": len(rec), "n_inside": int(rec["n_voxels"].sum()), "largest": int(rec["n_voxels"][0]) if len(rec) else 0}


def pruned_mask(rec, min_voxels, keep_largest):
    """which records go: n_voxels < min_voxels, or keep_largest > 0 and rank >= keep_largest"""
    rank = np.arange(len(rec))
    return (rec["n_voxels"] < np.uint64(min_voxels)) | ((keep_largest > 0) & (rank >= keep_largest))


def prune(vol, colour=None, min_voxels=0, keep_largest=0, fill=UNSEEN):
    """-> (volume, colour or None, stats): the volume with the pruned components' voxels filled, every other word as it was;
    colour: the (r, g, b, w) volume [Z, Y, X, 4] uint8, the pruned voxels' words 0"""
    lab = labels(vol)
    rec = records(vol, lab)
    Z, Y, X = lab.shape
    go = pruned_mask(rec, min_voxels, keep_largest)
    hit = np.isin(lab, root_lin(rec[go], (X, Y, Z)).astype(np.uint32)) & (lab != NONE)
    out = vol.copy()
    if fill == UNSEEN:
        out[hit] = 0
    else:
        out[hit, 0] = 32767
    col = None
    if colour is not None:
        col = colour.copy()
        col[hit] = 0
    st = {"n_components": len(rec), "n_pruned": int(go.sum()), "n_pruned_voxels": int(rec["n_voxels"][go].sum()),
          "n_kept_voxels": int(rec["n_voxels"][~go].sum())}
    return out, col, st


def default_min_voxels(size, dims, tau):
    """ceil((4 tau)^3 / (cell_x cell_y cell_z)) in binary64 from the binary32 truncation distance and cells"""
    cell = [float(f32(size[i]) / f32(dims[i])) for i in range(3)]
    e = 4.0 * float(f32(tau))
    return int(np.ceil(((e * e) * e) / ((cell[0] * cell[1]) * cell[2])))


def blocked_labels(lab):
    """a label volume [Z, Y, X] as the device stores its parents: the volume's 64-B block layout, padding planes NONE"""
    Z, Y, X = lab.shape
    out = np.full(X * Y * ((Z + 3) & ~3), NONE, np.uint32)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    idx = ((((z >> 2) * Y + y) * (X // 4) + (x >> 2)) * 16) + (z & 3) * 4 + (x & 3)
    out[idx.reshape(-1)] = lab.reshape(-1)
    return out
