"""numpy restatement of hsk_extract_mesh_simplified (include/hskinfu.h): quadric vertex clustering of the indexed
marching-cubes mesh (tests/mesh_twin.py, imported and left as it is) on cells of c voxels.  Integer sums per cluster, a binary64
solve in the order of housescan_amd/csrc/hsk_simplify_point.h -- every operator here is one IEEE operation on float64 arrays,
and a rotation that the C text skips (a[p][q] == 0) is skipped here by selecting the old values, never by rotating by zero."""
import numpy as np

from mesh_twin import mesh_indexed

f32, f64, i64 = np.float32, np.float64, np.int64
UNIT = 256
SWEEPS = 8
QUADRIC, MEAN = 0, 1
SHIFT = {2: 1, 4: 2, 8: 3, 16: 4}


def quantised_vertices(vol, edges):
    """the positions of the indexed mesh's vertices in 1/256 voxel, [n, 3] int64: 256 g, and on the edge's axis
    + (512 |Fa| + D) // (2 D), D = |Fb - Fa|, from the stored int16 values"""
    t = vol[..., 0].astype(i64)
    ez, ey, ex, ek = (edges[:, i].astype(i64) for i in range(4))
    fa = t[ez, ey, ex]
    fb = t[ez + (ek == 2), ey + (ek == 1), ex + (ek == 0)]
    d = np.abs(fb - fa)
    q = (512 * np.abs(fa) + d) // (2 * d)
    g = np.stack([ex, ey, ez], axis=1)
    p = UNIT * g
    p[np.arange(len(p)), ek] += q
    return p, g


def jacobi(A):
    """A [n, 3, 3] symmetric float64 -> (eigenvalues [n, 3] = the diagonal after SWEEPS cyclic sweeps, V [n, 3, 3], columns)"""
    a = A.copy()
    n = len(a)
    v = np.zeros((n, 3, 3), f64)
    v[:, 0, 0] = v[:, 1, 1] = v[:, 2, 2] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = a[:, p, q].copy()
                on = apq != 0.0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                mag = np.where(theta < 0.0, -theta, theta)
                t = 1.0 / (mag + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                app = a[:, p, p] - t * apq
                aqq = a[:, q, q] + t * apq
                arp = c * a[:, r, p] - s * a[:, r, q]
                arq = s * a[:, r, p] + c * a[:, r, q]
                vp = c[:, None] * v[:, :, p] - s[:, None] * v[:, :, q]
                vq = s[:, None] * v[:, :, p] + c[:, None] * v[:, :, q]
                a[:, p, p] = np.where(on, app, a[:, p, p])
                a[:, q, q] = np.where(on, aqq, a[:, q, q])
                zero = np.where(on, 0.0, a[:, p, q])
                a[:, p, q] = zero
                a[:, q, p] = zero
                a[:, r, p] = a[:, p, r] = np.where(on, arp, a[:, r, p])
                a[:, r, q] = a[:, q, r] = np.where(on, arq, a[:, r, q])
                v[:, :, p] = np.where(on[:, None], vp, v[:, :, p])
                v[:, :, q] = np.where(on[:, None], vq, v[:, :, q])
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), v


def cluster_vertex(sums, c, mode=QUADRIC, sv_floor=1e-3):
    """hsk_simplify_point.h's simp_vertex on rows of 16 sums [n, 16] int64 -> (x [n, 3] float64 in 1/256 voxel relative to the
    cell's centre, rank [n], clamped [n] bool)"""
    s = np.asarray(sums, i64).reshape(-1, 16)
    n = s[:, 0].astype(f64)
    m = np.stack([s[:, 1].astype(f64) / n, s[:, 2].astype(f64) / n, s[:, 3].astype(f64) / n], axis=1)
    x = m.copy()
    rank = np.zeros(len(s), np.int64)
    if mode == QUADRIC and len(s):
        A = np.empty((len(s), 3, 3), f64)
        for (i, j), col in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(7, 13)):
            A[:, i, j] = A[:, j, i] = s[:, col].astype(f64)
        lam, v = jacobi(A)
        r = np.stack([s[:, 13 + k].astype(f64) - ((A[:, k, 0] * m[:, 0] + A[:, k, 1] * m[:, 1]) + A[:, k, 2] * m[:, 2]) for k in range(3)], axis=1)
        lmax = np.maximum(np.maximum(lam[:, 0], lam[:, 1]), lam[:, 2])
        cut = f64(f32(sv_floor)) * lmax
        with np.errstate(all="ignore"):
            for i in range(3):
                keep = (lmax > 0.0) & (lam[:, i] > cut)
                coef = ((v[:, 0, i] * r[:, 0] + v[:, 1, i] * r[:, 1]) + v[:, 2, i] * r[:, 2]) / lam[:, i]
                for k in range(3):
                    x[:, k] = np.where(keep, x[:, k] + v[:, k, i] * coef, x[:, k])
                rank += keep
    clamped = np.zeros(len(s), bool)
    if mode == QUADRIC:
        lim = f64((UNIT // 2) * c + UNIT)
        clamped = (np.abs(x) > lim).any(axis=1)
        x = np.minimum(np.maximum(x, -lim), lim)
    return x, rank, clamped


def simplify(vol, ntri, codes, c=4, mode=QUADRIC, sv_floor=1e-3, size=3.0, col=None, mesh=None):
    """vol [Z, Y, X, 2] int16, col [Z, Y, X, 4] uint8 or None -> dict(vertices [n, 3] f32, normals [n, 3] f32, rgb [n, 3] uint8 or
    None, faces [m, 3] int32, stats (hsk_simplify_stats as a dict), and for the tests: clusters [n] (the output clusters' numbers),
    sums [n, 20] int64, x [n, 3] float64 (1/256 voxel relative to the cell's centre), pos_q [n, 3] float64 (absolute, 1/256
    voxel), rank [n]).  mesh: mesh_indexed's result on the same volume, when the caller has it"""
    Z, Y, X, _ = vol.shape
    s = SHIFT[c]
    CX, CY = (X + c - 1) >> s, (Y + c - 1) >> s
    if mesh is None:
        mesh = mesh_indexed(vol, ntri, codes, size=size, col=col, normals=False)
    faces_in = mesh["faces"].astype(i64)
    p, g = quantised_vertices(vol, mesh["edges"])
    cl3 = g >> s
    cl = (cl3[:, 2] * CY + cl3[:, 1]) * CX + cl3[:, 0]
    centre = UNIT * c * cl3 + (UNIT // 2) * c
    fc = cl[faces_in] if len(faces_in) else np.zeros((0, 3), i64)
    survive = (fc[:, 0] != fc[:, 1]) & (fc[:, 0] != fc[:, 2]) & (fc[:, 1] != fc[:, 2])
    out_cl = np.unique(fc[survive])
    faces = np.searchsorted(out_cl, fc[survive]).astype(np.int32)
    n_out = len(out_cl)
    sums = np.zeros((n_out, 20), i64)
    if n_out:
        def slot(ids):
            """(the members of `ids` that are output clusters, their output numbers)"""
            at = np.minimum(np.searchsorted(out_cl, ids), n_out - 1)
            ok = out_cl[at] == ids
            return ok, at[ok]
        ok, at = slot(cl)
        rel = (p - centre)[ok]
        np.add.at(sums[:, 0], at, 1)
        for k in range(3):
            np.add.at(sums[:, 1 + k], at, rel[:, k])
        if col is not None:
            # (a vertex is uncoloured when neither end of its edge has colour weight: mesh_indexed writes (0, 0, 0) for it and counts
            # it, but keeps no mask)
            rgb_in = mesh["rgb"].astype(i64)
            e = mesh["edges"].astype(i64)
            bz, by, bx = e[:, 0] + (e[:, 3] == 2), e[:, 1] + (e[:, 3] == 1), e[:, 2] + (e[:, 3] == 0)
            coloured = (col[e[:, 0], e[:, 1], e[:, 2], 3] != 0) | (col[bz, by, bx, 3] != 0)
            assert int((~coloured).sum()) == mesh["n_uncolored"]
            okc = ok & coloured
            atc = np.searchsorted(out_cl, cl[okc])
            for k in range(3):
                np.add.at(sums[:, 16 + k], atc, rgb_in[okc, k])
            np.add.at(sums[:, 19], atc, 1)
        # the triangles, once per cluster they touch: corner q's cluster takes it unless an earlier corner's is the same
        for q in range(3):
            first = np.ones(len(fc), bool)
            for e in range(q):
                first &= fc[:, e] != fc[:, q]
            ok, at = slot(np.where(first, fc[:, q], -1))
            f = faces_in[ok]
            ctr = centre[f[:, q]]
            p0, p1, p2 = p[f[:, 0]] - ctr, p[f[:, 1]] - ctr, p[f[:, 2]] - ctr
            N = np.cross(p1 - p0, p2 - p0)
            dN = (N * p0).sum(axis=1)
            for k in range(3):
                np.add.at(sums[:, 4 + k], at, N[:, k])
                np.add.at(sums[:, 13 + k], at, N[:, k] * dN)
            for col_, (i, j) in zip(range(7, 13), ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                np.add.at(sums[:, col_], at, N[:, i] * N[:, j])
    x, rank, clamped = cluster_vertex(sums[:, :16], c, mode, sv_floor) if n_out else (np.zeros((0, 3)), np.zeros(0, i64), np.zeros(0, bool))
    out3 = np.stack([out_cl % CX, (out_cl // CX) % CY, out_cl // (CX * CY)], axis=1) if n_out else np.zeros((0, 3), i64)
    sizes = (size,) * 3 if np.isscalar(size) else tuple(size)
    cell = np.array([f32(sizes[0]) / f32(X), f32(sizes[1]) / f32(Y), f32(sizes[2]) / f32(Z)], f32)
    pv = (c * out3 + c // 2).astype(f64) + x / f64(UNIT)
    verts = ((pv + 0.5) * cell.astype(f64)[None, :]).astype(f32)
    sn = sums[:, 4:7]
    with np.errstate(all="ignore"):
        nm = sn.astype(f64) / cell.astype(f64)[None, :]
        inv = 1.0 / np.sqrt((nm[:, 0] * nm[:, 0] + nm[:, 1] * nm[:, 1]) + nm[:, 2] * nm[:, 2])
        normals = (nm * inv[:, None]).astype(f32)
    normals[(sn == 0).all(axis=1)] = np.nan
    rgb, n_unc = None, 0
    if col is not None:
        nc = sums[:, 19]
        safe = np.maximum(nc, 1)
        rgb = np.where((nc > 0)[:, None], (sums[:, 16:19] + (nc // 2)[:, None]) // safe[:, None], 0).astype(np.uint8)
        n_unc = int((nc == 0).sum())
    stats = dict(n_in_vertices=len(p), n_in_faces=len(faces_in), n_clusters=len(np.unique(cl)), n_out_vertices=n_out, n_out_faces=len(faces),
                 n_faces_collapsed=len(faces_in) - len(faces), n_rank=[int((rank == r).sum()) for r in range(4)], n_clamped=int(clamped.sum()),
                 n_uncolored=n_unc)
    return dict(vertices=verts, normals=normals, rgb=rgb, faces=faces, stats=stats, clusters=out_cl, sums=sums, x=x, rank=rank,
                pos_q=f64(UNIT) * (c * out3 + c // 2).astype(f64) + x)
