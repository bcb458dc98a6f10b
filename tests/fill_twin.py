"""The hole-filling rule (include/hskinfu.h "Hole filling") in numpy: padded arrays and shifts, no skip logic.
A volume is [Z, Y, X, 2] int16 (tsdf raw, weight) as everywhere in the tests; a box is ((x, y, z) lo, (x, y, z) hi)."""
import numpy as np

UNKNOWN = -32768
SURFACE, ALL = 0, 1
# the six face neighbours as (array axis, step): -x, +x, -y, +y, -z, +z
NEIGHBOURS = ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))


def initial_states(vol):
    """[Z, Y, X] int32: a source's value (its raw TSDF, -32768 counting as -32767), UNKNOWN elsewhere"""
    raw = vol[..., 0].astype(np.int32)
    return np.where(vol[..., 1] != 0, np.maximum(raw, -32767), UNKNOWN).astype(np.int32)


def box_mask(shape, box):
    m = np.zeros(shape, bool)
    if box is None:
        m[...] = True
    else:
        (x0, y0, z0), (x1, y1, z1) = box
        m[z0:z1, y0:y1, x0:x1] = True
    return m


def shifted(a, axis, step, fill):
    """b[v] = a[v + step along axis], `fill` where that lies outside the grid"""
    k = abs(step)
    pad = [(0, 0)] * 3
    pad[axis] = (k, k)
    p = np.pad(a, pad, constant_values=fill)
    sl = [slice(None)] * 3
    sl[axis] = slice(k + step, k + step + a.shape[axis])
    return p[tuple(sl)]


def step(state, free):
    """one Jacobi iteration: the FREE voxels (non-sources inside the box) from the seven states of the previous one"""
    seven = [state] + [shifted(state, ax, d, UNKNOWN) for ax, d in NEIGHBOURS]
    n = np.zeros(state.shape, np.int64)
    U = np.zeros(state.shape, np.int64)
    for s in seven:
        known = s != UNKNOWN
        n += known
        U += np.where(known, s.astype(np.int64) + 32768, 0)
    mean = (2 * U + n) // np.maximum(2 * n, 1) - 32768
    new = np.where(n > 0, mean, UNKNOWN).astype(np.int32)
    return np.where(free, new, state)


def iterate(vol, iterations, box=None):
    """-> (final states, free, iterations_run): iterations_run is the number of the first iteration that changed no state, or
    `iterations`.  Every iteration asked for is computed: no early stop."""
    state = initial_states(vol)
    free = (vol[..., 1] == 0) & box_mask(state.shape, box)
    run = iterations
    for i in range(1, iterations + 1):
        new = step(state, free)
        if run == iterations and i < iterations and np.array_equal(new, state):
            run = i
        state = new
    return state, free, run


def crossing_voxels(state):
    """the voxels of a crossing: two face-adjacent KNOWN voxels, neither at 32767, one value > 0 and the other < 0"""
    usable = (state != UNKNOWN) & (state != 32767)
    out = np.zeros(state.shape, bool)
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        ok = usable[a] & usable[b] & (((state[a] > 0) & (state[b] < 0)) | ((state[a] < 0) & (state[b] > 0)))
        out[a] |= ok
        out[b] |= ok
    return out


def dilate(m, band):
    """the voxels within Chebyshev distance `band` of a set one"""
    out = m.copy()
    for ax in range(3):
        src = out.copy()
        for d in range(1, band + 1):
            out |= shifted(src, ax, d, False) | shifted(src, ax, -d, False)
    return out


def fill(vol, iterations, keep=SURFACE, band=2, fill_weight=1, box=None):
    """-> (the filled volume, the mask [Z, Y, X] uint8, stats without tile_visits)"""
    state, free, run = iterate(vol, iterations, box)
    filled = free & (state != UNKNOWN)
    written = filled if keep == ALL else filled & dilate(crossing_voxels(state), band)
    out = vol.copy()
    out[written, 0] = state[written].astype(np.int16)
    out[written, 1] = fill_weight
    stats = {"n_unseen": int(free.sum()), "n_reached": int(filled.sum()), "n_written": int(written.sum()),
             "n_written_negative": int((written & (state < 0)).sum()), "iterations_run": run}
    return out, written.astype(np.uint8), stats


def default_iterations(cells):
    """hsk_default_fill_params' iterations from the binary32 cells"""
    m = float(min(np.float32(c) for c in cells))
    return int(min(max(np.ceil(0.15 / m), 1), 255))


# ---- the planar wall with a hole (the issue's property case) -------------------------------------------------------------------------
def planar_wall(X=40, Y=40, Z=48, z0=30.3, tau=3.0, hole=12, hole_from=18, shift=(0, 0)):
    """the wall at z0 voxels, raw = rint(clip((z0 - z) / tau) 32767), observed with weight 1 for z < z0 + tau; a hole x hole column
    hole centred in x and y (moved by `shift`), never observed from z = hole_from on -> (volume, (x0, x1, y0, y1) of the hole)"""
    vol = np.zeros((Z, Y, X, 2), np.int16)
    z = np.arange(Z, dtype=np.float64)
    raw = np.rint(np.clip((z0 - z) / tau, -1.0, 1.0) * 32767).astype(np.int16)
    seen = z < z0 + tau
    vol[seen, :, :, 0] = raw[seen, None, None]
    vol[seen, :, :, 1] = 1
    x0, y0 = (X - hole) // 2 + shift[0], (Y - hole) // 2 + shift[1]
    vol[hole_from:, y0:y0 + hole, x0:x0 + hole] = 0
    return vol, (x0, x0 + hole, y0, y0 + hole)


def column_crossings(vol, x, y):
    """the z crossings of column (x, y), in extract_cloud's words, interpolated in voxel units: the list of z"""
    f = vol[:, y, x, 0].astype(np.float64)
    w = vol[:, y, x, 1]
    out = []
    for z in range(len(f) - 1):
        a, b = f[z], f[z + 1]
        if w[z] != 0 and w[z + 1] != 0 and a != 32767 and b != 32767 and ((a > 0 and b < 0) or (a < 0 and b > 0)):
            out.append(z + abs(a) / (abs(a) + abs(b)))
    return out
