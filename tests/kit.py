"""The suite's shared plumbing, in one plain module: the device's block layout, the two bit-for-bit predicates, the context every
volume test opens, the state a call must leave alone, and the build and run lines of the host harnesses and of the small C
programs that print integers.  No fixtures, no test functions; it imports no cases module and no test module."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# -ffp-contract=off is what makes the host text round like the numpy twins; the sanitizers' runtime is linked into the program
HARNESS_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan",
                 "-fno-sanitize-recover=all"]
C_FLAGS = ["-std=c99", "-Wall", "-Werror", "-pedantic"]


def blocked(vol):
    """a host volume [Z, Y, X, 2] as the device stores it: 64-B blocks of 4 x-adjacent voxels by 4 planes, the
    pair (tsdf, weight) in one 32-bit word"""
    Z, Y, X, _ = vol.shape
    out = np.zeros(X * Y * ((Z + 3) & ~3), np.uint32)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    idx = ((((z >> 2) * Y + y) * (X // 4) + (x >> 2)) * 16) + (z & 3) * 4 + (x & 3)
    out[idx.reshape(-1)] = ((vol[..., 0].astype(np.int64) & 0xffff) | ((vol[..., 1].astype(np.int64) & 0xffff) << 16)).reshape(-1)
    return out


def dims_of(vol):
    return vol.shape[2], vol.shape[1], vol.shape[0]


def same_bits(a, b):
    """the strict one: equal dtype, equal shape, equal bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_bits_nan(a, b):
    """NaN in the same places (its sign and payload are not part of the contract), everything else bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "f":
        return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a).view(np.uint32),
                                                                          np.nan_to_num(b).view(np.uint32))
    return np.array_equal(a, b)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    # NaNs: compare "is NaN" masks, then bit patterns elsewhere (the sign/payload of a NaN is not part of the contract)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), f"{what}: NaN masks differ at {np.argwhere(na != nb)[:5]}"
        ok = bits(np.where(na, 0, a).astype(a.dtype)) == bits(np.where(nb, 0, b).astype(b.dtype))
    else:
        ok = a == b
    if not ok.all():
        idx = np.argwhere(~ok)
        raise AssertionError(f"{what}: {len(idx)} of {ok.size} elements differ, first at {idx[:5].tolist()}: "
                             f"{a[tuple(idx[0])]} vs {b[tuple(idx[0])]}")


def volume_ctx(hsk, dims, size, color=False, **over):
    """a context whose volume is dims = (X, Y, Z) voxels over size metres, all of it its own; with a colour volume if asked"""
    trk = hsk.KinfuTracker(hsk.default_config(dims[2], vol_x=dims[0], vol_y=dims[1], vol_z=dims[2], vol_size_m=size, own_z1=dims[2], **over))
    if color:
        trk.enable_color()
    return trk


def state_of(trk, volume):
    """what a read-only call must leave alone: the pose, the volume if asked for, the model maps of every level"""
    return [trk.get_pose()] + ([trk.download_tsdf()] if volume else []) + [trk.download_map(kind, level) for kind in (2, 3) for level in (0, 1, 2)]


def assert_state(trk, before, what):
    """`before` is a state_of(trk, ...): with the volume if it has eight entries"""
    for a, b in zip(before, state_of(trk, len(before) == 8)):
        assert same_bits(a, b), what


def build_harness(name, out_dir):
    """tests/<name>_harness.cpp as a program under out_dir -> its path"""
    exe = out_dir / name
    subprocess.check_call(["g++"] + HARNESS_FLAGS + [os.path.join(ROOT, "tests", name + "_harness.cpp"), "-o", str(exe)])
    return exe


def run_harness(exe, *args, text=False):
    """runs a harness on its files; with text=True -> what it printed"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    cmd = [str(exe)] + [str(a) for a in args]
    return subprocess.check_output(cmd, text=True, env=env) if text else subprocess.check_call(cmd, env=env)


def c_values(tmp_path, expressions, header="hskinfu.h"):
    """the integer C expressions given, as a strict C99 program against include/<header> evaluates them"""
    src, exe = tmp_path / "values.c", tmp_path / "values"
    lines = "".join(f'    printf("%lld\\n", (long long)({e}));\n' for e in expressions)
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "{header}"\nint main(void)\n{{\n{lines}    return 0;\n}}\n')
    subprocess.check_call(["gcc"] + C_FLAGS + ["-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
