"""The C-ABI library loads without a GPU and exports every symbol include/hskinfu.h declares; every ctypes
mirror and every integer constant of housescan_amd/_lib.py has the C layout and the C value; without a HIP device the product fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from kit import ROOT, c_values

HEADER = os.path.join(ROOT, "include", "hskinfu.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hsk_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(hsk):
    from housescan_amd import _lib
    names = declared_functions()
    assert len(names) >= 40
    lib = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/hskinfu.h but not exported by libhskinfu.so"
        assert n in _lib.SYMBOLS, f"{n} has no ctypes binding in housescan_amd/_lib.py"
    assert set(_lib.SYMBOLS) <= set(names), set(_lib.SYMBOLS) - set(names)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (hsk_\w+)", out))
    assert set(names) <= exported


def test_house_header_symbols_are_exported_and_bound(hsk):
    """include/hshouse.h (host-side room stitching): same rule as the core header"""
    from housescan_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hshouse.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(hsh_[a-z0-9_]+)\s*\(", src)))
    assert len(names) >= 40
    lib = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/hshouse.h but not exported"
        assert n in _lib.HOUSE_SYMBOLS, f"{n} has no ctypes binding"
    assert set(_lib.HOUSE_SYMBOLS) <= set(names), set(_lib.HOUSE_SYMBOLS) - set(names)


def test_house_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "hshouse.h"\nint main(void){hsh_house* h = 0; (void)h; return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "c.o")])


# ---- the whole ABI's layout, generated from the mirrors ------------------------------------------------------------------------
# typedefs of the header without a body: handles, which have no layout to mirror
OPAQUE = {"hsk_ctx", "hsk_group", "hsk_depth_stream"}
# structs of the header that have a body and, on purpose, no mirror in _lib.py: {C name: reason}
NO_MIRROR = {}
MIN_STRUCTS, MIN_CONSTANTS = 50, 106            # the counts when this test was written: floors, to be raised when the tree grows


def header_structs():
    """(the names of the header's typedef'd structs that have a body, those that have none)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    bodied, opaque = set(), set()
    for m in re.finditer(r"\btypedef\s+struct\b\s*(\w*)\s*([{;\w])", src):
        if m[2] != "{":
            opaque.add(re.match(r"\w+", src[m.start(2):])[0])
            continue
        depth, k = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[k], 0)
            k += 1
        bodied.add(re.match(r"\s*(\w+)\s*;", src[k:])[1])
    return bodied, opaque


def c_name(cls):
    """HskFillParams -> hsk_fill_params"""
    return re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()


def mirror_members(cls, path="", base=0):
    """[(member path as C writes it, offset from the outermost struct, size)] of every field, nested structs entered"""
    out = []
    for name, typ, *bits in cls._fields_:
        assert not bits, f"{cls.__name__}.{name}: a bit field has no offsetof"
        f = getattr(cls, name)
        out.append((path + name, base + f.offset, f.size))
        if isinstance(typ, type) and issubclass(typ, C.Structure):
            out += mirror_members(typ, path + name + ".", base + f.offset)
    return out


def test_every_struct_mirror_has_the_c_layout(tmp_path):
    """sizeof of every ctypes.Structure of _lib.py, and offsetof and sizeof of every field, against a C99 program generated from the
    mirrors and compiled against the header; every struct of the header has a mirror, every mirror a struct of the header"""
    from housescan_amd import _lib
    mirrors = {c_name(v): v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    bodied, opaque = header_structs()
    assert opaque == OPAQUE, opaque ^ OPAQUE
    assert not set(mirrors) - bodied, f"mirrors without a struct in include/hskinfu.h: {sorted(set(mirrors) - bodied)}"
    assert bodied - set(mirrors) == set(NO_MIRROR), f"header structs without a mirror in _lib.py: {sorted(bodied - set(mirrors) - set(NO_MIRROR))}"
    what, expressions, want = [], [], []
    for name, cls in sorted(mirrors.items()):
        what.append(f"sizeof({name})")
        expressions.append(f"sizeof({name})")
        want.append(C.sizeof(cls))
        for member, offset, size in mirror_members(cls):
            what += [f"{name}.{member}: offset", f"{name}.{member}: size"]
            expressions += [f"offsetof({name}, {member})", f"sizeof((({name}*)0)->{member})"]
            want += [offset, size]
    got = c_values(tmp_path, expressions)
    wrong = [f"{w}: C {g} != ctypes {e}" for w, g, e in zip(what, got, want) if g != e]
    print(f"{len(mirrors)} structs, {(len(want) - len(mirrors)) // 2} fields, {len(want)} numbers")
    assert len(got) == len(want) and not wrong, "\n".join(wrong)
    assert len(mirrors) >= MIN_STRUCTS, len(mirrors)


def test_every_integer_constant_has_the_c_value(tmp_path):
    from housescan_amd import _lib
    constants = {k: v for k, v in vars(_lib).items() if k.startswith("HSK_") and isinstance(v, int) and not isinstance(v, bool)}
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    missing = [k for k in constants if not re.search(rf"\b{k}\b", src)]
    assert not missing, f"constants of _lib.py that include/hskinfu.h does not name: {missing}"
    got = c_values(tmp_path, sorted(constants))
    wrong = [f"{k}: C {g} != _lib.py {constants[k]}" for k, g in zip(sorted(constants), got) if g != constants[k]]
    print(f"{len(constants)} constants")
    assert len(got) == len(constants) and not wrong, "\n".join(wrong)
    assert len(constants) >= MIN_CONSTANTS, len(constants)


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "hskinfu.h"\nint main(void){hsk_config c; hsk_ctx* k = 0; (void)c; (void)k; return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "c.o")])


def test_default_config_values(hsk):
    c = hsk.default_config(512)
    assert (c.vol_x, c.vol_y, c.vol_z) == (512, 512, 512)
    assert list(c.vol_size_m) == [3.0, 3.0, 3.0] and abs(c.trunc_dist_m - 0.03) < 1e-9
    assert (c.width, c.height, c.fx, c.fy, c.cx, c.cy) == (640, 480, 525.0, 525.0, 319.5, 239.5)
    assert list(c.icp_iters) == [10, 5, 4]
    assert abs(c.icp_angle_thresh_sin - np.sin(np.radians(20))) < 1e-7
    pose = np.array(c.init_pose, np.float32).reshape(4, 4)
    assert np.allclose(pose[:3, :3], np.eye(3)) and np.allclose(pose[:3, 3], [1.5, 1.5, -0.3], atol=1e-6)
    assert (c.own_z0, c.own_z1, c.halo, c.use_graph) == (0, 512, 0, 0)


def test_no_gpu_fails_loudly(hsk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    with pytest.raises(hsk.KinfuError, match="no HIP device"):
        hsk.KinfuTracker(n=64)


def test_group_without_gpu_fails_loudly(hsk):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    with pytest.raises(hsk.KinfuError, match="no HIP device|device setup failed"):
        hsk.KinfuGroup(hsk.default_config(64), device_ids=[0, 0])


def test_host_solve_mirror_matches_oracle(hsk, oracle):
    """hsk_icp_solve is host code: the device solve's mirror must equal the oracle's bit for bit"""
    import ctypes
    lib = hsk._lib.load()
    rng = np.random.default_rng(11)
    for _ in range(20):
        J = rng.normal(size=(50, 6))
        A, b = J.T @ J, J.T @ rng.normal(size=50)
        s27 = np.array(sum([list(A[i, i:]) + [b[i]] for i in range(6)], []))
        x = np.empty(6, np.float32)
        ok = ctypes.c_int()
        lib.hsk_icp_solve(s27.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                          ctypes.byref(ok))
        xo, oko = oracle.icp_solve(s27)
        assert ok.value == 1 and oko and np.array_equal(x.view(np.uint32), xo.view(np.uint32))


def test_bilateral_tables_exact(hsk):
    ws, wc = hsk.bilateral_tables()
    s2, c2 = np.float32(0.5) / (np.float32(4.5) * np.float32(4.5)), np.float32(0.5) / (np.float32(30) * np.float32(30))
    dy, dx = np.mgrid[-6:7, -6:7]
    ref_s = np.exp(-((dx * dx + dy * dy).astype(np.float32) * s2).astype(np.float64)).astype(np.float32).reshape(-1)
    k = np.arange(512)
    ref_c = np.exp(-((k * k).astype(np.float32) * c2).astype(np.float64)).astype(np.float32)
    assert np.array_equal(ws, ref_s) and np.array_equal(wc, ref_c)


def test_native_rooms_harness_builds_against_the_header(tmp_path, hsk):
    """tools/rooms_native.c (bench.py's concurrent_rooms_one_gpu block compiles and runs it on the GPU box) is plain C11 against
    include/hskinfu.h and links with nothing but the library, libdl and pthreads"""
    from housescan_amd import _lib
    lib_dir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "rooms_native")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "rooms_native.c"), "-L" + lib_dir, "-lhskinfu", "-ldl", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe, "0"], capture_output=True, text=True, timeout=60)   # (0 rooms: the argument check, no GPU touched)
    assert r.returncode == 2

