"""Volume alignment without a GPU: the host step hsk_align_step against the numpy twin (tests/align_twin.py), bit for bit; the
properties DESIGN.md 8f claims for the rule, shown on the twin with the analytic scene (a room seen from inside with a box on its
floor, as an 80 x 64 x 48 volume over 3 m: three different cells); the header, the C layout of the new structs and their Python
mirror."""
import ctypes as C

import numpy as np
import pytest

import align_twin as AT
import kit
from align_cases import HALF_CELL_M, M_TRUE, PERTURBED, TAU, _CACHE, scene
from kit import blocked, same_bits

f32 = np.float32


def run(name, M0, **kw):
    """a twin run, made once per name"""
    if name not in _CACHE:
        vol, ps, ns = scene()
        _CACHE[name] = AT.align(vol, AT.DST_SIZE, TAU, ps, ns, M0, **kw)
    return _CACHE[name]


def test_the_scene_is_the_one_the_rule_was_tried_on():
    vol, ps, ns = scene()
    assert float(TAU) == pytest.approx(0.13125, abs=1e-6)
    assert 8000 <= len(ps) <= 20000 and vol.shape == (48, 64, 80, 2)
    assert (vol[..., 1] == 0).any() and (vol[..., 0] < 0).any() and (vol[..., 0] == 32767).any()
    assert np.allclose(np.linalg.norm(ns.astype(np.float64), axis=1), 1.0, atol=1e-6)


# ---- 1. hsk_align_step against the twin ---------------------------------------------------------------------
def test_align_step_equals_the_twin_bit_for_bit(hsk):
    from housescan_amd import products
    vol, ps, ns = scene()
    cases = []
    for M in (PERTURBED, M_TRUE.astype(f32)):
        s, n, _ = AT.iteration(vol, AT.DST_SIZE, TAU, ps, ns, M)
        assert n > 5000
        cases.append((s[:27], M, (1.5, 1.5, 1.5)))
        cases.append((s[:27], M, (0.0, 0.0, 0.0)))
        cases.append((s[:27], M, (0.25, -1.75, 3.5)))        # a centre that is not the volume's
    for s27, M, c in cases:
        ref_m, ref_x, ref_ok = AT.step(s27, M, c)
        m, x, ok = products.align_step(s27, M, c)
        assert ok and ref_ok
        assert same_bits(m, ref_m) and same_bits(x, ref_x), (m, ref_m)
        assert not same_bits(m, np.asarray(M, f32))
    # the centre matters: the same sums about two centres give two matrices
    assert not same_bits(products.align_step(cases[0][0], cases[0][1], cases[0][2])[0], products.align_step(cases[1][0], cases[1][1], cases[1][2])[0])


def test_align_step_of_a_singular_system_hands_the_matrix_back(hsk):
    from housescan_amd import products
    vol, ps, ns = scene()
    wall = np.abs(ns.astype(np.float64) @ np.linalg.inv(M_TRUE)[:3, :3] - np.array([1.0, 0, 0])).max(axis=1) < 1e-3   # one wall's normals
    assert wall.sum() > 500
    for s27 in (np.zeros(27), AT.iteration(vol, AT.DST_SIZE, TAU, ps[wall][:1], ns[wall][:1], M_TRUE.astype(f32))[0][:27]):
        ref_m, ref_x, ref_ok = AT.step(s27, PERTURBED, (1.5, 1.5, 1.5))
        m, x, ok = products.align_step(s27, PERTURBED, (1.5, 1.5, 1.5))
        assert not ok and not ref_ok
        assert same_bits(m, PERTURBED) and same_bits(ref_m, PERTURBED) and same_bits(x, np.zeros(6, f32)) and same_bits(ref_x, x)
    lib = hsk._lib.load()
    assert lib.hsk_align_step(None, None, None, None, None, None) == -1


# ---- 2. the rule's properties, on the twin --------------------------------------------------------------------
def test_a_start_at_the_truth_converges_within_two_iterations():
    M, st = run("truth", M_TRUE.astype(f32))
    print(f"truth: {AT.STATUS[st['status']]} after {st['iterations']}, n_used {st['n_used']}, rms {st['rms_m']}, "
          f"error {AT.point_error(M, M_TRUE, scene()[1]) * 1e3:.3f} mm")
    assert st["status"] == AT.CONVERGED and st["iterations"] <= 2


def test_a_perturbed_start_is_recovered_to_half_a_cell():
    """2 degrees about (1, 2, 3) and (150, -100, 120) mm: the twin ends 0.19 mm from the truth (bar: half the smallest cell)"""
    M, st = run("perturbed", PERTURBED)
    vol, ps, ns = scene()
    err = AT.point_error(M, M_TRUE, ps[st["index"]][st["used"]])
    print(f"perturbed: {AT.STATUS[st['status']]} after {st['iterations']}, n_used {st['n_used']}, rms {st['rms_m']}, error {err * 1e3:.3f} mm "
          f"(start {AT.point_error(PERTURBED, M_TRUE, ps) * 1e3:.1f} mm)")
    assert st["status"] == AT.CONVERGED
    assert st["used"].sum() > 5000
    assert err <= HALF_CELL_M


def test_the_probes_bite_on_a_shift_of_two_and_a_half_truncation_distances():
    shift = np.eye(4)
    shift[0, 3] = 2.5 * float(TAU)
    M0 = (shift @ M_TRUE).astype(f32)
    _, st3 = run("shift3", M0, J=3)
    _, st0 = run("shift0", M0, J=0, max_shift_m=1.0)       # (the default bound 2 (J + 1) tau would stop J = 0 first)
    print(f"J = 3: {AT.STATUS[st3['status']]} {st3['iterations']} iterations, n_used {st3['n_used']}; "
          f"J = 0: {AT.STATUS[st0['status']]} {st0['iterations']} iterations, n_used {st0['n_used']}")
    assert st3["status"] == AT.CONVERGED
    assert st3["n_used"][0] > st0["n_used"][0]
    assert st3["iterations"] < st0["iterations"]


def test_points_outside_the_destination_are_few():
    away = np.eye(4)
    away[:3, 3] = (40.0, 0.0, 0.0)
    M0 = (away @ M_TRUE).astype(f32)
    M, st = run("away", M0)
    assert st["status"] == AT.FEW and st["iterations"] == 1 and st["n_used"] == [0] and same_bits(M, M0)
    assert same_bits(st["rms_m"], np.zeros(1, f32))


def test_a_shift_bound_below_the_perturbation_diverges_and_hands_the_start_back():
    M, st = run("bounded", PERTURBED, max_shift_m=0.05)
    assert st["status"] == AT.DIVERGED and same_bits(M, PERTURBED)
    assert 1 <= st["iterations"] < run("perturbed", PERTURBED)[1]["iterations"]


def test_the_sums_do_not_depend_on_the_order_of_the_points():
    vol, ps, ns = scene()
    a, na, _ = AT.iteration(vol, AT.DST_SIZE, TAU, ps, ns, PERTURBED)
    b, nb, _ = AT.iteration(vol, AT.DST_SIZE, TAU, ps[::-1], ns[::-1], PERTURBED)
    assert na == nb > 5000 and same_bits(a, b)
    rng = np.random.default_rng(2)
    o = rng.permutation(len(ps))
    c, nc, _ = AT.iteration(vol, AT.DST_SIZE, TAU, ps[o], ns[o], PERTURBED)
    assert nc == na and same_bits(a, c)
    # the sums are multiples of 2^-26
    assert np.array_equal(np.rint(a * 67108864.0), a * 67108864.0)


def test_nan_normals_never_contribute_and_the_subsample_is_every_stride_th_point():
    vol, ps, ns = scene()
    bad = ns.copy()
    bad[::2] = np.nan
    s_all, n_all, used = AT.iteration(vol, AT.DST_SIZE, TAU, ps, bad, PERTURBED)
    s_half, n_half, _ = AT.iteration(vol, AT.DST_SIZE, TAU, ps[1::2], ns[1::2], PERTURBED)
    assert not used[::2].any() and n_all == n_half and same_bits(s_all, s_half)
    stride, idx = AT.subsample(len(ps), 4000)
    assert stride == -(-len(ps) // 4000) and np.array_equal(idx, np.arange(0, len(ps), stride)) and len(idx) <= 4000
    stride, idx = AT.subsample(0, 4000)
    assert stride == 1 and len(idx) == 0


# ---- 2b. the kernel's work on one point, compiled for the host ------------------------------------------------------
def test_the_kernels_point_function_equals_the_twin_on_the_host(tmp_path):
    """housescan_amd/csrc/hsk_align_point.h -- the text every lane of k_align_iter runs -- built for the host with the address and
    undefined-behaviour sanitizers (their runtime linked into the program): the 28 sums (as integers in units of 2^-26) and
    n_used against the twin, zero differences; points that are NaN, infinite or kilometres away gather inside the volume like
    any other"""
    exe = kit.build_harness("align_point", tmp_path)
    vol, ps, ns = scene()
    words = blocked(vol)
    rng = np.random.default_rng(1)
    odd = ps.copy()
    odd[5], odd[7], odd[9], odd[11] = np.nan, 1e9, -1e30, np.inf
    holes = ns.copy()
    holes[::3] = np.nan
    half = np.eye(4)
    half[0, 3] = 1.2                       # half the cloud outside the box, part of it on the shell
    cases = {"3 probes": (ps, ns, PERTURBED, 3, 0.5), "direct": (ps, ns, PERTURBED, 0, 0.5), "8 probes": (ps, ns, M_TRUE.astype(f32), 8, 0.5),
             "odd points": (odd, holes, PERTURBED, 3, 0.5), "half outside": (ps, ns, (half @ M_TRUE).astype(f32), 3, 0.5),
             "noisy, wide gate": ((ps + rng.normal(0, 0.05, ps.shape)).astype(f32), ns, PERTURBED, 5, 0.2)}
    for name, (p, n, M, J, gate) in cases.items():
        path = tmp_path / "in.bin"
        with open(path, "wb") as f:
            for part in (np.array(AT.DST_DIMS, np.int32), np.array(AT.DST_SIZE, f32), np.asarray(M, f32), f32(TAU), f32(gate), np.int32(J),
                         np.uint32(len(p)), words, np.ascontiguousarray(np.concatenate([p.T, n.T]), f32)):
                f.write(part.tobytes())
        out = kit.run_harness(exe, path, text=True).split()
        got, n_used = np.array([int(v) for v in out[:28]], np.int64), int(out[28])
        ref, ref_used, _ = AT.iteration(vol, AT.DST_SIZE, TAU, p, n, M, J, gate)
        ref = np.rint(ref * 67108864.0).astype(np.int64)
        print(f"{name}: n_used {n_used} of {len(p)}")
        assert n_used == ref_used and np.array_equal(got, ref), f"{name}: {n_used} != {ref_used} or sums differ by {np.abs(got - ref).max()}"
        assert name == "direct" or n_used > 1000, name


# ---- 3. header, C layout, Python mirror -------------------------------------------------------------------------
def test_align_structs_have_the_c_layout(hsk):
    from housescan_amd import _lib
    P, S = _lib.HskAlignParams, _lib.HskAlignStats
    assert [n for n, _ in P._fields_] == ["max_iters", "probes", "cos_gate", "max_points", "min_points", "eps_rot", "eps_trans_m", "max_rot",
                                          "max_shift_m"]
    assert (_lib.HSK_ALIGN_CONVERGED, _lib.HSK_ALIGN_MAX_ITERS, _lib.HSK_ALIGN_FEW, _lib.HSK_ALIGN_DEGENERATE, _lib.HSK_ALIGN_DIVERGED) == (
        AT.CONVERGED, AT.MAX_ITERS, AT.FEW, AT.DEGENERATE, AT.DIVERGED)


def test_default_align_params_without_a_context(hsk):
    from housescan_amd import _lib
    p = _lib.HskAlignParams()
    _lib.load().hsk_default_align_params(None, C.byref(p))
    d = AT.DEFAULTS
    assert (p.max_iters, p.probes, p.max_points, p.min_points) == (d["max_iters"], d["J"], d["max_points"], d["min_points"])
    assert (p.cos_gate, p.eps_rot, p.eps_trans_m, p.max_rot) == (f32(d["cos_gate"]), f32(d["eps_rot"]), f32(d["eps_trans_m"]), f32(d["max_rot"]))
    assert p.max_shift_m == 0.0        # (it comes from a context's truncation distance)
    _lib.load().hsk_default_align_params(None, None)


def test_the_tracker_has_the_python_mirror(hsk):
    for name in ("align_cloud", "align_from", "default_align_params"):
        assert callable(getattr(hsk.KinfuTracker, name))
    with pytest.raises(TypeError, match="unknown alignment parameter"):
        hsk.KinfuTracker._align_params(None, {"no_such_field": 1})
    p = hsk.KinfuTracker._align_params(0, {"min_points": 1})
    assert (p.probes, p.min_points, p.max_iters) == (hsk._lib.HSK_ALIGN_DIRECT, 1, 0)
