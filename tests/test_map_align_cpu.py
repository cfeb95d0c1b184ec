"""Aligning world maps without a GPU (include/dsi_map_align.h; DESIGN.md 7j "Aligning"): the host solver against a numpy
SVD Kabsch and, bit for bit, against its restatement (tests/map_align_reference.py), the refusals of degenerate pairs, the
pose composition, every argument check of the six dsx_* entry points, the restatement's ICP loop on the scene the GPU
tests use, and the new kernels' metadata.  One refusal of the header has no test on either side: a table that overflowed in
an earlier call (see test_gpu_map_align.py's docstring)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_align_reference as ar
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsx_map_align_step", "dsx_map_align_fetch", "dsx_pose_compose", "dsx_map_align_solve", "dsx_map_align",
       "dsx_map_integrate_map")
NEW_KERNELS = ("k_map_align_step", "k_map_align_gather", "k_map_integrate_map")
QUANTUM = ar.LEAF_B * 2.0 ** -10


def solver_cases():
    """(name, U, V) of seeded pairs under known motions: rotations from 0 to 5 degrees about random axes with a
    translation of a fraction of a leaf, the identity, and a planar (rank 2) set"""
    rng = np.random.default_rng(41)
    out = []
    for k, deg in enumerate((0.0, 0.01, 0.3, 1.0, 2.0, 3.5, 5.0)):
        P = rng.uniform(-1.0, 1.0, (400, 3)) * (0.4, 0.7, 1.0)
        T = ar.axis_angle_pose(rng.normal(size=3), math.radians(deg), rng.uniform(-0.6, 0.6, 3) * ar.LEAF_B)
        Q = ref.world_positions(P.astype(np.float32), T) + rng.normal(0.0, 0.003, P.shape)
        out.append(("rot %g deg" % deg, ar.quantise(P.astype(np.float32).astype(np.float64), QUANTUM), ar.quantise(Q, QUANTUM)))
    P = rng.uniform(-1.0, 1.0, (400, 3))
    U = ar.quantise(P, QUANTUM)
    out.append(("identity", U, U.copy()))
    P = rng.uniform(-1.0, 1.0, (400, 3)) * (1.0, 0.8, 0.0) + (0.0, 0.0, 0.25)
    T = ar.axis_angle_pose((0.2, 1.0, -0.4), math.radians(2.5), (0.01, -0.02, 0.015))
    out.append(("planar", ar.quantise(P, QUANTUM), ar.quantise(ref.world_positions(P.astype(np.float32), T), QUANTUM)))
    return out


def test_solver_against_an_svd_kabsch_and_its_restatement(built):
    """Both are double-precision solves of one least-squares problem; no bound is derived.  Measured on the build machine
    over these nine cases: the largest difference of an entry of R 6.93e-15, of t / extent 2.32e-16, the largest entry of
    R^T R - I 2.22e-16, |det R - 1| 1.11e-16 (printed below).  Asserted: 16 x those."""
    worst = {"R": 0.0, "t": 0.0, "orth": 0.0, "det": 0.0}
    for name, U, V in solver_cases():
        m = ar.moments_of(U, V, len(U), QUANTUM, 2)
        T, info = d.solve_alignment(m)
        Tr, info_r = ar.solve(m)
        assert np.array_equal(T, Tr) and info == info_r, name                    # the restatement, bit for bit
        R, t = T.reshape(3, 4)[:, :3], T.reshape(3, 4)[:, 3]
        P, Q = U.astype(np.float64) * QUANTUM, V.astype(np.float64) * QUANTUM
        Rk, tk = ar.kabsch(P, Q)
        extent = float(np.abs(np.concatenate([P, Q])).max())
        fig = {"R": float(np.abs(R - Rk).max()), "t": float(np.abs(t - tk).max()) / extent,
               "orth": float(np.abs(R.T @ R - np.eye(3)).max()), "det": abs(float(np.linalg.det(R)) - 1.0)}
        print(name, fig, info)
        worst = {k: max(worst[k], fig[k]) for k in worst}
        assert info["n_matched"] == len(U) and info["lambda"][0] > info["lambda"][1]
        res = Q - (P @ R.T + t)
        assert info["rms"] == math.sqrt((float(m["e2"]) * (QUANTUM * QUANTUM)) / float(len(U)))
        assert math.sqrt((res ** 2).sum() / len(U)) <= info["rms"] * (1 + 1e-9) + 1e-12   # the solve does not worsen the pairs
    print("worst", worst)
    assert worst["R"] <= 16 * 6.93e-15 and worst["t"] <= 16 * 2.32e-16           # measured: 6.93e-15, 2.32e-16
    assert worst["orth"] <= 16 * 2.22e-16 and worst["det"] <= 16 * 1.11e-16      # measured: 2.22e-16, 1.11e-16


def test_the_identity_is_recovered_exactly_enough(built):
    name, U, V = solver_cases()[7]
    T, info = d.solve_alignment(ar.moments_of(U, V, len(U), QUANTUM, 1))
    assert info["rms"] == 0.0 and info["angle"] <= 1e-15 and info["trans"] <= 1e-15
    assert np.abs(T - ar.IDENTITY).max() <= 1e-15


def degenerate_cases():
    rng = np.random.default_rng(43)
    s = rng.integers(-20000, 20000, 50)
    line = np.stack([3 * s + 7, -2 * s + 1, 5 * s - 4], axis=1).astype(np.int64)
    yield "collinear", line, line + np.array([5, -3, 2]), "degenerate"
    two = np.array([[100, 200, 300], [-4000, 50, 60]], np.int64)
    yield "two pairs", two, two + 3, "n_matched"
    one = np.tile(np.array([[1234, -567, 89]], np.int64), (10, 1))
    yield "a single repeated pair", one, one + 2, "degenerate"


def test_degenerate_pairs_are_refused_and_leave_the_pose_untouched(built):
    L = d.load_library()
    for name, U, V, word in degenerate_cases():
        m = ar.moments_of(U, V, len(U), QUANTUM, 1)
        with pytest.raises(ar.Refused) as e:
            ar.solve(m)
        assert e.value.args[0] == word, name
        T = np.full(12, 7.25)
        info = E._MapAlignSolveInfo()
        assert L.dsx_map_align_solve(C.byref(E._moments_struct(m)), T.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info)) == E.ERR_INVALID
        assert word.encode() in L.dsi_last_error(), (name, L.dsi_last_error())
        assert (T == 7.25).all(), name
        with pytest.raises(d.DsiError):
            d.solve_alignment(m)


def test_pose_composition(built):
    rng = np.random.default_rng(47)
    for k in range(20):
        A = ar.axis_angle_pose(rng.normal(size=3), rng.uniform(0, 3.0), rng.normal(size=3))
        B = ar.axis_angle_pose(rng.normal(size=3), rng.uniform(0, 3.0), rng.normal(size=3) * 10.0)
        got = d.compose_pose(A, B)
        assert np.array_equal(got, ar.compose(A, B))                              # the stated rounding order
        A4, B4 = (np.vstack([M.reshape(3, 4), [0, 0, 0, 1]]) for M in (A, B))
        assert np.abs(got.reshape(3, 4) - (A4 @ B4)[:3]).max() <= 8 * np.finfo(np.float64).eps * 11.0
        # compose(T, invert(T)) is the identity within a few ulp of the entries' size
        near = d.compose_pose(A, d.invert_pose(A))
        assert np.abs(near - ar.IDENTITY).max() <= 8 * np.finfo(np.float64).eps * max(1.0, float(np.abs(A).max()))
    out = A.copy()                                                                 # out may alias an input
    L = d.load_library()
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dsx_pose_compose(p, B.ctypes.data_as(C.POINTER(C.c_double)), p) == E.OK and np.array_equal(out, ar.compose(A, B))


def test_abi_argument_checks_need_no_gpu(built):
    L = d.load_library()
    INV = E.ERR_INVALID
    fake, other = C.c_void_p(0x1000), C.c_void_p(0x2000)                        # never dereferenced: the checks come first
    good = (C.c_double * 12)(*ar.IDENTITY.tolist())
    out = (C.c_double * 12)()
    m, info, n = E._MapAlignMoments(), E._MapAlignInfo(), C.c_size_t()
    opts = lambda radius=0.1, max_iterations=5, eps_rot=1e-6, eps_trans=1e-6: E._MapAlignOpts(1, 1, 1, 1, radius, max_iterations, 0, 3,
                                                                                           eps_rot, eps_trans)
    bad_poses = []
    for k, v in ((0, float("nan")), (3, float("inf")), (11, float("-inf"))):
        T = ar.IDENTITY.copy()
        T[k] = v
        bad_poses.append((C.c_double * 12)(*T.tolist()))
    # the step: opts, then T, then the maps
    assert L.dsx_map_align_step(fake, other, None, good, C.byref(m)) == INV and b"opts is null" in L.dsi_last_error()
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert L.dsx_map_align_step(None, None, C.byref(opts(radius=radius)), good, C.byref(m)) == INV and b"radius" in L.dsi_last_error()
        assert L.dsx_map_align(None, None, C.byref(opts(radius=radius)), good, out, C.byref(info)) == INV and b"radius" in L.dsi_last_error()
    assert L.dsx_map_align_step(None, None, C.byref(opts()), None, C.byref(m)) == INV and b"T is null" in L.dsi_last_error()
    for T in bad_poses:
        assert L.dsx_map_align_step(None, None, C.byref(opts()), T, C.byref(m)) == INV and b"not finite" in L.dsi_last_error()
        assert L.dsx_map_align(None, None, C.byref(opts()), T, out, C.byref(info)) == INV and b"not finite" in L.dsi_last_error()
        assert L.dsx_map_integrate_map(fake, other, T, 1, 1, None, None) == INV and b"not finite" in L.dsi_last_error()
    assert L.dsx_map_align_step(None, fake, C.byref(opts()), good, C.byref(m)) == INV and b"map is null" in L.dsi_last_error()
    assert L.dsx_map_align_step(fake, None, C.byref(opts()), good, C.byref(m)) == INV and b"map is null" in L.dsi_last_error()
    # the fetch
    assert L.dsx_map_align_fetch(None, None, None, None, 0, C.byref(n)) == INV and b"null" in L.dsi_last_error()
    assert L.dsx_map_align_fetch(fake, None, None, None, 0, None) == INV and b"null" in L.dsi_last_error()
    # the loop: its own options first
    assert L.dsx_map_align(fake, other, None, good, out, C.byref(info)) == INV and b"opts is null" in L.dsi_last_error()
    for it in (0, -1, 65):
        assert L.dsx_map_align(None, None, C.byref(opts(max_iterations=it)), good, out, None) == INV
        assert b"max_iterations" in L.dsi_last_error()
    for eps in (-1e-9, float("nan"), float("inf")):
        assert L.dsx_map_align(None, None, C.byref(opts(eps_rot=eps)), good, out, None) == INV and b"eps_rot" in L.dsi_last_error()
        assert L.dsx_map_align(None, None, C.byref(opts(eps_trans=eps)), good, out, None) == INV and b"eps_trans" in L.dsi_last_error()
    assert L.dsx_map_align(None, None, C.byref(opts()), good, None, None) == INV and b"T_out is null" in L.dsi_last_error()
    assert L.dsx_map_align(None, None, C.byref(opts()), None, out, None) == INV and b"T_init is null" in L.dsi_last_error()
    for it in (1, 64):                                                           # the bounds themselves are legal
        assert L.dsx_map_align(None, fake, C.byref(opts(max_iterations=it, eps_rot=0.0, eps_trans=0.0)), good, out, None) == INV
        assert b"map is null" in L.dsi_last_error()
    # one map into another
    assert L.dsx_map_integrate_map(None, other, good, 1, 1, None, None) == INV and b"dst is null" in L.dsi_last_error()
    assert L.dsx_map_integrate_map(fake, None, good, 1, 1, None, None) == INV and b"src is null" in L.dsi_last_error()
    assert L.dsx_map_integrate_map(fake, other, None, 1, 1, None, None) == INV and b"T is null" in L.dsi_last_error()
    assert L.dsx_map_integrate_map(fake, fake, good, 1, 1, None, None) == INV and b"same map" in L.dsi_last_error()
    # the host routines
    assert L.dsx_pose_compose(None, good, out) == INV and L.dsx_pose_compose(good, None, out) == INV
    assert L.dsx_pose_compose(good, good, None) == INV and b"null" in L.dsi_last_error()
    assert L.dsx_map_align_solve(None, out, None) == INV and L.dsx_map_align_solve(C.byref(m), None, None) == INV
    m.n_matched, m.quantum = 5, 0.0
    assert L.dsx_map_align_solve(C.byref(m), out, None) == INV and b"quantum" in L.dsi_last_error()
    assert L.dsi_abi_version() == 10


def test_quantisation_bounds_of_the_header():
    """|V| < 2^30 and |U| < 2^30 + 3073 at the edge of the key range, and the split of a product of either sign is exact"""
    leaf = 0.04
    top = np.float32((ref.CELL_MAX + 1) * leaf)                                   # no centroid reaches 2^20 - 1 leaves
    V = int(ar.quantise(np.float64(top), leaf * 2.0 ** -10))
    assert V < 1 << 30 and V > (1 << 30) - 2048
    U = int(ar.quantise(np.float64(top) + 3 * leaf, leaf * 2.0 ** -10))
    assert U - V <= 3073 and U < (1 << 30) + 3073
    for u, v in ((U, V), (-U, V), (U, -V), (-U, -V), (3, -5), (-1, 1)):
        m = ar.moments_of([[u, 0, 0]], [[v, 0, 0]], 1, leaf * 2.0 ** -10, 1)
        assert m["suv_hi"][0] * (1 << 32) + m["suv_lo"][0] == u * v and 0 <= m["suv_lo"][0] <= ar.MASK32
        assert -(1 << 62) < u * v < 1 << 62 and -(1 << 30) - 1 <= m["suv_hi"][0] < 1 << 30


@pytest.fixture(scope="module")
def scene1():
    ca, cb = ar.scene1_calls()
    return ar.reference_map(ca, ar.LEAF_A).extract(), ar.reference_map(cb, ar.LEAF_B).extract()


def test_scene_1_is_not_vacuous(scene1):
    ea, eb = scene1
    assert (len(ea["keys"]), len(eb["keys"])) == ar.SCENE1_CELLS and all(n % 64 for n in ar.SCENE1_CELLS)
    for radius, reach in zip(ar.SCENE1_RADII, (1, 2, 3)):
        m = ar.step(ea, eb, ar.LEAF_B, radius, ar.T_TRUE_1)
        print(radius, m["n_matched"], m["n_unmatched"])
        assert m["reach"] == reach and m["n_matched"] >= 1500 and m["n_unmatched"] >= 500
    far = ar.step(ea, eb, ar.LEAF_B, 0.08, ar.T_FAR)
    assert far["n_matched"] == 0 and far["e2"] == 0 and not any(far["su"] + far["sv"] + far["suv_hi"] + far["suv_lo"])
    assert not far["keys_other"].any() and np.isposinf(far["dist"]).all()


def test_the_restatement_recovers_the_known_motion_on_scene_1(built, scene1):
    """The loop with the restatement's step and the library's solver: what test_gpu_map_align.py must reproduce bit for
    bit.  The figures are recorded in map_align_reference.SCENE1_LOOP_RESULT."""
    ea, eb = scene1
    T, info, history = ar.align(ea, eb, ar.LEAF_B, solver=d.solve_alignment, composer=d.compose_pose, **ar.SCENE1_LOOP)
    err = ar.pose_error(T, ar.T_TRUE_1)
    start = ar.pose_error(ar.IDENTITY, ar.T_TRUE_1)
    print(info, err, start, T.tolist())
    assert info["rms_last"] < info["rms_first"]
    assert err[0] < 0.25 * start[0] and err[1] < ar.LEAF_B                       # within a leaf, the rotation mostly undone
    want = ar.SCENE1_LOOP_RESULT
    assert info["iterations"] == want["iterations"] and info["converged"] == want["converged"]
    assert (info["n_matched_first"], info["n_matched_last"]) == (want["n_matched_first"], want["n_matched_last"])
    assert (info["rms_first"], info["rms_last"]) == (want["rms_first"], want["rms_last"])
    assert err == want["pose_error"]
    # the same loop through the restatement's own solver and composition: the same bits
    T2, info2, _ = ar.align(ea, eb, ar.LEAF_B, **ar.SCENE1_LOOP)
    assert np.array_equal(T, T2) and info == info2


def test_the_loop_refuses_too_few_matches_with_the_last_good_pose(scene1):
    ea, eb = scene1
    with pytest.raises(ar.Refused) as e:
        ar.align(ea, eb, ar.LEAF_B, 0.08, T_init=ar.T_FAR, min_matched=1)
    assert e.value.info["stopped"] == 1 and e.value.info["iterations"] == 1 and np.array_equal(e.value.T, ar.T_FAR)


def test_integrate_map_in_the_restatement(scene1):
    ca, _ = ar.scene1_calls()
    src = ar.reference_map(ca, ar.LEAF_A)
    dst, want = ar.reference_map([], ar.LEAF_B), ar.reference_map([], ar.LEAF_B)
    n, rej = ar.integrate_map(dst, src, ar.T_TRUE_1, 2, 1)
    assert 0 < n < len(src.keys) and rej == 0
    want.integrate(src.extract(2, 1)["xyz"], ar.T_TRUE_1)
    assert np.array_equal(dst.export_state()["S"], want.export_state()["S"]) and dst.calls == 1


def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    core = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", core))) == 176 and "dsx_" not in core
    header = open(os.path.join(ROOT, "include", "dsi_map_align.h")).read()
    declared = re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header)
    assert sorted(declared) == sorted(NEW)
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name                      # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    assert (C.sizeof(E._MapAlignOpts), C.sizeof(E._MapAlignMoments), C.sizeof(E._MapAlignSolveInfo), C.sizeof(E._MapAlignInfo)) == \
        (56, 240, 48, 72)                                                        # the header's layout
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "dsi_map_align.h" in readme and all(name in readme for name in NEW)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "dsi_map_align.h" in integration and all(name in integration for name in NEW)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Aligning" in design and "k_map_align_step" in design
    for name in ("alignStep", "fetchAlignment", "align", "integrateMap"):
        assert hasattr(d.WorldMap, name), name
    assert callable(d.compose_pose) and callable(d.solve_alignment)
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for name in ("align_step(", "MapAlignResult align(", "integrate_map(", "compose_pose(", "dsi_map_align.h"):
        assert name in hpp, name
    from dvs_mcemvs_amd import build, process as proc
    assert callable(proc.align_world_maps) and "align" in proc.score_world_map_3d.__code__.co_varnames
    assert any(h.endswith("dsi_map_align.h") for h in build.HEADERS)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    text = kernel_asm_text()
    seen = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = [k for k in NEW_KERNELS if re.search(r"\d+%sE" % k, name)]
        if not short:
            continue
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, name
        assert val("wavefront_size") == 64 and val("max_flat_workgroup_size") == 256, name
        seen[short[0]] = (val("vgpr_count"), val("sgpr_count"), val("group_segment_fixed_size"))
    print(seen)
    assert set(seen) == set(NEW_KERNELS), seen
    # 25 sums, two counts and the pose in LDS; four waves of the step fit a SIMD -- all that its grid offers one
    assert seen["k_map_align_step"][2] <= 25 * 8 + 8 + 12 * 8 and seen["k_map_align_step"][0] <= 128
    # the lookups only read, and the 25 sums leave a workgroup as one 64-bit atomic each: one global atomic instruction for
    # the two counts and one for the sums, never a compare-and-swap on a table
    m = re.search(r"^(_ZN\w*\d+k_map_align_stepE\w*):.*?$(.*?)s_endpgm", text, re.S | re.M)
    body = m.group(2)
    assert "atomic_cmpswap" not in body and len(re.findall(r"^\s+global_atomic_add_x2", body, re.M)) == 2
    assert len(re.findall(r"^\s+ds_add_u64", body, re.M)) == 25
