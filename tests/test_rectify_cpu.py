"""Lens rectification, the part that needs no GPU: the numpy restatement (tests/rectify_reference.py) against
first principles, the host-side entry points (dsi_lens_check, dsi_lens_rr), the exported symbols, and dsi::lens_of of the C++
adapter on stand-in camera types."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import rectify_cases as cases
import rectify_reference as rr
from dvs_mcemvs_amd import engine
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["plumb_bob_A", "plumb_bob_C", "fisheye_A"])
def test_restatement_inverts_the_forward_model(name):
    """R = I, P = [K | 0]: the table's entry is K applied to the undistorted point, so the forward (distortion) model
    applied to it gives the raw pixel back.  What is left is the error of the fixed number of rounds plus the float32
    rounding of the table; tests/test_gpu_rectify.py derives its round-trip bound from the same figure."""
    lens, w, h = cases.simple(name)
    lut = rr.rectify_lut(lens, w, h)
    res = rr.round_trip_residual(lens, lut, w, h)
    print("%s: largest round-trip residual %.3e pixels" % (name, res))
    assert np.isfinite(lut).all()
    # first principles, not a measurement: an inverse that is any good returns to within a fraction of a pixel, a wrong
    # formula (a sign of p1, x and y swapped, a missing coefficient) is off by pixels on these lenses
    assert res < 0.25
    # and the model does something: the table is not the identity
    x, y = rr.pixel_grid(w, h)
    assert max(np.abs(lut[:, 0] - x).max(), np.abs(lut[:, 1] - y).max()) > 1.0


def test_restatement_fisheye_centre_is_exact():
    """The Kannala-Brandt inverse converges to 1e-8 in theta, so near the centre the round trip is at float32 rounding."""
    lens, w, h = cases.simple("fisheye_A")
    lut = rr.rectify_lut(lens, w, h)
    x, y = rr.pixel_grid(w, h)
    near = (np.abs(x - 640) < 100) & (np.abs(y - 360) < 100)
    res = rr.round_trip_residual(lens, lut, w, h, keep=near)
    assert res <= 2 * cases.ulp32(800.0)


@pytest.mark.parametrize("model,D", [(engine.LENS_PLUMB_BOB, ()), (engine.LENS_PLUMB_BOB, (0.0,) * 5),
                                     (engine.LENS_PLUMB_BOB, (0.0,) * 8), (engine.LENS_FISHEYE, (0.0,) * 4)])
def test_zero_distortion_is_the_identity_table(model, D):
    # (a power-of-two focal length and a dyadic centre keep (x - cx) / f * f + cx exact, so "exactly" can be asked of
    #  plumb_bob; fisheye goes through tan(atan-like Newton) and is exact only where theta_d is 0)
    K = np.array([[64.0, 0, 20.5], [0, 128.0, 11.25], [0, 0, 1.0]])
    lens = engine.Lens(model, K, D)
    w, h = 41, 23
    lut = rr.rectify_lut(lens, w, h)
    x, y = rr.pixel_grid(w, h)
    if model == engine.LENS_PLUMB_BOB:
        assert np.array_equal(lut[:, 0], x.astype(np.float32)) and np.array_equal(lut[:, 1], y.astype(np.float32))
    else:
        # k = 0: theta = theta_d, the table is f tan(theta_d) (x - c) / (f theta_d) + c: the ideal fisheye -> pinhole map
        r = np.hypot((x - 20.5) / 64.0, (y - 11.25) / 128.0)
        s = np.where(r > 0, np.tan(r) / np.where(r > 0, r, 1.0), 0.0)
        assert np.allclose(lut[:, 0], (x - 20.5) * s + 20.5, rtol=0, atol=1e-4)
        assert np.allclose(lut[:, 1], (y - 11.25) * s + 11.25, rtol=0, atol=1e-4)


def test_the_cameras_reach_the_branches_they_are_there_for():
    """plumb_bob B2: icdist < 0 for some pixels, the main branch for others.  (plumb_bob B as specified, D = (-0.6, 0.1, 0,
    0, 0), cannot reach it: 1 - 0.6 r2 + 0.1 r2^2 has a negative discriminant and is positive for every r2.  B stays in
    the bit-for-bit check; B2, the same camera with k2 = 0.05, is the one that takes the branch.)  fisheye B: sentinels,
    finite entries, a clamped theta_d and a pixel with theta_d <= 1e-8."""
    lens, w, h = cases.camera("plumb_bob_B")
    _, info = rr.rectify_lut(lens, w, h, return_info=True)
    assert not info["icdist_negative"].any()
    r2 = np.linspace(0.0, 1e3, 200001)
    assert (1.0 - 0.6 * r2 + 0.1 * r2 * r2 > 0).all()
    lens, w, h = cases.camera("plumb_bob_B2")
    lut, info = rr.rectify_lut(lens, w, h, return_info=True)
    assert info["icdist_negative"].any() and (~info["icdist_negative"]).any()
    assert np.isfinite(lut).all()
    lens, w, h = cases.camera("fisheye_B")
    lut, info = rr.rectify_lut(lens, w, h, return_info=True)
    sent = (lut == np.float32(rr.SENTINEL)).all(axis=1)
    assert np.array_equal(sent, info["sentinel"])
    assert sent.any() and (~sent).any() and np.isfinite(lut).all()
    assert info["small"].sum() == 1 and info["clamped"].any()
    assert info["not_converged"].any() and info["flipped"].any()
    c = 22 * w + 33                                       # the principal point: X = Y = 0, the table holds it
    assert info["small"][c] and tuple(lut[c]) == (33.0, 22.0)


def _raw(lens):
    return lens._c()


def test_lens_check_refusals(built):
    L = d.load_library()
    K = np.array([[100.0, 0, 50.0], [0, 101.0, 40.0], [0, 0, 1.0]])
    ok = [d.Lens("plumb_bob", K, ()), d.Lens("plumb_bob", K, (0.1,) * 4), d.Lens("plumb_bob", K, (0.1,) * 5),
          d.Lens("plumb_bob", K, (0.1,) * 8), d.Lens("fisheye", K, (0.1,) * 4), d.Lens(engine.LENS_FISHEYE, K, (0.0,) * 4)]
    for lens in ok:
        assert L.dsi_lens_check(C.byref(_raw(lens))) == engine.OK
        lens.check()
    bad = [d.Lens(2, K, (0.1,) * 4), d.Lens(-1, K, ()),                                   # unknown model
           d.Lens("plumb_bob", K, (0.1,) * 3), d.Lens("plumb_bob", K, (0.1,) * 6),         # counts plumb_bob does not have
           d.Lens("fisheye", K, (0.1,) * 5), d.Lens("fisheye", K, ()),                     # fisheye: 4 only
           d.Lens("plumb_bob", np.array([[0.0, 0, 50], [0, 101, 40], [0, 0, 1]]), ()),     # fx = 0
           d.Lens("plumb_bob", np.array([[100.0, 0, 50], [0, 0, 40], [0, 0, 1]]), ()),     # fy = 0
           d.Lens("plumb_bob", K, (), P=[[100, 0, 50, 0], [0, 101, 40, 0], [0, np.nan, 1, 0]]),   # a NaN in P
           d.Lens("plumb_bob", K, (), P=[[100, 0, 50, np.nan], [0, 101, 40, 0], [0, 0, 1, 0]]),   # ... in its unread column too
           d.Lens("plumb_bob", K, (0.1, np.inf, 0, 0)),
           d.Lens("plumb_bob", K, (), R=np.full((3, 3), np.nan))]
    for lens in bad:
        assert L.dsi_lens_check(C.byref(_raw(lens))) == engine.ERR_INVALID
        assert L.dsi_last_error()
        with pytest.raises(d.DsiError) as e:
            lens.check()
        assert e.value.code == engine.ERR_INVALID
    # 12 coefficients (thin-prism) do not fit dsi_lens_t; the count alone is refused
    raw = _raw(ok[0])
    raw.n_dist = 12
    assert L.dsi_lens_check(C.byref(raw)) == engine.ERR_INVALID
    with pytest.raises(ValueError):
        d.Lens("plumb_bob", K, (0.0,) * 12)
    with pytest.raises(ValueError):
        d.Lens("equidistant", K, (0.0,) * 4)
    assert L.dsi_lens_check(None) == engine.ERR_INVALID
    # a coefficient beyond n_dist is not read
    raw = _raw(ok[1])
    raw.D[6] = np.nan
    assert L.dsi_lens_check(C.byref(raw)) == engine.OK
    # refusals of the device entry points that are decided before the GPU is touched
    out = np.zeros(8, np.float32)
    f32p = out.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dsi_rectify_lut(None, C.byref(_raw(ok[0])), 2, 2, f32p) == engine.ERR_INVALID
    assert L.dsi_mapper_create_with_lens(None, None, None, None) == engine.ERR_INVALID


def test_lens_rr_is_the_restatements_product_bit_for_bit(built):
    for name in ("plumb_bob_A", "plumb_bob_C", "fisheye_A"):          # rotated stereo pairs
        lens, _, _ = cases.camera(name)
        got = lens.rr()
        want = rr.rr_of(lens.R, lens.P)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
        assert not np.array_equal(got, lens.P[:, :3])                # the rotation is in it
        assert np.allclose(got, lens.P[:, :3] @ lens.R, rtol=1e-15, atol=0)
    # the order of the additions is the contract: a case where (a + b) + c and a + (b + c) differ
    lens = d.Lens("plumb_bob", np.eye(3), (), R=[[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0]],
                  P=[[1e16, 1.0, 1.0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])
    assert lens.rr()[0, 0] == (1e16 + 1.0) + 1.0 == 1e16 and 1e16 + (1.0 + 1.0) != 1e16
    assert np.array_equal(lens.rr(), rr.rr_of(lens.R, lens.P))
    # defaults: R = I, P = [K | 0] -> RR = K exactly
    K = np.array([[226.38, 0, 173.65], [0, 226.15, 133.73], [0, 0, 1.0]])
    assert np.array_equal(d.Lens("fisheye", K, (0,) * 4).rr(), K)


def test_new_symbols_are_exported_and_bound(built):
    L = d.load_library()
    for name in ("dsi_lens_check", "dsi_lens_rr", "dsi_rectify_lut", "dsi_rectify_lut_dev", "dsi_mapper_create_with_lens"):
        assert getattr(L, name).argtypes is not None, name
    assert L.dsi_abi_version() == 10
    hdr = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert "DSI_ENGINE_ABI_VERSION 10" in hdr
    # dsi_lens_t as the header lays it out: two ints, then 38 doubles
    assert C.sizeof(engine._Lens) == 8 + 8 * (9 + 8 + 9 + 12)
    for name in ("Lens", "rectify_lut", "rectify_lut_dev", "LENS_PLUMB_BOB", "LENS_FISHEYE"):
        assert name in d.__all__ and hasattr(d, name)
    assert (d.LENS_PLUMB_BOB, d.LENS_FISHEYE) == (0, 1)


def test_python_lens_defaults_and_exclusive_arguments(built):
    K = [[100.0, 0, 50.0], [0, 101.0, 40.0], [0, 0, 1.0]]
    lens = d.Lens("fisheye", K, (0.1, 0.2, 0.3, 0.4))
    assert lens.model == d.LENS_FISHEYE and np.array_equal(lens.R, np.eye(3))
    assert np.array_equal(lens.P, np.hstack([np.array(K), np.zeros((3, 1))]))
    raw = lens._c()
    assert raw.n_dist == 4 and list(raw.D) == [0.1, 0.2, 0.3, 0.4, 0, 0, 0, 0] and list(raw.K) == list(np.ravel(K))
    # lut= and lens= exclude each other, decided before anything touches the GPU
    with pytest.raises(ValueError):
        d.MapperEMVS(None, (4, 4, 1.0, 1.0, 2.0, 2.0), d.ShapeDSI(0, 0, 4, 1.0, 2.0, 0.0), lut=np.zeros((16, 2), np.float32),
                     lens=lens)


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_rectify")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_rectify.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_cpp_lens_of_reads_stand_in_camera_types(built, tmp_path):
    """dsi::lens_of on a camera whose matrices look like cv::Matx / cv::Mat_<double> and on one with plain cv::Mat-like
    matrices and a std::vector of coefficients: K, D, R, P and the model arrive as they are; unknown models and coefficient
    counts are refused; the host camera_of(cam, &out) still calls rectifyPoint for plumb_bob and refuses fisheye."""
    exe = build_cpp(tmp_path)
    r = subprocess.run([exe, "--lens-of"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK")
    got = {}
    for ln in r.stdout.splitlines()[:-1]:
        cam, tag, *vals = ln.split()
        got[cam, tag] = vals
    a, _, _ = cases.camera("plumb_bob_A")
    c, _, _ = cases.camera("plumb_bob_C")

    def nums(key):
        return np.array([float(v) for v in got[key]])

    assert got["matx", "model"] == ["plumb_bob", "n_dist", "4"]
    assert got["fisheye", "model"] == ["fisheye", "n_dist", "4"]
    assert got["plain", "model"] == ["plumb_bob", "n_dist", "8"]          # no cameraInfo(): image_geometry's default
    for cam in ("matx", "plain"):
        assert np.array_equal(nums((cam, "K")), a.K.ravel())
        assert np.array_equal(nums((cam, "P")), a.P.ravel())
        assert np.allclose(nums((cam, "R")), a.R.ravel(), rtol=0, atol=1e-15)   # (cos / sin of the C library and numpy's)
    assert np.array_equal(nums(("matx", "D")), np.concatenate([a.D, np.zeros(4)]))
    assert np.array_equal(nums(("plain", "D")), c.D)
    assert np.array_equal(nums(("fisheye", "K")), [180.5, 0, 172.0, 0, 180.1, 131.0, 0, 0, 1])
    assert np.array_equal(nums(("fisheye", "D")), [-0.04, 0.003, -0.002, 0.0003, 0, 0, 0, 0])
    # dsi::Lens().set_K(...).set_D(...): R = I, P = [K | 0]
    assert got["own", "model"] == ["plumb_bob", "n_dist", "4"]
    assert np.array_equal(nums(("own", "R")), np.eye(3).ravel())
    assert np.array_equal(nums(("own", "P")), [100, 0, 50, 0, 0, 101, 40, 0, 0, 0, 1, 0])
    assert np.array_equal(nums(("own", "K")), [100, 0, 50, 0, 101, 40, 0, 0, 1])


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_rectify_kernels_use_registers_only():
    """k_rectify_lut<plumb_bob> and <fisheye>: no scratch, no spills, no LDS, no atomics; 256-thread workgroups; the
    coefficients and RR (21 doubles) arrive in the kernel-argument segment."""
    text = kernel_asm_text()
    seen = set()
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_rectify_lut" not in name:
            continue
        seen.add(name)
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, name
        assert val("group_segment_fixed_size") == 0, name
        assert val("wavefront_size") == 64 and val("max_flat_workgroup_size") == 256 and val("vgpr_count") <= 64, name
        assert val("kernarg_segment_size") >= 21 * 8 + 4 + 8 + 8, name
    assert len(seen) == 2, seen
    bodies = list(re.finditer(r"^(_ZN\w*k_rectify_lut\w*):.*?$(.*?)s_endpgm", text, re.S | re.M))
    assert len(bodies) == 2, [m.group(1) for m in bodies]
    for m in bodies:
        body = m.group(2)
        assert "atomic" not in body and "ds_" not in body and "scratch_" not in body, m.group(1)
        assert "global_store_dwordx2" in body                    # the float2 entry, one vector store
