"""The volume filters without a GPU: the numpy restatement (tests/volume_filters_reference.py) against what the compiled
reference wrote into tests/golden/volume_filters.npz, subnormal handling, the diffusion's step counts, Moran's index on
volumes whose structure is known, and the new entry points' declarations and null-handle checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import volume_filters_reference as vf
from dvs_mcemvs_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TINY = np.finfo(F).tiny          # 2^-126
SYMBOLS = ("dsi_grid_laplacian", "dsi_grid_smooth_diffuse", "dsi_grid_smooth_iir", "dsi_grid_mean_std", "dsi_grid_moran_index")


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "volume_filters.npz"))
    return {k: z[k] for k in z.files}


def subnormals(v):
    return int(((v != 0) & (np.abs(v) < TINY)).sum())


def test_restatement_equals_the_compiled_reference_bit_for_bit(golden):
    names = [str(n) for n in golden["names"]]
    assert set(names) >= {"a", "b", "c", "impulse"}
    assert golden["in_a"].shape == (3, 5, 7) and golden["in_b"].shape == (5, 12, 35) and golden["in_c"].shape == (1, 4, 65)
    assert golden["in_impulse"].shape == (3, 5, 70) and list(golden["sigma_impulse"]) == [F(0.5)] * 3
    for n in names:
        got = vf.iir3(golden["in_" + n], *golden["sigma_" + n], numsteps=int(golden["steps_" + n]))
        assert vf.same_bits(got, golden["iir_" + n]).all(), n


def test_impulse_output_holds_subnormals(golden):
    assert golden["in_impulse"].sum() == 1 and (golden["in_impulse"] != 0).sum() == 1
    assert subnormals(golden["iir_impulse"]) >= 1
    assert subnormals(vf.iir3(golden["in_impulse"], 0.5, 0.5, 0.5)) == subnormals(golden["iir_impulse"])


def test_restated_diffusion_and_laplacian_are_what_the_file_holds(golden):
    for n in ("a", "b"):
        assert vf.same_bits(vf.laplacian(golden["in_" + n]), golden["restated_laplacian_" + n]).all()
        got, steps = vf.diffuse(golden["in_" + n], golden["restated_diffuse_sigma_" + n])
        assert steps == int(golden["restated_diffuse_steps_" + n])
        assert vf.same_bits(got, golden["restated_diffuse_" + n]).all()


def test_diffusion_step_counts():
    assert [vf.diffusion_schedule(s)[1] for s in (1.0, 2.0, 0.3, 0.7)] == [12, 48, 2, 6]
    assert vf.diffusion_schedule(0.5)[1] == 3


def test_diffusion_of_an_impulse_runs_through_subnormals():
    v = np.zeros((2, 3, 70), F)
    v[0, 1, 0] = 1
    out, steps = vf.diffuse(v, 2.0)
    assert steps == 48
    assert subnormals(out) >= 1


def test_laplacian_by_hand():
    v = np.zeros((1, 1, 3), F)
    v[0, 0] = [1, 4, 9]
    # clamped neighbours: y and z differences vanish; x: (4 - 2) + 1, (9 - 8) + 1, (9 - 18) + 4
    assert list(vf.laplacian(v)[0, 0]) == [3, 2, -5]
    assert vf.laplacian(np.full((2, 1, 1), 7, F)).tolist() == [[[0.0]], [[0.0]]]


def test_a_line_of_one_voxel_is_scaled_twice_per_step():
    v = np.full((1, 1, 1), 3, F)
    want = F(3)
    post = F(1)
    for s in (0.7, 1.3, 2.0):
        nu, bs, p = vf.iir_coefficients(s, 3)
        post = F(post * p)
        for _ in range(3):
            want = F(F(want * bs) * bs)
    assert vf.iir3(v, 0.7, 1.3, 2.0)[0, 0, 0] == F(want * post)


def test_iir_leaves_the_volume_alone_for_a_zero_sigma_or_no_steps():
    v = np.random.default_rng(3).random((2, 3, 4)).astype(F)
    assert vf.same_bits(vf.iir3(v, 0.0, 1, 1), v).all() and vf.same_bits(vf.iir3(v, 1, 1, 1, numsteps=0), v).all()


def test_moran_index_tells_structure_from_noise():
    rng = np.random.default_rng(5)
    noise = rng.random((6, 20, 35)).astype(F)
    smooth = vf.iir3(noise, 3, 3, 3)
    assert vf.moran(smooth, 1.0) > 0.8
    assert vf.moran(noise, 1.0) < 0.1
    # sigma below 0.2 is raised to 0.2: kernel size 5
    assert vf.moran_kernel(0.1)[:2] == (F(0.2), 5)
    assert vf.moran_kernel(0.1)[2] == vf.moran_kernel(0.2)[2]
    assert vf.moran(noise, 0.1) == vf.moran(noise, 0.2)
    assert vf.moran_kernel(1.0)[1] == 13


def test_mean_std_definition():
    v = np.array([[[1, 2, 3, 6]]], F)
    assert vf.mean_std(v) == (3.0, np.sqrt(3.5))


def test_header_declares_the_five_symbols():
    text = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    for s in SYMBOLS:
        assert re.search(r"DSI_API\s+int\s+%s\s*\(" % s, text), s
    assert re.search(r"#define\s+DSI_ENGINE_ABI_VERSION\s+10\b", text)
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for member in ("smoothInPlace(const float sigma = 1.f)", "laplacianInPlace()", "computeMoranIndexGaussianWeights(float sigma) const",
                   "computeMeanStd(double* mean, double* stddev) const",
                   "smoothInPlaceIIR3D(const float sigma_x = 1.f, const float sigma_y = 1.f, const float sigma_z = 1.f)"):
        assert member in hpp, member


def test_null_handles_are_refused_without_a_gpu(built):
    L = d.load_library()
    a, b = ctypes.c_double(), ctypes.c_double()
    n = ctypes.c_int()
    assert L.dsi_abi_version() == 10
    assert L.dsi_grid_laplacian(None) == engine.ERR_INVALID
    assert b"null" in L.dsi_last_error()
    assert L.dsi_grid_smooth_diffuse(None, 1.0, ctypes.byref(n)) == engine.ERR_INVALID
    assert L.dsi_grid_smooth_iir(None, 1.0, 1.0, 1.0, 3) == engine.ERR_INVALID
    assert L.dsi_grid_mean_std(None, ctypes.byref(a), ctypes.byref(b)) == engine.ERR_INVALID
    assert L.dsi_grid_moran_index(None, 1.0, ctypes.byref(a)) == engine.ERR_INVALID
    for name in ("laplacian", "smooth_diffuse", "smooth_iir", "mean_std", "moran_index"):
        assert callable(getattr(d.Grid3D, name))
