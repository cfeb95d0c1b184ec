"""The volume filters on the MI355X: the IIR Gaussian bit for bit against the compiled reference's outputs
(tests/golden/volume_filters.npz) and against the restatement of tests/volume_filters_reference.py on shapes that straddle
waves, tiles and the LDS capacity; the Laplacian and the diffusion bit for bit against the restatement; mean / deviation;
Moran's index; a smoothed DSI through the arg-max; the C++ members."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import volume_filters_reference as vf
from dvs_mcemvs_amd import engine, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TINY = np.finfo(F).tiny
# (z, y, x).  (2, 65, 130): more than one wave of lanes and of rows; (2, 3, 1030) / (2, 1030, 3) / (256, 3, 5): long lines
# along each axis -- 1030 along y does not fit the LDS line set (640 voxels), 256 along z fills 64 KiB exactly; (700, 2, 3)
# and (1, 2, 5200): z lines beyond the LDS line set and x rows too long for eight of them to fit the LDS
SHAPES = [(3, 5, 7), (9, 33, 70), (2, 65, 130), (1, 4, 65), (2, 3, 1030), (2, 1030, 3), (256, 3, 5), (2, 1, 1),
          (700, 2, 3), (1, 2, 5200)]
SIGMAS = [(0.7, 1.3, 2.0), (0.5, 0.5, 0.5)]


def grid_of(ctx, vol):
    nz, ny, nx = vol.shape
    g = d.Grid3D(ctx, nx, ny, nz)
    g.upload(vol)
    return g


def code_of(fn):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code


def volume(shape, seed=0):
    """Vote-like magnitudes, a third of them exactly zero."""
    rng = np.random.default_rng(1000 + seed)
    v = (rng.random(shape) * 50).astype(F)
    v[rng.random(shape) < 0.33] = 0
    return v


def assert_same(got, want, what=""):
    bad = np.argwhere(~vf.same_bits(got, want))
    assert bad.shape[0] == 0, "%s: %d of %d voxels differ, first %s" % (
        what, bad.shape[0], want.size, [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in bad[:4]])


def subnormals(v):
    return int(((v != 0) & (np.abs(v) < TINY)).sum())


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "volume_filters.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def moran_volumes():
    rng = np.random.default_rng(5)
    noise = rng.random((6, 20, 35)).astype(F)
    return {"noise": noise, "smooth": vf.iir3(noise, 3, 3, 3), "votes": volume((9, 33, 70), 7)}


# ------------------------------------------------------------------------------------------------------------ IIR
def test_iir_equals_the_compiled_reference(ctx, golden):
    for name in (str(n) for n in golden["names"]):
        g = grid_of(ctx, golden["in_" + name])
        g.smooth_iir(*[float(s) for s in golden["sigma_" + name]], numsteps=int(golden["steps_" + name]))
        assert_same(g.download(), golden["iir_" + name], name)
        g.close()
    g = grid_of(ctx, golden["in_impulse"])
    g.smoothInPlaceIIR3D(0.5, 0.5, 0.5)
    got = g.download()
    assert subnormals(got) == subnormals(golden["iir_impulse"]) >= 1      # nothing flushed
    g.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_iir_equals_the_restatement(ctx, shape):
    v = volume(shape)
    g = d.Grid3D(ctx, shape[2], shape[1], shape[0])
    ptr = g.device_ptr
    for sig in SIGMAS:
        g.upload(v)
        g.smooth_iir(*sig)
        assert_same(g.download(), vf.iir3(v, *sig), "%s sigma %s" % (shape, sig))
    assert g.device_ptr == ptr
    g.close()


def test_iir_impulses_run_through_subnormals(ctx):
    for shape, at in (((3, 5, 70), (2, 4, 69)), ((2, 70, 3), (0, 0, 1)), ((70, 2, 3), (69, 1, 2))):
        v = np.zeros(shape, F)
        v[at] = 1
        want = vf.iir3(v, 0.5, 0.5, 0.5)
        assert subnormals(want) >= 1
        g = grid_of(ctx, v)
        g.smooth_iir(0.5, 0.5, 0.5)
        assert_same(g.download(), want, "impulse %s" % (shape,))
        g.close()


def test_iir_numsteps_and_the_cases_that_change_nothing(ctx):
    v = volume((9, 33, 70), 1)
    g = grid_of(ctx, v)
    for numsteps in (1, 4):
        g.upload(v)
        g.smooth_iir(0.7, 1.3, 2.0, numsteps=numsteps)
        assert_same(g.download(), vf.iir3(v, 0.7, 1.3, 2.0, numsteps=numsteps), "numsteps %d" % numsteps)
    g.upload(v)
    for args in ((0.0, 1.0, 1.0, 3), (1.0, -1.0, 1.0, 3), (1.0, 1.0, 0.0, 3), (1.0, 1.0, 1.0, 0), (1.0, 1.0, 1.0, -2)):
        g.smooth_iir(*args)
        assert_same(g.download(), v, "unchanged %s" % (args,))
    assert code_of(lambda: g.smooth_iir(1.0, 1.0, 1.0, 17)) == engine.ERR_INVALID
    g.smooth_iir(1.0, 1.0, 1.0, 16)
    assert_same(g.download(), vf.iir3(v, 1.0, 1.0, 1.0, numsteps=16), "numsteps 16")
    g.close()


# ------------------------------------------------------------------------------------------- Laplacian, diffusion
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_laplacian_and_diffusion_equal_the_restatement(ctx, shape):
    v = volume(shape, 2)
    g = d.Grid3D(ctx, shape[2], shape[1], shape[0])
    ptr = g.device_ptr
    g.upload(v)
    g.laplacian()
    assert_same(g.download(), vf.laplacian(v), "laplacian %s" % (shape,))
    g.upload(v)
    want, steps = vf.diffuse(v, 0.3)
    assert steps == 2 and g.smooth_diffuse(0.3) == steps          # even: the last step lands in the grid
    assert_same(g.download(), want, "diffuse 0.3 %s" % (shape,))
    assert g.device_ptr == ptr
    g.close()


def test_diffusion_with_an_odd_step_count_and_the_golden_volumes(ctx, golden):
    v = volume((9, 33, 70), 3)
    g = grid_of(ctx, v)
    want, steps = vf.diffuse(v, 0.5)
    assert steps == 3 and g.smooth_diffuse(0.5) == 3              # odd: copied back from the scratch volume
    assert_same(g.download(), want, "diffuse 0.5")
    g.upload(v)
    want, steps = vf.diffuse(v, 1.0)
    assert steps == 12 and g.smoothInPlace() == 12
    assert_same(g.download(), want, "diffuse 1")
    g.close()
    for n in ("a", "b"):
        g = grid_of(ctx, golden["in_" + n])
        g.laplacian()
        assert_same(g.download(), golden["restated_laplacian_" + n], "golden laplacian " + n)
        g.upload(golden["in_" + n])
        assert g.smooth_diffuse(float(golden["restated_diffuse_sigma_" + n])) == int(golden["restated_diffuse_steps_" + n])
        assert_same(g.download(), golden["restated_diffuse_" + n], "golden diffusion " + n)
        g.close()


def test_diffusion_of_an_impulse_keeps_subnormals(ctx):
    v = np.zeros((2, 3, 70), F)
    v[0, 1, 0] = 1
    want, steps = vf.diffuse(v, 2.0)
    assert steps == 48 and subnormals(want) >= 1
    g = grid_of(ctx, v)
    assert g.smooth_diffuse(2.0) == 48
    assert_same(g.download(), want, "impulse")
    g.close()


def test_diffusion_refuses_sigmas_without_a_schedule(ctx):
    v = volume((3, 5, 7), 4)
    g = grid_of(ctx, v)
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e4):
        assert code_of(lambda: g.smooth_diffuse(sigma)) == engine.ERR_INVALID, sigma
    assert_same(g.download(), v, "refused calls change nothing")
    assert engine.load_library().dsi_grid_smooth_diffuse(g._h, 0.3, None) == 0      # steps_out is optional
    g.close()


def test_filters_on_a_wrapped_grid_and_on_a_mappers_grid(ctx):
    v = volume((5, 12, 35), 5)
    owner = d.Grid3D(ctx, 35, 12, 5)
    w = d.Grid3D(ctx, 35, 12, 5, device_ptr=owner.device_ptr)
    assert w.device_ptr == owner.device_ptr
    for run, want in ((lambda g: g.laplacian(), vf.laplacian(v)), (lambda g: g.smooth_diffuse(0.5), vf.diffuse(v, 0.5)[0]),
                      (lambda g: g.smooth_iir(0.7, 1.3, 2.0), vf.iir3(v, 0.7, 1.3, 2.0))):
        w.upload(v)
        run(w)
        assert w.device_ptr == owner.device_ptr
        assert_same(owner.download(), want, "wrapped")             # the result is in the caller's memory
    w.close()
    owner.close()
    rig = syn.stereo_rig(20000, width=96, height=72, duration=0.2, seed=7)
    m = d.MapperEMVS(ctx, rig["cam"], d.ShapeDSI(0, 0, 32, 4.0, 200.0, 0.0))
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    dsi = m.dsi_.download()
    ptr = m.dsi_.device_ptr
    m.dsi_.laplacian()
    assert_same(m.dsi_.download(), vf.laplacian(dsi), "mapper laplacian")
    m.dsi_.upload(dsi)
    m.dsi_.smooth_diffuse(0.5)
    assert_same(m.dsi_.download(), vf.diffuse(dsi, 0.5)[0], "mapper diffusion")
    assert m.dsi_.device_ptr == ptr
    m.close()


# ------------------------------------------------------------------------------------------------ mean, deviation
def test_mean_std(ctx, moran_volumes):
    for v in (moran_volumes["votes"], volume((2, 65, 130), 6), volume((256, 3, 5), 6), np.full((2, 1, 1), 3, F)):
        g = grid_of(ctx, v)
        mean, std = g.mean_std()
        want_mean, want_std = vf.mean_std(v)
        print("mean_std %s: %r %r (want %r %r)" % (v.shape, mean, std, want_mean, want_std))
        assert abs(mean - want_mean) <= 1e-10 * abs(want_mean)
        assert abs(std - want_std) <= 1e-10 * abs(want_std)
        again = g.mean_std()
        assert np.array([mean, std]).tobytes() == np.array(again).tobytes()     # a fixed tree: the same bits
        assert_same(g.download(), v, "mean_std reads only")
        g.close()


# ---------------------------------------------------------------------------------------------------------- Moran
@pytest.mark.parametrize("name", ["noise", "smooth", "votes"])
def test_moran_index(ctx, moran_volumes, name):
    """|I_gpu - I_ref| <= 1e-9 sum |t_i| / (denom + 1e-6): summing in another order moves the numerator by at most
    N 2^-53 sum |t| (under 2e-12 sum |t| here), a mean or deviation that differs in its last bits flips the fp32 rounding of
    about 2e-6 of the z_i by one ulp; a wrong centre weight or post-scale moves I by 1e-2."""
    v = moran_volumes[name]
    want, t, denom = vf.moran(v, 1.0, details=True)
    g = grid_of(ctx, v)
    got = g.moran_index(1.0)
    bound = 1e-9 * float(np.abs(t).sum()) / (denom + 1e-6)
    print("moran %s: gpu %r reference %r difference %.3g bound %.3g" % (name, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound
    assert_same(g.download(), v, "the grid is not modified")
    if name == "noise":
        assert got < 0.1 and g.moran_index(0.1) == g.moran_index(0.2)         # sigma below 0.2 is raised to 0.2
        want, t, denom = vf.moran(v, 0.2, details=True)
        assert abs(g.moran_index(0.1) - want) <= 1e-9 * float(np.abs(t).sum()) / (denom + 1e-6)
    if name == "smooth":
        assert got > 0.8
    g.close()


def test_moran_index_refuses_a_constant_grid(ctx):
    g = grid_of(ctx, np.full((3, 5, 7), 2.5, F))
    assert code_of(lambda: g.moran_index(1.0)) == engine.ERR_INVALID
    assert code_of(lambda: g.moran_index(float("nan"))) == engine.ERR_INVALID
    g.close()


# ----------------------------------------------------------------------------------------------------- end to end
def test_smoothed_dsi_through_the_arg_max(ctx):
    rig = syn.stereo_rig(20000, width=96, height=72, duration=0.2, seed=7)
    m = d.MapperEMVS(ctx, rig["cam"], d.ShapeDSI(0, 0, 32, 4.0, 200.0, 0.0))
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    dsi = m.dsi_.download()
    assert (dsi > 0).mean() > 0.01
    m.dsi_.smooth_iir(1.0, 1.0, 1.0)
    want = vf.iir3(dsi, 1.0, 1.0, 1.0)
    assert_same(m.dsi_.download(), want, "smoothed DSI")
    engine._check(engine.load_library().dsi_mapper_depth_map_of(m._h, m.dsi_._h))
    depth, conf, idx = m.fetchDepthMap()
    want_idx = np.argmax(want, axis=0)                              # the first maximum wins
    assert np.array_equal(idx, want_idx.astype(np.uint8))
    assert_same(conf, np.take_along_axis(want, want_idx[None], 0)[0], "confidence")
    m.dsi_.upload(dsi)
    m.dsi_.smooth_diffuse(1.0)
    want = vf.diffuse(dsi, 1.0)[0]
    engine._check(engine.load_library().dsi_mapper_depth_map_of(m._h, m.dsi_._h))
    depth, conf, idx = m.fetchDepthMap()
    want_idx = np.argmax(want, axis=0)
    assert np.array_equal(idx, want_idx.astype(np.uint8))
    assert_same(conf, np.take_along_axis(want, want_idx[None], 0)[0], "confidence after diffusion")
    m.close()


# --------------------------------------------------------------------------------------------------------- C++
def test_cpp_call_sites(built, ctx, tmp_path):
    exe = str(tmp_path / "test_volume_filters")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_volume_filters.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    nx, ny, nz = 37, 21, 12
    v = volume((nz, ny, nx), 8)
    data = tmp_path / "data"
    data.mkdir()
    v.tofile(str(data / "in.f32"))
    vf.laplacian(v).tofile(str(data / "want_laplacian.f32"))
    vf.diffuse(v, 1.0)[0].tofile(str(data / "want_diffuse_default.f32"))
    vf.diffuse(v, 0.7)[0].tofile(str(data / "want_diffuse_07.f32"))
    vf.iir3(v, 1.0, 1.0, 1.0).tofile(str(data / "want_iir_default.f32"))
    vf.iir3(v, 0.7, 1.3, 2.0).tofile(str(data / "want_iir_mixed.f32"))
    moran, t, denom = vf.moran(v, 1.0, details=True)
    np.array(vf.mean_std(v) + (moran, 1e-9 * float(np.abs(t).sum()) / (denom + 1e-6)), np.float64).tofile(str(data / "stats.f64"))
    r = subprocess.run([exe, str(data), str(nx), str(ny), str(nz)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
