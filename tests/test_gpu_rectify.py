"""Lens rectification on the device: k_rectify_lut against the numpy restatement of
tests/rectify_reference.py, a round trip through the forward models that does not use the restatement, and the table's way
into the mappers (dsi_mapper_create_with_lens, MapperEMVS(lens=), the C++ constructor, full_sequence(lenses=)).

plumb_bob B is the camera the feature was specified with; its D = (-0.6, 0.1, 0, 0, 0) cannot make icdist negative
(1 - 0.6 r2 + 0.1 r2^2 > 0 for every r2: tests/test_rectify_cpu.py), so plumb_bob B2 -- the same camera with k2 = 0.05 -- stands
beside it and is the one asked to take that branch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import rectify_cases as cases
import rectify_reference as rr
from dvs_mcemvs_amd import engine, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_REF = {}


def reference(name):
    """The restatement's table of a camera, computed once."""
    if name not in _REF:
        lens, w, h = cases.camera(name)
        lut, info = rr.rectify_lut(lens, w, h, return_info=True)
        lut.setflags(write=False)
        _REF[name] = (lut, info)
    return _REF[name]


# ---------------------------------------------------------------------------------------- 1. plumb_bob: bit for bit
@pytest.mark.parametrize("name", cases.PLUMB_BOB)
def test_plumb_bob_table_equals_the_restatement_bit_for_bit(ctx, name):
    lens, w, h = cases.camera(name)
    want, info = reference(name)
    if name == "plumb_bob_B2":
        assert info["icdist_negative"].any() and (~info["icdist_negative"]).any()
    got = d.rectify_lut(ctx, lens, w, h)
    assert got.dtype == np.float32 and got.shape == (w * h, 2)
    diff = got.view(np.uint32) != want.view(np.uint32)
    print("%s: %d of %d entries differ" % (name, int(diff.sum()), diff.size))
    assert not diff.any(), "first differing entries: %s" % (np.argwhere(diff)[:5].tolist(),)


def test_unread_entries_are_not_read(ctx):
    """P's fourth column and the coefficients beyond n_dist do not enter."""
    lens, w, h = cases.camera("plumb_bob_A")
    assert lens.P[0, 3] != 0.0
    want = d.rectify_lut(ctx, lens, w, h)
    other = d.Lens(lens.model, lens.K, lens.D, lens.R, lens.P.copy())
    other.P[:, 3] = (123.0, -4.0, 0.5)
    assert np.array_equal(d.rectify_lut(ctx, other, w, h), want)
    raw = lens._c()
    raw.D[4], raw.D[7] = 0.3, -0.2                     # n_dist = 4: k3 and k6 are 0 whatever the array holds
    got = np.empty_like(want)
    engine._check(d.load_library().dsi_rectify_lut(ctx._h, C.byref(raw), w, h, got.ctypes.data_as(C.POINTER(C.c_float))))
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------ 2. fisheye
@pytest.mark.parametrize("name", cases.FISHEYE)
def test_fisheye_table_against_the_restatement(ctx, name):
    """The same sentinel pixels; every other entry within 1 float32 ulp; at most 4 entries that differ at all (only tan is
    not correctly rounded: a couple of double ulps flip a float32 rounding with a probability of the order of 1e-8)."""
    lens, w, h = cases.camera(name)
    want, info = reference(name)
    if name == "fisheye_B":
        sent = info["sentinel"]
        assert sent.any() and (~sent).any() and np.isfinite(want[~sent]).all()
        assert info["small"].any()                      # theta_d <= 1e-8 at the principal point
    got = d.rectify_lut(ctx, lens, w, h)
    s_got = got == np.float32(rr.SENTINEL)
    s_want = want == np.float32(rr.SENTINEL)
    assert np.array_equal(s_got, s_want)
    assert np.array_equal(s_want[:, 0], info["sentinel"]) and np.array_equal(s_want[:, 1], info["sentinel"])
    keep = ~s_want
    differ = got.view(np.uint32) != want.view(np.uint32)
    ulps = np.abs(got[keep].astype(np.float64) - want[keep].astype(np.float64)) / np.spacing(np.abs(want[keep])).astype(np.float64)
    print("%s: %d of %d entries differ, largest difference %.1f float32 ulp, %d sentinel pixels" %
          (name, int(differ.sum()), differ.size, float(ulps.max()), int(info["sentinel"].sum())))
    assert np.isfinite(got[keep]).all() and ulps.max() <= 1.0
    assert int(differ.sum()) <= 4


# ----------------------------------------------------------------------------- 3. round trip, without the restatement
@pytest.mark.parametrize("name", ["plumb_bob_A", "fisheye_A"])
def test_round_trip_through_the_forward_model(ctx, name):
    """R = I, P = [K | 0]: the forward model applied to the ENGINE's table returns the raw pixel.  Bound: twice the largest
    residual the restatement's own table leaves on this camera (the error of the fixed number of rounds; computed here as in
    tests/test_rectify_cpu.py, not fixed in advance) plus 2 float32 ulps of the largest coordinate."""
    lens, w, h = cases.simple(name)
    own = rr.round_trip_residual(lens, rr.rectify_lut(lens, w, h), w, h)
    got = d.rectify_lut(ctx, lens, w, h)
    assert not (got == np.float32(rr.SENTINEL)).any() and np.isfinite(got).all()
    res = rr.round_trip_residual(lens, got, w, h)
    bound = 2.0 * own + 2.0 * cases.ulp32(np.abs(got).max())
    print("%s: engine residual %.3e pixels, restatement's %.3e, bound %.3e" % (name, res, own, bound))
    assert res <= bound


# ------------------------------------------------------------------------------------------------- 4. mapper path
def _rig():
    return syn.stereo_rig(8192, width=346, height=260, duration=0.3, seed=21)


def _dsi_of(mapper, rig):
    assert mapper.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    return mapper.dsi_.download()


def _config(cam, shape):
    w, h, fx, fy, cx, cy = cam
    cfg = engine._MapperConfig()
    cfg.sensor_width, cfg.sensor_height = int(w), int(h)
    cfg.K = (C.c_float * 4)(fx, fy, cx, cy)
    cfg.dim_x, cfg.dim_y, cfg.dim_z = shape.dimX_, shape.dimY_, shape.dimZ_
    cfg.min_depth, cfg.max_depth, cfg.fov_deg = shape.min_depth_, shape.max_depth_, shape.fov_
    return cfg


def test_mapper_with_lens_equals_mapper_with_the_table(ctx):
    """346 x 260 x 32, one batch of 8 packets: the DSI of a mapper whose table was made on the device in place is that of a
    mapper given dsi_rectify_lut's host table, bit for bit; both differ from a mapper without a table."""
    lens, w, h = cases.camera("plumb_bob_A")
    rig = _rig()
    assert rig["events"][0][0].shape[0] == 8192 and rig["cam"][:2] == (w, h)
    shape = d.ShapeDSI(0, 0, 32, 4.0, 200.0, 0.0)
    lut = d.rectify_lut(ctx, lens, w, h)
    with_lens = d.MapperEMVS(ctx, rig["cam"], shape, lens=lens)            # dsi_mapper_create_with_lens
    with_table = d.MapperEMVS(ctx, rig["cam"], shape, lut=lut)             # dsi_mapper_create
    without = d.MapperEMVS(ctx, rig["cam"], shape)
    a, b, c = (_dsi_of(m, rig) for m in (with_lens, with_table, without))
    assert a.shape == (32, h, w) and a.sum() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, c) and not np.array_equal(b, c)
    for m in (with_lens, with_table, without):
        m.close()
    with pytest.raises(ValueError):
        d.MapperEMVS(ctx, rig["cam"], shape, lut=lut, lens=lens)


def test_cpp_constructor_and_camera_of(built, ctx, tmp_path):
    """tests/cpp/test_rectify.cpp: camera_of(ctx, cam, &out) for both models without a call of rectifyPoint, MapperEMVS(ctx,
    cam, lens, shape) against the table and against no table; the tables it got are the Python binding's."""
    exe = str(tmp_path / "test_rectify")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_rectify.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK")
    lens, w, h = cases.camera("plumb_bob_A")
    got = np.fromfile(out / "plumb_bob.lut.f32", np.float32).reshape(-1, 2)
    # (R comes from the C library's cos / sin there and from numpy's here, which may differ in the last bit: the program's
    #  tables are compared with the restatement loosely -- the bit-for-bit comparison is tests 1 and 2 -- and the DSIs they
    #  produce are compared exactly inside the program)
    assert got.shape == (w * h, 2)
    assert np.allclose(got, reference("plumb_bob_A")[0], rtol=0, atol=1e-3)
    fish = d.Lens("fisheye", [[180.5, 0, 172.0], [0, 180.1, 131.0], [0, 0, 1]], (-0.04, 0.003, -0.002, 0.0003), lens.R, lens.P)
    gotf = np.fromfile(out / "fisheye.lut.f32", np.float32).reshape(-1, 2)
    assert np.allclose(gotf, rr.rectify_lut(fish, w, h), rtol=0, atol=1e-3)
    assert not np.allclose(gotf, got, rtol=0, atol=1.0)


# ------------------------------------------------------------------------------------------ 5. full_sequence(lenses=)
def test_full_sequence_with_lenses_equals_luts(ctx):
    """Two windows at 67 x 45 x 16: lenses= gives what the same call with lut-constructed mappers gives."""
    lens_b, w, h = cases.camera("plumb_bob_B")
    lens_b2, _, _ = cases.camera("plumb_bob_B2")
    rig = syn.stereo_rig(30_000, width=w, height=h, t0=3.0, duration=0.6, seed=9)
    shape = d.ShapeDSI(0, 0, 16, 4.0, 100.0, 0.0)
    args = (ctx, (rig["cam"],) * 2, shape, rig["events"], rig["trajectories"], 3.0, 3.6, 0.3, 0.3)
    luts = (d.rectify_lut(ctx, lens_b, w, h), d.rectify_lut(ctx, lens_b2, w, h))
    want = list(proc.full_sequence(*args, luts=luts))
    got = list(proc.full_sequence(*args, lenses=(lens_b, lens_b2)))
    plain = list(proc.full_sequence(*args))
    assert len(want) == len(got) == len(plain) == 2
    for g, q in zip(got, want):
        assert len(g) == len(q) == 4 and g[0] == q[0]
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(g[1:], q[1:]))
    assert any(not np.array_equal(g[3], p[3]) for g, p in zip(got, plain))          # the lenses are applied
    # Alg. 2 windows take the same argument (the materialising path makes its own mappers from it)
    kw = dict(process_method=2, num_subintervals=2, temporal_fusion=4)
    want2 = list(proc.full_sequence(*args, luts=luts, **kw))
    got2 = list(proc.full_sequence(*args, lenses=(lens_b, lens_b2), **kw))
    assert len(want2) == len(got2) == 2
    for g, q in zip(got2, want2):
        for a, b in zip(g[1:], q[1:]):
            assert (a is None) == (b is None)
            if a is not None:
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# --------------------------------------------------------------------------------------- 6. refusals on the device path
def test_refusals_on_the_device_path(built):
    L = d.load_library()
    own = d.Context(0)                                   # (its destruction is refused while an object created from it lives)
    lens, w, h = cases.camera("plumb_bob_A")
    shape = d.ShapeDSI(0, 0, 32, 4.0, 200.0, 0.0)
    cam = (w, h, 199.65, 199.65, 177.43, 126.81)
    cfg = _config(cam, shape)
    table = np.zeros((w * h, 2), np.float32)
    cfg.lut = table.ctypes.data_as(C.POINTER(C.c_float))
    handle = C.c_void_p(0xdead)
    assert L.dsi_mapper_create_with_lens(own._h, C.byref(cfg), C.byref(lens._c()), C.byref(handle)) == engine.ERR_INVALID
    assert not handle.value and b"exclude" in L.dsi_last_error()
    cfg = _config(cam, shape)
    bad = d.Lens("plumb_bob", lens.K, (0.1, 0.2, 0.3))
    assert L.dsi_mapper_create_with_lens(own._h, C.byref(cfg), C.byref(bad._c()), C.byref(handle)) == engine.ERR_INVALID
    assert not handle.value
    for ww, hh in ((0, h), (w, 0), (0, 0), (-3, h)):      # width * height == 0 (and below)
        cfg = _config((ww, hh) + cam[2:], shape)
        assert L.dsi_mapper_create_with_lens(own._h, C.byref(cfg), C.byref(lens._c()), C.byref(handle)) == engine.ERR_INVALID
        assert not handle.value
        out = np.zeros(8, np.float32)
        assert L.dsi_rectify_lut(own._h, C.byref(lens._c()), ww, hh, out.ctypes.data_as(C.POINTER(C.c_float))) == engine.ERR_INVALID
        with pytest.raises(d.DsiError):
            d.rectify_lut(own, lens, ww, hh)
    with pytest.raises(d.DsiError) as e:
        d.rectify_lut(own, bad, w, h)
    assert e.value.code == engine.ERR_INVALID
    with pytest.raises(d.DsiError):
        d.MapperEMVS(own, cam, shape, lens=bad)
    # a good one still works here, and nothing was leaked: the context goes
    m = d.MapperEMVS(own, cam, shape, lens=lens)
    m.close()
    own.close()


def test_device_twin_writes_the_same_table(ctx):
    """dsi_rectify_lut_dev into memory of the caller's (a grid of 2 x H x W floats), queued on the stream."""
    lens, w, h = cases.camera("plumb_bob_C")
    g = d.Grid3D(ctx, w, h, 2)
    d.rectify_lut_dev(ctx, lens, w, h, g.device_ptr)
    got = g.download().reshape(-1, 2)
    assert np.array_equal(got.view(np.uint32), reference("plumb_bob_C")[0].view(np.uint32))
    g.close()
