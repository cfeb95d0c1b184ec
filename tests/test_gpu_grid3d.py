"""The Grid3D completion on the MI355X: subtract / ratio / quadratic mean / cubic mean against the outputs
of the genuine reference header (tests/golden/grid3d_ops.npz) and the restatement of tests/grid3d_reference.py, getMinMax
(first minimum, last maximum), getSlice, the 8-bit slice images of imwriteSlices byte for byte, accumulateZSliceAt, the
single-voxel accessors, imwriteSlices from Python and from C++, and the argument checks.  NaN results compare as NaN
(gfx950 and x86 produce different default NaNs); everything else bit for bit."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import grid3d_reference as gr
from dvs_mcemvs_amd import engine, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
OPS = {"subtract": gr.OP_SUBTRACT, "ratio": gr.OP_RATIO, "quadratic_mean": gr.OP_QUADRATIC_MEAN,
       "cubic_mean": gr.OP_CUBIC_MEAN}


def grid_of(ctx, vol):
    nz, ny, nx = vol.shape
    g = d.Grid3D(ctx, nx, ny, nz)
    g.upload(vol)
    return g


def code_of(fn):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "grid3d_ops.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dsi(ctx):
    """One configs[1]-sized DSI (346 x 260 x 100) from evaluateDSI; the grid and its host copy."""
    rig = syn.stereo_rig(400_000, seed=77)
    m = d.MapperEMVS(ctx, rig["cam"], d.ShapeDSI(0, 0, 100, 4.0, 200.0, 0.0))
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    vol = m.dsi_.download()
    assert vol.shape == (100, 260, 346) and (vol > 0).mean() > 0.01
    yield m.dsi_, vol
    m.close()


# ------------------------------------------------------------------------------------------------ binary ops
@pytest.mark.parametrize("name", sorted(OPS))
def test_binary_ops_on_the_fixture(ctx, fixture, name):
    """The fixture's 8,192 pairs as a 32 x 16 x 16 volume: the genuine header's bits."""
    a = fixture["a"].reshape(16, 16, 32)
    g = fixture["g"].reshape(16, 16, 32)
    ga, gg = grid_of(ctx, a), grid_of(ctx, g)
    ga._binary(gg, OPS[name])
    got = ga.download()
    bad = np.argwhere(~gr.same_bits(got, fixture[name].reshape(a.shape)))
    assert bad.shape[0] == 0, [(a[tuple(i)], g[tuple(i)], got[tuple(i)]) for i in bad[:5]]
    assert gr.same_bits(gg.download(), g).all()                        # the second operand is untouched
    ga.close()
    gg.close()


def test_binary_ops_tail_and_in_place(ctx, fixture):
    """7 x 5 x 3 = 105 elements: 26 float4 groups and a tail of one; dst == src is op(a, a)."""
    a = fixture["a"][:105].reshape(3, 5, 7)
    g = fixture["g"][4000:4105].reshape(3, 5, 7)
    for op in OPS.values():
        ga, gg = grid_of(ctx, a), grid_of(ctx, g)
        ga._binary(gg, op)
        assert gr.same_bits(ga.download(), gr.binary_op(a, g, op)).all(), op
        gg._binary(gg, op)
        assert gr.same_bits(gg.download(), gr.binary_op(g, g, op)).all(), op
        ga.close()
        gg.close()
    ga, gg = grid_of(ctx, a), grid_of(ctx, g)
    names = ("subtractTwoGrids", "ratioTwoGrids", "quadraticMeanTwoGrids", "cubicMeanTwoGrids")
    for op, member in zip((1, 2, 3, 4), names):
        ga.upload(a)
        getattr(ga, member)(gg)
        assert gr.same_bits(ga.download(), gr.binary_op(a, g, op)).all(), member
    ga.upload(a)
    ga.ratioTwoGrids(gg, 1e-1)
    assert code_of(lambda: ga.ratioTwoGrids(gg, 1e-2)) == engine.ERR_INVALID
    ga.close()
    gg.close()


def test_binary_op_errors_and_fuse2_still_refuses(ctx):
    a = d.Grid3D(ctx, 7, 5, 3)
    b = d.Grid3D(ctx, 7, 5, 4)
    c = d.Grid3D(ctx, 7, 5, 3)
    assert code_of(lambda: a._binary(b, 1)) == engine.ERR_SHAPE
    for op in (0, 5, 6, 7, -1):
        assert code_of(lambda: a._binary(c, op)) == engine.ERR_BAD_OP
    for op in (0, 7, 8, 9, 10):                                        # the camera fusions did not grow
        assert code_of(lambda: a._fuse(c, op)) == engine.ERR_BAD_OP
        assert code_of(lambda: a.setToFusionOf(c, c, op)) == engine.ERR_BAD_OP
    for o in (a, b, c):
        o.close()


# --------------------------------------------------------------------------------------------------- min / max
def check_min_max(ctx, vol):
    g = grid_of(ctx, vol)
    lo, hi, lp, hp = g.getMinMax()
    rlo, rhi, rlp, rhp = gr.min_max(vol)
    assert (lp, hp) == (rlp, rhp), (vol.shape, lp, hp, rlp, rhp)
    assert F(lo).view(np.uint32) == F(rlo).view(np.uint32) and F(hi).view(np.uint32) == F(rhi).view(np.uint32)
    g.close()
    return lo, hi, lp, hp


def test_min_max_unique_extremes(ctx):
    rng = np.random.default_rng(1)
    vol = rng.permutation(105).astype(F).reshape(3, 5, 7) - F(40)
    lo, hi, lp, hp = check_min_max(ctx, vol)
    assert (lo, hi) == (-40, 64)


@pytest.mark.parametrize("span", ["whole", "one_wave"])
def test_min_max_ties(ctx, span):
    """130 x 70 x 9 = 81,900 elements over many workgroups: the extremes planted at the first, a middle and the last flat
    position (and, for one_wave, at neighbouring positions inside one wave's reach as well): first minimum, last maximum."""
    rng = np.random.default_rng(2)
    vol = rng.uniform(1.0, 2.0, (9, 70, 130)).astype(F)
    flat = vol.reshape(-1)
    n = flat.size
    spots = [0, n // 2 + 3, n - 1] if span == "whole" else [40001, 40002, 40005, 40063, 40130]
    other = [7, n // 3, n - 2] if span == "whole" else [40003, 40004, 40064, 40200]
    flat[spots] = F(-5.0)
    flat[other] = F(9.0)
    lo, hi, lp, hp = check_min_max(ctx, vol)
    assert (lo, hi, lp, hp) == (-5.0, 9.0, min(spots), max(other))
    flat[other] = F(-5.0)                                              # swapped roles at the same places
    flat[spots] = F(9.0)
    lo, hi, lp, hp = check_min_max(ctx, vol)
    assert (lp, hp) == (min(other), max(spots))


def test_min_max_equal_zero_signs_negative(ctx):
    n = 130 * 70 * 9
    lo, hi, lp, hp = check_min_max(ctx, np.full((9, 70, 130), 2.5, F))
    assert (lp, hp) == (0, n - 1)
    z = np.zeros(n, F)
    z[1::2] = -0.0                                                     # +0 first, -0 last: min is +0, max is -0
    lo, hi, lp, hp = check_min_max(ctx, z.reshape(9, 70, 130))
    assert (lp, hp) == (0, n - 1) and not np.signbit(lo) and np.signbit(hi)
    lo, hi, lp, hp = check_min_max(ctx, (-z).reshape(9, 70, 130))
    assert np.signbit(lo) and not np.signbit(hi)
    rng = np.random.default_rng(3)
    lo, hi, lp, hp = check_min_max(ctx, -rng.uniform(1.0, 1e30, (3, 5, 7)).astype(F))
    assert hi < 0
    lo, hi, lp, hp = check_min_max(ctx, np.array([-np.inf, 3, np.inf, np.inf, -np.inf], F).reshape(1, 1, 5))
    assert (lp, hp) == (0, 3)


def test_min_max_of_a_dsi(ctx, dsi):
    g, vol = dsi
    lo, hi, lp, hp = g.getMinMax()
    assert (lo, hi, lp, hp) == gr.min_max(vol) and lo == 0 and hi > 0
    nan = vol[:2].copy()
    nan[1, 5, 5] = np.nan                                              # unspecified result, but a status and no fault
    gn = grid_of(ctx, nan)
    gn.getMinMax()
    gn.close()


# ----------------------------------------------------------------------------------------------------- slices
@pytest.mark.parametrize("shape", [(3, 5, 7), (9, 33, 70)])
def test_get_slice(ctx, shape):
    rng = np.random.default_rng(4)
    vol = rng.uniform(-3, 3, shape).astype(F)
    nz, ny, nx = shape
    g = grid_of(ctx, vol)
    for dim, size in ((0, nx), (1, ny), (2, nz)):
        for i in range(size):
            got = g.getSlice(i, dim)
            assert got.dtype == F and np.array_equal(got, gr.get_slice(vol, i, dim)), (dim, i)
        assert code_of(lambda: g.getSlice(size, dim)) == engine.ERR_INVALID
    assert code_of(lambda: g.getSlice(0, 3)) == engine.ERR_INVALID
    assert code_of(lambda: g.getSlice(-1, 0)) == engine.ERR_INVALID
    L = d.load_library()
    buf = (ctypes.c_float * (nx * ny * nz))()
    assert L.dsi_grid_get_slice(g._h, 0, 3, buf) == engine.ERR_INVALID
    assert L.dsi_grid_get_slice(g._h, nx, 0, buf) == engine.ERR_INVALID
    assert L.dsi_grid_get_slice(g._h, 0, 0, None) == engine.ERR_INVALID
    g.close()


def check_slices_u8(ctx, vol, g=None):
    own = g is None
    g = grid_of(ctx, vol) if own else g
    for dim in range(3):
        for by_minmax in (True, False):
            got = g.slicesU8(dim, by_minmax)
            want = gr.slices_u8(vol, dim, by_minmax)
            assert got.shape == want.shape and got.dtype == np.uint8
            bad = np.argwhere(got != want)
            assert bad.shape[0] == 0, (vol.shape, dim, by_minmax, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    if own:
        g.close()


# one past and one short of the 64-wide tile on each axis; dimZ a multiple of 4 (packed stores) and not (byte stores)
@pytest.mark.parametrize("shape", [(3, 5, 7), (63, 64, 65), (64, 65, 63), (9, 70, 130), (100, 3, 66)])
def test_slices_u8_shapes(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    vol = rng.uniform(0.0, 50.0, shape).astype(F)
    vol[rng.random(shape) < 0.2] = 0.0
    check_slices_u8(ctx, vol)


def test_slices_u8_of_a_dsi(ctx, dsi):
    g, vol = dsi
    check_slices_u8(ctx, vol, g)


def test_slices_u8_constant_negative_inf(ctx):
    rng = np.random.default_rng(6)
    const = np.full((8, 6, 70), 3.25, F)
    g = grid_of(ctx, const)
    for dim in range(3):
        assert not g.slicesU8(dim, True).any() and not g.slicesU8(dim, False).any()
    g.close()
    check_slices_u8(ctx, const)
    neg = rng.uniform(-20.0, 5.0, (8, 6, 70)).astype(F)
    neg[3] = -7.5                                                      # a constant slice among the others
    check_slices_u8(ctx, neg)
    inf = rng.uniform(0.0, 5.0, (8, 6, 70)).astype(F)
    inf[2, 3, 40] = np.inf
    check_slices_u8(ctx, inf)
    halves = (np.arange(8 * 6 * 70) % 511).astype(F).reshape(8, 6, 70)  # (v - 0) / 510 * 255 = v / 2: ties to even
    halves[0, 0, 0], halves[7, 5, 69] = 0, 510
    check_slices_u8(ctx, halves)
    assert code_of(lambda: grid_of(ctx, const).slicesU8(3)) == engine.ERR_INVALID


def test_slices_u8_dev_matches_host_form(ctx):
    """The device-output forms, written into the memory of a second grid (zeroed when created)."""
    rng = np.random.default_rng(7)
    vol = rng.uniform(0.0, 9.0, (12, 10, 70)).astype(F)
    g = grid_of(ctx, vol)
    out = d.Grid3D(ctx, 70, 10, 12)                                    # 4 bytes per voxel: room for the images and more
    L = d.load_library()
    for dim in range(3):
        engine._check(L.dsi_grid_slices_u8_dev(g._h, dim, 0, ctypes.c_void_p(out.device_ptr)))
        ctx.synchronize()
        got = out.download().view(np.uint8).ravel()
        assert np.array_equal(got[:vol.size], gr.slices_u8(vol, dim, False).ravel())
        assert not got[vol.size:].any()                                # nothing behind the last image
    assert L.dsi_grid_slices_u8_dev(g._h, 0, 1, ctypes.c_void_p(out.device_ptr + 1)) == engine.ERR_INVALID
    assert L.dsi_grid_slices_u8_dev(g._h, 3, 1, ctypes.c_void_p(out.device_ptr)) == engine.ERR_INVALID
    out.resetGrid()
    engine._check(L.dsi_grid_get_slice_dev(g._h, 69, 0, ctypes.c_void_p(out.device_ptr)))
    ctx.synchronize()
    got = out.download().ravel()
    assert np.array_equal(got[:120].reshape(10, 12), gr.get_slice(vol, 69, 0)) and not got[120:].any()
    g.close()
    out.close()


# ------------------------------------------------------------------------------- accumulateZSliceAt, accessors
def test_accumulate_z_slice(ctx):
    rng = np.random.default_rng(8)
    vol = rng.uniform(0, 4, (5, 9, 70)).astype(F)
    g = grid_of(ctx, vol)
    full = rng.uniform(0, 1, (9, 70)).astype(F)
    g.accumulateZSliceAt(2, full)
    want = gr.accumulate_z_slice(vol, 2, full)
    assert gr.same_bits(g.download(), want).all()
    small = rng.uniform(0, 1, (4, 33)).astype(F)
    g.accumulateZSliceAt(4, small)
    want = gr.accumulate_z_slice(want, 4, small)
    got = g.download()
    assert gr.same_bits(got, want).all()
    assert np.array_equal(got[[0, 1, 3]], vol[[0, 1, 3]]) and np.array_equal(got[4, 4:], vol[4, 4:])
    assert np.array_equal(got[4, :, 33:], vol[4, :, 33:])
    g.accumulateZSliceAt(0, np.zeros((0, 5), F))                       # an empty image: nothing happens
    for iz, img in ((5, full), (0, np.zeros((10, 70), F)), (0, np.zeros((9, 71), F))):
        assert code_of(lambda: g.accumulateZSliceAt(iz, img)) == engine.ERR_INVALID
    assert code_of(lambda: g.accumulateZSliceAt(-1, full)) == engine.ERR_INVALID
    assert gr.same_bits(g.download(), want).all()
    g.close()


def test_single_voxel_accessors(ctx):
    rng = np.random.default_rng(9)
    vol = rng.uniform(0, 4, (3, 5, 7)).astype(F)
    g = grid_of(ctx, vol)
    p = 4 + 7 * (2 + 5 * 1)
    assert g.getGridValueAt(p) == vol[1, 2, 4] == g.getGridValueAt(4, 2, 1)
    g.setGridValueAt(p, 0.1)
    g.accumulateGridValueAt(p, 0.2)
    assert g.getGridValueAt(p) == F(F(0.1) + F(0.2))
    vol[1, 2, 4] = F(F(0.1) + F(0.2))
    g.setGridValueAt(104, -1.0)
    vol[2, 4, 6] = -1.0
    assert np.array_equal(g.download(), vol)
    for fn in (lambda: g.getGridValueAt(105), lambda: g.setGridValueAt(105, 1.0), lambda: g.accumulateGridValueAt(105, 1.0),
               lambda: g.getGridValueAt(7, 0, 0), lambda: g.getGridValueAt(0, 5, 0), lambda: g.getGridValueAt(0, 0, 3),
               lambda: g.getGridValueAt(-1)):
        assert code_of(fn) == engine.ERR_INVALID
    assert np.array_equal(g.download(), vol)
    g.close()


# ------------------------------------------------------------------------------------------------ imwriteSlices
def test_imwrite_slices_python(ctx, tmp_path):
    rng = np.random.default_rng(10)
    vol = rng.uniform(0, 4, (11, 6, 9)).astype(F)
    g = grid_of(ctx, vol)
    for dim, size in ((0, 9), (1, 6), (2, 11)):
        for by_minmax in (True, False):
            sub = tmp_path / ("d%d_%d" % (dim, by_minmax))
            sub.mkdir()
            names = g.imwriteSlices(str(sub / "slice_"), dim, by_minmax)
            assert sorted(os.listdir(str(sub))) == ["slice_%03d.png" % i for i in range(size)]
            assert names == [str(sub / ("slice_%03d.png" % i)) for i in range(size)]
            u = g.slicesU8(dim, by_minmax)
            for i, nm in enumerate(names):
                assert np.array_equal(gr.decode_png_gray8(open(nm, "rb").read()), u[i])
    g.close()


def test_cpp_call_sites(built, ctx, tmp_path):
    exe = str(tmp_path / "test_grid3d")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_grid3d.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    nx, ny, nz = 37, 21, 12
    vol = np.fromfile(str(out / "vol.f32"), F).reshape(nz, ny, nx)
    for dim, (prefix, size) in enumerate((("x_", nx), ("y_", ny), ("z_", nz))):
        want = gr.slices_u8(vol, dim, True)
        u = np.fromfile(str(out / ("u8_%d.bin" % dim)), np.uint8).reshape(want.shape)
        assert np.array_equal(u, want)
        files = sorted(glob.glob(str(out / (prefix + "*.png"))))
        assert [os.path.basename(f) for f in files] == ["%s%03d.png" % (prefix, i) for i in range(size)]
        for i, f in enumerate(files):
            assert np.array_equal(gr.decode_png_gray8(open(f, "rb").read()), want[i])
    want = gr.slices_u8(vol, 1, False)
    assert np.array_equal(np.fromfile(str(out / "u8_1_per_slice.bin"), np.uint8).reshape(want.shape), want)
    files = sorted(glob.glob(str(out / "w_*.png")))
    assert len(files) == ny
    for i, f in enumerate(files):
        assert np.array_equal(gr.decode_png_gray8(open(f, "rb").read()), want[i])
