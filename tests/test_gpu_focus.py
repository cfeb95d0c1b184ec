"""The focus-based collapses (Grid3D::collapseZSliceBy*, collapseMinZSlice, computeLocalFocusInPlace;
cartesian3dgrid.cpp:139-483) on the MI355X against the restatement of tests/focus_reference.py, bit for bit: a
configs[1]-sized DSI from evaluateDSI, random volumes, a 1024 x 1024 x 256 volume (checked on a strip), tiny and
adversarial shapes; getDepthMapFromDSI's method switch, fuseDSIs_HarmonicMeanOfLocalFocus (Python and C++) and the
argument checks."""
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import focus_reference as fr
from dvs_mcemvs_amd import process as proc, synthetic as syn
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(0, 1), (1, 1), (2, 0), (2, 1), (2, 2), (3, 1), (4, 1)]   # (method, half_patchsize)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def grid_of(ctx, vol):
    nz, ny, nx = vol.shape
    g = d.Grid3D(ctx, nx, ny, nz)
    g.upload(vol)
    return g


def check_all(ctx, vol, cases=CASES, local=True, strips=None, restated=None):
    """strips: row ranges the restatement is evaluated on (None: the whole map); restated: dict to keep the
    restated collapses in, by (method, half_patchsize)."""
    g = grid_of(ctx, vol)
    for method, h in cases:
        conf, idx = g._collapse_focus(method, h)
        for rows in strips or [None]:
            rc, ri = fr.collapse_focus(vol, method, h, rows=rows)
            sl = slice(None) if rows is None else slice(*rows)
            assert bits_equal(conf[sl], rc) and np.array_equal(idx[sl], ri), (vol.shape, method, h, rows)
            if restated is not None and rows is None:
                restated[(method, h)] = (rc, ri)
    v, i = g.collapseMinZSlice()
    rv, ri = fr.collapse_min_z(vol)
    assert bits_equal(v, rv) and np.array_equal(i, ri), vol.shape
    if local:
        nz, ny, nx = vol.shape
        for f in (0, 1):
            dst = d.Grid3D(ctx, nx, ny, nz)
            dst.setToLocalFocusOf(g, f)
            assert bits_equal(dst.download(), fr.local_focus(vol, f)), (vol.shape, f)
            dst.close()
        g.computeLocalFocusInPlace(0)                 # in place: the same volume
        assert bits_equal(g.download(), fr.local_focus(vol, 0))
    g.close()


@pytest.fixture(scope="module")
def configs1(ctx):
    """configs[1]'s shape: stereo, 346 x 260 x 100, harmonic fusion of two evaluateDSI volumes."""
    rig = syn.stereo_rig(2_000_000, seed=1234)
    shape = d.ShapeDSI(0, 0, 100, 4.0, 200.0, 0.0)
    ms = []
    for c in range(2):
        m = d.MapperEMVS(ctx, rig["cam"], shape)
        assert m.evaluateDSI(rig["events"][c], rig["trajectories"][c], rig["T_rv_w"])
        ms.append(m)
    fused = d.Grid3D(ctx, *ms[0].dsi_.getDimensions())
    fused.setToFusionOf(ms[0].dsi_, ms[1].dsi_, d.FUSE_HM)
    yield dict(rig=rig, shape=shape, mappers=ms, fused=fused, vol=fused.download(), restated={})
    for o in ms + [fused]:
        o.close()


def test_configs1_dsi(ctx, configs1):
    vol = configs1["vol"]
    assert vol.shape == (100, 260, 346) and (vol > 0).mean() > 0.05
    check_all(ctx, vol, restated=configs1["restated"])


def test_random_512(ctx):
    """512 x 512 x 200; the restatement on the top, a middle and the bottom strip (each the exact rows of the map)."""
    rng = np.random.default_rng(5)
    vol = rng.uniform(0.0, 10.0, (200, 512, 512)).astype(np.float32)
    vol[rng.random(vol.shape) < 0.3] = 0.0
    check_all(ctx, vol, local=False, strips=[(0, 20), (250, 270), (496, 512)])


def test_large_strip(ctx):
    """1024 x 1024 x 256 (u8 indices at their limit), DoG and LocalVar checked on a 64-row strip."""
    rng = np.random.default_rng(6)
    vol = rng.integers(0, 8, (256, 1024, 1024)).astype(np.float32)
    g = grid_of(ctx, vol)
    for method in (fr.DOG, fr.LOCAL_VAR):
        conf, idx = g._collapse_focus(method, 1)
        for rows in ((480, 544), (960, 1024)):
            rc, ri = fr.collapse_focus(vol, method, 1, rows=rows)
            assert bits_equal(conf[rows[0]: rows[1]], rc) and np.array_equal(idx[rows[0]: rows[1]], ri), (method, rows)
        assert idx.max() == 255 or (idx > 200).any()
    g.close()


@pytest.mark.parametrize("nx", [1, 2, 3, 5])
@pytest.mark.parametrize("ny", [1, 2, 3, 5, 70])
def test_tiny_shapes(ctx, nx, ny):
    rng = np.random.default_rng(nx * 100 + ny)
    for nz in (1, 256):
        vol = rng.uniform(-1.0, 3.0, (nz, ny, nx)).astype(np.float32)
        check_all(ctx, vol, local=(nz == 1))


def test_adversarial_planes(ctx):
    rng = np.random.default_rng(9)
    nz, ny, nx = 24, 37, 131
    vol = rng.uniform(0.0, 2.0, (nz, ny, nx)).astype(np.float32)
    vol[3] = vol[2]                                   # duplicated planes: the first one wins
    vol[10] = vol[2]
    vol[4] = 1.5                                      # constant slice: no gradient, no variance
    vol[5] = -0.0
    vol[6, ::2] = 0.0
    vol[6, 1::2] = -0.0
    vol[7] = rng.uniform(0, 1, (ny, nx)).astype(np.float32) * np.float32(1e-39)      # denormals
    vol[8] = rng.uniform(0, 1, (ny, nx)).astype(np.float32) * np.float32(3e-38)      # squares underflow
    vol[9] = np.float32(2e19) * (1 + rng.integers(0, 4, (ny, nx))).astype(np.float32)  # squares overflow
    vol[11, 5:9, 20:30] = np.inf
    vol[12, 15:19, 40:44] = np.nan
    vol[13, 30, 100] = -np.inf
    vol[14] = vol[2] * np.float32(-1)
    check_all(ctx, vol)


def test_argument_checks(ctx):
    vol = np.ones((257, 4, 4), np.float32)
    g = grid_of(ctx, vol)
    for fn in (lambda: g.collapseZSliceByDoG(), lambda: g.collapseMinZSlice()):
        with pytest.raises(d.DsiError) as e:
            fn()
        assert e.value.code == d.engine.ERR_INVALID
    g.close()
    g = grid_of(ctx, np.ones((5, 4, 4), np.float32))
    for method, h, code in ((5, 1, d.engine.ERR_BAD_OP), (-1, 1, d.engine.ERR_BAD_OP), (2, 9, d.engine.ERR_INVALID),
                            (2, -1, d.engine.ERR_INVALID)):
        with pytest.raises(d.DsiError) as e:
            g._collapse_focus(method, h)
        assert e.value.code == code, (method, h)
    g.close()


def test_get_depth_map_from_dsi_methods(ctx, configs1):
    s = configs1
    m = d.MapperEMVS(ctx, s["rig"]["cam"], s["shape"])
    opts = d.OptionsDepthMap()
    vol = s["vol"]
    for method in range(5):
        rc, ri = s["restated"].get((method, 1)) or fr.collapse_focus(vol, method, 1)
        want = orc.depth_map_filters(rc, ri, m.raw_depths_vec_, 5, 5.0, 5, 0.0)
        depth, conf, mask = m.getDepthMapFromDSI(s["fused"], opts, method=method)
        assert bits_equal(depth, want["depth"]) and bits_equal(conf, want["confidence"]), method
        assert np.array_equal(mask, want["mask"]), method
        raw_depth, raw_conf, raw_idx = m.getDepthMapFromDSI(s["fused"], method=method)   # without the filters
        assert bits_equal(raw_conf, rc) and np.array_equal(raw_idx, ri)
        assert bits_equal(raw_depth, m.raw_depths_vec_[ri])
    today = m.getDepthMapFromDSI(s["fused"], opts)
    for method in (-1, 7):
        got = m.getDepthMapFromDSI(s["fused"], opts, method=method)
        assert all(bits_equal(a, b) if a.dtype == np.float32 else np.array_equal(a, b) for a, b in zip(got, today))
    m.close()


def test_fuse_harmonic_mean_of_local_focus(ctx, configs1):
    s = configs1
    m0, m1 = s["mappers"]
    out = d.MapperEMVS(ctx, s["rig"]["cam"], s["shape"])
    v0, v1 = m0.dsi_.download(), m1.dsi_.download()
    for f in (0, 1):
        proc.fuseDSIs_HarmonicMeanOfLocalFocus(m0, m1, s["rig"]["cam"], s["rig"]["cam"], s["shape"], f, out)
        want = orc.fuse2(fr.local_focus(v0, f), fr.local_focus(v1, f), d.FUSE_HM)
        assert bits_equal(out.dsi_.download(), want), f
    assert bits_equal(m0.dsi_.download(), v0) and bits_equal(m1.dsi_.download(), v1)
    out.close()


def test_cpp_call_sites(built, ctx, tmp_path):
    exe = str(tmp_path / "test_focus")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_focus.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dt)
    nx, ny, nz = 96, 72, 40
    v0 = rd("dsi0.f32", np.float32).reshape(nz, ny, nx)
    v1 = rd("dsi1.f32", np.float32).reshape(nz, ny, nx)
    m = d.MapperEMVS(ctx, (96, 72, 48.0, 48.0, 48.0, 36.0), d.ShapeDSI(0, 0, nz, 4.0, 200.0, 0.0))
    rc, ri = fr.collapse_focus(v0, fr.LAPLACIAN, 1)
    want = orc.depth_map_filters(rc, ri, m.raw_depths_vec_, 5, 5.0, 5, 0.0)
    m.close()
    assert bits_equal(rd("method3.depth.f32", np.float32).reshape(ny, nx), want["depth"])
    assert bits_equal(rd("method3.conf.f32", np.float32).reshape(ny, nx), want["confidence"])
    assert np.array_equal(rd("method3.mask.u8", np.uint8).reshape(ny, nx), want["mask"])
    rc, ri = fr.collapse_focus(v0, fr.DOG, 1)
    assert bits_equal(rd("dog.conf.f32", np.float32).reshape(ny, nx), rc)
    assert np.array_equal(rd("dog.idx.u8", np.uint8).reshape(ny, nx), ri)
    rv, ri = fr.collapse_min_z(v0)
    assert bits_equal(rd("min.val.f32", np.float32).reshape(ny, nx), rv)
    assert np.array_equal(rd("min.idx.u8", np.uint8).reshape(ny, nx), ri)
    assert bits_equal(rd("lms.f32", np.float32).reshape(nz, ny, nx), fr.local_focus(v0, 1))
    want = orc.fuse2(fr.local_focus(v0, 0), fr.local_focus(v1, 0), d.FUSE_HM)
    assert bits_equal(rd("fused.f32", np.float32).reshape(nz, ny, nx), want)
