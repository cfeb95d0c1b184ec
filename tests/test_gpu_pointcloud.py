"""MapperEMVS::getPointcloud (mapper_emvs_stereo.cpp:440-480) on the MI355X against the restatement of
tests/pointcloud_reference.py: the back-projection bit for bit and in pixel order, the radius filter's keep-set exactly
(on the configs[1] scene and on adversarial geometry), the device-resident form, the window stream at configs[2] size,
the C++ call sites and the argument checks."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import pointcloud_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def configs1(ctx):
    """BASELINE configs[1]: stereo, 10 M events per camera, 346 x 260 x 100, harmonic fusion; the filtered maps of
    getDepthMapFromDSI(..., OptionsDepthMap()) (main.cpp:281)."""
    rig = syn.stereo_rig(10_000_000, seed=1234)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 100, 4.0, 200.0, 0.0)
    ms = []
    for c in range(2):
        m = d.MapperEMVS(ctx, cam, shape)
        assert m.evaluateDSI(rig["events"][c], rig["trajectories"][c], rig["T_rv_w"])
        ms.append(m)
    fused = d.Grid3D(ctx, *ms[0].dsi_.getDimensions())
    fused.setToFusionOf(ms[0].dsi_, ms[1].dsi_, d.FUSE_HM)
    out = d.MapperEMVS(ctx, cam, shape)
    depth, conf, mask = out.getDepthMapFromDSI(fused, d.OptionsDepthMap())
    pts = ref.backproject(depth, mask, *out.virtual_cam_)
    yield dict(cam=cam, shape=shape, fused=fused, mapper=out, depth=depth, mask=mask, pts=pts)
    for o in ms + [out, fused]:
        o.close()


def test_backprojection_bit_equal_configs1(configs1):
    s = configs1
    m = s["mapper"]
    got = m.getPointcloud(s["depth"], s["mask"], d.OptionsPointCloud(0.05, 0))   # k = 0: every finite point stays
    assert m.n_unfiltered_ == len(s["pts"]) == int((s["mask"] > 0).sum()) > 1000
    assert bits_equal(got, s["pts"])


def test_backprojection_bit_equal_hand_made(configs1):
    m = configs1["mapper"]
    ny, nx = configs1["depth"].shape
    rng = np.random.default_rng(11)
    dm = rng.uniform(-50.0, 200.0, (ny, nx)).astype(np.float32)
    dm[rng.random((ny, nx)) < 0.05] = 0.0
    dm[rng.random((ny, nx)) < 0.02] = -0.0
    big = rng.random((ny, nx)) < 0.03
    dm[big] = np.float32(1e30) * np.sign(rng.random(big.sum()) - 0.5).astype(np.float32)
    dm[0, 0], dm[0, -1], dm[-1, 0], dm[-1, -1] = 0.0, -3.0, 1e35, 1e-30
    mk = (rng.random((ny, nx)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (ny, nx)).astype(np.uint8)
    mk[0, 0] = mk[0, -1] = mk[-1, 0] = mk[-1, -1] = 1
    dm[mk == 0] = np.nan                      # unmasked pixels are never read
    want = ref.backproject(dm, mk, *m.virtual_cam_)
    got = m.getPointcloud(dm, mk, d.OptionsPointCloud(0.05, 0))
    assert m.n_unfiltered_ == len(want) == int((mk > 0).sum())
    keep = ref.keep_kdtree(want, 0.05, 0)
    assert keep.all()
    assert bits_equal(got, want)
    assert bits_equal(got[0], want[0]) and got[0, 2] == 0.0 and np.isinf(got[0, 3])   # corner (0, 0): depth 0


@pytest.mark.parametrize("radius", [0.05, 0.5, 2.0])
def test_keep_set_configs1(configs1, radius):
    s = configs1
    m = s["mapper"]
    cnt = ref.counts_kdtree(s["pts"], radius)
    for k in (0, 1, 3, 10):
        got = m.getPointcloud(s["depth"], s["mask"], d.OptionsPointCloud(radius, k))
        keep = cnt >= k + 1
        print("configs[1] radius %.2f min_neighbors %2d: %d of %d points kept" % (radius, k, keep.sum(), len(keep)))
        assert bits_equal(got, s["pts"][keep]), (radius, k)
    if radius == 2.0:
        assert 0 < (cnt >= 4).sum() < len(cnt)       # a real mix


def _check_filter(ctx, xyz, r, k):
    want = ref.keep_bruteforce(xyz, r, k)
    got = d.radius_outlier_removal(ctx, xyz, r, k)
    assert np.array_equal(got, want), (r, k, int(got.sum()), int(want.sum()))
    if len(xyz):      # stride 4: the fourth float is not a coordinate
        x4 = np.concatenate([np.asarray(xyz, np.float32)[:, :3], np.full((len(xyz), 1), np.nan, np.float32)], axis=1)
        assert np.array_equal(d.radius_outlier_removal(ctx, x4, r, k), want)
    return want


def test_filter_on_lattices_at_the_radius(ctx):
    r32 = np.float32(0.25)
    for offset in ((0.0, 0.0, 0.0), (3.0, -7.5, 100.0), (-1000.0, 0.5, 2.0)):
        base = ref.lattice(8, 0.25, offset)
        for xyz in (base, ref.perturb_ulps(base, 0.3, 5), ref.perturb_ulps(base, 0.05, 6)):
            for r in (r32, np.nextafter(r32, np.float32(0)), np.nextafter(r32, np.float32(1))):
                for k in (1, 3, 6):
                    _check_filter(ctx, xyz, r, k)
    base = ref.lattice(8, 0.25)
    assert d.radius_outlier_removal(ctx, base, r32, 6).sum() == 6 ** 3     # d2 == r^2 exactly is within


def test_filter_on_duplicates_one_cell_and_collisions(ctx):
    rng = np.random.default_rng(4)
    dup = np.repeat(rng.normal(0, 1, (10, 3)).astype(np.float32), 50, axis=0)
    xyz = np.concatenate([dup, rng.normal(0, 1, (500, 3)).astype(np.float32)])
    xyz = xyz[rng.permutation(len(xyz))]
    for k in (0, 5, 49, 50, 100):
        _check_filter(ctx, xyz, 0.01, k)
    box = rng.uniform(0, 1, (1500, 3)).astype(np.float32)          # r larger than the cloud: all in one cell
    for k in (0, 3, 1499, 1500):
        kept = _check_filter(ctx, box, 10.0, k)
        assert kept.all() == (k < 1500)
    coll, n_cells = ref.colliding_cloud(1.0, 3000, seed=9)
    assert n_cells >= 20
    for k in (0, 2, 5, 20):
        _check_filter(ctx, coll, 1.0, k)
    odd = rng.normal(0, 1, (2000, 3)).astype(np.float32)
    odd[:10] = np.nan
    odd[10:20] = np.inf
    odd[20:30] = np.float32(3e38)
    odd[30:40] = -np.float32(3e38)
    for k in (0, 3):
        kept = _check_filter(ctx, odd, 0.3, k)
        assert not kept[:20].any()


@pytest.mark.parametrize("k", [0, 3])
def test_filter_small_n(ctx, k):
    rng = np.random.default_rng(k)
    for n in sorted({0, 1, k, k + 1}):
        for xyz in (np.zeros((n, 3), np.float32), rng.normal(0, 0.01, (n, 3)).astype(np.float32)):
            _check_filter(ctx, xyz, 0.05, k)
    assert d.radius_outlier_removal(ctx, np.zeros((k + 1, 3), np.float32), 0.05, k).all()
    assert not d.radius_outlier_removal(ctx, np.zeros((k, 3), np.float32), 0.05, k).any()


def test_filter_million_points_against_kdtree(ctx):
    n = 1_048_576                                   # configs[4]'s pixel count
    rng = np.random.default_rng(2024)
    xyz = rng.uniform(0, 5.0, (n, 3)).astype(np.float32)   # ~4 neighbours within 0.05 on average
    xyz[: n // 8] = xyz[n // 8: n // 4] + rng.normal(0, 0.01, (n // 8, 3)).astype(np.float32)
    got = d.radius_outlier_removal(ctx, xyz, 0.05, 3)
    t0 = time.perf_counter()
    for _ in range(3):
        d.radius_outlier_removal(ctx, xyz, 0.05, 3)
    ms = (time.perf_counter() - t0) / 3 * 1e3
    want = ref.keep_kdtree(xyz, 0.05, 3)
    print("1,048,576 points: %d kept; %.2f ms per call incl. upload and download" % (want.sum(), ms))
    assert 0.1 * n < want.sum() < 0.9 * n
    assert np.array_equal(got, want)


def test_device_resident_form(ctx, configs1):
    s = configs1
    m = d.MapperEMVS(ctx, s["cam"], s["shape"])
    opts = d.OptionsPointCloud(0.5, 3)
    with pytest.raises(d.DsiError) as e:
        m.getPointcloud(options_pc=opts)        # no filtered map yet
    assert e.value.code == E.ERR_INVALID and "filtered depth map" in str(e.value)
    depth, conf, mask = m.getDepthMapFromDSI(s["fused"], d.OptionsDepthMap())
    a = m.getPointcloud(options_pc=opts)
    b = m.getPointcloud(depth, mask, opts)
    assert len(a) > 0 and bits_equal(a, b)
    assert bits_equal(m.getPointcloud(options_pc=opts), a)       # the maps stay
    m.computeDepthMap(s["fused"])                                # a new (raw) depth map
    with pytest.raises(d.DsiError) as e:
        m.getPointcloud(options_pc=opts)
    assert e.value.code == E.ERR_INVALID
    m.filterDepthMap(d.OptionsDepthMap())
    assert bits_equal(m.getPointcloud(options_pc=opts), a)
    m.close()


def test_window_stream_configs2(ctx):
    n_win, ev_win, dur, t0 = 8, 250_000, 0.05, 10.0
    rig = syn.stereo_rig(n_win * ev_win, width=640, height=480, t0=t0, duration=n_win * dur, seed=77, n_points=6000)
    cam = rig["cam"]
    shape = d.ShapeDSI(512, 512, 200, 4.0, 200.0, 0.0)
    opts_dm, opts_pc = d.OptionsDepthMap(), d.OptionsPointCloud(0.5, 3)
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    on = list(proc.full_sequence(*args, options_depth_map=opts_dm, options_point_cloud=opts_pc))
    off = list(proc.full_sequence(*args, options_depth_map=opts_dm))
    assert len(on) == len(off) >= 8
    vm = d.MapperEMVS(ctx, cam, shape)
    vcam = vm.virtual_cam_
    vm.close()
    total = 0
    for a, b in zip(on, off):
        assert len(a) == 5 and len(b) == 4 and a[0] == b[0]
        for x, y in zip(a[1:4], b[1:4]):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        pts = ref.backproject(a[1], a[3], *vcam)
        keep = ref.keep_kdtree(pts, 0.5, 3)
        assert bits_equal(a[4], pts[keep])
        total += len(a[4])
        print("window ts %.3f: %d points, %d after the filter" % (a[0], len(pts), len(a[4])))
    assert total > 0
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, options_point_cloud=opts_pc))


def _read(path, dtype):
    return np.fromfile(path, dtype)


def test_cpp_call_sites(built, ctx, tmp_path):
    exe = str(tmp_path / "test_pointcloud")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_pointcloud.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    for mode in ("--cloud", "--stream"):
        r = subprocess.run([exe, mode, str(tmp_path)], capture_output=True, text=True, timeout=300)
        print(r.stdout)
        assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    # --cloud: the reference's spelling gives what the Python path and the restatement give
    cam = (346, 260, 173.0, 173.0, 173.0, 130.0)
    m = d.MapperEMVS(ctx, cam, d.ShapeDSI(0, 0, 100, 4.0, 200.0, 0.0))
    depth = _read(tmp_path / "depth.f32", np.float32).reshape(260, 346)
    mask = _read(tmp_path / "mask.u8", np.uint8).reshape(260, 346)
    cpp = _read(tmp_path / "cloud.f32", np.float32).reshape(-1, 4)
    py = m.getPointcloud(depth, mask, d.OptionsPointCloud(0.5, 3))
    pts = ref.backproject(depth, mask, *m.virtual_cam_)
    assert len(cpp) > 0 and bits_equal(cpp, py) and bits_equal(py, pts[ref.keep_kdtree(pts, 0.5, 3)])
    m.close()
    # --stream: every window's cloud is the restatement of that window's filtered maps
    m = d.MapperEMVS(ctx, (240, 180, 120.0, 120.0, 120.0, 90.0), d.ShapeDSI(0, 0, 64, 4.0, 100.0, 0.0))
    vcam = m.virtual_cam_
    m.close()
    windows = sorted(f for f in os.listdir(tmp_path) if f.endswith(".cloud.f32") and f.startswith("window_"))
    assert len(windows) >= 6
    for f in windows:
        base = str(tmp_path / f[: -len(".cloud.f32")])
        depth = _read(base + ".depth.f32", np.float32).reshape(180, 240)
        mask = _read(base + ".mask.u8", np.uint8).reshape(180, 240)
        pts = ref.backproject(depth, mask, *vcam)
        assert bits_equal(_read(base + ".cloud.f32", np.float32).reshape(-1, 4), pts[ref.keep_kdtree(pts, 1.0, 2)]), f


def test_argument_checks(ctx, configs1):
    s = configs1
    m = s["mapper"]
    xyz = np.zeros((10, 3), np.float32)

    def refused(fn, text):
        with pytest.raises(d.DsiError) as e:
            fn()
        assert e.value.code == E.ERR_INVALID and text in str(e.value), str(e.value)

    for r in (0.0, -1.0, np.nan, np.inf):
        refused(lambda: d.radius_outlier_removal(ctx, xyz, r, 3), "radius_search")
        refused(lambda: m.getPointcloud(s["depth"], s["mask"], d.OptionsPointCloud(r, 3)), "radius_search")
    refused(lambda: d.radius_outlier_removal(ctx, xyz, 0.05, -1), "min_num_neighbors")
    refused(lambda: m.getPointcloud(s["depth"], s["mask"], d.OptionsPointCloud(0.05, -1)), "min_num_neighbors")
    L = d.load_library()
    keep = np.zeros(10, np.uint8)
    assert L.dsi_radius_outlier_removal(ctx._h, E._ptr(np.zeros((10, 5), np.float32), C.c_float), 5, 10, C.c_float(0.1), 3,
                                        E._ptr(keep, C.c_uint8)) == E.ERR_INVALID
    assert b"stride" in L.dsi_last_error()
    ys, xs = np.nonzero(s["mask"])
    for bad in (np.nan, np.inf, -np.inf):
        dm = s["depth"].copy()
        dm[ys[5], xs[5]] = bad
        refused(lambda: m.getPointcloud(dm, s["mask"], d.OptionsPointCloud()), "non-finite depth")
    dm = s["depth"].copy()
    dm[s["mask"] == 0] = np.nan                                  # unmasked pixels may hold anything
    m.getPointcloud(dm, s["mask"], d.OptionsPointCloud())
    # capacity too small: nothing written, the size needed reported
    opts = E._PointCloudOptions(0.5, 0)
    n, n0 = C.c_size_t(), C.c_size_t()
    out = np.full((4, 4), 7.0, np.float32)
    dep, msk = np.ascontiguousarray(s["depth"]), np.ascontiguousarray(s["mask"])
    rc = L.dsi_mapper_get_pointcloud(m._h, E._ptr(dep, C.c_float), E._ptr(msk, C.c_uint8), C.byref(opts),
                                     E._ptr(out, C.c_float), 1, C.byref(n), C.byref(n0))
    assert rc == E.ERR_INVALID and b"capacity" in L.dsi_last_error()
    assert n.value == len(s["pts"]) and (out == 7.0).all()
    # one map without the other
    rc = L.dsi_mapper_get_pointcloud(m._h, E._ptr(dep, C.c_float), None, C.byref(opts), E._ptr(out, C.c_float), 4,
                                     C.byref(n), None)
    assert rc == E.ERR_INVALID and b"both" in L.dsi_last_error()
    # a plane shard holds no whole arg-max
    shard = d.MapperEMVS(ctx, s["cam"], s["shape"], plane_range=(0, 50))
    refused(lambda: shard.getPointcloud(s["depth"], s["mask"]), "plane-sharded")
    shard.close()
