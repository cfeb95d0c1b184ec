"""The world map (dsi_map_*, engine.WorldMap) on the MI355X against the numpy restatement of
tests/world_map_reference.py: every comparison is array_equal on keys, n, windows and the float bits of xyz."""
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def random_pose(rng, scale=3.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return E.pose_matrix(np.concatenate([rng.uniform(-scale, scale, 3), q]))


def both(ctx, leaf, calls, capacity_log2=16):
    """the calls through a WorldMap and through the restatement: (map, reference map); the rejected counts agree"""
    wm, rm = d.WorldMap(ctx, leaf, capacity_log2), ref.ReferenceMap(leaf)
    for pts, T in calls:
        assert wm.integrate(pts, T) == rm.integrate(pts, T)
    return wm, rm


def test_random_clouds(ctx):
    rng = np.random.default_rng(1)
    calls = [(rng.uniform(-2, 2, (5000 + 37 * k, 3 + (k & 1))).astype(np.float32), random_pose(rng)) for k in range(3)]
    wm, rm = both(ctx, 0.05, calls)
    got, want = wm.extract(), rm.extract()
    assert len(want["keys"]) > 10000 and want["n"].max() > 1
    ref.assert_maps_equal(got, want)
    for mp, mw in ((2, 1), (1, 2), (2, 2), (0, 0), (1, 4)):
        ref.assert_maps_equal(wm.extract(mp, mw), rm.extract(mp, mw))
        assert wm.count(mp, mw) == len(rm.extract(mp, mw)["keys"])
    i = wm.info()
    assert (i["occupied"], i["calls"], i["accepted"], i["rejected"]) == (len(want["keys"]), 3, rm.accepted, 0)
    assert i["leaf"] == 0.05 and i["capacity"] >= 1 << 16
    # the table's order is stable while the map is unchanged, and sorting it gives the sorted extraction
    a, b = wm.extract(sort=False), wm.extract(sort=False)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(np.sort(a["keys"]), got["keys"])
    wm.close()


def test_order_and_split_freedom(ctx):
    rng = np.random.default_rng(2)
    T = random_pose(rng)
    pts = rng.uniform(-1.5, 1.5, (15000, 3)).astype(np.float32)
    pts[rng.integers(0, 15000, 4000)] = pts[rng.integers(0, 15000, 4000)]       # cells with many points
    one, one_ref = both(ctx, 0.05, [(pts, T)])
    cuts = [0, 1, 500, 501, 4000, 9000, 9003, 15000]
    shuffled = pts[rng.permutation(15000)]
    seven, seven_ref = both(ctx, 0.05, [(shuffled[a:b], T) for a, b in zip(cuts[:-1], cuts[1:])], capacity_log2=12)
    a, b = one.extract(), seven.extract()
    for k in ("keys", "n"):
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(a["xyz"].view(np.uint32), b["xyz"].view(np.uint32))
    ref.assert_maps_equal(a, one_ref.extract())
    ref.assert_maps_equal(b, seven_ref.extract())
    assert a["windows"].max() == 1 and b["windows"].max() > 2
    assert seven.info()["calls"] == 7 and seven.info()["growths"] >= 1
    one.close()
    seven.close()


def test_growth_from_the_smallest_table(ctx):
    # 20,000 distinct cells over two calls into 2^8 slots: the table doubles at least six times; 150 cells in the first
    # 256 slots collide by pigeonhole long before that
    n = 20000
    idx = np.arange(n)
    cells = np.stack([idx % 40 - 20, (idx // 40) % 40 - 20, idx // 1600 - 6], axis=1)
    rng = np.random.default_rng(3)
    pts = ((cells + rng.uniform(0.1, 0.9, (n, 3))) * 0.5).astype(np.float32)
    pts = pts[rng.permutation(n)]
    wm, rm = both(ctx, 0.5, [(pts[:10000], IDENTITY), (pts[10000:], IDENTITY)], capacity_log2=8)
    want = rm.extract()
    assert len(want["keys"]) == n
    ref.assert_maps_equal(wm.extract(), want)
    i = wm.info()
    assert i["growths"] >= 6 and i["rejected"] == 0 and i["occupied"] == n and i["accepted"] == n
    assert i["capacity"] == 1 << (8 + i["growths"]) and 4 * n <= 3 * i["capacity"]
    wm.close()
    # 150 cells in 256 slots: no growth (150 <= 192), probing must resolve the collisions
    wm, rm = both(ctx, 0.5, [(pts[:150], IDENTITY)], capacity_log2=8)
    assert wm.info()["growths"] == 0 and wm.info()["capacity"] == 256
    ref.assert_maps_equal(wm.extract(), rm.extract())
    wm.close()


def test_contention_on_one_cell(ctx):
    p = np.float32([0.3337, -1.2345, 2.5])
    pts = np.tile(p, (70000, 1))
    wm, rm = both(ctx, 0.05, [(pts, IDENTITY)])
    got = wm.extract()
    ref.assert_maps_equal(got, rm.extract())
    assert len(got["keys"]) == 1 and got["n"][0] == 70000 and got["windows"][0] == 1
    # the centroid is the point's own quantised position: (c + floor(f 2^32) 2^-32) leaf
    ok, c, F = ref.cells(p[None], IDENTITY, 0.05)
    own = ((c[0].astype(np.float64) + F[0].astype(np.float64) * 2.0 ** -32) * 0.05).astype(np.float32)
    assert np.array_equal(got["xyz"][0], own) and np.abs(own - p).max() <= np.spacing(np.float32(2.5))
    wm.close()


def test_adversarial_points_empty_call_reset_and_capacity(ctx):
    leaf = 0.125
    k = np.arange(-9, 10, dtype=np.float32) * np.float32(leaf)
    faces = np.stack(np.meshgrid(k, k[:5], k[:3], indexing="ij"), axis=-1).reshape(-1, 3)
    up = np.nextafter(faces, np.float32(np.inf))
    down = np.nextafter(faces, np.float32(-np.inf))              # (around 0: the denormals, and f = 1 below it)
    edge = np.float32((2 ** 20 - 2) * leaf)
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan], [3e38, 3e38, 3e38],
                        [edge, 0, 0], [edge + np.float32(leaf), 0, 0], [-edge, -edge, -edge], [-edge - np.float32(leaf), 0, 0],
                        [-0.0, -0.0, -0.0], [1e-45, -1e-45, 0]], np.float32)
    rng = np.random.default_rng(4)
    pts = np.concatenate([faces, up, down, special])
    pts = pts[rng.permutation(len(pts))]
    wm, rm = d.WorldMap(ctx, leaf, 10), ref.ReferenceMap(leaf)
    rej = wm.integrate(pts, IDENTITY)
    assert rej == rm.integrate(pts, IDENTITY) == 7
    ref.assert_maps_equal(wm.extract(), rm.extract())
    # a pose that makes finite points non-finite, and one that moves them out of range
    big = IDENTITY.copy()
    big[3] = 1e308
    big[0] = 1e300
    far = IDENTITY.copy()
    far[7] = 2.0 ** 20 * leaf
    for T in (big, far):
        assert wm.integrate(pts, T) == rm.integrate(pts, T) > 0
    # an empty call is a call
    assert wm.integrate(np.zeros((0, 3), np.float32), IDENTITY) == rm.integrate(np.zeros((0, 3), np.float32), IDENTITY) == 0
    got, want = wm.extract(), rm.extract()
    ref.assert_maps_equal(got, want)
    i = wm.info()
    assert (i["calls"], i["accepted"], i["rejected"]) == (4, rm.accepted, rm.rejected) and got["windows"].max() <= 3
    # too small a capacity: the size needed comes back, nothing is written
    L = d.load_library()
    m = len(want["keys"])
    xyz = np.full((m, 3), -7.0, np.float32)
    keys = np.full(m, 99, np.uint64)
    n = C.c_size_t()
    rc = L.dsi_map_extract(wm._h, 1, 1, xyz.ctypes.data_as(C.POINTER(C.c_float)), None, None,
                           keys.ctypes.data_as(C.POINTER(C.c_uint64)), m - 1, C.byref(n))
    assert rc == E.ERR_INVALID and n.value == m and (xyz == -7.0).all() and (keys == 99).all()
    rc = L.dsi_map_extract(wm._h, 1, 1, None, None, None, keys.ctypes.data_as(C.POINTER(C.c_uint64)), m, C.byref(n))
    assert rc == E.OK and np.array_equal(np.sort(keys), want["keys"])                # any output may be NULL
    # reset: an empty map that works again
    wm.reset()
    rm.reset()
    i = wm.info()
    assert (i["occupied"], i["calls"], i["accepted"], i["rejected"], i["growths"]) == (0, 0, 0, 0, 0)
    assert wm.count(0, 0) == 0 and len(wm.extract()["keys"]) == 0
    assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY)
    ref.assert_maps_equal(wm.extract(), rm.extract())
    with pytest.raises(d.DsiError):
        d.WorldMap(ctx, 0.0)
    with pytest.raises(d.DsiError):
        d.WorldMap(ctx, 0.05, 28)
    wm.close()


def test_first_principles_scene_seen_from_three_poses(ctx):
    """No restatement: scene points at cell centres, seen from three poses, each call with noise of its own.  A cell
    seen in two windows holds a scene point; single-window cells are mostly noise."""
    rng = np.random.default_rng(8)
    leaf = 0.1
    scene_cells = np.unique(rng.integers(-30, 30, (400, 3)), axis=0)
    scene = (scene_cells + 0.5) * leaf                            # cell centres: the round trip's 1e-7 cannot leave the cell
    wm = d.WorldMap(ctx, leaf, 12)
    for k in range(3):
        T_w_rv = random_pose(rng, 1.0)
        R, t = T_w_rv.reshape(3, 4)[:, :3], T_w_rv.reshape(3, 4)[:, 3]
        local = (scene - t) @ R                                    # R^T (X - t) in the view
        # noise on a lattice of its own per call (offsets 1000 k cells apart): no two calls share a noise cell
        noise = (rng.integers(0, 200, (300, 3)) + 0.5) * leaf + 1000.0 * (k + 1) * leaf
        noise_local = (noise - t) @ R
        assert wm.integrate(np.concatenate([local, noise_local]).astype(np.float32), T_w_rv) == 0
    twice = wm.extract(min_windows=2)
    once = wm.extract(min_windows=1)
    assert len(once["keys"]) > len(twice["keys"]) == len(scene_cells)
    assert np.array_equal(np.unique(ref.unpack_key(twice["keys"]), axis=0), scene_cells)
    assert (twice["windows"] == 3).all() and (twice["n"] == 3).all()
    assert np.abs(twice["xyz"] - (ref.unpack_key(twice["keys"]) + 0.5) * leaf).max() < 1e-4
    wm.close()


def test_device_path_through_full_sequence(ctx):
    """full_sequence(..., world_map=) integrates each window's cloud where it lies; a second map fed with the clouds the
    stream returned, through the same poses, is the same map, and the per-window outputs do not change."""
    n_win, dur, t0 = 4, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    opts_dm, opts_pc = d.OptionsDepthMap(), d.OptionsPointCloud(2.0, 1)
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    wm = d.WorldMap(ctx, 0.5, 8)
    on = list(proc.full_sequence(*args, options_depth_map=opts_dm, options_point_cloud=opts_pc, world_map=wm))
    off = list(proc.full_sequence(*args, options_depth_map=opts_dm, options_point_cloud=opts_pc))
    assert len(on) == len(off) == n_win
    host, rm = d.WorldMap(ctx, 0.5, 16), ref.ReferenceMap(0.5)
    for a, b in zip(on, off):
        assert len(a) == len(b) == 5 and a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        T_w_rv = d.invert_pose(proc.reference_view_process1(rig["trajectories"][0], a[0]))
        assert host.integrate(a[4], T_w_rv) == rm.integrate(a[4], T_w_rv)
    got = wm.extract()
    print("windows' clouds:", [len(a[4]) for a in on], "cells:", len(got["keys"]), wm.info())
    assert len(got["keys"]) > 20 and wm.info()["calls"] == n_win and wm.info()["accepted"] == sum(len(a[4]) for a in on)
    ref.assert_maps_equal(got, host.extract())
    ref.assert_maps_equal(got, rm.extract())
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, options_depth_map=opts_dm, world_map=wm))
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, options_depth_map=opts_dm, options_point_cloud=opts_pc, world_map=wm, concurrent=True))
    # Alg. 2 windows: the time_camera output's cloud, against T_rv_w = T_w_l(ts)^-1
    wm.reset()
    host.reset()
    for w in proc.full_sequence(*args, options_depth_map=opts_dm, options_point_cloud=opts_pc, world_map=wm, process_method=2):
        host.integrate(w[1][3], d.invert_pose(proc.reference_view_process2(rig["trajectories"][0], w[0])))
    assert wm.info()["calls"] == n_win and wm.info()["occupied"] > 0
    ref.assert_maps_equal(wm.extract(), host.extract())
    # a mapper of another context is refused
    other = d.Context(0)
    m = d.MapperEMVS(other, cam, shape)
    with pytest.raises(d.DsiError) as e:
        wm.integrate_mapper(m, IDENTITY, opts_pc)
    assert e.value.code == E.ERR_CONTEXT
    m.close()
    other.close()
    host.close()
    wm.close()
