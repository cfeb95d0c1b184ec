"""Pruning the world map (dsx_map_prune*, engine.WorldMap.prune / classifyPrune / fetchPruneReasons; DESIGN.md 7j "Pruning")
on the MI355X against the numpy restatement of tests/map_prune_reference.py: every comparison is array_equal -- the map
through world_map_reference.assert_maps_equal, the verdicts as equal key and reason arrays, the counts as integers."""
import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_prune_reference as pref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = pref.IDENTITY
COUNTERS = ("calls", "accepted", "rejected", "growths")


def both(ctx, leaf, calls, capacity_log2=10):
    """the calls through a WorldMap and through the restatement: (map, reference map)"""
    wm, rm = d.WorldMap(ctx, leaf, capacity_log2), pref.PruneReferenceMap(leaf)
    for pts, T in calls:
        assert wm.integrate(pts, T) == rm.integrate(pts, T)
    return wm, rm


def check_classify(wm, rm, **opts):
    """the dry run equals the restatement: counts, and (key, reason) per cell; the map is untouched"""
    before = wm.info()
    info, want = wm.classifyPrune(**opts), rm.classify(**opts)
    assert (info["n_cells"], info["n_kept"], info["n_removed"]) == (want["n_cells"], want["n_kept"], want["n_removed"]), (info, opts)
    assert info["capacity"] == before["capacity"] and wm.info() == before
    got = wm.fetchPruneReasons()
    assert got["reason"].dtype == np.uint8 and np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["reason"], want["reason"])
    ref.assert_maps_equal(wm.extract(), rm.extract())
    return info


def check_prune(wm, rm, **opts):
    """the prune equals the restatement's: counts, the map's bits, and the map's own counters"""
    before = wm.info()
    info, want = wm.prune(**opts), rm.prune(**{k: v for k, v in opts.items() if k != "shrink"})
    assert (info["n_cells"], info["n_kept"], info["n_removed"]) == (want["n_cells"], want["n_kept"], want["n_removed"]), (info, opts)
    assert info["n_cells"] == before["occupied"] == info["n_kept"] + sum(info["n_removed"])
    after = wm.info()
    assert after["occupied"] == info["n_kept"] == len(rm.keys) and all(after[k] == before[k] for k in COUNTERS)
    assert info["capacity"] == after["capacity"] == (pref.shrunk_capacity(info["n_kept"]) if opts.get("shrink") else before["capacity"])
    ref.assert_maps_equal(wm.extract(), rm.extract())
    assert wm.count(0, 0) == info["n_kept"]
    with pytest.raises(d.DsiError) as e:
        wm.fetchPruneReasons()
    assert e.value.code == E.ERR_INVALID
    return info


def check_stamps(wm, rm):
    """the stamps, which no extraction shows, through criterion 3 at every age that occurs"""
    for age in range(int(rm.calls) + 1):
        check_classify(wm, rm, max_age=age)


def refused(fn):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code == E.ERR_INVALID


def test_random_scene(ctx):
    wm, rm = both(ctx, pref.LEAF, pref.scene_calls())
    assert refused(wm.fetchPruneReasons)                                       # nothing classified yet
    view = (E.pose_matrix([0, 0, 2.0, 0, 0, 0, 1]), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 6.0)
    r0 = wm.render(*view)
    c0 = wm.compare(wm, 0.05, distances=True)
    assert r0["n_drawn"] > 100 and c0["n_matched"] == len(rm.keys)
    info = check_classify(wm, rm, **pref.SCENE_OPTS)
    assert info["n_kept"] >= 20 and min(info["n_removed"]) >= 20
    r1, c1 = wm.fetchRender(), wm.fetchDistances()                             # still valid, and unchanged
    assert all(np.array_equal(r0[k], r1[k]) for k in r1) and all(np.array_equal(c0[k], c1[k]) for k in c1)
    check_stamps(wm, rm)
    check_classify(wm, rm, **pref.SCENE_OPTS)
    check_prune(wm, rm, **pref.SCENE_OPTS)
    assert refused(wm.fetchRender) and refused(wm.fetchDistances) and refused(wm.fetchPruneReasons)
    check_stamps(wm, rm)                                                       # every kept cell moved with its stamp
    # ages go on counting, and a removed cell that a later call reaches starts from zero
    pts = pref.scene_calls()[0][0]
    assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY)
    ref.assert_maps_equal(wm.extract(), rm.extract())
    assert wm.info()["calls"] == rm.calls == 9
    check_stamps(wm, rm)
    wm.close()


def test_order_and_table_freedom(ctx):
    calls = pref.scene_calls()
    rng = np.random.default_rng(5)
    small, rm = both(ctx, pref.LEAF, calls, capacity_log2=8)
    large, rm2 = both(ctx, pref.LEAF, [(p[rng.permutation(len(p))], T) for p, T in calls], capacity_log2=16)
    assert small.info()["growths"] >= 3 and large.info()["growths"] == 0
    a, b = check_prune(small, rm, shrink=True, **pref.SCENE_OPTS), check_prune(large, rm2, **pref.SCENE_OPTS)
    assert {k: a[k] for k in a if k != "capacity"} == {k: b[k] for k in b if k != "capacity"} and a["capacity"] < b["capacity"] == 1 << 16
    ref.assert_maps_equal(small.extract(), large.extract())
    check_stamps(small, rm)
    check_stamps(large, rm2)
    small.close()
    large.close()
    # split into other calls: windows and stamps differ, so criteria 1, 4 and 5 alone; keys, n and the centroids' bits agree
    pts = np.concatenate([p for p, _ in calls])
    opts = dict(min_points=2, box=pref.SCENE_OPTS["box"], reach=1, min_neighbors=2)
    one, one_ref = both(ctx, pref.LEAF, [(pts, IDENTITY)], capacity_log2=16)
    shuffled = pts[rng.permutation(len(pts))]
    cuts = [0, 1, 700, 701, 2500, len(pts)]
    five, five_ref = both(ctx, pref.LEAF, [(shuffled[i:j], IDENTITY) for i, j in zip(cuts[:-1], cuts[1:])], capacity_log2=8)
    check_prune(one, one_ref, **opts)
    check_prune(five, five_ref, shrink=True, **opts)
    x, y = one.extract(), five.extract()
    assert len(x["keys"]) > 100 and np.array_equal(x["keys"], y["keys"]) and np.array_equal(x["n"], y["n"])
    assert np.array_equal(x["xyz"].view(np.uint32), y["xyz"].view(np.uint32))
    one.close()
    five.close()


def pc_hash(keys, mask):
    """the table's hash (the 64-bit finaliser of MurmurHash3), for the wrap-around test's premise"""
    k = np.asarray(keys, np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return (k & np.uint64(mask)).astype(np.int64)


def test_probe_chains_that_wrap_around_a_full_small_table(ctx):
    # the scene pruned by the box alone, with shrink, to between 3/8 and 3/4 of 2^8 slots; the box is narrowed on the
    # restatement until the load is near 3/4, then one prune on the device
    wm, rm = both(ctx, pref.LEAF, pref.scene_calls())
    hi = 0.7
    while rm.classify(box=((-0.7, -0.7, -0.2), (hi, 0.7, 0.15)))["n_kept"] > 192:
        hi -= 0.01
    info = check_prune(wm, rm, shrink=True, box=((-0.7, -0.7, -0.2), (hi, 0.7, 0.15)))
    assert info["capacity"] == 256 and 180 <= info["n_kept"] <= 192
    # linear probing fills the same SET of slots whatever the order of insertion: simulate it to see that a chain wraps
    slots = np.zeros(256, bool)
    wrapped = 0
    for h in pc_hash(rm.keys, 255):
        s = int(h)
        while slots[s]:
            s = (s + 1) & 255
        slots[s] = True
        wrapped += s < h
    assert wrapped >= 1
    check_classify(wm, rm, reach=1, min_neighbors=3)
    check_classify(wm, rm, reach=2, min_neighbors=30)
    check_prune(wm, rm, reach=1, min_neighbors=3)
    check_stamps(wm, rm)
    wm.close()


def test_the_strided_walk(ctx):
    # 2^19 slots: 2048 tiles for at most 1024 workgroups, so every workgroup walks two rounds (at 2^18 and below, one)
    wm, rm = both(ctx, pref.LEAF, pref.scene_calls(), capacity_log2=19)
    assert wm.info()["capacity"] == 1 << 19 and 500 < len(rm.keys) < 5000
    check_classify(wm, rm, **pref.SCENE_OPTS)
    info = check_prune(wm, rm, **pref.SCENE_OPTS)
    assert info["capacity"] == 1 << 19
    check_stamps(wm, rm)
    check_prune(wm, rm, shrink=True, reach=2, min_neighbors=12)
    wm.close()


def test_shrink_and_regrowth(ctx):
    n = 20000
    idx = np.arange(n)
    cells = np.stack([idx % 40 - 20, (idx // 40) % 40 - 20, idx // 1600 - 6], axis=1)
    rng = np.random.default_rng(3)
    pts = ((cells + rng.uniform(0.1, 0.9, (n, 3))) * 0.5).astype(np.float32)
    pts = pts[rng.permutation(n)]
    calls = [(pts[:10000], IDENTITY), (pts[10000:], IDENTITY)]
    box = ((-2.5, -2.5, -1.0), (0.0, 0.0, 1.0))                                 # 5 x 5 x 4 cells
    wm, rm = both(ctx, 0.5, calls, capacity_log2=8)
    grown = wm.info()
    assert grown["occupied"] == n and grown["capacity"] == 1 << 15
    info = check_prune(wm, rm, box=box)                                         # without shrink the capacity stays
    assert info["capacity"] == 1 << 15 and 80 <= info["n_kept"] <= 120 and info["n_removed"][3] == n - info["n_kept"]
    for p, T in calls:                                                          # the removed cells come back, from zero
        assert wm.integrate(p, T) == rm.integrate(p, T)
    got = wm.extract()
    ref.assert_maps_equal(got, rm.extract())
    assert len(got["keys"]) == n and sorted(np.unique(got["n"]).tolist()) == [1, 2] and (got["n"] == got["windows"]).all()
    assert wm.info()["growths"] == grown["growths"]
    info = check_prune(wm, rm, box=box, shrink=True)
    assert info["capacity"] == 256 and wm.info()["growths"] == grown["growths"]
    check_stamps(wm, rm)
    for p, T in calls:                                                          # regrowth from 2^8 slots
        assert wm.integrate(p, T) == rm.integrate(p, T)
    got = wm.extract()
    ref.assert_maps_equal(got, rm.extract())
    after = wm.info()
    assert after["occupied"] == n and after["capacity"] == 1 << 15 and after["growths"] == grown["growths"] + 7
    assert sorted(np.unique(got["n"]).tolist()) == [1, 3] and got["windows"][got["n"] == 1].max() == 1
    check_stamps(wm, rm)
    wm.close()


SINGLE = [dict(min_points=2), dict(min_points=3), dict(min_windows=2), dict(min_windows=3), dict(max_age=0), dict(max_age=4),
          dict(box=pref.SCENE_OPTS["box"]), dict(box=((-np.inf, -0.1, -np.inf), (np.inf, 0.1, np.inf))),
          dict(reach=1, min_neighbors=1), dict(reach=1, min_neighbors=26), dict(reach=2, min_neighbors=5), dict(reach=2, min_neighbors=124)]


def test_every_criterion_on_its_own_then_all_five(ctx):
    wm, rm = both(ctx, pref.LEAF, pref.scene_calls())
    for opts in SINGLE:
        info = check_classify(wm, rm, **opts)
        which = [i for i, v in enumerate(info["n_removed"]) if v]
        want = 0 if "min_points" in opts else 1 if "min_windows" in opts else 2 if "max_age" in opts else 3 if "box" in opts else 4
        assert which == [want], (opts, info)
    for opts in SINGLE[::2]:                                                    # each on a map of its own: the rebuild
        m2, r2 = both(ctx, pref.LEAF, pref.scene_calls())
        check_prune(m2, r2, **opts)
        m2.close()
    check_prune(wm, rm, **pref.SCENE_OPTS)
    wm.close()


def test_degenerate_maps(ctx):
    calls = pref.scene_calls()
    wm, rm = both(ctx, pref.LEAF, calls)
    before = wm.extract(sort=False)
    info = check_prune(wm, rm)                                                  # removes nothing: the map is unchanged
    assert info["n_removed"] == [0] * 5 and all(np.array_equal(v, wm.extract(sort=False)[k]) for k, v in before.items())
    info = check_prune(wm, rm, shrink=True)                                     # nothing removed, but the table shrinks to fit
    assert info["n_removed"] == [0] * 5 and info["capacity"] == pref.shrunk_capacity(len(rm.keys))
    info = check_prune(wm, rm, min_points=2 ** 32 - 1)                          # removes everything
    assert info["n_kept"] == 0 and wm.info()["occupied"] == 0 and len(wm.extract()["keys"]) == 0
    info = check_prune(wm, rm, shrink=True, **pref.SCENE_OPTS)                  # an empty map
    assert info["n_cells"] == 0 and info["capacity"] == 256
    check_classify(wm, rm, **pref.SCENE_OPTS)
    assert len(wm.fetchPruneReasons()["keys"]) == 0
    for pts, T in calls[:3]:                                                    # later integrates work, and grow the table again
        assert wm.integrate(pts, T) == rm.integrate(pts, T)
    ref.assert_maps_equal(wm.extract(), rm.extract())
    assert wm.info()["calls"] == rm.calls == 11
    check_classify(wm, rm, **dict(pref.SCENE_OPTS, max_age=1))
    # the fetch's capacity protocol, and invalidation by reset
    import ctypes as C
    L = d.load_library()
    m = len(rm.keys)
    reasons, keys, n = np.full(m, 77, np.uint8), np.full(m, 99, np.uint64), C.c_size_t()
    rc = L.dsx_map_prune_fetch(wm._h, reasons.ctypes.data_as(C.POINTER(C.c_uint8)), keys.ctypes.data_as(C.POINTER(C.c_uint64)), m - 1,
                               C.byref(n))
    assert rc == E.ERR_INVALID and n.value == m and (reasons == 77).all() and (keys == 99).all()
    assert L.dsx_map_prune_fetch(wm._h, reasons.ctypes.data_as(C.POINTER(C.c_uint8)), None, m, C.byref(n)) == E.OK   # an output may be NULL
    assert np.array_equal(np.sort(reasons), np.sort(rm.classify(**dict(pref.SCENE_OPTS, max_age=1))["reason"]))
    wm.reset()
    assert refused(wm.fetchPruneReasons)
    with pytest.raises(d.DsiError):
        wm.prune(reach=1)
    with pytest.raises(ValueError):
        wm.prune(max_age=-2)
    wm.close()


@pytest.mark.parametrize("case", pref.hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(ctx, case):
    wm = pref.run_hand_case(case, lambda leaf: d.WorldMap(ctx, leaf, 8))
    rm = pref.run_hand_case(case, pref.PruneReferenceMap)
    check_classify(wm, rm, **case["opts"])
    keys, reasons = pref.wanted_reasons(case)
    got = wm.fetchPruneReasons()
    assert np.array_equal(got["keys"], keys) and np.array_equal(got["reason"], reasons)
    check_prune(wm, rm, **case["opts"])
    assert np.array_equal(wm.extract()["keys"], keys[reasons == 0])
    wm.close()


def test_local_map_through_full_sequence(ctx):
    """full_sequence(..., world_map=, world_map_prune=) with local_box and every=2: the final map equals the restatement
    driven by the clouds the stream returned, through the same poses and the same prunes; None leaves the run as it is."""
    n_win, dur, t0 = 4, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    kw = dict(options_depth_map=d.OptionsDepthMap(), options_point_cloud=d.OptionsPointCloud(2.0, 1))
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    plain_map = d.WorldMap(ctx, 0.5, 8)
    plain = list(proc.full_sequence(*args, world_map=plain_map, world_map_prune=None, **kw))
    poses = [d.invert_pose(proc.reference_view_process1(rig["trajectories"][0], w[0])) for w in plain]
    # half extents from the first window's cloud in the world frame: about half of its points lie within them per axis
    first = ref.world_positions(plain[0][4], poses[0])
    half = np.median(np.abs(first - poses[0][[3, 7, 11]]), axis=0) * 1.25
    prune = dict(local_box=tuple(half.tolist()), every=2, shrink=True, min_points=1)
    wm = d.WorldMap(ctx, 0.5, 8)
    on = list(proc.full_sequence(*args, world_map=wm, world_map_prune=prune, **kw))
    assert len(on) == len(plain) == n_win
    rm, unpruned = pref.PruneReferenceMap(0.5), pref.PruneReferenceMap(0.5)
    for k, (a, b) in enumerate(zip(on, plain)):
        assert len(b) == 5 and len(a) == (6 if k % 2 else 5) and a[0] == b[0]
        for x, y in zip(a[1:5], b[1:]):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        rm.integrate(a[4], poses[k])
        unpruned.integrate(b[4], poses[k])
        if k % 2:
            t = poses[k][[3, 7, 11]]
            want = rm.prune(box=(t - half, t + half))
            got = a[5]["world_map_prune"]
            print("window %d: %s" % (k, got))
            assert (got["n_cells"], got["n_kept"], got["n_removed"]) == (want["n_cells"], want["n_kept"], want["n_removed"])
            assert got["capacity"] == pref.shrunk_capacity(got["n_kept"]) and got["n_kept"] >= 1 and got["n_removed"][3] >= 1
            assert got["n_removed"][:3] + got["n_removed"][4:] == [0, 0, 0, 0]
    ref.assert_maps_equal(wm.extract(), rm.extract())
    ref.assert_maps_equal(plain_map.extract(), unpruned.extract())
    assert wm.info()["calls"] == plain_map.info()["calls"] == n_win and wm.info()["occupied"] < plain_map.info()["occupied"]
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map_prune=prune, **kw))            # no map to prune
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map=wm, world_map_prune=dict(prune, every=0), **kw))
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map=wm, world_map_prune=dict(prune, box=((0, 0, 0), (1, 1, 1))), **kw))
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map=wm, world_map_prune=dict(prune, radius=1.0), **kw))
    wm.close()
    plain_map.close()
