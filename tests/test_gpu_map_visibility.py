"""The world map's visibility tally on the GPU (include/dsi_map_visibility.h; DESIGN.md 7j "Visibility") against the numpy
restatement tests/map_visibility_reference.py: array_equal on every counter, the three tally columns, keys, reasons and the
pruned map's exact state.  tests/test_map_visibility_cpu.py proves the restatement against plain reasoning and a scalar loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_layout_cases as lc
import map_merge_reference as mref
import map_pca_reference as pr
import map_prune_reference as pref
import map_visibility_reference as vr
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = vr.IDENTITY
COUNTERS = ("calls", "accepted", "rejected", "growths")


def device_map(ctx, leaf, calls, capacity_log2=10):
    wm = d.WorldMap(ctx, leaf, capacity_log2)
    for pts, T in calls:
        wm.integrate(pts, T)
    return wm


def refused(fn, word="visibility tally", code=E.ERR_INVALID):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code == code and (word is None or word in str(e.value))


def check_views(wm, rm, views):
    """the views observed one after the other equal the restatement's: every view's counts, then the rows; the map is
    untouched.  Returns the restatement's tally."""
    before = wm.info()
    tally = vr.Tally(rm)
    wm.clearVisibility()
    for v in views:
        got, want = wm.observe(*v), tally.observe(*v)
        print(got)
        vr.assert_counts_equal(got, want)
    rows = wm.fetchVisibility(sort=True)
    assert set(rows) == {"keys", "seen", "agree", "through"}
    vr.assert_rows_equal(rows, tally.rows())
    assert wm.info() == before
    return tally


def check_select(wm, tally, min_through, agree_weight):
    before = wm.info()
    info, want = wm.selectCarved(min_through, agree_weight), tally.select(min_through, agree_weight)
    assert all(info[f] == want[f] for f in ("n_cells", "n_kept", "n_removed")), (info, {k: v for k, v in want.items() if k != "reason"})
    assert info["capacity"] == before["capacity"] and wm.info() == before
    rows = wm.fetchVisibility(sort=True)
    assert rows["reason"].dtype == np.uint8 and np.array_equal(rows["keys"], tally.keys) and np.array_equal(rows["reason"], want["reason"])
    return info


def check_prune(wm, rm, tally, min_through, agree_weight, shrink=False):
    """the prune equals the restatement's: counts, the map's exact state and its counters; every visibility call is refused after"""
    before = wm.info()
    info, want = wm.pruneCarved(min_through, agree_weight, shrink=shrink), tally.prune(rm, min_through, agree_weight)
    assert all(info[f] == want[f] for f in ("n_cells", "n_kept", "n_removed")), info
    assert info["n_cells"] == before["occupied"] == info["n_kept"] + info["n_removed"]
    after = wm.info()
    assert after["occupied"] == info["n_kept"] == len(rm.keys) and all(after[k] == before[k] for k in COUNTERS)
    assert info["capacity"] == after["capacity"] == (pref.shrunk_capacity(info["n_kept"]) if shrink else before["capacity"])
    mref.assert_states_equal(wm.exportState(), rm.export_state())
    assert all(refused(fn) for fn in (wm.fetchVisibility, wm.selectCarved, wm.pruneCarved))
    return info


# ---- 1. the constructed scene: the verdicts are known without the restatement ----
def test_constructed_scene_in_the_smallest_table(ctx):
    s = vr.wall_scene()
    wm = d.WorldMap(ctx, vr.WALL_LEAF, 8)
    for part in np.array_split(s["points"], 3):                                # 439 cells from 2^8 slots: the table grows twice
        wm.integrate(part, IDENTITY)
    assert wm.info()["growths"] == 2 and wm.info()["occupied"] == len(s["points"])
    depth, mask = vr.wall_depth()
    counts = wm.observe(depth, mask, window=0, **vr.WALL_VIEW)
    want = vr.wall_expected()
    assert counts == {"n_cells": len(want), "n_valid_pixels": int(mask.sum()), "views": 1,
                      **{name: int((want == code).sum()) for code, name in enumerate(vr.VERDICTS)}}
    assert all(counts[name] > 0 for name in vr.VERDICTS)
    rows = wm.fetchVisibility()
    ok, c, _ = ref.cells(s["points"], IDENTITY, vr.WALL_LEAF)
    row = np.searchsorted(rows["keys"], ref.pack_key(c))
    assert np.array_equal(rows["keys"][row], ref.pack_key(c))
    assert np.array_equal(rows["seen"][row], (want >= vr.AGREE).astype(np.uint32))
    assert np.array_equal(rows["agree"][row], (want == vr.AGREE).astype(np.uint32))
    assert np.array_equal(rows["through"][row], (want == vr.THROUGH).astype(np.uint32))
    # the same view twice more: the floaters on wall pixels, and only they, are carved at min_through = 3
    for views in (2, 3):
        assert wm.observe(depth, mask, window=0, **vr.WALL_VIEW) == dict(counts, views=views)
    assert np.array_equal(wm.fetchVisibility()["through"][row], 3 * (want == vr.THROUGH).astype(np.uint32))
    info = wm.pruneCarved(min_through=3, agree_weight=1, shrink=True)
    assert info == {"n_cells": len(want), "n_kept": len(want) - counts["n_through"], "n_removed": counts["n_through"], "capacity": 1024}
    assert np.array_equal(wm.extract()["keys"], np.sort(ref.pack_key(c)[want != vr.THROUGH]))
    wm.close()


# ---- 2. accumulated views of the local-shape scene; table size ----
def test_three_views_accumulate_as_the_restatement(ctx):
    calls, rm = pr.scene_calls(), pr.scene_reference()
    wm, big = device_map(ctx, pr.LEAF, calls, 8), device_map(ctx, pr.LEAF, calls, 12)      # grown to 2^12, and created there
    assert wm.info()["growths"] == 4 and big.info()["growths"] == 0 and wm.info()["capacity"] == big.info()["capacity"] == 1 << 12
    assert not np.array_equal(wm.extract(sort=False)["keys"], big.extract(sort=False)["keys"])   # the same cells, laid out differently
    assert refused(wm.fetchVisibility)                                         # before the first observation
    got = []
    for which in (0, 1):                                                       # clearVisibility, then another list of views on the unchanged map
        tally = check_views(wm, rm, vr.scene_views(which))
        vr.assert_rows_equal(tally.rows(), vr.scene_tally(which)[0].rows())
        check_views(big, rm, vr.scene_views(which))
        if which:                                                              # and in a table of another size
            wide = device_map(ctx, pr.LEAF, calls, 14)
            check_views(wide, rm, vr.scene_views(which))
            wide.close()
        got.append((wm.fetchVisibility(), big.fetchVisibility()))
        assert all(np.array_equal(got[-1][0][f], got[-1][1][f]) for f in got[-1][0])   # the tally does not depend on the capacity
    assert not np.array_equal(got[0][0]["through"], got[1][0]["through"])
    wm.close()
    big.close()


# ---- 3. layouts: more slots than one stride, and a chain across the table's end ----
@pytest.mark.parametrize("name", ("sparse", "dense"))
def test_tables_of_two_rounds(ctx, name):
    calls, rm = (lc.sparse_calls(), lc.sparse_reference()) if name == "sparse" else (lc.dense_calls(), lc.dense_reference())
    wm = device_map(ctx, lc.LEAF, calls, lc.BIG_LOG2)
    assert wm.info()["capacity"] == 1 << lc.BIG_LOG2 and wm.info()["growths"] == 0
    before = wm.info()
    want, want_counts = vr.layout_tally(name)
    for v, c in zip(vr.layout_views(name), want_counts):
        vr.assert_counts_equal(wm.observe(*v), c)
    vr.assert_rows_equal(wm.fetchVisibility(sort=True), want.rows())
    info, sel = wm.selectCarved(1, 1), want.select(1, 1)
    assert all(info[f] == sel[f] for f in ("n_cells", "n_kept", "n_removed")) and np.array_equal(wm.fetchVisibility(sort=True)["reason"], sel["reason"])
    assert wm.info() == before
    rm = lc.fresh(rm)
    check_prune(wm, rm, want, 1, 1)
    wm.close()


def test_chain_across_the_tables_end(ctx):
    ch = lc.chain("2^8")
    calls = [ch["first"], ch["again"]]
    rm = lc.chain_reference("2^8")
    wm, twice = device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"]), device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"] + 1)
    assert wm.info()["capacity"] == ch["capacity"] and twice.info()["capacity"] == 2 * ch["capacity"]
    for m in (wm, twice):
        tally = check_views(m, rm, vr.chain_views("2^8"))
        check_select(m, tally, 1, 0)
    check_prune(wm, rm, tally, 1, 0)
    wm.close()
    twice.close()


# ---- 4. the mapper's filtered depth map, read where it lies ----
def test_observe_mapper_equals_observe_of_the_fetched_maps(ctx):
    rig = syn.stereo_rig(60_000, width=64, height=48, t0=10.0, duration=0.05, seed=5, n_points=400)
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    m = d.MapperEMVS(ctx, rig["cam"], shape)
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    wm, host = d.WorldMap(ctx, 0.5, 8), d.WorldMap(ctx, 0.5, 8)
    K, lo, hi = m.virtual_cam_, 4.0, 50.0
    assert refused(lambda: wm.observeMapper(m, K, lo, hi, IDENTITY), "no filtered depth map")
    depth, _, mask = m.getDepthMapFromDSI(None, d.OptionsDepthMap())
    assert mask.sum() > 50
    opts_pc = d.OptionsPointCloud(2.0, 1)
    cloud = m.getPointcloud(options_pc=opts_pc)
    rng = np.random.default_rng(5)
    clutter = np.concatenate([cloud[:, :3] * np.float32(0.6), cloud[:, :3] * np.float32(1.5), rng.uniform(-20, 20, (300, 3)).astype(np.float32)])
    rm = vr.reference_of([(cloud[:, :3], IDENTITY), (clutter, IDENTITY)], 0.5)
    for w in (wm, host):
        w.integrate(cloud, IDENTITY)
        w.integrate(clutter, IDENTITY)
    tally = vr.Tally(rm)
    shifted = np.array([1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 1.0], np.float64)
    for T, window, abs_tol, rel_tol in ((IDENTITY, 0, 0.5, 0.0), (shifted, 2, 0.0, 0.05)):
        got = wm.observeMapper(m, K, lo, hi, T, window, abs_tol, rel_tol)
        print(got)
        assert got == host.observe(depth, mask, K, lo, hi, T, window, abs_tol, rel_tol)
        vr.assert_counts_equal(got, tally.observe(depth, mask, K, lo, hi, T, window, abs_tol, rel_tol))
    a, b = wm.fetchVisibility(), host.fetchVisibility()
    assert all(np.array_equal(a[f], b[f]) for f in a) and a["seen"].sum() > 20
    vr.assert_rows_equal(a, tally.rows())
    # refusals: the size is the mapper's; a mapper of another context
    o = wm._observation(m.dimX + 1, m.dimY, K, lo, hi, IDENTITY, 1, 0.0, 0.0)
    assert d.load_library().dsx_map_observe_mapper(wm._h, m._h, C.byref(o), None) == E.ERR_INVALID
    other = d.Context(0)
    m2 = d.MapperEMVS(other, rig["cam"], shape)
    assert refused(lambda: wm.observeMapper(m2, K, lo, hi, IDENTITY), None, E.ERR_CONTEXT)
    vr.assert_rows_equal(wm.fetchVisibility(), tally.rows())                   # a refused observation leaves the tally as it was
    for o in (m2, other, m, wm, host):
        o.close()


# ---- 5. select, fetch with reasons, prune ----
@pytest.mark.parametrize("shrink", (False, True))
def test_select_and_prune_equal_the_restatement_bit_for_bit(ctx, shrink):
    calls = pr.scene_calls()
    wm, rm = device_map(ctx, pr.LEAF, calls), vr.reference_of(calls, pr.LEAF)
    tally = check_views(wm, rm, vr.scene_views(0))
    assert tally.through.max() >= 2 and ((tally.through == tally.agree) & (tally.through > 0)).sum() >= 20
    for min_through, agree_weight in ((1, 1), (2, 1), (1, 0), (2, 0), (1, 2), (1, 0xffffffff), (3, 0), (0xffffffff, 0)):
        check_select(wm, tally, min_through, agree_weight)
    assert wm.selectCarved() == wm.selectCarved(2, 1) and wm.selectCarved(1, 0)["n_removed"] == int((tally.through > 0).sum())
    info = check_prune(wm, rm, tally, 1, 1, shrink)
    assert info["n_removed"] >= 100
    # the kept cells moved with n, S, windows and stamp; the map goes on: integrate, observe again, prune again
    assert wm.integrate(calls[0][0], IDENTITY) == rm.integrate(calls[0][0], IDENTITY)
    mref.assert_states_equal(wm.exportState(), rm.export_state())
    tally = check_views(wm, rm, vr.scene_views(1))
    check_prune(wm, rm, tally, 1, 0, shrink)
    tally = check_views(wm, rm, vr.scene_views(1)[1:])
    before = wm.info()
    check_prune(wm, rm, tally, 3, 0)                                           # two views cannot reach three: nothing leaves, the table stays
    assert wm.info() == before
    wm.close()


# ---- 6. invalidation ----
def test_every_change_of_the_map_ends_the_tally(ctx):
    calls = pr.scene_calls()
    wm, other = device_map(ctx, pr.LEAF, calls), device_map(ctx, pr.LEAF, calls[:2])
    readers = (wm.fetchVisibility, wm.selectCarved, wm.pruneCarved)
    state = other.exportState()
    view = vr.scene_views(0)[1]
    assert all(refused(fn) for fn in readers)
    for change in (lambda: wm.integrate(calls[0][0], IDENTITY), lambda: wm.integrate(np.zeros((0, 3), np.float32), IDENTITY),
                   lambda: wm.integrateDepth(view[0], view[1], view[2], view[3], view[4], IDENTITY), lambda: wm.integrateMap(other),
                   lambda: wm.merge(other), lambda: wm.importState(state), lambda: wm.prune(), lambda: wm.prune(min_points=2),
                   lambda: (wm.components(), wm.pruneComponents(min_cells=2)), lambda: (wm.knn(4, 0.1), wm.pruneOutliers(1.0)),
                   lambda: (wm.pca(4, 0.1), wm.pruneShapes(7, False)), lambda: wm.pruneCarved(1, 1), lambda: wm.pruneCarved(0xffffffff, 0),
                   wm.clearVisibility, wm.reset):
        assert wm.observe(*view)["views"] == 1 and wm.observe(*view)["views"] == 2
        wm.selectCarved()
        assert "reason" in wm.fetchVisibility()
        change()
        assert all(refused(fn) for fn in readers)
    # an observation leaves every other stage's result valid, and ends only its own selection
    for pts, T in calls:
        wm.integrate(pts, T)
    wm.render(E.pose_matrix([0, 0, -2.0, 0, 0, 0, 1]), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 6.0)
    wm.compare(wm, 0.05, distances=True)
    wm.classifyPrune(min_points=2)
    wm.alignStep(wm, 0.05)
    wm.components()
    wm.knn(4, 0.1)
    wm.pca(4, 0.1)
    fetches = (wm.fetchRender, wm.fetchDistances, wm.fetchPruneReasons, wm.fetchAlignment, wm.fetchComponents, wm.fetchKnn, wm.fetchPca)
    kept = [f() for f in fetches]
    wm.observe(*view)
    wm.selectCarved()
    wm.observe(*view)
    for f, was in zip(fetches, kept):
        now = f()
        assert all(np.array_equal(now[k], was[k], equal_nan=(now[k].dtype.kind == "f")) for k in was)
    rows = wm.fetchVisibility()
    assert "reason" not in rows and rows["seen"].max() == 2
    # reasons before a select, the capacity protocol, and NULL outputs
    L = d.load_library()
    m = wm.count()
    keys, seen, reasons, n = np.full(m, 99, np.uint64), np.full(m, 98, np.uint32), np.full(m, 77, np.uint8), C.c_size_t()
    kp, sp, rp = (a.ctypes.data_as(C.POINTER(t)) for a, t in ((keys, C.c_uint64), (seen, C.c_uint32), (reasons, C.c_uint8)))
    assert L.dsx_map_visibility_fetch(wm._h, kp, sp, None, None, rp, m, C.byref(n)) == E.ERR_INVALID and b"select" in L.dsi_last_error()
    assert L.dsx_map_visibility_fetch(wm._h, kp, sp, None, None, None, m - 1, C.byref(n)) == E.ERR_INVALID and n.value == m
    assert (keys == 99).all() and (seen == 98).all() and (reasons == 77).all()
    wm.selectCarved(1, 0)
    assert L.dsx_map_visibility_fetch(wm._h, None, None, None, None, rp, m, C.byref(n)) == E.OK and n.value == m
    assert set(np.unique(reasons).tolist()) == {0, 1} and (keys == 99).all()
    assert L.dsx_map_visibility_fetch(wm._h, kp, sp, None, None, None, m, C.byref(n)) == E.OK
    assert np.array_equal(keys, wm.extract(sort=False)["keys"]) and seen.max() == 2      # the order is extract's
    wm.close()
    other.close()


# ---- 7. refusals, before the GPU is touched ----
def test_every_violated_bound_is_refused(ctx):
    L = d.load_library()
    wm = device_map(ctx, vr.WALL_LEAF, [(vr.wall_scene()["points"], IDENTITY)], 8)
    depth, mask = vr.wall_depth()
    good = dict(vr.WALL_VIEW, window=1, abs_tol=0.0, rel_tol=0.0)
    wm.observe(depth, mask, **good)
    before = wm.fetchVisibility()
    nan, inf = float("nan"), float("inf")
    for bad in (dict(window=4), dict(window=-1), dict(abs_tol=-1e-9), dict(rel_tol=-1.0), dict(abs_tol=nan), dict(rel_tol=inf), dict(abs_tol=inf),
                dict(min_depth=0.0), dict(min_depth=5.0), dict(max_depth=inf), dict(K=(0.0, 9.0, 16.0, 12.0)), dict(K=(9.0, 9.0, nan, 12.0))):
        assert refused(lambda: wm.observe(depth, mask, **dict(good, **bad)), None), bad
    for bad in (lambda: wm.selectCarved(0), lambda: wm.pruneCarved(0)):
        assert refused(bad, None)
    # a refused call changes nothing: the tally is as it was, with its one view
    now = wm.fetchVisibility()
    assert all(np.array_equal(now[f], before[f]) for f in before) and wm.observe(depth, mask, **good)["views"] == 2
    # the bounds are judged with no map at hand; then the NULL arguments
    o = wm._observation(33, 25, good["K"], 0.5, 4.0, IDENTITY, 4, 0.0, 0.0)
    info, sel, sinfo = E._MapObserveInfo(), E._MapVisibilitySelection(0, 1, 0), E._MapVisibilitySelectInfo()
    dp = depth.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dsx_map_observe(None, dp, None, C.byref(o), C.byref(info)) == E.ERR_INVALID and b"window" in L.dsi_last_error()
    assert L.dsx_map_observe_mapper(None, None, C.byref(o), C.byref(info)) == E.ERR_INVALID and b"window" in L.dsi_last_error()
    assert L.dsx_map_visibility_select(None, C.byref(sel), C.byref(sinfo)) == E.ERR_INVALID and b"min_through" in L.dsi_last_error()
    assert L.dsx_map_prune_visibility(None, C.byref(sel), C.byref(sinfo)) == E.ERR_INVALID and b"min_through" in L.dsi_last_error()
    o.window, sel.min_through = 1, 1
    n = C.c_size_t()
    assert L.dsx_map_observe(None, dp, None, C.byref(o), None) == E.ERR_INVALID and L.dsx_map_observe(wm._h, None, None, C.byref(o), None) == E.ERR_INVALID
    assert L.dsx_map_observe(wm._h, dp, None, None, None) == E.ERR_INVALID and L.dsx_map_observe_mapper(wm._h, None, C.byref(o), None) == E.ERR_INVALID
    assert L.dsx_map_visibility_clear(None) == E.ERR_INVALID and L.dsx_map_visibility_fetch(None, None, None, None, None, None, 0, C.byref(n)) == E.ERR_INVALID
    assert L.dsx_map_visibility_select(None, C.byref(sel), None) == E.ERR_INVALID and L.dsx_map_visibility_select(wm._h, None, None) == E.ERR_INVALID
    assert L.dsx_map_prune_visibility(None, C.byref(sel), None) == E.ERR_INVALID and L.dsx_map_prune_visibility(wm._h, None, None) == E.ERR_INVALID
    assert L.dsx_map_observe(wm._h, dp, None, C.byref(o), None) == E.OK         # info may be NULL
    assert L.dsx_map_visibility_select(wm._h, C.byref(sel), None) == E.OK and wm.fetchVisibility()["seen"].max() == 3
    # an empty map
    empty = d.WorldMap(ctx, 0.5, 8)
    c = empty.observe(depth, mask, **good)
    assert c == dict(c, n_cells=0, n_agree=0, n_through=0, views=1) and c["n_valid_pixels"] == int(mask.sum())
    assert all(len(v) == 0 for v in empty.fetchVisibility().values()) and empty.pruneCarved()["n_kept"] == 0
    empty.close()
    wm.close()


# ---- 8. the stream (the C++ adapter: tests/test_gpu_map_visibility_cpp.py) ----
def test_carving_through_full_sequence(ctx):
    """full_sequence(..., world_map=, world_map_carve=) with views=2 and every=2 equals carve_world_map replayed by hand on a
    second map, fed with the clouds and depth maps the stream returned; None leaves the run as it is."""
    n_win, dur, t0 = 4, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    kw = dict(options_depth_map=d.OptionsDepthMap(), options_point_cloud=d.OptionsPointCloud(2.0, 1))
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    plain_map, wm, hand = (d.WorldMap(ctx, 0.5, 8) for _ in range(3))
    plain = list(proc.full_sequence(*args, world_map=plain_map, world_map_carve=None, **kw))
    opts = {"views": 2, "every": 2, "window": 1, "abs_tol": 0.25, "rel_tol": 0.02, "min_through": 1, "agree_weight": 1, "shrink": True}
    on = list(proc.full_sequence(*args, world_map=wm, world_map_carve=opts, **kw))
    assert len(on) == len(plain) == n_win
    probe = d.MapperEMVS(ctx, cam, shape)
    K, lo, hi = probe.virtual_cam_, float(probe.raw_depths_vec_.min()), float(probe.raw_depths_vec_.max())
    probe.close()
    T_rv_w = [proc.reference_view_process1(rig["trajectories"][0], w[0]) for w in plain]
    removed = 0
    for k, (a, b) in enumerate(zip(on, plain)):
        assert len(b) == 5 and len(a) == (6 if k % 2 else 5) and a[0] == b[0]
        for x, y in zip(a[1:5], b[1:]):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        hand.integrate(a[4], d.invert_pose(T_rv_w[k]))
        if k % 2:
            views = [(on[j][1], on[j][3], T_rv_w[j]) for j in (k - 1, k)]
            counts = proc.carve_world_map(hand, views, K, lo, hi, window=1, abs_tol=0.25, rel_tol=0.02, min_through=1, agree_weight=1, shrink=True)
            print("window %d: %s" % (k, counts))
            assert a[5] == {"world_map_carve": counts} and counts["views"] == 2 and counts["n_cells"] > 20
            removed += counts["prune"]["n_removed"]
    mref.assert_states_equal(wm.exportState(), hand.exportState())
    assert wm.info() == hand.info() and plain_map.info()["occupied"] - removed <= wm.info()["occupied"] <= plain_map.info()["occupied"]
    # after world_map_shapes=, on the same window
    both_map, by_hand = d.WorldMap(ctx, 0.5, 8), d.WorldMap(ctx, 0.5, 8)
    shapes = {"every": 2, "k": 0, "radius": 1.5, "min_found": 3, "keep": ("linear", "planar", "scattered"), "remove_sparse": True}
    both = list(proc.full_sequence(*args, world_map=both_map, world_map_shapes=shapes, world_map_carve=dict(opts, views=3), **kw))
    for k, a in enumerate(both):
        by_hand.integrate(a[4], d.invert_pose(T_rv_w[k]))
        if k % 2:
            assert len(a) == 7 and "world_map_shapes" in a[5] and "world_map_carve" in a[6]
            by_hand.pca(0, 1.5, 3)
            by_hand.pruneShapes(("linear", "planar", "scattered"), True)
            views = [(both[j][1], both[j][3], T_rv_w[j]) for j in range(max(0, k - 2), k + 1)]
            counts = proc.carve_world_map(by_hand, views, K, lo, hi, window=1, abs_tol=0.25, rel_tol=0.02, min_through=1, agree_weight=1, shrink=True)
            assert a[6]["world_map_carve"] == counts and counts["views"] == len(views) == min(k + 1, 3)
    mref.assert_states_equal(both_map.exportState(), by_hand.exportState())
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map_carve=opts, **kw))             # no map to carve
    for m in (plain_map, wm, hand, both_map, by_hand):
        m.close()


# ---- 10. the boundary: every symbol of the header is exported, and the ABI version stays ----
def test_header_symbols_are_exported():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "dsi_map_visibility.h")).read()
    names = re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header)
    assert sorted(names) == ["dsx_map_observe", "dsx_map_observe_mapper", "dsx_map_prune_visibility", "dsx_map_visibility_clear",
                             "dsx_map_visibility_fetch", "dsx_map_visibility_select"]
    raw = C.CDLL(d.load_library()._name)                                       # the library itself, not engine.py's table of bindings
    for name in names:
        assert getattr(raw, name) is not None and getattr(d.load_library(), name).argtypes is not None, name
    assert d.load_library().dsi_abi_version() == 10 and "DSI_ENGINE_ABI_VERSION 10" in open(os.path.join(root, "include", "dsi_engine.h")).read()
