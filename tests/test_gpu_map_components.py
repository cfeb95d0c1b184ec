"""The world map's connected components (dsx_map_components*, dsx_map_prune_components; engine.WorldMap.components /
fetchComponents / listComponents / selectComponents / pruneComponents; DESIGN.md 7j "Components") on the MI355X against the
restatement of tests/map_components_reference.py: every comparison is array_equal -- the (key, label) rows, the component
list and the reasons as equal arrays, the counts as integers, the pruned map through world_map_reference.assert_maps_equal."""
import copy
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_components_reference as cref
import map_layout_cases as lc
import map_prune_reference as pref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = pref.IDENTITY
COUNTERS = ("calls", "accepted", "rejected", "growths")
FILTERS = ((1, 1), (2, 1), (1, 2))
SCENE_SELECTION = dict(min_cells=2, min_component_points=6, keep_largest=3)


def device_map(ctx, leaf, calls, capacity_log2=10):
    wm = d.WorldMap(ctx, leaf, capacity_log2)
    for pts, T in calls:
        wm.integrate(pts, T)
    return wm


def refused(fn, word=None):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code == E.ERR_INVALID and (word is None or word in str(e.value))


def check_components(wm, comp, connectivity):
    """the labelling equals the restatement's `comp`: the counts, the (key, label) rows and the component list"""
    before = wm.info()
    info = wm.components(*comp["filter"], connectivity)
    assert info == comp["info"], (info, comp["info"])
    rows = wm.fetchComponents()
    assert set(rows) == {"keys", "labels"} and rows["labels"].dtype == np.uint64
    assert np.array_equal(rows["keys"], comp["keys"]) and np.array_equal(rows["labels"], comp["labels"])
    lst = wm.listComponents()
    for k in ("labels", "cells", "points"):
        assert lst[k].dtype == np.uint64 and np.array_equal(lst[k], comp["list"][k]), k
    assert wm.info() == before
    return info


def check_select(wm, rm, comp, **sel):
    """the dry run equals the restatement's: counts and per-node reasons; the map is untouched"""
    before = wm.info()
    info, want = wm.selectComponents(**sel), cref.select(rm, comp, **sel)
    got = (info["n_cells"], info["n_kept"], info["n_removed"], info["n_components_kept"])
    assert got == (want["n_cells"], want["n_kept"], want["n_removed"], want["n_components_kept"]), (info, sel)
    assert info["capacity"] == before["capacity"] and wm.info() == before
    rows = wm.fetchComponents()
    assert rows["reason"].dtype == np.uint8 and np.array_equal(rows["keys"], comp["keys"]) and np.array_equal(rows["labels"], comp["labels"])
    assert np.array_equal(rows["reason"], want["node_reason"])
    return info


def check_prune(wm, rm, comp, **sel):
    """the prune equals the restatement's: counts, the map's bits and its counters; everything derived is refused after"""
    before = wm.info()
    info = wm.pruneComponents(**sel)
    want = cref.prune_components(rm, comp, **{k: v for k, v in sel.items() if k != "shrink"})
    got = (info["n_cells"], info["n_kept"], info["n_removed"], info["n_components_kept"])
    assert got == (want["n_cells"], want["n_kept"], want["n_removed"], want["n_components_kept"]), (info, sel)
    assert info["n_cells"] == before["occupied"] == info["n_kept"] + sum(info["n_removed"])
    after = wm.info()
    assert after["occupied"] == info["n_kept"] == len(rm.keys) and all(after[k] == before[k] for k in COUNTERS)
    assert info["capacity"] == after["capacity"] == (pref.shrunk_capacity(info["n_kept"]) if sel.get("shrink") else before["capacity"])
    ref.assert_maps_equal(wm.extract(), rm.extract())
    assert wm.count(0, 0) == info["n_kept"]
    for fn in (wm.fetchComponents, wm.listComponents, wm.selectComponents, wm.pruneComponents):
        assert refused(fn, "labelling")
    return info


def check_stamps(wm, rm):
    """the stamps, which no extraction shows, through prune's criterion 3 at every age that occurs"""
    for age in range(int(rm.calls) + 1):
        info, want = wm.classifyPrune(max_age=age), rm.classify(max_age=age)
        assert (info["n_kept"], info["n_removed"]) == (want["n_kept"], want["n_removed"])
        got = wm.fetchPruneReasons()
        assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["reason"], want["reason"])


# ---- 1. pairs ----
@pytest.mark.parametrize("offset", list(cref.PAIR_OFFSETS), ids=str)
def test_pairs(ctx, offset):
    calls = [(cref.centres(cref.pair_cells(offset), cref.PAIR_LEAF), IDENTITY)]
    wm, rm = device_map(ctx, cref.PAIR_LEAF, calls, 8), cref.map_of(calls, cref.PAIR_LEAF)
    for conn in cref.CONNECTIVITIES:
        info = check_components(wm, cref.components(rm, connectivity=conn), conn)
        joined = conn in cref.PAIR_OFFSETS[offset]
        assert info["n_components"] == (1 if joined else 2) and info["n_singletons"] == (0 if joined else 2)
        assert info["largest_cells"] == (2 if joined else 1) and info["largest_label"] == int(rm.keys[0])
    wm.close()


def test_pairs_at_the_index_bound(ctx):
    calls = [(cref.centres(cref.edge_pairs(), cref.EDGE_LEAF), IDENTITY)]
    wm, rm = device_map(ctx, cref.EDGE_LEAF, calls, 8), cref.map_of(calls, cref.EDGE_LEAF)
    assert len(rm.keys) == 12
    for conn in cref.CONNECTIVITIES:
        info = check_components(wm, cref.components(rm, connectivity=conn), conn)
        assert info["n_components"] == 6 and info["largest_cells"] == 2
    wm.close()


# ---- 2. the random scene ----
def test_random_scene(ctx):
    wm, rm = device_map(ctx, pref.LEAF, pref.scene_calls()), cref.scene_reference()
    for fn in (wm.fetchComponents, wm.listComponents, wm.selectComponents, wm.pruneComponents):
        assert refused(fn, "labelling")                                        # nothing labelled yet
    view = (E.pose_matrix([0, 0, 2.0, 0, 0, 0, 1]), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 6.0)
    r0 = wm.render(*view)
    c0 = wm.compare(wm, 0.05, distances=True)
    p0 = wm.classifyPrune(**pref.SCENE_OPTS)
    wm.alignStep(wm, 0.05)
    reasons0, pairs0, cells0, info0 = wm.fetchPruneReasons(), wm.fetchAlignment(), wm.extract(sort=False), wm.info()
    assert r0["n_drawn"] > 100 and c0["n_matched"] == len(rm.keys) and p0["n_kept"] >= 20
    for conn in cref.CONNECTIVITIES:
        for flt in FILTERS:
            comp = cref.scene_components(*flt, conn)
            info = check_components(wm, comp, conn)
            assert info["n_components"] >= 5 and (flt == (1, 1)) == (info["n_unlabelled"] == 0)
    comp = cref.scene_components(2, 1, 26)
    check_components(wm, comp, 26)
    info = check_select(wm, rm, comp, **SCENE_SELECTION)
    assert info["n_kept"] >= 5 and min(info["n_removed"]) >= 1 and info["n_components_kept"] == 3
    # labelling and selecting changed nothing: the map, its counters, the render, the compare, the alignment step and the
    # classification
    r1, c1, reasons1, cells1 = wm.fetchRender(), wm.fetchDistances(), wm.fetchPruneReasons(), wm.extract(sort=False)
    pairs1 = wm.fetchAlignment()
    assert wm.info() == info0 and len(pairs1["keys"]) == len(rm.keys) and all(np.array_equal(pairs0[k], pairs1[k]) for k in pairs1)
    assert all(np.array_equal(r0[k], r1[k]) for k in r1) and all(np.array_equal(c0[k], c1[k]) for k in c1)
    assert all(np.array_equal(reasons0[k], reasons1[k]) for k in reasons1) and all(np.array_equal(cells0[k], cells1[k]) for k in cells1)
    # a classification does not invalidate the labelling either
    wm.classifyPrune(reach=1, min_neighbors=2)
    check_select(wm, rm, comp, min_cells=3)
    wm.close()


# ---- 3. table and order freedom ----
def test_table_and_order_freedom(ctx):
    calls = pref.scene_calls()
    rng = np.random.default_rng(5)
    small, large = device_map(ctx, pref.LEAF, calls, 8), device_map(ctx, pref.LEAF, calls, 16)
    assert small.info()["growths"] >= 3 and large.info()["growths"] == 0
    pts = np.concatenate([p for p, _ in calls])
    shuffled = pts[rng.permutation(len(pts))]
    cuts = [0, 1, 700, 701, 2500, len(pts)]
    recut = device_map(ctx, pref.LEAF, [(shuffled[i:j], IDENTITY) for i, j in zip(cuts[:-1], cuts[1:])], 8)
    for conn in cref.CONNECTIVITIES:
        for flt in FILTERS:
            comp = cref.scene_components(*flt, conn)
            check_components(small, comp, conn)
            check_components(large, comp, conn)
        check_components(recut, cref.scene_components(1, 1, conn), conn)        # (windows differ: the filter (1, 1) alone)
    for wm in (small, large, recut):
        wm.close()


# ---- 4. the snake ----
def test_snake(ctx):
    wm, rm = device_map(ctx, cref.SNAKE_LEAF, cref.snake_calls(), cref.SNAKE_LOG2), cref.snake_reference()
    assert wm.info()["capacity"] == 1 << cref.SNAKE_LOG2 and wm.info()["growths"] == 0
    per_layer = len(rm.keys) // 3
    for conn, want in ((6, 3), (18, 3), (26, 3), (124, 2)):
        comp = cref.components(rm, connectivity=conn)
        info = check_components(wm, comp, conn)
        assert info["n_components"] == want and info["n_singletons"] == 0
        assert info["largest_cells"] == (per_layer if want == 3 else 2 * per_layer) and info["largest_label"] == int(rm.keys[0])
    # keep_largest on three components of equal size: the tie goes to the smaller label
    comp = cref.components(rm, connectivity=26)
    check_components(wm, comp, 26)
    check_select(wm, rm, comp, keep_largest=2)
    rm = copy.deepcopy(rm)
    info = check_prune(wm, rm, comp, keep_largest=1, shrink=True)
    assert info["n_kept"] == per_layer and info["n_removed"] == [0, 0, 0, 2 * per_layer] and info["n_components_kept"] == 1
    assert (ref.unpack_key(wm.extract()["keys"])[:, 2] == 0).all()              # the layer z = 0 holds the smallest key
    wm.close()


# ---- 5. one giant component, and the sparse scene of the layout cases ----
def test_one_giant_component(ctx):
    wm, rm = device_map(ctx, lc.LEAF, lc.dense_calls(), lc.BIG_LOG2), lc.dense_reference()
    assert wm.info()["occupied"] == lc.DENSE_CELLS and wm.info()["growths"] == 0
    for conn in cref.CONNECTIVITIES:
        info = wm.components(connectivity=conn)
        assert info == dict(n_cells=lc.DENSE_CELLS, n_unlabelled=0, n_components=1, n_singletons=0, largest_label=int(rm.keys.min()),
                            largest_cells=lc.DENSE_CELLS, largest_points=lc.DENSE_CELLS), (conn, info)
        lst = wm.listComponents()
        assert lst["labels"].tolist() == [int(rm.keys.min())] and lst["cells"].tolist() == [lc.DENSE_CELLS]
    rows = wm.fetchComponents()
    assert np.array_equal(rows["keys"], rm.keys) and (rows["labels"] == rm.keys.min()).all()
    info = wm.selectComponents(min_cells=lc.DENSE_CELLS + 1)
    assert info["n_removed"] == [0, lc.DENSE_CELLS, 0, 0] and info["n_components_kept"] == 0
    wm.close()


def test_sparse_scene_in_a_table_of_two_rounds(ctx):
    wm, rm = device_map(ctx, lc.LEAF, lc.sparse_calls(), lc.BIG_LOG2), lc.sparse_reference()
    low, high = lc.halves(rm.keys)
    assert low.sum() >= 100 and high.sum() >= 100
    for conn in cref.CONNECTIVITIES:
        for flt in ((1, 1), (2, 3)):
            info = check_components(wm, cref.components(rm, *flt, conn), conn)
            assert info["n_components"] >= 2
    comp = cref.components(rm, 2, 2, 124)
    check_components(wm, comp, 124)
    check_select(wm, rm, comp, min_cells=3, min_component_points=10, keep_largest=5)
    check_prune(wm, lc.fresh(rm), comp, min_cells=3, min_component_points=10, keep_largest=5)
    wm.close()


# ---- 6. across the table's end ----
@pytest.mark.parametrize("name", list(lc.CHAINS))
def test_chains_across_the_tables_end(ctx, name):
    ch = lc.chain(name)
    calls = [ch["first"], ch["again"]]
    rm = lc.chain_reference(name)
    wm, twice = device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"]), device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"] + 1)
    assert wm.info()["capacity"] == ch["capacity"] and twice.info()["capacity"] == 2 * ch["capacity"]
    for conn in cref.CONNECTIVITIES:
        comp = cref.components(rm, connectivity=conn)
        a, b = check_components(wm, comp, conn), check_components(twice, comp, conn)
        assert a == b and a["n_components"] >= 2
    comp = cref.components(rm, connectivity=26)
    check_components(wm, comp, 26)
    check_select(wm, rm, comp, min_cells=2)
    check_prune(wm, lc.fresh(rm), comp, min_cells=2)
    wm.close()
    twice.close()


# ---- 7. select and prune ----
def test_select_and_prune(ctx):
    calls = pref.scene_calls()
    wm, rm = device_map(ctx, pref.LEAF, calls), copy.deepcopy(cref.scene_reference())
    comp = cref.scene_components(2, 1, 26)
    check_components(wm, comp, 26)
    for sel in (dict(), dict(min_cells=2), dict(min_cells=5), dict(min_component_points=4), dict(min_component_points=2 ** 40),
                dict(keep_largest=1), dict(keep_largest=4), dict(keep_largest=16), dict(min_cells=0, min_component_points=0), SCENE_SELECTION,
                dict(min_cells=3, keep_largest=2, shrink=True)):
        check_select(wm, rm, comp, **sel)
    wm.render(E.pose_matrix([0, 0, 2.0, 0, 0, 0, 1]), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 6.0)
    wm.compare(wm, 0.05, distances=True)
    wm.classifyPrune(min_points=2)
    wm.alignStep(wm, 0.05)
    check_stamps(wm, rm)
    check_components(wm, comp, 26)
    grown = wm.info()["capacity"]
    info = check_prune(wm, rm, comp, shrink=True, **SCENE_SELECTION)
    assert info["capacity"] == pref.shrunk_capacity(info["n_kept"]) < grown
    assert refused(wm.fetchRender) and refused(wm.fetchDistances) and refused(wm.fetchPruneReasons) and refused(wm.fetchAlignment)
    check_stamps(wm, rm)                                                       # every kept cell moved with its stamp
    # ages go on counting, and a removed cell that a later call reaches starts from zero
    pts = calls[0][0]
    assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY)
    ref.assert_maps_equal(wm.extract(), rm.extract())
    assert wm.info()["calls"] == rm.calls == 9
    check_stamps(wm, rm)
    # without shrink the capacity stays; the tie of the selection's hand cases on the device
    comp = cref.components(rm, connectivity=6)
    check_components(wm, comp, 6)
    check_prune(wm, rm, comp, min_cells=2)
    wm.close()


@pytest.mark.parametrize("case", cref.selection_hand_cases(), ids=lambda c: c["name"])
def test_selection_hand_cases(ctx, case):
    calls = cref.selection_case_calls(case)
    wm, rm = device_map(ctx, cref.PAIR_LEAF, calls, 8), cref.map_of(calls, cref.PAIR_LEAF)
    comp = cref.components(rm, connectivity=26)
    check_components(wm, comp, 26)
    check_select(wm, rm, comp, **case["sel"])
    labels = [int(ref.pack_key(np.asarray(c)).min()) for c in case["comps"]]
    rows = wm.fetchComponents()
    assert sorted(np.unique(rows["labels"][rows["reason"] == 0]).tolist()) == sorted(labels[i] for i in case["want_kept"])
    check_prune(wm, rm, comp, **case["sel"])
    kept = np.concatenate([np.asarray(case["comps"][i]) for i in case["want_kept"]])
    assert np.array_equal(wm.extract()["keys"], np.sort(ref.pack_key(kept)))
    wm.close()


# ---- 8. invalidation and refusals ----
def test_invalidation_and_refusals(ctx):
    calls = pref.scene_calls()
    wm, other = device_map(ctx, pref.LEAF, calls), device_map(ctx, pref.LEAF, calls[:2])
    readers = (wm.fetchComponents, wm.listComponents, wm.selectComponents, wm.pruneComponents)
    state = other.exportState()

    def all_refused():
        return all(refused(fn, "labelling") for fn in readers)
    assert all_refused()                                                       # before components
    for change in (lambda: wm.integrate(calls[0][0], IDENTITY), lambda: wm.integrate(np.zeros((0, 3), np.float32), IDENTITY),
                   lambda: wm.merge(other), lambda: wm.importState(state), lambda: wm.prune(min_points=2), wm.reset):
        wm.components()
        wm.selectComponents()
        assert len(wm.listComponents()["labels"]) == wm.components()["n_components"]
        change()
        assert all_refused()
    # an empty table: all zero, nothing to fetch
    info = wm.components()
    assert info == dict.fromkeys(info, 0) and len(info) == 7
    assert all(len(v) == 0 for v in wm.fetchComponents().values()) and all(len(v) == 0 for v in wm.listComponents().values())
    sel = wm.selectComponents(keep_largest=3)
    assert sel["n_cells"] == sel["n_kept"] == sel["n_components_kept"] == 0 and sel["n_removed"] == [0] * 4
    assert wm.pruneComponents(shrink=True)["capacity"] == 256 and all_refused()
    # reasons before a select, and the capacity protocol
    for pts, T in calls[:3]:
        wm.integrate(pts, T)
    L = d.load_library()
    m = wm.components(2, 1, 26)["n_cells"]
    keys, labels, reasons, n = np.full(m, 99, np.uint64), np.full(m, 98, np.uint64), np.full(m, 77, np.uint8), C.c_size_t()
    kp, lp, rp = (a.ctypes.data_as(C.POINTER(t)) for a, t in ((keys, C.c_uint64), (labels, C.c_uint64), (reasons, C.c_uint8)))
    assert L.dsx_map_components_fetch(wm._h, kp, lp, rp, m, C.byref(n)) == E.ERR_INVALID and b"select" in L.dsi_last_error()
    assert (reasons == 77).all() and (keys == 99).all()
    assert L.dsx_map_components_fetch(wm._h, kp, lp, None, m - 1, C.byref(n)) == E.ERR_INVALID and n.value == m and (keys == 99).all()
    wm.selectComponents(min_cells=2)
    assert L.dsx_map_components_fetch(wm._h, None, None, rp, m, C.byref(n)) == E.OK and n.value == m    # an output may be NULL
    assert set(np.unique(reasons).tolist()) <= {0, 2} and (keys == 99).all()
    count = wm.components(2, 1, 26)["n_components"]                            # a new labelling: the selection is gone with the old one
    assert L.dsx_map_components_fetch(wm._h, kp, lp, rp, m, C.byref(n)) == E.ERR_INVALID
    cells = np.full(count, 55, np.uint64)
    cp = cells.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.dsx_map_components_list(wm._h, None, cp, None, count - 1, C.byref(n)) == E.ERR_INVALID and n.value == count and (cells == 55).all()
    assert L.dsx_map_components_list(wm._h, None, cp, None, count, C.byref(n)) == E.OK and int(cells.sum()) == m
    with pytest.raises(d.DsiError):
        wm.components(connectivity=7)
    with pytest.raises(d.DsiError):
        wm.pruneComponents(keep_largest=17)
    assert len(wm.listComponents()["labels"]) == count                         # a refused call leaves the labelling valid
    wm.close()
    other.close()


# ---- 9. the stream ----
def test_components_through_full_sequence(ctx):
    """full_sequence(..., world_map=, world_map_components=) with every=2: the final map equals the restatement driven by the
    clouds the stream returned, through the same poses and the same prunes; None leaves the run as it is."""
    n_win, dur, t0 = 4, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    kw = dict(options_depth_map=d.OptionsDepthMap(), options_point_cloud=d.OptionsPointCloud(2.0, 1))
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    bare_map, plain_map, wm = d.WorldMap(ctx, 0.5, 8), d.WorldMap(ctx, 0.5, 8), d.WorldMap(ctx, 0.5, 8)
    bare = list(proc.full_sequence(*args, world_map=bare_map, **kw))
    plain = list(proc.full_sequence(*args, world_map=plain_map, world_map_components=None, **kw))
    opts = {"every": 2, "min_cells": 3}
    on = list(proc.full_sequence(*args, world_map=wm, world_map_components=opts, **kw))
    assert len(on) == len(plain) == len(bare) == n_win
    poses = [d.invert_pose(proc.reference_view_process1(rig["trajectories"][0], w[0])) for w in plain]
    rm, whole = pref.PruneReferenceMap(0.5), pref.PruneReferenceMap(0.5)
    for k, (a, b, c) in enumerate(zip(on, plain, bare)):
        assert len(b) == len(c) == 5 and len(a) == (6 if k % 2 else 5) and a[0] == b[0] == c[0]
        for x, y, z in zip(a[1:5], b[1:], c[1:]):
            assert x.dtype == y.dtype == z.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
            assert np.array_equal(y.view(np.uint8), z.view(np.uint8))
        rm.integrate(a[4], poses[k])
        whole.integrate(b[4], poses[k])
        if k % 2:
            comp = cref.components(rm)
            want = cref.prune_components(rm, comp, min_cells=3)
            got = a[5]["world_map_components"]
            print("window %d: %s" % (k, got))
            assert {key: got[key] for key in comp["info"]} == comp["info"]
            pruned = got["prune"]
            assert (pruned["n_cells"], pruned["n_kept"], pruned["n_removed"], pruned["n_components_kept"]) == \
                (want["n_cells"], want["n_kept"], want["n_removed"], want["n_components_kept"])
            assert pruned["n_kept"] >= 1 and pruned["n_removed"][1] >= 1 and pruned["n_removed"][0] == pruned["n_removed"][2] == 0
    ref.assert_maps_equal(wm.extract(), rm.extract())
    ref.assert_maps_equal(plain_map.extract(), whole.extract())
    ref.assert_maps_equal(bare_map.extract(), whole.extract())
    assert wm.info()["calls"] == plain_map.info()["calls"] == n_win and wm.info()["occupied"] < plain_map.info()["occupied"]
    # with both keywords the prune runs first
    both_map, rb = d.WorldMap(ctx, 0.5, 8), pref.PruneReferenceMap(0.5)
    both = list(proc.full_sequence(*args, world_map=both_map, world_map_prune={"every": 2, "min_points": 2}, world_map_components=opts, **kw))
    for k, a in enumerate(both):
        rb.integrate(a[4], poses[k])
        if k % 2:
            assert len(a) == 7 and "world_map_prune" in a[5] and "world_map_components" in a[6]
            first = rb.prune(min_points=2)
            assert a[5]["world_map_prune"]["n_removed"] == first["n_removed"]
            comp = cref.components(rb)
            assert {key: a[6]["world_map_components"][key] for key in comp["info"]} == comp["info"]
            cref.prune_components(rb, comp, min_cells=3)
    ref.assert_maps_equal(both_map.extract(), rb.extract())
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map_components=opts, **kw))        # no map to label
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map=wm, world_map_components=dict(opts, every=0), **kw))
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map=wm, world_map_components=dict(opts, reach=1), **kw))
    for m in (bare_map, plain_map, wm, both_map):
        m.close()
