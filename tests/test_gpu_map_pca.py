"""The world map's local shape on the GPU (include/dsi_map_pca.h; DESIGN.md 7j "Local shape") against the numpy restatement
tests/map_pca_reference.py: array_equal on keys, members, the nine integer moments, labels, flags, the float bits of normals,
tangents and eigenvalues, every counter, the reasons and the pruned map's exact state.  tests/test_map_pca_cpu.py proves the
restatement against brute force and the solver against numpy.linalg.eigh."""
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_knn_reference as kref
import map_layout_cases as lc
import map_merge_reference as mref
import map_pca_reference as pr
import map_prune_reference as pref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, io as dio, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = pref.IDENTITY
COUNTERS = ("calls", "accepted", "rejected", "growths")
KEEPS = tuple(range(1, 8))


def device_map(ctx, leaf, calls, capacity_log2=10):
    wm = d.WorldMap(ctx, leaf, capacity_log2)
    for pts, T in calls:
        wm.integrate(pts, T)
    return wm


def refused(fn, word=None):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code == E.ERR_INVALID and (word is None or word in str(e.value))


def check_pass(wm, want, k, radius, min_found=2, orient=False, **flt):
    """the pass equals the restatement's: counts and rows; every solved row's bits come back from engine.pca_solve of its
    fetched moments; the map is untouched"""
    before = wm.info()
    info = wm.pca(k, radius, min_found, orient, pr.VIEWPOINT if orient else None, keep_moments=True, **flt)
    rows = wm.fetchPca(sort=True)
    assert set(rows) == {"keys", "normal", "tangent", "eval", "members", "label", "flags", "moments"}
    pr.assert_passes_equal(info, rows, want)
    assert wm.info() == before
    return rows


def check_rows_from_moments(rows, xyz, leaf, orient):
    quantum = float(pr.quantum_of(leaf))
    for i in np.flatnonzero(rows["label"] > 0):
        got = E.pca_solve(int(rows["members"][i]), rows["moments"][i, :3], rows["moments"][i, 3:], quantum, orient,
                          pr.VIEWPOINT if orient else None, xyz[i].astype(np.float64) if orient else None)
        assert got["label"] == rows["label"][i] and got["flags"] == rows["flags"][i], i
        for f in ("normal", "tangent", "eval"):
            assert np.array_equal(pr.bits(got[f]), pr.bits(rows[f][i])), (f, i)


def check_select(wm, rm, sp, keep, remove_sparse):
    before = wm.info()
    info, want = wm.selectShapes(keep, remove_sparse), pr.select(rm, sp, keep, remove_sparse)
    for f in ("n_cells", "n_kept", "n_removed"):
        assert info[f] == want[f], (f, info[f], want[f])
    assert info["capacity"] == before["capacity"] and wm.info() == before
    rows = wm.fetchPca(sort=True)
    assert rows["reason"].dtype == np.uint8 and np.array_equal(rows["keys"], sp["keys"]) and np.array_equal(rows["reason"], want["reason"])
    return info


def check_prune(wm, rm, sp, keep, remove_sparse, shrink=False):
    """the prune equals the restatement's: counts, the map's exact state and its counters; the pass is refused after"""
    before = wm.info()
    info = wm.pruneShapes(keep, remove_sparse, shrink=shrink)
    want = rm.prune_shapes(sp, keep, remove_sparse)
    for f in ("n_cells", "n_kept", "n_removed"):
        assert info[f] == want[f], (f, info[f], want[f])
    assert info["n_cells"] == before["occupied"] == info["n_kept"] + sum(info["n_removed"])
    after = wm.info()
    assert after["occupied"] == info["n_kept"] == len(rm.keys) and all(after[k] == before[k] for k in COUNTERS)
    assert info["capacity"] == after["capacity"] == (pref.shrunk_capacity(info["n_kept"]) if shrink else before["capacity"])
    mref.assert_states_equal(wm.exportState(), rm.export_state())
    for fn in (wm.fetchPca, wm.selectShapes, wm.pruneShapes):
        assert refused(fn, "local-shape pass")
    return info


# ---- 1. exact shapes, without the restatement ----
def row_of(rows, c):
    i = np.flatnonzero(rows["keys"] == np.uint64(pr.centre_key(c)))
    assert len(i) == 1
    return {f: v[i[0]] for f, v in rows.items()}


def test_exact_sheet(ctx):
    wm = device_map(ctx, pr.SHAPE_LEAF, pr.block_calls(9, 9, 1), 8)
    radius = 1.5 * pr.SHAPE_LEAF                                                # the eight cells around an interior one
    info = wm.pca(0, radius, keep_moments=True)
    rows = wm.fetchPca()
    assert info["n_cells"] == 81 and info["reach"] == 2 and info["n_sparse"] == 0
    cz = int(ref.unpack_key(rows["keys"][:1])[0, 2])
    interior = [(x, y, cz) for x in range(-3, 4) for y in range(-3, 4)]
    for c in interior:
        r = row_of(rows, c)
        assert r["label"] == 2 and r["members"] == 9 and r["flags"] == 1       # planar; lambda1 == lambda2 exactly: no tangent
        assert r["normal"].tolist() == [0.0, 0.0, 1.0] and r["eval"][0] == 0.0 and r["eval"][1] == r["eval"][2] > 0
        assert r["moments"].tolist() == [0, 0, 0, 6 << 20, 0, 0, 6 << 20, 0, 0]
    below = wm.pca(0, radius, orient=True, viewpoint=(0.0, 0.0, -10.0))
    assert below == info
    rows = wm.fetchPca()
    for c in interior:
        assert row_of(rows, c)["normal"].tolist() == [0.0, 0.0, -1.0]
    wm.pca(0, radius, orient=True, viewpoint=(0.0, 0.0, 10.0))
    assert row_of(wm.fetchPca(), interior[0])["normal"].tolist() == [0.0, 0.0, 1.0]
    wm.pca(4, radius, min_found=4)                                              # the four face neighbours
    r = row_of(wm.fetchPca(), interior[5])
    assert r["label"] == 2 and r["members"] == 5 and r["normal"].tolist() == [0.0, 0.0, 1.0]
    wm.close()


def test_exact_row_block_and_lone_cell(ctx):
    wm = device_map(ctx, pr.SHAPE_LEAF, pr.block_calls(1, 1, 9), 8)
    info = wm.pca(0, 1.5 * pr.SHAPE_LEAF)
    rows = wm.fetchPca()
    assert info["n_cells"] == 9 and info["n_label"] == [7, 0, 0] and info["n_sparse"] == 2     # the two ends have one neighbour
    cx, cy = (int(v) for v in ref.unpack_key(rows["keys"][:1])[0, :2])
    for z in range(-3, 4):
        r = row_of(rows, (cx, cy, z))
        assert r["label"] == 1 and r["flags"] == 2 and r["tangent"].tolist() == [0.0, 0.0, 1.0]  # linear; no normal
        assert r["eval"][0] == r["eval"][1] == 0.0 and r["members"] == 3
    end = row_of(rows, (cx, cy, 4))
    assert end["label"] == 0 and end["flags"] == 0 and end["members"] == 2 and not end["normal"].any() and not end["tangent"].any()
    assert np.isposinf(end["eval"]).all()
    wm.close()
    wm = device_map(ctx, pr.SHAPE_LEAF, pr.block_calls(5, 5, 5), 8)
    info = wm.pca(0, 1.8 * pr.SHAPE_LEAF, keep_moments=True)
    rows = wm.fetchPca()
    centre = row_of(rows, (0, 0, 0))
    # 26 neighbours, symmetric: the off-diagonals are exact zeros, every rotation is skipped and V stays the identity
    assert centre["members"] == 27 and centre["label"] == 3 and centre["flags"] == 0
    assert centre["normal"].tolist() == [1.0, 0.0, 0.0] and centre["tangent"].tolist() == [0.0, 1.0, 0.0]
    assert centre["moments"].tolist() == [0, 0, 0, 18 << 20, 0, 0, 18 << 20, 0, 18 << 20]
    assert centre["eval"][0] == centre["eval"][1] == centre["eval"][2] == np.float32((18.0 / 27.0) * 0.25)
    wm.close()
    wm = device_map(ctx, pr.SHAPE_LEAF, pr.block_calls(1, 1, 1), 8)
    info = wm.pca(8, 1.0)
    assert info == dict(info, n_cells=1, n_sparse=1, n_label=[0, 0, 0], sum_members=1, n_normal_determined=0, n_tangent_determined=0)
    wm.close()


# ---- 2. jittered scenes: every reach, every instantiation ----
@pytest.fixture(scope="module")
def scene(ctx):
    wm = device_map(ctx, pr.LEAF, pr.scene_calls())
    yield wm, pr.scene_reference()
    wm.close()


@pytest.mark.parametrize("radius", pr.RADII)
def test_scene_equals_the_restatement(scene, radius):
    wm, rm = scene
    assert np.array_equal(wm.extract()["keys"], rm.keys) and 1800 <= len(rm.keys) <= 2400
    for k in pr.KS:
        orient = k in (0, 5)
        want = pr.scene_pass(k, radius, 2, orient)
        assert want["reach"] == pr.RADII.index(radius) + 1
        rows = check_pass(wm, want, k, radius, 2, orient)
        check_rows_from_moments(rows, want["xyz"], pr.LEAF, orient)
    want = pr.scene_pass(8, radius, 8)                                          # min_found at its top
    check_pass(wm, want, 8, radius, 8)
    for k in (2, 4):                                                            # the instantiations that pr.KS leaves out
        check_pass(wm, pr.scene_pass(k, radius), k, radius)


# ---- 3. the knn lattice: equal distances, the key decides the members ----
def test_lattice_ties_show_in_the_moments(ctx):
    calls = kref.lattice_calls()
    wm, rm = device_map(ctx, kref.LEAF, calls, 12), pr.reference_of(calls, kref.LEAF)
    for k, radius in ((1, 0.05), (3, 0.05), (5, 0.05), (3, 0.1), (8, 0.15)):   # below the six (and eighteen) equidistant neighbours
        want = pr.shape_pass(rm, k, radius)
        rows = check_pass(wm, want, k, radius)
        full = want["found"] == k
        assert full.sum() >= 300 and (np.abs(rows["moments"][full][:, :3]).sum(axis=1) > 0).sum() >= 300    # a cut through a tie is lopsided
    wm.close()


# ---- 4. filters; table size and call order ----
def test_filters_and_table_and_order_freedom(scene, ctx):
    wm, rm = scene
    for flt in (dict(min_windows=2), dict(min_points=2), dict(min_points=2, min_windows=2)):
        want = pr.shape_pass(rm, 8, 0.1, **flt)
        assert want["n_unqueried"] >= 100 and want["n_cells"] >= 100
        check_pass(wm, want, 8, 0.1, **flt)
    calls = pr.scene_calls()
    pts = np.concatenate([p for p, _ in calls])
    rng = np.random.default_rng(73)
    shuffled = pr.reference_of([(pts[rng.permutation(len(pts))], IDENTITY)], pr.LEAF)   # one window: the same cells, another order
    want0, want8 = pr.shape_pass(shuffled, 0, 0.15), pr.shape_pass(shuffled, 8, 0.1)
    got = []
    for log2 in (8, 14):
        m = d.WorldMap(ctx, pr.LEAF, log2)
        for part in np.array_split(pts[rng.permutation(len(pts))], 5):
            m.integrate(part, IDENTITY)
        assert (m.info()["growths"] > 0) == (log2 == 8)
        got.append((check_pass(m, want0, 0, 0.15), check_pass(m, want8, 8, 0.1)))
        m.close()
    for a, b in zip(got[0], got[1]):
        assert all(np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)) for f in a)


# ---- 5. layouts: more slots than one stride, and a chain across the table's end ----
def test_dense_scene_in_a_table_of_two_rounds(ctx):
    wm, rm = device_map(ctx, lc.LEAF, lc.dense_calls(), lc.BIG_LOG2), lc.dense_reference()
    assert wm.info()["capacity"] == 1 << lc.BIG_LOG2
    want = pr.dense_pass()
    info = wm.pca(pr.DENSE_K, pr.DENSE_RADIUS, keep_moments=True)
    rows = wm.fetchPca(sort=True)
    pr.assert_passes_equal(info, rows, want)
    sel, want_sel = wm.selectShapes(("planar",), True), pr.select(rm, want, ("planar",), True)
    assert all(sel[f] == want_sel[f] for f in ("n_cells", "n_kept", "n_removed"))
    assert np.array_equal(wm.fetchPca(sort=True)["reason"], want_sel["reason"])
    wm.close()


@pytest.mark.parametrize("name", list(lc.CHAINS))
def test_chains_across_the_tables_end(ctx, name):
    ch = lc.chain(name)
    calls = [ch["first"], ch["again"]]
    rm = pr.reference_of(calls, lc.CHAIN_LEAF)
    wm, twice = device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"]), device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"] + 1)
    assert wm.info()["capacity"] == ch["capacity"] and twice.info()["capacity"] == 2 * ch["capacity"]
    for k in (0, 4):
        want = pr.shape_pass(rm, k, lc.CHAIN_RADIUS)
        for m in (wm, twice):
            check_pass(m, want, k, lc.CHAIN_RADIUS)
            check_select(m, rm, want, ("linear",), True)
    check_prune(wm, rm, want, ("linear",), True)
    wm.close()
    twice.close()


# ---- 6. select and prune ----
def test_every_mask_selects_as_the_restatement(scene):
    wm, rm = scene
    want = pr.scene_pass(8, 0.1, 4)
    assert want["n_sparse"] >= 20 and min(want["n_label"]) >= 20
    check_pass(wm, want, 8, 0.1, 4)
    for keep in KEEPS:
        for remove_sparse in (True, False):
            check_select(wm, rm, want, keep, remove_sparse)
    assert wm.selectShapes() == wm.selectShapes(("planar", "linear"), True) == wm.selectShapes(3, True)
    two = pr.shape_pass(rm, 8, 0.1, 4, min_windows=2)                           # reason 1 too
    check_pass(wm, two, 8, 0.1, 4, min_windows=2)
    info = check_select(wm, rm, two, ("linear", "planar"), True)
    assert min(info["n_removed"]) >= 5


@pytest.mark.parametrize("shrink", (False, True))
def test_prune_equals_the_restatement_bit_for_bit(ctx, shrink):
    calls = pr.scene_calls()
    wm, rm = device_map(ctx, pr.LEAF, calls), pr.reference_of(calls, pr.LEAF)
    grown = wm.info()["capacity"]
    want = pr.shape_pass(rm, 8, 0.1, 4, min_windows=2)
    check_pass(wm, want, 8, 0.1, 4, min_windows=2)
    info = check_prune(wm, rm, want, ("linear", "planar"), True, shrink)
    assert min(info["n_removed"]) >= 5 and (info["capacity"] < grown) == shrink
    # the kept cells moved with n, S, windows and stamp; the map goes on: integrate, analyse again, prune again
    assert wm.integrate(calls[0][0], IDENTITY) == rm.integrate(calls[0][0], IDENTITY)
    mref.assert_states_equal(wm.exportState(), rm.export_state())
    want = pr.shape_pass(rm, 0, 0.1, 3)
    check_pass(wm, want, 0, 0.1, 3)
    check_prune(wm, rm, want, ("scattered",), False, shrink)
    want = pr.shape_pass(rm, 4, 0.15)
    check_pass(wm, want, 4, 0.15)
    if want["n_sparse"] == 0:                                                   # a prune that removes nothing leaves the table as it is
        before = wm.info()
        check_prune(wm, rm, want, 7, True)
        assert wm.info() == before
    wm.close()


def test_invalidation_and_refusals(ctx):
    calls = pr.scene_calls()
    wm, other = device_map(ctx, pr.LEAF, calls), device_map(ctx, pr.LEAF, calls[:2])
    readers = (wm.fetchPca, wm.selectShapes, wm.pruneShapes)
    state = other.exportState()

    def all_refused():
        return all(refused(fn, "local-shape pass") for fn in readers)
    assert all_refused()                                                       # before pca
    for change in (lambda: wm.integrate(calls[0][0], IDENTITY), lambda: wm.integrate(np.zeros((0, 3), np.float32), IDENTITY),
                   lambda: wm.merge(other), lambda: wm.importState(state), lambda: wm.prune(min_points=2),
                   lambda: (wm.components(), wm.pruneComponents(min_cells=2)), lambda: (wm.knn(4, 0.1), wm.pruneOutliers(1.0)),
                   lambda: wm.pruneShapes(7, False), wm.reset):
        wm.pca(4, 0.1)
        wm.selectShapes()
        assert "reason" in wm.fetchPca()
        change()
        assert all_refused()
    # pca leaves a render, a compare, a classification, an alignment step, a labelling and a self query valid
    for pts, T in calls:
        wm.integrate(pts, T)
    rm = pr.reference_of(calls, pr.LEAF)
    wm.render(E.pose_matrix([0, 0, -2.0, 0, 0, 0, 1]), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 6.0)
    wm.compare(wm, 0.05, distances=True)
    wm.classifyPrune(min_points=2)
    wm.alignStep(wm, 0.05)
    wm.components()
    wm.knn(4, 0.1)
    check_pass(wm, pr.shape_pass(rm, 4, 0.1), 4, 0.1)
    wm.selectShapes()
    for fetch in (wm.fetchRender, wm.fetchDistances, wm.fetchPruneReasons, wm.fetchAlignment, wm.fetchComponents, wm.fetchKnn, wm.fetchPca):
        fetch()
    # moments without keep_moments, reasons before a select, the capacity protocol, and NULL outputs
    L = d.load_library()
    m = wm.pca(4, 0.1, min_windows=2)["n_cells"]
    assert "moments" not in wm.fetchPca()
    keys, label, reasons, mom, n = np.full(m, 99, np.uint64), np.full(m, 98, np.uint8), np.full(m, 77, np.uint8), np.zeros((m, 9), np.int64), C.c_size_t()
    kp, lp, rp = (a.ctypes.data_as(C.POINTER(t)) for a, t in ((keys, C.c_uint64), (label, C.c_uint8), (reasons, C.c_uint8)))
    mp = mom.ctypes.data_as(C.POINTER(C.c_int64))
    none = (None,) * 4
    assert L.dsx_map_pca_fetch(wm._h, kp, *none, lp, None, mp, None, m, C.byref(n)) == E.ERR_INVALID and b"keep_moments" in L.dsi_last_error()
    assert L.dsx_map_pca_fetch(wm._h, kp, *none, lp, None, None, rp, m, C.byref(n)) == E.ERR_INVALID and b"select" in L.dsi_last_error()
    assert (reasons == 77).all() and (keys == 99).all()
    assert L.dsx_map_pca_fetch(wm._h, kp, *none, lp, None, None, None, m - 1, C.byref(n)) == E.ERR_INVALID and n.value == m and (keys == 99).all()
    wm.selectShapes()
    assert L.dsx_map_pca_fetch(wm._h, None, *none, None, None, None, rp, m, C.byref(n)) == E.OK and n.value == m
    assert set(np.unique(reasons).tolist()) <= {0, 2, 3} and (keys == 99).all()
    wm.pca(4, 0.1)                                                              # a new pass: the selection is gone with the old one
    assert L.dsx_map_pca_fetch(wm._h, kp, *none, lp, None, None, rp, m, C.byref(n)) == E.ERR_INVALID
    for bad in (lambda: wm.pca(17, 0.1), lambda: wm.pca(4, 0.1, min_found=5), lambda: wm.pca(4, 0.1, min_found=1),
                lambda: wm.pca(0, 0.1, min_found=343), lambda: wm.pca(4, 0.1, orient=True, viewpoint=(0, float("nan"), 0)),
                lambda: wm.pca(4, 4 * pr.LEAF), lambda: wm.pruneShapes(0), lambda: wm.pruneShapes(8)):
        with pytest.raises(d.DsiError):
            bad()
    assert wm.pca(0, 0.15, min_found=342)["reach"] == 3
    assert len(wm.fetchPca()["keys"]) == wm.count()
    wm.close()
    other.close()


# ---- 7. edge cases ----
def test_edge_cases(ctx):
    wm = d.WorldMap(ctx, pr.LEAF, 8)
    info = wm.pca(4, 0.1)                                                       # an empty map
    assert info == dict(info, n_cells=0, n_unqueried=0, n_sparse=0, n_label=[0, 0, 0], sum_members=0, reach=2)
    assert all(len(v) == 0 for v in wm.fetchPca().values())
    sel = wm.selectShapes()
    assert sel["n_cells"] == sel["n_kept"] == 0 and wm.pruneShapes()["n_kept"] == 0
    rng = np.random.default_rng(74)
    crowd = (rng.uniform(0.001, 0.049, (70_000, 3))).astype(np.float32)        # 70,000 points in one cell: one member, sparse
    wm.integrate(crowd, IDENTITY)
    rm = pr.reference_of([(crowd, IDENTITY)], pr.LEAF)
    assert wm.info()["occupied"] == 1
    rows = check_pass(wm, pr.shape_pass(rm, 4, 0.1), 4, 0.1)
    assert rows["members"].tolist() == [1] and rows["label"].tolist() == [0]
    filtered = wm.pca(4, 0.1, min_windows=2)                                    # every cell fails the filter
    assert filtered["n_cells"] == 0 and filtered["n_unqueried"] == 1 and len(wm.fetchPca()["keys"]) == 0
    assert wm.selectShapes()["n_removed"] == [1, 0, 0]
    assert wm.pruneShapes(shrink=True) == {"n_cells": 1, "n_kept": 0, "n_removed": [1, 0, 0], "capacity": 256}
    wm.close()
    calls = kref.edge_calls()                                                   # cells at |c| = 2^20 - 2: offsets that leave the key range are skipped
    wm, rm = device_map(ctx, kref.EDGE_LEAF, calls, 8), pr.reference_of(calls, kref.EDGE_LEAF)
    for k, radius in ((0, 1.2), (4, 1.2), (16, 1.5)):
        want = pr.shape_pass(rm, k, radius)
        assert want["members"].tolist() == [3] * 9
        check_pass(wm, want, k, radius)
    wm.close()


# ---- 8. the stream (the C++ adapter: tests/test_gpu_map_pca_cpp.py) ----
def test_shapes_through_full_sequence(ctx):
    """full_sequence(..., world_map=, world_map_shapes=) with every=2 equals the same calls made by hand on a second map, fed
    with the clouds the stream returned; None leaves the run as it is."""
    n_win, dur, t0 = 4, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    kw = dict(options_depth_map=d.OptionsDepthMap(), options_point_cloud=d.OptionsPointCloud(2.0, 1))
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    plain_map, wm, hand = (d.WorldMap(ctx, 0.5, 8) for _ in range(3))
    plain = list(proc.full_sequence(*args, world_map=plain_map, world_map_shapes=None, **kw))
    opts = {"every": 2, "k": 0, "radius": 1.5, "min_found": 3, "keep": ("linear", "planar"), "remove_sparse": True, "shrink": True}
    on = list(proc.full_sequence(*args, world_map=wm, world_map_shapes=opts, **kw))
    assert len(on) == len(plain) == n_win
    poses = [d.invert_pose(proc.reference_view_process1(rig["trajectories"][0], w[0])) for w in plain]
    for k, (a, b) in enumerate(zip(on, plain)):
        assert len(b) == 5 and len(a) == (6 if k % 2 else 5) and a[0] == b[0]
        for x, y in zip(a[1:5], b[1:]):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        hand.integrate(a[4], poses[k])
        if k % 2:
            counts = hand.pca(0, 1.5, 3)
            counts["prune"] = hand.pruneShapes(("linear", "planar"), True, shrink=True)
            print("window %d: %s" % (k, counts))
            assert a[5] == {"world_map_shapes": counts}
            assert counts["prune"]["n_kept"] >= 1 and sum(counts["prune"]["n_removed"]) >= 1
    mref.assert_states_equal(wm.exportState(), hand.exportState())
    assert wm.info() == hand.info() and wm.info()["occupied"] < plain_map.info()["occupied"]
    # after world_map_outliers=, on the same window
    both_map, by_hand = d.WorldMap(ctx, 0.5, 8), d.WorldMap(ctx, 0.5, 8)
    outl = {"every": 2, "k": 4, "radius": 1.0, "min_found": 2, "std_mult": 2.0}
    both = list(proc.full_sequence(*args, world_map=both_map, world_map_outliers=outl, world_map_shapes=opts, **kw))
    for k, a in enumerate(both):
        by_hand.integrate(a[4], poses[k])
        if k % 2:
            assert len(a) == 7 and "world_map_outliers" in a[5] and "world_map_shapes" in a[6]
            by_hand.knn(4, 1.0, 2)
            by_hand.pruneOutliers(2.0)
            counts = by_hand.pca(0, 1.5, 3)
            counts["prune"] = by_hand.pruneShapes(("linear", "planar"), True, shrink=True)
            assert a[6]["world_map_shapes"] == counts
    mref.assert_states_equal(both_map.exportState(), by_hand.exportState())
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map_shapes=opts, **kw))            # no map to analyse
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map=wm, world_map_shapes=dict(opts, keep=()), **kw))
    for m in (plain_map, wm, hand, both_map, by_hand):
        m.close()


# ---- 9. the PCD file with normals ----
def test_pcd_with_normals_round_trips(scene, tmp_path):
    wm, rm = scene
    wm.pca(0, 0.15, orient=True, viewpoint=pr.VIEWPOINT)
    rows, cells = wm.fetchPca(), wm.extract(sort=False)
    assert np.array_equal(rows["keys"], cells["keys"])                          # fetchPca's order is extract's
    curvature = dio.pcd_curvature(rows["eval"])
    e = rows["eval"].astype(np.float64)
    solved = rows["label"] > 0
    assert solved.sum() >= 1000
    assert np.array_equal(curvature[solved], e[solved, 0] / ((e[solved, 0] + e[solved, 1]) + e[solved, 2]))
    assert np.isnan(curvature[~solved]).all() and (curvature[solved] >= 0).all() and (curvature[solved] < 0.34).all()
    path = str(tmp_path / "cloud.pcd")
    assert dio.save_pcd_normals_ascii(path, cells["xyz"], rows["normal"], curvature) == len(rows["keys"])
    back = dio.load_pcd_normals_ascii(path)
    assert np.array_equal(pr.bits(back["points"]), pr.bits(cells["xyz"])) and np.array_equal(pr.bits(back["normals"]), pr.bits(rows["normal"]))
    assert np.array_equal(back["curvature"][solved], curvature[solved].astype(np.float32)) and np.isnan(back["curvature"][~solved]).all()
    assert open(path).read().split("\n")[2] == "FIELDS x y z normal_x normal_y normal_z curvature"
