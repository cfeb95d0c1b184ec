"""The world map's k nearest cells and statistical outliers on the GPU (include/dsi_map_knn.h; DESIGN.md 7j "Neighbours and
statistical outliers") against the numpy restatement tests/map_knn_reference.py: array_equal on keys, found, q, the float bits
of distances and means, the exact moments and the reasons.  tests/test_map_knn_cpu.py proves what the scenes must meet."""
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_knn_reference as kref
import map_layout_cases as lc
import map_merge_reference as mref
import map_prune_reference as pref
import world_map_reference as ref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = pref.IDENTITY
COUNTERS = ("calls", "accepted", "rejected", "growths")


def device_map(ctx, leaf, calls, capacity_log2=10):
    wm = d.WorldMap(ctx, leaf, capacity_log2)
    for pts, T in calls:
        wm.integrate(pts, T)
    return wm


def refused(fn, word=None):
    with pytest.raises(d.DsiError) as e:
        fn()
    return e.value.code == E.ERR_INVALID and (word is None or word in str(e.value))


def check_query(wm, rm, points, k, radius, **flt):
    got, want = wm.query(points, k, radius, **flt), kref.query(rm, points, k, radius, **flt)
    assert got["keys"].shape == (len(points), k)
    kref.assert_queries_equal(got, want)
    return got


def check_self(wm, rm, k, radius, min_found=1, **flt):
    """the self query equals the restatement's: counts, moments and rows; the map is untouched"""
    before = wm.info()
    want = kref.self_query(rm, k, radius, min_found, **flt)
    info = wm.knn(k, radius, min_found, **flt)
    rows = wm.fetchKnn()
    assert set(rows) == {"keys", "found", "mean", "q"}
    kref.assert_self_queries_equal(info, rows, want)
    assert wm.info() == before
    return want


def check_select(wm, rm, sq, std_mult, **kw):
    before = wm.info()
    info, want = wm.selectOutliers(std_mult, **kw), kref.select(rm, sq, std_mult)
    for f in ("n_cells", "n_kept", "n_removed", "T_q", "mu", "sigma"):
        assert info[f] == want[f], (f, info[f], want[f])
    assert info == dict(info, **E.knn_threshold(sq["n_scored"], sq["sum_q"], sq["sum_q2"], std_mult))
    assert info["capacity"] == before["capacity"] and wm.info() == before
    rows = wm.fetchKnn()
    assert rows["reason"].dtype == np.uint8 and np.array_equal(rows["keys"], sq["keys"]) and np.array_equal(rows["reason"], want["reason"])
    return info


def check_prune(wm, rm, sq, std_mult, shrink=False):
    """the prune equals the restatement's: counts, the map's exact state and its counters; the self query is refused after"""
    before = wm.info()
    info = wm.pruneOutliers(std_mult, shrink=shrink)
    want = rm.prune_outliers(sq, std_mult)
    for f in ("n_cells", "n_kept", "n_removed", "T_q", "mu", "sigma"):
        assert info[f] == want[f], (f, info[f], want[f])
    assert info["n_cells"] == before["occupied"] == info["n_kept"] + sum(info["n_removed"])
    after = wm.info()
    assert after["occupied"] == info["n_kept"] == len(rm.keys) and all(after[k] == before[k] for k in COUNTERS)
    assert info["capacity"] == after["capacity"] == (pref.shrunk_capacity(info["n_kept"]) if shrink else before["capacity"])
    mref.assert_states_equal(wm.exportState(), rm.export_state())
    for fn in (wm.fetchKnn, wm.selectOutliers, wm.pruneOutliers):
        assert refused(fn, "self query")
    return info


# ---- 1. the lattice: ties that the key decides ----
@pytest.mark.parametrize("radius", kref.LATTICE_RADII)
def test_lattice_with_ties(ctx, radius):
    wm, rm = device_map(ctx, kref.LEAF, kref.lattice_calls()), kref.reference_of(kref.lattice_calls(), kref.LEAF)
    for k in kref.LATTICE_KS:
        check_query(wm, rm, kref.lattice_queries(), k, radius)
        want = check_self(wm, rm, k, radius, min_found=k)
        assert want["reach"] == kref.reach_of(radius, kref.LEAF)
    for k in (2, 4, 5, 9):                                                      # the other instantiations, and a truncated one
        check_query(wm, rm, kref.lattice_queries()[::5], k, radius)
        check_self(wm, rm, k, radius)
    wm.close()


# ---- 2. sparse cells: admitted < k ----
def test_sparse_cells_padding_and_found(ctx):
    calls = kref.sparse_calls()
    wm, rm = device_map(ctx, kref.LEAF, calls), kref.reference_of(calls, kref.LEAF)
    k, radius = kref.SPARSE_K, kref.SPARSE_RADIUS
    got = check_query(wm, rm, kref.sparse_queries(), k, radius)                 # (N, 4) points: stride 4
    short = got["found"] < k
    assert short.sum() >= 100 and (got["found"] == k).sum() >= 20
    pad = np.arange(k)[None, :] >= got["found"][:, None]
    assert (got["keys"][pad] == 0).all() and np.isposinf(got["dist"][pad]).all()
    assert (got["keys"][~pad] != 0).all() and (got["dist"][~pad] <= np.float32(radius)).all()
    check_query(wm, rm, kref.sparse_queries()[:, :3].copy(), k, radius, min_windows=2)
    check_query(wm, rm, kref.sparse_queries(), 16, radius, min_points=2)
    for flt in (dict(), dict(min_windows=2), dict(min_points=2, min_windows=2)):
        for min_found in (1, 2, k):
            want = check_self(wm, rm, k, radius, min_found, **flt)
            for std_mult in (1.0, 0.0, 2.5, -1.0):
                check_select(wm, rm, want, std_mult)
    wm.close()


# ---- 3. edge queries ----
def test_edge_queries(ctx):
    wm, rm = d.WorldMap(ctx, kref.LEAF, 8), kref.KnnReferenceMap(kref.LEAF)
    pts = np.array([[0.01, 0.02, 0.03], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0], [-1e30, 1e30, 1e30]], np.float32)
    # an empty map, and no points
    got = wm.query(pts, 4, 0.1)
    assert (got["found"] == 0).all() and (got["keys"] == 0).all() and np.isposinf(got["dist"]).all()
    none = wm.query(np.zeros((0, 3), np.float32), 4, 0.1)
    assert none["keys"].shape == (0, 4) and none["dist"].shape == (0, 4) and none["found"].shape == (0,)
    info = wm.knn(4, 0.1)
    assert info == dict(info, n_cells=0, n_unqueried=0, n_scored=0, n_isolated=0, sum_q=0, sum_q2=0, reach=2)
    assert all(len(v) == 0 for v in wm.fetchKnn().values())
    sel = wm.selectOutliers()
    assert sel["n_cells"] == sel["n_kept"] == 0 and sel["T_q"] == 1 << 30 and sel["mu"] == sel["sigma"] == 0.0
    # 70,000 points in one cell: one centroid, found by every finite query near it
    rng = np.random.default_rng(66)
    crowd = (rng.uniform(0.001, 0.049, (70_000, 3))).astype(np.float32)
    wm.integrate(crowd, IDENTITY)
    rm.integrate(crowd, IDENTITY)
    assert wm.info()["occupied"] == 1
    got = check_query(wm, rm, pts, 4, 0.1)
    assert got["found"].tolist() == [1, 0, 0, 0, 0, 0]
    want = check_self(wm, rm, 4, 0.1)
    assert want["n_isolated"] == 1 and want["n_scored"] == 0
    assert wm.query(np.zeros((0, 4), np.float32), 1, 0.05)["found"].shape == (0,)
    wm.close()
    # cells and queries at |c| = 2^20 - 2: the offsets that leave the key range are skipped
    calls = kref.edge_calls()
    wm, rm = device_map(ctx, kref.EDGE_LEAF, calls, 8), kref.reference_of(calls, kref.EDGE_LEAF)
    q = np.concatenate([calls[0][0], calls[0][0] + np.float32(0.25), np.float32(2.0) * calls[0][0]])
    got = check_query(wm, rm, q, 4, 1.2)
    assert (got["found"][:9] == 3).all() and (got["found"][18:] == 0).all()
    check_self(wm, rm, 4, 1.2)
    check_self(wm, rm, 16, 1.5)
    # a reach of 4 is refused with the map at hand (its leaf decides), before anything is computed; 3 is the last legal one
    assert refused(lambda: wm.knn(4, 1.6), "reach") and refused(lambda: wm.query(q, 4, 1.6), "reach")
    assert wm.knn(4, 1.5)["reach"] == 3
    wm.close()


# ---- 4. invariance: table size, growth, call order ----
def test_table_and_order_freedom(ctx):
    calls = kref.sparse_calls()
    rm = kref.reference_of(calls, kref.LEAF)
    want_q = kref.query(rm, kref.sparse_queries(), 5, 0.1)
    want_s = kref.self_query(rm, 5, 0.1, 2)
    rng = np.random.default_rng(67)
    pts = np.concatenate([p for p, _ in calls])
    for log2, shuffled in ((8, False), (16, False), (8, True)):
        wm = d.WorldMap(ctx, kref.LEAF, log2)
        made = calls
        if shuffled:                                                            # the same cells from other calls, in another order
            made = [(part, IDENTITY) for part in np.array_split(pts[rng.permutation(len(pts))], 7)]
        for p, T in made:
            wm.integrate(p, T)
        assert wm.info()["capacity"] == lc.grown_from(made, kref.LEAF, log2) and (wm.info()["growths"] > 0) == (log2 == 8)
        assert np.array_equal(wm.extract()["keys"], rm.keys)
        kref.assert_queries_equal(wm.query(kref.sparse_queries(), 5, 0.1), want_q)
        info = wm.knn(5, 0.1, 2)
        kref.assert_self_queries_equal(info, wm.fetchKnn(), want_s)
        wm.close()


# ---- 5. layouts: more slots than one stride, and a chain across the table's end ----
def test_dense_scene_in_a_table_of_two_rounds(ctx):
    wm, rm = device_map(ctx, lc.LEAF, lc.dense_calls(), lc.BIG_LOG2), lc.dense_reference()
    assert wm.info()["capacity"] == 1 << lc.BIG_LOG2
    want = kref.dense_self_query()
    info = wm.knn(kref.DENSE_K, kref.DENSE_RADIUS)
    kref.assert_self_queries_equal(info, wm.fetchKnn(), want)
    assert info["sum_q2"] > 1 << 64
    # the point query of every centroid: more points than one stride of the point kernel; rank 1 is the cell itself
    cells = rm.extract()
    got = wm.query(cells["xyz"], 1, kref.DENSE_RADIUS)
    assert len(cells["keys"]) > lc.ROUND and np.array_equal(got["keys"][:, 0], cells["keys"]) and (got["dist"] == 0).all()
    tail = slice(lc.ROUND - 300, lc.ROUND + 600)                                # across the stride's end, against the restatement
    kref.assert_queries_equal({f: v[tail] for f, v in wm.query(cells["xyz"], 3, kref.DENSE_RADIUS).items()},
                              kref.query(rm, cells["xyz"][tail], 3, kref.DENSE_RADIUS))
    wm.close()


@pytest.mark.parametrize("name", list(lc.CHAINS))
def test_chains_across_the_tables_end(ctx, name):
    ch = lc.chain(name)
    calls = [ch["first"], ch["again"]]
    rm = kref.reference_of(calls, lc.CHAIN_LEAF)
    wm, twice = device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"]), device_map(ctx, lc.CHAIN_LEAF, calls, ch["log2"] + 1)
    assert wm.info()["capacity"] == ch["capacity"] and twice.info()["capacity"] == 2 * ch["capacity"]
    q = np.concatenate([p for p, _ in ch["other_calls"]])                      # present keys, and absent ones with a home in the run
    for m in (wm, twice):
        check_query(m, rm, q, 4, lc.CHAIN_RADIUS)
        want = check_self(m, rm, 4, lc.CHAIN_RADIUS)
        check_select(m, rm, want, 0.5)
    check_prune(wm, rm, want, 0.5)
    wm.close()
    twice.close()


# ---- 6. self exclusion by key ----
def test_self_exclusion_is_by_key(ctx):
    calls = kref.face_calls()
    wm, rm = device_map(ctx, kref.FACE_LEAF, calls), kref.reference_of(calls, kref.FACE_LEAF)
    assert kref.moved_cells(rm).any()                                          # (test_map_knn_cpu.py: what that means for the rows)
    for k in (1, 4, 16):
        check_self(wm, rm, k, kref.FACE_LEAF)
    # the same rows through the point query: a cell's own centroid finds the cell itself first, at distance 0
    cells = rm.extract()
    got = check_query(wm, rm, cells["xyz"], 5, kref.FACE_LEAF)
    sq = kref.self_query(rm, 4, kref.FACE_LEAF)
    dup = got["dist"][:, 1] == 0                                                # two cells with one centroid: either may come first
    assert (got["dist"][:, 0] == 0).all()
    assert np.array_equal(got["keys"][~dup, 0], cells["keys"][~dup]) and np.array_equal(got["keys"][~dup, 1:], sq["rows"]["keys"][~dup])
    wm.close()


# ---- 7. first principles, no restatement ----
def test_first_principles_patch(ctx):
    calls, n_patch = kref.patch_calls()
    wm = device_map(ctx, kref.PATCH_LEAF, calls, 8)
    s, radius = kref.PATCH_SPACING, kref.PATCH_RADIUS
    info = wm.knn(4, radius)
    assert info["n_cells"] == n_patch + 11 and info["n_scored"] == n_patch + 6 and info["n_isolated"] == 5 and info["reach"] == 3
    rows, cells = wm.fetchKnn(), wm.extract()
    assert np.array_equal(rows["keys"], cells["keys"])
    xyz = cells["xyz"].astype(np.float64)
    in_patch = (xyz[:, 0] > 0) & (xyz[:, 0] < 1.2) & (xyz[:, 1] > 0) & (xyz[:, 1] < 1.2)
    interior = in_patch & (xyz[:, 0] > 0.1) & (xyz[:, 0] < 1.1) & (xyz[:, 1] > 0.1) & (xyz[:, 1] < 1.1)
    assert in_patch.sum() == n_patch and interior.sum() == 100
    # float32 coordinates up to 1.2 carry half an ulp of 1.2e-7 each: a distance between two of them is s to within 1e-6
    assert (rows["found"][interior] == 4).all() and np.abs(rows["mean"][interior].astype(np.float64) - s).max() < 1e-6
    assert np.abs(rows["mean"][in_patch].astype(np.float64) - s).max() < 1e-6  # at the rim: 3 or 2 neighbours, all at s
    assert sorted(np.unique(rows["found"][in_patch]).tolist()) == [2, 3, 4]
    pairs, singles = xyz[:, 0] > 2, xyz[:, 0] < -2
    assert pairs.sum() == 6 and singles.sum() == 5
    assert (rows["found"][pairs] == 1).all() and np.abs(rows["mean"][pairs].astype(np.float64) - kref.PATCH_PAIR).max() < 1e-6
    assert (rows["found"][singles] == 0).all() and np.isposinf(rows["mean"][singles]).all() and (rows["q"][singles] == 0).all()
    q_want = np.floor(rows["mean"][~singles].astype(np.float64) / radius * 2.0 ** 30)
    assert np.abs(rows["q"][~singles].astype(np.float64) - q_want).max() <= 65  # (q is made of the double mean, the row shows its float32: 2^30 * 2^-24, and the floor)
    sel = wm.selectOutliers(1.0)
    reason = wm.fetchKnn()["reason"]
    assert (reason[singles] == 2).all() and (reason[pairs] == 3).all() and (reason[in_patch] == 0).all()
    assert sel["n_removed"] == [0, 5, 6] and sel["n_kept"] == n_patch
    off = wm.selectOutliers(-1.0)                                               # criterion 3 off: only the isolated cells leave
    assert off["n_removed"] == [0, 5, 0]
    kept = cells["keys"][in_patch]
    info = wm.pruneOutliers(1.0, shrink=True)
    assert info["n_kept"] == n_patch and info["capacity"] == 256
    assert np.array_equal(wm.extract()["keys"], kept)
    wm.close()


# ---- 8. prune ----
@pytest.mark.parametrize("shrink", (False, True))
def test_prune_equals_the_restatement_bit_for_bit(ctx, shrink):
    calls = kref.sparse_calls()
    wm, rm = device_map(ctx, kref.LEAF, calls), kref.reference_of(calls, kref.LEAF)
    grown = wm.info()["capacity"]
    want = check_self(wm, rm, kref.SPARSE_K, kref.SPARSE_RADIUS, 2, min_windows=2)
    check_select(wm, rm, want, 1.0, shrink=shrink)
    info = check_prune(wm, rm, want, 1.0, shrink)
    assert min(info["n_removed"]) >= 5 and (info["capacity"] < grown) == shrink
    # the kept cells moved with n, S, windows and stamp; the map goes on: integrate, query again, prune again
    assert wm.integrate(calls[0][0], IDENTITY) == rm.integrate(calls[0][0], IDENTITY)
    mref.assert_states_equal(wm.exportState(), rm.export_state())
    want = check_self(wm, rm, 4, 0.1)
    check_prune(wm, rm, want, 0.0, shrink)
    nothing = check_self(wm, rm, 1, 0.15)                                       # a prune that removes nothing leaves the table as it is
    if nothing["n_isolated"] == 0:
        before = wm.info()
        check_prune(wm, rm, nothing, -1.0)
        assert wm.info() == before
    wm.close()


# ---- 9. invalidation ----
def test_invalidation_and_refusals(ctx):
    calls = kref.sparse_calls()
    wm, other = device_map(ctx, kref.LEAF, calls), device_map(ctx, kref.LEAF, calls[:2])
    rm = kref.reference_of(calls, kref.LEAF)
    readers = (wm.fetchKnn, wm.selectOutliers, wm.pruneOutliers)
    state = other.exportState()

    def all_refused():
        return all(refused(fn, "self query") for fn in readers)
    assert all_refused()                                                       # before knn
    for change in (lambda: wm.integrate(calls[0][0], IDENTITY), lambda: wm.integrate(np.zeros((0, 3), np.float32), IDENTITY),
                   lambda: wm.merge(other), lambda: wm.importState(state), lambda: wm.prune(min_points=2),
                   lambda: (wm.components(), wm.pruneComponents(min_cells=2)), lambda: (wm.knn(4, 0.1), wm.pruneOutliers(1.0)), wm.reset):
        wm.knn(4, 0.1)
        wm.selectOutliers()
        assert "reason" in wm.fetchKnn()
        change()
        assert all_refused()
    # knn and query leave a render, a compare, a classification, an alignment step and a labelling valid -- and each other
    for pts, T in calls:
        wm.integrate(pts, T)
    wm.render(E.pose_matrix([0, 0, -2.0, 0, 0, 0, 1]), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 6.0)
    wm.compare(wm, 0.05, distances=True)
    wm.classifyPrune(min_points=2)
    wm.alignStep(wm, 0.05)
    wm.components()
    want = check_self(wm, rm, 4, 0.1)
    check_query(wm, rm, kref.sparse_queries(), 4, 0.1)
    check_select(wm, rm, want, 1.0)
    for fetch in (wm.fetchRender, wm.fetchDistances, wm.fetchPruneReasons, wm.fetchAlignment, wm.fetchComponents, wm.fetchKnn):
        fetch()
    # reasons before a select, the capacity protocol, and NULL outputs
    L = d.load_library()
    m = wm.knn(4, 0.1, 2, min_windows=2)["n_cells"]
    keys, found, reasons, n = np.full(m, 99, np.uint64), np.full(m, 98, np.uint8), np.full(m, 77, np.uint8), C.c_size_t()
    kp, fp, rp = (a.ctypes.data_as(C.POINTER(t)) for a, t in ((keys, C.c_uint64), (found, C.c_uint8), (reasons, C.c_uint8)))
    assert L.dsx_map_knn_fetch(wm._h, kp, fp, None, None, rp, m, C.byref(n)) == E.ERR_INVALID and b"select" in L.dsi_last_error()
    assert (reasons == 77).all() and (keys == 99).all()
    assert L.dsx_map_knn_fetch(wm._h, kp, fp, None, None, None, m - 1, C.byref(n)) == E.ERR_INVALID and n.value == m and (keys == 99).all()
    wm.selectOutliers(1.0)
    assert L.dsx_map_knn_fetch(wm._h, None, None, None, None, rp, m, C.byref(n)) == E.OK and n.value == m
    assert set(np.unique(reasons).tolist()) == {0, 2, 3} and (keys == 99).all()
    wm.knn(4, 0.1)                                                              # a new query: the selection is gone with the old one
    assert L.dsx_map_knn_fetch(wm._h, kp, fp, None, None, rp, m, C.byref(n)) == E.ERR_INVALID
    with pytest.raises(d.DsiError):
        wm.knn(17, 0.1)
    with pytest.raises(d.DsiError):
        wm.pruneOutliers(float("nan"))
    assert len(wm.fetchKnn()["keys"]) == wm.count()                             # a refused call leaves the query valid
    o = E._MapKnnOpts(1, 1, 4, 1, 0.1)
    pts = kref.sparse_queries()
    pp = pts.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dsx_map_knn_points(wm._h, pp, 5, 3, C.byref(o), None, None, None) == E.ERR_INVALID and b"stride" in L.dsi_last_error()
    assert L.dsx_map_knn_points(wm._h, None, 4, 3, C.byref(o), None, None, None) == E.ERR_INVALID and b"xyz_host" in L.dsi_last_error()
    assert L.dsx_map_knn_points(wm._h, pp, 4, (1 << 27) + 1, C.byref(o), None, None, None) == E.ERR_INVALID
    assert L.dsx_map_knn_points(wm._h, pp, 4, len(pts), C.byref(o), None, None, None) == E.OK             # every output may be NULL
    only = np.zeros(len(pts), np.uint8)
    assert L.dsx_map_knn_points(wm._h, pp, 4, len(pts), C.byref(o), None, None, only.ctypes.data_as(C.POINTER(C.c_uint8))) == E.OK
    assert np.array_equal(only, kref.query(rm, pts, 4, 0.1)["found"])
    wm.close()
    other.close()


# ---- 10. the stream ----
def test_outliers_through_full_sequence(ctx):
    """full_sequence(..., world_map=, world_map_outliers=) with every=2 equals the same calls made by hand on a second map, fed
    with the clouds the stream returned; None leaves the run as it is."""
    n_win, dur, t0 = 4, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    kw = dict(options_depth_map=d.OptionsDepthMap(), options_point_cloud=d.OptionsPointCloud(2.0, 1))
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    bare_map, plain_map, wm, hand = (d.WorldMap(ctx, 0.5, 8) for _ in range(4))
    bare = list(proc.full_sequence(*args, world_map=bare_map, **kw))
    plain = list(proc.full_sequence(*args, world_map=plain_map, world_map_outliers=None, **kw))
    opts = {"every": 2, "k": 4, "radius": 1.0, "min_found": 2, "std_mult": 1.0, "shrink": True}
    on = list(proc.full_sequence(*args, world_map=wm, world_map_outliers=opts, **kw))
    assert len(on) == len(plain) == len(bare) == n_win
    poses = [d.invert_pose(proc.reference_view_process1(rig["trajectories"][0], w[0])) for w in plain]
    for k, (a, b, c) in enumerate(zip(on, plain, bare)):
        assert len(b) == len(c) == 5 and len(a) == (6 if k % 2 else 5) and a[0] == b[0] == c[0]
        for x, y, z in zip(a[1:5], b[1:], c[1:]):
            assert x.dtype == y.dtype == z.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
            assert np.array_equal(y.view(np.uint8), z.view(np.uint8))
        hand.integrate(a[4], poses[k])
        if k % 2:
            counts = hand.knn(4, 1.0, 2)
            counts["prune"] = hand.pruneOutliers(1.0, shrink=True)
            print("window %d: %s" % (k, counts))
            assert a[5] == {"world_map_outliers": counts}
            assert counts["prune"]["n_kept"] >= 1 and sum(counts["prune"]["n_removed"]) >= 1
    mref.assert_states_equal(wm.exportState(), hand.exportState())
    mref.assert_states_equal(plain_map.exportState(), bare_map.exportState())
    assert wm.info() == hand.info() and wm.info()["occupied"] < plain_map.info()["occupied"]
    # with the other two keywords the outliers come last
    both_map, by_hand = d.WorldMap(ctx, 0.5, 8), d.WorldMap(ctx, 0.5, 8)
    both = list(proc.full_sequence(*args, world_map=both_map, world_map_prune={"every": 2, "min_points": 2},
                                   world_map_components={"every": 2, "min_cells": 2}, world_map_outliers=opts, **kw))
    for k, a in enumerate(both):
        by_hand.integrate(a[4], poses[k])
        if k % 2:
            assert len(a) == 8 and "world_map_prune" in a[5] and "world_map_components" in a[6] and "world_map_outliers" in a[7]
            by_hand.prune(min_points=2)
            by_hand.components()
            by_hand.pruneComponents(min_cells=2)
            counts = by_hand.knn(4, 1.0, 2)
            counts["prune"] = by_hand.pruneOutliers(1.0, shrink=True)
            assert a[7]["world_map_outliers"] == counts
    mref.assert_states_equal(both_map.exportState(), by_hand.exportState())
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map_outliers=opts, **kw))          # no map to query
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, world_map=wm, world_map_outliers=dict(opts, every=0), **kw))
    for m in (bare_map, plain_map, wm, hand, both_map, by_hand):
        m.close()
