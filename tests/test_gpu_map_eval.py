"""The world map scored in 3-D (dsx_map_*, engine.WorldMap.integrateDepth / compare, engine.map_f_score) on
the MI355X against the numpy restatement of tests/map_eval_reference.py: every comparison is array_equal -- keys, n,
windows and centroid bits of an integrated depth image; histogram, counts, sum_q, reach and distance bits of a compare."""
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_eval_reference as mref
import world_map_reference as ref
import world_map_render_reference as rref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = rref.IDENTITY
Q_IMAGE = np.eye(4)                                                 # the projector that copies its input
K_IMAGE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)


def code_of(fn):
    try:
        fn()
    except d.DsiError as e:
        return e.code
    return E.OK


def build(ctx, leaf, calls, log2=16):
    wm, rm = d.WorldMap(ctx, leaf, log2), ref.ReferenceMap(leaf)
    for pts in calls:
        assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY) == 0
    return wm, rm


@pytest.fixture(scope="module")
def scene(ctx):
    """(map A, its reference, map B, its reference): leaf 0.05 against leaf 0.04, tables of 2^16 slots"""
    a, ra = build(ctx, mref.LEAF_A, rref.scene_calls())
    b, rb = build(ctx, mref.LEAF_B, mref.scene_b_calls())
    ref.assert_maps_equal(a.extract(), ra.extract())
    ref.assert_maps_equal(b.extract(), rb.extract())
    yield a, ra, b, rb
    a.close()
    b.close()


def check(first, first_ref, second, second_ref, radius, n_bins=mref.N_BINS, mp=1, mw=1, mpo=1, mwo=1):
    got = first.compare(second, radius, n_bins, mp, mw, mpo, mwo, distances=True)
    want = mref.compare(first_ref.extract(mp, mw), second_ref.extract(mpo, mwo), second_ref.leaf, radius, n_bins)
    mref.assert_compares_equal(got, want)
    return got


# ---- depth images into a map ----

@pytest.mark.parametrize("shape", [(67, 5), (64, 48)])
def test_depth_image_equals_the_back_projected_points(ctx, shape):
    w, h = shape
    depth, mask, lo, hi = mref.depth_image(w, h, 3 + w)
    K = (40.0, 41.0, (w - 1) / 2.0, (h - 1) / 2.5)
    leaf = 0.05
    img, pts_map, rm = d.WorldMap(ctx, leaf, 16), d.WorldMap(ctx, leaf, 16), ref.ReferenceMap(leaf)
    grown = d.WorldMap(ctx, leaf, 8)
    total = 0
    T = mref.camera_pose(w % 3)
    for m in (mask, None):                                          # two calls: masked, then every pixel -- windows 2 and 1
        pts = mref.backproject(depth, m, *K, lo, hi)
        want_rejected = rm.integrate(pts, T)
        assert pts_map.integrate(pts, T) == want_rejected == 0
        assert img.integrateDepth(depth, m, K, lo, hi, T) == (len(pts), 0)
        assert grown.integrateDepth(depth, m, np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]), lo, hi, T) == (len(pts), 0)
        total += len(pts)
    assert 0.5 * w * h < total < 2 * w * h
    want = rm.extract()
    assert (want["windows"] == 2).sum() > 20 and (want["windows"] == 1).sum() > 20
    for got in (img, pts_map, grown):
        ref.assert_maps_equal(got.extract(), want)
        assert got.info()["calls"] == 2 and got.info()["accepted"] == total
    assert grown.info()["growths"] >= 1
    # points rejected by rule 3: a pose that throws everything beyond the key range, and one that makes it non-finite
    far = IDENTITY.copy()
    far[3] = 1e9
    pts = mref.backproject(depth, mask, *K, lo, hi)
    assert img.integrateDepth(depth, mask, K, lo, hi, far) == (len(pts), len(pts)) and rm.integrate(pts, far) == len(pts)
    far[3] = np.nan
    assert img.integrateDepth(depth, mask, K, lo, hi, far) == (len(pts), len(pts)) and rm.integrate(pts, far) == len(pts)
    ref.assert_maps_equal(img.extract(), rm.extract())
    assert img.info()["rejected"] == 2 * len(pts) and img.info()["calls"] == 4
    # a refused call leaves the map as it was; a mask of another shape never reaches the engine
    assert code_of(lambda: img.integrateDepth(depth, mask, (0.0, 41.0, 1.0, 1.0), lo, hi, IDENTITY)) == E.ERR_INVALID
    assert code_of(lambda: img.integrateDepth(depth, mask, K, hi, lo, IDENTITY)) == E.ERR_INVALID
    with pytest.raises(ValueError):
        img.integrateDepth(depth, mask[:, :-1], K, lo, hi, IDENTITY)
    ref.assert_maps_equal(img.extract(), rm.extract())
    assert img.info()["calls"] == 4
    for o in (img, pts_map, grown):
        o.close()


def test_ground_truth_projector_where_it_lies(ctx):
    w, h = 64, 48
    depth, _, lo, hi = mref.depth_image(w, h, 9)
    disp = np.where(np.isfinite(depth) & (depth > 0), depth, 0.0).astype(np.float32)
    p = d.GroundTruthProjector(ctx, w, h, Q_IMAGE, np.eye(4), K_IMAGE)
    p.project(disp)
    held = p.fetch()[0]
    assert (held > 0).sum() > 2000
    K, T = (40.0, 40.0, 31.5, 23.5), mref.camera_pose(2)
    a, b, rm = d.WorldMap(ctx, 0.05, 8), d.WorldMap(ctx, 0.05, 8), ref.ReferenceMap(0.05)
    pts = mref.backproject(held, None, *K, lo, hi)
    assert a.integrateGroundTruth(p, K, lo, hi, T) == b.integrateDepth(held, None, K, lo, hi, T) == (len(pts), rm.integrate(pts, T))
    ref.assert_maps_equal(a.extract(), b.extract())
    ref.assert_maps_equal(a.extract(), rm.extract())
    # process.ground_truth_map takes either form
    g = proc.ground_truth_map(ctx, [(p, T), (held, mref.camera_pose(0))], (w, h) + K, 0.05, lo, hi, capacity_log2=8)
    rm.integrate(mref.backproject(held, None, *K, lo, hi), mref.camera_pose(0))
    ref.assert_maps_equal(g.extract(), rm.extract())
    assert code_of(lambda: a.integrateGroundTruth(p, (40.0, float("nan"), 1.0, 1.0), lo, hi, T)) == E.ERR_INVALID
    other = d.Context(0)
    q = d.GroundTruthProjector(other, w, h, Q_IMAGE, np.eye(4), K_IMAGE)
    assert code_of(lambda: a.integrateGroundTruth(q, K, lo, hi, T)) == E.ERR_CONTEXT
    for o in (q, p, a, b, g):
        o.close()
    other.close()


# ---- comparing maps ----

@pytest.mark.parametrize("radius", mref.RADII)
@pytest.mark.parametrize("way", ["a->b", "b->a"])
def test_scene(scene, way, radius):
    a, ra, b, rb = scene
    first = (a, ra, b, rb) if way == "a->b" else (b, rb, a, ra)
    r = check(*first, radius)
    assert r["n_matched"] >= 5000 and r["n_unmatched"] >= 300 and (r["hist"] > 0).all()
    assert r["reach"] == mref.reach_of(radius, first[3].leaf) and 0.0 < r["mean"] < radius
    # only cells of the second map that two calls reached
    two = check(*first, radius, mwo=2)
    assert 0 < two["n_matched"] < r["n_matched"] and two["n_cells"] == r["n_cells"]
    # and only such cells of the first
    few = check(*first, radius, mw=2)
    assert 0 < few["n_cells"] < r["n_cells"]


def test_the_same_map_built_another_way(ctx, scene):
    a, ra, b, rb = scene
    rng = np.random.default_rng(12)
    pts = np.concatenate(rref.scene_calls())
    pts = pts[rng.permutation(len(pts))]
    cuts = [0, 1, 700, 701, 5000, 11000, 11003, len(pts)]
    seven, seven_ref = build(ctx, mref.LEAF_A, [pts[i:j] for i, j in zip(cuts[:-1], cuts[1:])], log2=8)
    assert seven.info()["growths"] >= 6 and seven.info()["capacity"] != a.info()["capacity"]
    for radius in (0.04, 0.1):
        first, other = check(a, ra, b, rb, radius), check(seven, seven_ref, b, rb, radius)
        mref.assert_compares_equal(other, first)                    # as the first map: centroids and keys are the same
        first, other = check(b, rb, a, ra, radius), check(b, rb, seven, seven_ref, radius)
        mref.assert_compares_equal(other, first)                    # and as the second, looked up in a table of another size
    seven.close()


def test_a_map_against_itself_and_empty_maps(ctx, scene):
    a, ra, b, rb = scene
    r = check(a, ra, a, ra, 0.08)
    assert r["n_matched"] == r["n_cells"] == a.count() and r["sum_q"] == 0 and r["mean"] == 0.0 and not r["dist"].any()
    assert r["hist"][0] == r["n_cells"] and not r["hist"][1:].any()
    empty, empty_ref = d.WorldMap(ctx, 0.04, 8), ref.ReferenceMap(0.04)
    r = check(a, ra, empty, empty_ref, 0.08)
    assert r["n_matched"] == 0 and r["n_unmatched"] == a.count() and np.isposinf(r["dist"]).all() and np.isnan(r["mean"])
    r = check(empty, empty_ref, a, ra, 0.08)
    assert r["n_cells"] == 0 and r["dist"].shape == (0,) and r["keys"].shape == (0,)
    r = check(empty, empty_ref, empty, empty_ref, 0.08)
    assert r["n_cells"] == 0
    r = check(a, ra, b, rb, 0.08, mp=1000)                          # a filter nothing passes
    assert r["n_cells"] == 0 and r["dist"].shape == (0,)
    f = d.map_f_score(a, empty, 0.08, 16)
    assert not f["precision"].any() and not f["recall"].any() and not f["f1"].any()
    empty.close()


def test_hand_cases_on_the_device(ctx):
    """the hand cases of test_map_eval_cpu.py: d == radius, the last bin, and neighbours beyond the key range"""
    a, ra = build(ctx, 0.5, [np.float32([[0.25, 0.25, 0.25]])], log2=8)
    b, rb = build(ctx, 0.5, [np.float32([[0.75, 0.25, 0.25]])], log2=8)
    r = check(a, ra, b, rb, 0.5, 8)
    assert r["n_matched"] == 1 and r["hist"].tolist() == [0] * 7 + [1] and r["sum_q"] == 1 << 32 and r["dist"][0] == np.float32(0.5)
    r = check(a, ra, b, rb, float(np.nextafter(0.5, 0.0)), 8)
    assert r["n_matched"] == 0 and np.isposinf(r["dist"][0])
    assert check(a, ra, b, rb, 0.5625, 8)["hist"].tolist() == [0] * 7 + [1]
    r = check(a, ra, b, rb, 1.0, 8)
    assert r["reach"] == 2 and r["hist"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and r["sum_q"] == 1 << 31
    for n_bins in (1, 4096):
        r = check(a, ra, b, rb, 1.0, n_bins)
        assert r["hist"].sum() == 1 and r["hist"][n_bins // 2] == 1
    top = float(ref.CELL_MAX)
    hi, hi_ref = build(ctx, 1.0, [np.float32([[top + 0.5, 0.5, 0.5]])], log2=8)
    nb, nb_ref = build(ctx, 1.0, [np.float32([[top - 0.5, 0.5, 0.5], [-top + 0.5, 0.5, 0.5]])], log2=8)
    assert check(hi, hi_ref, nb, nb_ref, 1.0, 4)["n_matched"] == 1
    r = check(nb, nb_ref, hi, hi_ref, 1.0, 4)
    assert r["n_matched"] == 1 and r["n_unmatched"] == 1
    for radius in (1.0, 2.0, 3.0):
        assert check(nb, nb_ref, nb, nb_ref, radius, 4)["n_matched"] == 2
    # a second map so fine that the first one's centroids lie far beyond its key range: no candidates, no wrap-around
    fine, fine_ref = build(ctx, 1e-3, [np.float32([[0.0005, 0.0005, 0.0005]])], log2=8)
    r = check(hi, hi_ref, fine, fine_ref, 2e-3, 4)
    assert r["n_unmatched"] == 1
    # the bounds that need a map: reach 0 cannot be, reach 4 is refused, as is a map of another context
    assert code_of(lambda: a.compare(b, 1.5 + 1e-9)) == E.ERR_INVALID
    assert a.compare(b, 1.5)["reach"] == 3
    other = d.Context(0)
    foreign = d.WorldMap(other, 0.5, 8)
    assert code_of(lambda: a.compare(foreign, 0.5)) == E.ERR_CONTEXT
    assert code_of(lambda: foreign.compare(a, 0.5)) == E.ERR_CONTEXT
    for o in (foreign, a, b, hi, nb, fine):
        o.close()
    other.close()


def test_fetch_protocol_guards_and_invalidation(ctx, scene):
    a, ra, b, rb = scene
    L = d.load_library()
    mine, mine_ref = build(ctx, mref.LEAF_A, rref.scene_calls()[:2], log2=8)
    assert code_of(mine.fetchDistances) == E.ERR_INVALID            # before the first compare
    want = mref.compare(mine_ref.extract(1, 2), rb.extract(), mref.LEAF_B, 0.08, 16)
    got = mine.compare(b, 0.08, 16, min_windows=2)
    m = got["n_cells"]
    assert m == want["n_cells"] and 0 < m < mine.count()
    n = C.c_size_t()
    # too small a capacity: nothing is written, the size needed comes back
    pad = 1024
    dist = np.full(m + 2 * pad, -77.0, np.float32)
    keys = np.full(m + 2 * pad, 0xA5A5A5A5A5A5A5A5, np.uint64)
    fptr = lambda x: x[pad:].ctypes.data_as(C.POINTER(C.c_float))
    kptr = lambda x: x[pad:].ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.dsx_map_compare_fetch(mine._h, fptr(dist), kptr(keys), m - 1, C.byref(n)) == E.ERR_INVALID and n.value == m
    assert (dist == -77.0).all() and (keys == 0xA5A5A5A5A5A5A5A5).all()
    assert L.dsx_map_compare_fetch(mine._h, fptr(dist), kptr(keys), m, C.byref(n)) == E.OK and n.value == m
    for buf, guard in ((dist, np.float32(-77.0)), (keys, np.uint64(0xA5A5A5A5A5A5A5A5))):
        assert (buf[:pad] == guard).all() and (buf[pad + m:] == guard).all()
    order = np.argsort(keys[pad:pad + m], kind="stable")
    assert np.array_equal(keys[pad:pad + m][order], want["keys"])
    assert np.array_equal(dist[pad:pad + m][order].view(np.uint32), want["dist"].view(np.uint32))
    # the order is dsi_map_extract's for the same filter; either output may be left out
    assert np.array_equal(keys[pad:pad + m], mine.extract(1, 2, sort=False)["keys"])
    only = np.empty(m, np.float32)
    assert L.dsx_map_compare_fetch(mine._h, only.ctypes.data_as(C.POINTER(C.c_float)), None, m, C.byref(n)) == E.OK
    assert np.array_equal(only.view(np.uint32), dist[pad:pad + m].view(np.uint32))
    # a change to the second map does not invalidate the result; a render of the first does not either
    other, _ = build(ctx, mref.LEAF_B, mref.scene_b_calls()[:1], log2=8)
    mine.compare(other, 0.08, 16)
    before = mine.fetchDistances()
    other.integrate(np.float32([[0, 0, 2]]), IDENTITY)
    other.reset()
    mine.render(IDENTITY, 7, 5, 1.0, 1.0, 3.0, 2.0, 0.5, 100.0, fetch=False)
    after = mine.fetchDistances()
    assert np.array_equal(after["keys"], before["keys"]) and np.array_equal(after["dist"].view(np.uint32), before["dist"].view(np.uint32))
    # any integrate call on the first map does, even an empty one, and so do a depth image and a reset
    mine.integrate(np.zeros((0, 3), np.float32), IDENTITY)
    assert code_of(mine.fetchDistances) == E.ERR_INVALID
    mine.compare(b, 0.08, 16)
    mine.integrateDepth(np.ones((2, 2), np.float32), None, (1.0, 1.0, 0.5, 0.5), 0.5, 2.0, IDENTITY)
    assert code_of(mine.fetchDistances) == E.ERR_INVALID
    mine.compare(b, 0.08, 16)
    assert len(mine.fetchDistances()["keys"]) == mine.count()
    mine.reset()
    assert code_of(mine.fetchDistances) == E.ERR_INVALID
    # a refused compare leaves the last result standing (the map is empty now)
    mine.compare(b, 0.08, 16)
    assert code_of(lambda: mine.compare(b, 0.08, 0)) == E.ERR_INVALID
    assert len(mine.fetchDistances()["keys"]) == 0
    for o in (mine, other):
        o.close()


# ---- the layers above ----

def test_f_score_equals_the_formulas_on_the_restatements_counts(scene):
    a, ra, b, rb = scene
    for radius in (0.04, 0.1):
        f = d.map_f_score(a, b, radius, mref.N_BINS)
        fwd = mref.compare(ra.extract(), rb.extract(), mref.LEAF_B, radius, mref.N_BINS)
        bwd = mref.compare(rb.extract(), ra.extract(), mref.LEAF_A, radius, mref.N_BINS)
        want = mref.f_score(fwd, bwd, radius, mref.N_BINS)
        for k in ("thresholds", "precision", "recall", "f1"):
            assert f[k].dtype == np.float64 and np.array_equal(f[k], want[k]), k
        mref.assert_compares_equal(f["est"], fwd, distances=False)
        mref.assert_compares_equal(f["gt"], bwd, distances=False)
        assert 50.0 < f["precision"][-1] < 100.0 and 50.0 < f["recall"][-1] < 100.0 and (np.diff(f["f1"]) >= 0).all()
    # the filters travel to the right side in each direction
    f = d.map_f_score(a, b, 0.08, 8, min_windows=2, min_points_gt=2)
    fwd = mref.compare(ra.extract(1, 2), rb.extract(2, 1), mref.LEAF_B, 0.08, 8)
    bwd = mref.compare(rb.extract(2, 1), ra.extract(1, 2), mref.LEAF_A, 0.08, 8)
    mref.assert_compares_equal(f["est"], fwd, distances=False)
    mref.assert_compares_equal(f["gt"], bwd, distances=False)


def test_score_world_map_3d_on_a_run(ctx):
    """A tiny full_sequence(..., world_map=) run scored against a ground-truth map made from the same synthetic scene: every
    window's own filtered depth map, back-projected from its reference view."""
    n_win, dur, t0 = 3, 0.05, 10.0
    rig = syn.stereo_rig(n_win * 60_000, width=64, height=48, t0=t0, duration=n_win * dur, seed=5, n_points=400)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0)
    opts_dm, opts_pc = d.OptionsDepthMap(), d.OptionsPointCloud(2.0, 1)
    leaf = 0.5
    wm = d.WorldMap(ctx, leaf, 8)
    frames, clouds = [], []
    for w in proc.full_sequence(ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur,
                                options_depth_map=opts_dm, options_point_cloud=opts_pc, world_map=wm):
        T_w_rv = d.invert_pose(proc.reference_view_process1(rig["trajectories"][0], w[0]))
        frames.append((np.where(w[3] > 0, w[1], 0.0).astype(np.float32), T_w_rv))
        clouds.append(len(w[4]))
    assert wm.info()["calls"] == n_win and min(clouds) > 20
    gt = proc.ground_truth_map(ctx, frames, cam, leaf, 4.0, 50.0, capacity_log2=8)
    rm = ref.ReferenceMap(leaf)
    for depth, T in frames:
        rm.integrate(mref.backproject(depth, None, cam[2], cam[3], cam[4], cam[5], 4.0, 50.0), T)
    ref.assert_maps_equal(gt.extract(), rm.extract())
    s = proc.score_world_map_3d(wm, gt, leaf, 8)
    fwd = mref.compare(wm.extract(), rm.extract(), leaf, leaf, 8)
    bwd = mref.compare(rm.extract(), wm.extract(), leaf, leaf, 8)
    want = mref.f_score(fwd, bwd, leaf, 8)
    for k in ("thresholds", "precision", "recall", "f1"):
        assert np.array_equal(s[k], want[k]), k
    mref.assert_compares_equal(s["est"], fwd, distances=False)
    mref.assert_compares_equal(s["gt"], bwd, distances=False)
    print("cells %d / %d, precision %.1f %%, recall %.1f %%" % (fwd["n_cells"], bwd["n_cells"], s["precision"][-1], s["recall"][-1]))
    # the map is made of a subset of those very depth maps' pixels (the radius filter drops some): every cell of it lies
    # within a cell's edge of ground truth
    assert s["est"]["n_cells"] == wm.count() > 20 and s["precision"][-1] > 80.0 and s["recall"][-1] > 50.0
    gt.close()
    wm.close()
