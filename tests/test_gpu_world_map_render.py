"""The world map's render (dsi_map_render*, engine.WorldMap.render) on the MI355X against the numpy
restatement of tests/world_map_render_reference.py: every comparison is array_equal on the depth bits, windows, hits, mask
and the five counts."""
import ctypes as C

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import world_map_reference as ref
import world_map_render_reference as rref
from dvs_mcemvs_amd import engine as E, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

IDENTITY = rref.IDENTITY
REALS = ("sum_di", "sum_di2", "sum_are", "sum_abs", "max_gt", "silog", "are", "lrmse", "badp", "mean_abs", "median_abs")
# the projector that copies its input: (X, Y, Z) = (x, y, d), u = X, v = Y, value = Z
Q_IMAGE = np.eye(4)
K_IMAGE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)


def code_of(fn):
    try:
        fn()
    except d.DsiError as e:
        return e.code
    return E.OK


def same_metrics(a, b):
    bits = lambda m: np.array([m[k] for k in REALS] + list(m["delta"]), np.float64).tobytes()
    ints = lambda m: {k: v for k, v in m.items() if k not in REALS and k != "delta"}
    return bits(a) == bits(b) and ints(a) == ints(b)


def check(wm, cells, T, splat=0, min_points=1, min_windows=1, **view):
    """one render against the restatement of the cells given; returns it"""
    got = wm.render(T, view["width"], view["height"], view["fx"], view["fy"], view["cx"], view["cy"], view["min_depth"],
                    view["max_depth"], splat=splat, min_points=min_points, min_windows=min_windows)
    want = rref.render(cells, T, splat=splat, **view)
    rref.assert_renders_equal(got, want)
    return got


@pytest.fixture(scope="module")
def scene(ctx):
    """the random scene in one call order, table 2^16: (map, reference map)"""
    wm, rm = d.WorldMap(ctx, rref.SCENE_LEAF, 16), ref.ReferenceMap(rref.SCENE_LEAF)
    for pts in rref.scene_calls():
        assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY) == 0
    ref.assert_maps_equal(wm.extract(), rm.extract())
    yield wm, rm
    wm.close()


@pytest.mark.parametrize("min_windows", [1, 2])
@pytest.mark.parametrize("splat", [0, 1, 2])
def test_random_scene(scene, splat, min_windows):
    wm, rm = scene
    r = check(wm, rm.extract(min_windows=min_windows), rref.scene_pose(), splat=splat, min_windows=min_windows, **rref.SCENE_VIEW)
    assert r["n_drawn"] > 50 and r["n_clipped"] > 0 and r["n_outside"] > 0
    if min_windows == 1:
        assert (r["hits"] >= 2).sum() * 2 >= r["n_pixels"]


def test_the_same_map_built_three_ways(ctx, scene):
    wm, rm = scene
    pose, view = rref.scene_pose(), rref.SCENE_VIEW
    first = check(wm, rm.extract(), pose, splat=1, **view)
    again = check(wm, rm.extract(), pose, splat=1, **view)           # a render repeated: the buffers were cleared
    rref.assert_renders_equal(again, first)
    # shuffled points in seven uneven calls, a table that starts at 2^8 and grows
    rng = np.random.default_rng(12)
    pts = np.concatenate(rref.scene_calls())
    pts = pts[rng.permutation(len(pts))]
    cuts = [0, 1, 700, 701, 5000, 11000, 11003, len(pts)]
    seven, seven_ref = d.WorldMap(ctx, rref.SCENE_LEAF, 8), ref.ReferenceMap(rref.SCENE_LEAF)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert seven.integrate(pts[a:b], IDENTITY) == seven_ref.integrate(pts[a:b], IDENTITY) == 0
    assert seven.info()["growths"] >= 6
    other = check(seven, seven_ref.extract(), pose, splat=1, **view)
    # the cells and their centroids are the same, the window counts are not: depth, hits and mask agree, windows is
    # compared like with like (each with its own restatement, above)
    for k in ("hits", "mask") + rref.COUNTS:
        assert np.array_equal(other[k], first[k]), k
    assert np.array_equal(other["depth"].view(np.uint32), first["depth"].view(np.uint32))
    # one call holding everything: every cell has windows == 1, and so has every covered pixel
    one, one_ref = d.WorldMap(ctx, rref.SCENE_LEAF, 16), ref.ReferenceMap(rref.SCENE_LEAF)
    assert one.integrate(pts, IDENTITY) == one_ref.integrate(pts, IDENTITY) == 0
    single = check(one, one_ref.extract(), pose, splat=1, **view)
    assert np.array_equal(single["windows"], single["mask"].astype(np.uint32))
    assert np.array_equal(single["hits"], first["hits"])
    # at splat 0 no depth tie is decided by the counts unless two cells tie exactly; the depth images agree either way
    a, b = check(wm, rm.extract(), pose, **view), check(one, one_ref.extract(), pose, **view)
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))
    seven.close()
    one.close()


def test_awkward_shapes_reallocation_and_an_empty_map(ctx, scene):
    wm, rm = scene
    cells, pose = rm.extract(), rref.scene_pose()
    for w, h in ((1, 1), (67, 5), (5, 67), (1, 1), (64, 48)):       # every change reallocates the view's buffers
        view = dict(width=w, height=h, fx=40.0, fy=40.0, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, min_depth=0.5, max_depth=5.0)
        r = check(wm, cells, pose, splat=2, **view)
        assert r["depth"].shape == (h, w) and r["n_drawn"] > 0
    empty = d.WorldMap(ctx, 0.05, 8)
    none = {"xyz": np.zeros((0, 3), np.float32), "windows": np.zeros(0, np.uint32)}
    r = check(empty, none, pose, splat=4, **rref.SCENE_VIEW)
    assert [r[k] for k in rref.COUNTS] == [0, 0, 0, 0, 0] and not r["depth"].any() and not r["mask"].any()
    # a filter nothing passes
    r = check(wm, rm.extract(min_points=1000), pose, min_points=1000, **rref.SCENE_VIEW)
    assert r["n_cells"] == 0
    empty.close()


def guarded_fetch(wm, shape):
    """dsi_map_render_fetch into the middle of guard-patterned arrays: (images, guards intact)"""
    n, pad = shape[0] * shape[1], 4096
    bufs = {"depth": np.full(n + 2 * pad, -77.0, np.float32), "windows": np.full(n + 2 * pad, 0xA5A5A5A5, np.uint32),
            "hits": np.full(n + 2 * pad, 0x5A5A5A5A, np.uint32), "mask": np.full(n + 2 * pad, 0xC3, np.uint8)}
    before = {k: v.copy() for k, v in bufs.items()}
    mid = {k: v[pad:pad + n] for k, v in bufs.items()}
    L = d.load_library()
    assert L.dsi_map_render_fetch(wm._h, mid["depth"].ctypes.data_as(C.POINTER(C.c_float)),
                                  mid["windows"].ctypes.data_as(C.POINTER(C.c_uint32)),
                                  mid["hits"].ctypes.data_as(C.POINTER(C.c_uint32)),
                                  mid["mask"].ctypes.data_as(C.POINTER(C.c_uint8))) == E.OK
    intact = all(np.array_equal(bufs[k][:pad], before[k][:pad]) and np.array_equal(bufs[k][pad + n:], before[k][pad + n:])
                 for k in bufs)
    return {k: v.reshape(shape).copy() for k, v in mid.items()}, intact


def test_hostile_cells(ctx):
    leaf = 0.125
    k = np.arange(-6, 7, dtype=np.float32)
    grid = (np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + np.float32(0.5)) * np.float32(leaf)
    wm, rm = d.WorldMap(ctx, leaf, 10), ref.ReferenceMap(leaf)
    assert wm.integrate(grid, IDENTITY) == rm.integrate(grid, IDENTITY) == 0
    cells = rm.extract()
    view = dict(width=33, height=21, fx=20.0, fy=20.0, cx=16.0, cy=10.0)
    # behind the camera: the view looks along -z of the world, from the middle of the block
    back = np.array([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0], np.float64)
    r = check(wm, cells, back, splat=1, min_depth=0.05, max_depth=10.0, **view)
    assert r["n_clipped"] > len(grid) // 2 and r["n_drawn"] > 0
    # clip planes within an ulp of the cells' depths: the centroids are exact multiples of leaf / 2, and so are the
    # depths under a pose that shifts z by 2.0
    shift = IDENTITY.copy()
    shift[11] = 2.0
    zs = np.unique(cells["xyz"][:, 2].astype(np.float64) + 2.0)
    for lo, hi in ((zs[2], zs[-3]), (np.nextafter(zs[2], np.inf), np.nextafter(zs[-3], -np.inf)),
                   (np.nextafter(zs[2], -np.inf), np.nextafter(zs[-3], np.inf))):
        r = check(wm, cells, shift, min_depth=float(lo), max_depth=float(hi), **view)
        assert r["n_clipped"] > 0 and r["n_drawn"] > 0
    counts = [check(wm, cells, shift, min_depth=float(lo), max_depth=float(hi), **view)["n_clipped"]
              for lo, hi in ((zs[2], zs[-3]), (np.nextafter(zs[2], np.inf), np.nextafter(zs[-3], -np.inf)))]
    assert counts[1] - counts[0] == 2 * 13 * 13                    # the two planes of cells that sat on the clip planes
    # |u| beyond 2^31, beyond 2^63 and infinite: dropped, never saturated; the fetch stays inside its arrays
    huge, huge_ref = d.WorldMap(ctx, 0.5, 8), ref.ReferenceMap(0.5)
    assert huge.integrate(rref.HUGE_POINTS, IDENTITY) == huge_ref.integrate(rref.HUGE_POINTS, IDENTITY) == 0
    assert np.array_equal(np.sort(huge_ref.extract()["xyz"], axis=0), np.sort(rref.HUGE_POINTS, axis=0))
    for f, r22 in rref.HUGE_CASES:
        hv = rref.hand_view(f=f, lo=1e-35, hi=10.0)
        r = check(huge, huge_ref.extract(), rref.huge_pose(r22), splat=4, **hv)
        assert [r[k] for k in rref.COUNTS] == rref.HUGE_COUNTS and (r["hits"] == 1).all()
        got, intact = guarded_fetch(huge, (hv["height"], hv["width"]))
        assert intact
        for name in ("depth", "windows", "hits", "mask"):
            assert np.array_equal(got[name].view(np.uint8), r[name].view(np.uint8)), name
    huge.close()
    # a large focal length on the block itself: X / Z near 1 times 1e12
    r = check(wm, cells, shift, splat=4, min_depth=0.05, max_depth=10.0, width=33, height=21, fx=1e12, fy=-1e12, cx=16.0, cy=10.0)
    assert r["n_outside"] > 0
    got, intact = guarded_fetch(wm, (21, 33))
    assert intact and np.array_equal(got["hits"], r["hits"])
    # a pose that makes every coordinate non-finite
    nan = IDENTITY.copy()
    nan[3] = np.nan
    r = check(wm, cells, nan, min_depth=0.05, max_depth=10.0, **view)
    assert r["n_clipped"] == r["n_cells"] == len(cells["keys"])
    wm.close()


def test_hand_cases_on_the_device(ctx):
    """the hand cases of test_world_map_render_cpu.py: a leaf of 0.5 puts each hand point at the centre of a cell of its
    own when its coordinates are odd multiples of 0.25"""
    wm, rm = d.WorldMap(ctx, 0.5, 8), ref.ReferenceMap(0.5)
    pts = np.float32([[0.25, 0.25, 2.25], [-6.75, -4.25, 2.25], [6.75, 4.75, 2.25], [-3.25, 0.25, 2.25]])
    assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY) == 0
    cells = rm.extract()
    assert np.array_equal(np.sort(cells["xyz"], axis=0), np.sort(pts, axis=0))
    for splat in (0, 1, 4):
        for f in (1.0, 2.25, 4.5):
            check(wm, cells, IDENTITY, splat=splat, **rref.hand_view(f=f))
    # one cell on the optical axis, exactly one pixel
    one, one_ref = d.WorldMap(ctx, 4.0, 8), ref.ReferenceMap(4.0)
    p = np.float32([[0, 0, 2]])
    one.integrate(p, IDENTITY), one_ref.integrate(p, IDENTITY)
    assert np.array_equal(one_ref.extract()["xyz"], p)             # (a single point is its cell's centroid)
    r = check(one, one_ref.extract(), IDENTITY, **rref.hand_view())
    want = np.zeros((5, 7), np.float32)
    want[2, 3] = 2.0
    assert np.array_equal(r["depth"], want) and r["hits"].sum() == 1
    # the half-pixel boundary and the pixel left of the image, by moving the view instead of the cell
    for tx, col in ((-1.5, 2), (np.nextafter(-1.5, -2.0), 1), (-3.5, 0), (np.nextafter(-3.5, -4.0), None)):
        T = IDENTITY.copy()
        T[3], T[11] = tx, -1.0                                     # X = tx, Z = 1: u = tx + 3
        r = check(one, one_ref.extract(), T, **rref.hand_view())
        if col is None:
            assert r["n_outside"] == 1 and not r["hits"].any()
        else:
            assert r["hits"][2, col] == 1 and r["hits"].sum() == 1
    # Z on the clip planes is kept, an ulp beyond is clipped; Z = 0 and Z < 0 are clipped
    for tz, lo, hi, drawn in ((0.0, 2.0, 3.0, 1), (0.0, 1.0, 2.0, 1), (0.0, float(np.nextafter(2.0, 3.0)), 3.0, 0),
                              (0.0, 1.0, float(np.nextafter(2.0, 1.0)), 0), (-2.0, rref.FLT_MIN, 3.0, 0), (-5.0, rref.FLT_MIN, 3.0, 0)):
        T = IDENTITY.copy()
        T[11] = tz
        r = check(one, one_ref.extract(), T, **rref.hand_view(lo=lo, hi=hi))
        assert (r["n_drawn"], r["n_clipped"]) == (drawn, 1 - drawn)
    wm.close()
    one.close()


@pytest.mark.parametrize("second_twice", [True, False])
def test_exact_tie_on_the_device(ctx, second_twice):
    wm, rm = d.WorldMap(ctx, 0.5, 8), ref.ReferenceMap(0.5)
    for pts in rref.tie_calls(second_twice):
        assert wm.integrate(pts, IDENTITY) == rm.integrate(pts, IDENTITY) == 0
    ref.assert_maps_equal(wm.extract(), rm.extract())
    r = check(wm, rm.extract(), IDENTITY, **rref.hand_view())
    assert r["hits"][2, 3] == 2 and r["windows"][2, 3] == 2 and r["depth"][2, 3] == np.float32(10.25) and r["n_pixels"] == 1
    r = check(wm, rm.extract(min_windows=2), IDENTITY, min_windows=2, **rref.hand_view())
    assert r["hits"][2, 3] == 1 and r["windows"][2, 3] == 2
    wm.close()


def test_round_trip_from_first_principles(ctx):
    """No restatement: a mapper's filtered depth map goes into a map of 0.1 mm cells and is rendered back through the
    mapper's own virtual camera.  The centroid of a cell holding one point lies at most two quanta leaf * 2^-32 (plus double
    roundings) below the point -- far under half a float ulp at depths >= 0.1 m -- so the depth is expected back exactly;
    1 ulp is the allowance."""
    rig = syn.stereo_rig(60_000, width=64, height=48, t0=10.0, duration=0.05, seed=5, n_points=400)
    cam = rig["cam"]
    m = d.MapperEMVS(ctx, cam, d.ShapeDSI(0, 0, 16, 4.0, 50.0, 0.0))
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    depth, _, mask = m.getDepthMapFromDSI(None, d.OptionsDepthMap())
    opts_pc = d.OptionsPointCloud(2.0, 1)
    cloud = m.getPointcloud(options_pc=opts_pc)
    leaf = 1e-4
    wm = d.WorldMap(ctx, leaf, 8)
    n, rejected = wm.integrate_mapper(m, IDENTITY, opts_pc)
    assert n == len(cloud) > 50 and rejected == 0
    fx, fy, cx, cy = m.virtual_cam_
    r = wm.render(IDENTITY, m.dimX, m.dimY, fx, fy, cx, cy, 0.1, 100.0)
    assert r["n_cells"] == r["n_drawn"] == wm.count() and r["n_clipped"] == r["n_outside"] == 0
    # the pixels that survived the point-cloud filter: each point lies on its pixel's ray, at the map's depth
    xyz = cloud[:, :3].astype(np.float64)
    u = np.rint(fx * xyz[:, 0] / xyz[:, 2] + cx).astype(int)
    v = np.rint(fy * xyz[:, 1] / xyz[:, 2] + cy).astype(int)
    assert (mask[v, u] > 0).all() and np.array_equal(depth[v, u], cloud[:, 2]) and len(set(zip(u.tolist(), v.tolist()))) == len(cloud)
    # two points in one 0.1 mm cell would share a centroid: such pixels are skipped, at most 1 % of them
    ok, c, _ = ref.cells(cloud, IDENTITY, leaf)
    assert ok.all()
    keys = ref.pack_key(c)
    uniq, inverse, count = np.unique(keys, return_inverse=True, return_counts=True)
    alone = count[inverse] == 1
    print("points %d, sharing a cell %d" % (len(cloud), int((~alone).sum())))
    assert (~alone).sum() * 100 <= len(cloud)
    got = r["depth"][v[alone], u[alone]]
    assert (r["mask"][v[alone], u[alone]] == 1).all() and (r["hits"][v[alone], u[alone]] >= 1).all()
    z = cloud[alone, 2]
    assert (np.abs(got.astype(np.float64) - z.astype(np.float64)) <= np.spacing(z).astype(np.float64)).all()
    print("depths returned exactly: %d of %d" % (int((got == z).sum()), len(z)))
    if alone.all():
        assert r["n_pixels"] == len(cloud)
    # the picture of it
    img = wm.renderImage(4.0, 50.0)
    assert img.shape == (m.dimY, m.dimX, 3) and img.dtype == np.uint8
    neg, want = d.depth_images(ctx, r["depth"], np.zeros_like(r["depth"]), r["mask"], 4.0, 50.0)
    assert np.array_equal(img, want)
    m.close()
    wm.close()


def test_score_glue(ctx, scene):
    wm, rm = scene
    v = rref.SCENE_VIEW
    rng = np.random.default_rng(14)
    shape = (v["height"], v["width"])
    poses = []
    for k in range(3):                                            # camera poses in the world: T_w_v
        a = 0.05 * (k - 1)
        poses.append(np.array([np.cos(a), 0, np.sin(a), 0.1 * k, 0, 1, 0, 0.02 * k, -np.sin(a), 0, np.cos(a), -0.1 * k], np.float64))
    gts = [np.where(rng.random(shape) < 0.8, rng.uniform(0.5, 5.0, shape), 0.0).astype(np.float32) for _ in poses]
    cam = (v["width"], v["height"], v["fx"], v["fy"], v["cx"], v["cy"])
    args = (v["width"], v["height"], v["fx"], v["fy"], v["cx"], v["cy"], v["min_depth"], v["max_depth"])
    new = lambda: d.DepthScore(ctx, 3 * shape[0] * shape[1], 0.6, v["fx"])
    # one frame: the render where it lies == the fetched arrays uploaded again
    r = wm.render(d.invert_pose(poses[0]), *args, splat=1)
    a, b = new(), new()
    a.addMapRender(wm, gts[0])
    b.add(r["depth"], r["mask"], gts[0])
    assert a.metrics()["n_joint"] > 500 and same_metrics(a.metrics(), b.metrics())
    # the same through a projector (one that copies its input)
    p = d.GroundTruthProjector(ctx, v["width"], v["height"], Q_IMAGE, np.eye(4), K_IMAGE)
    p.project(gts[0])
    held = p.fetch()[0]
    assert (held > 0).sum() > 1000
    a, b = new(), new()
    a.addMapRender(wm, p)
    b.add(r["depth"], r["mask"], held)
    assert a.metrics()["n_joint"] > 500 and same_metrics(a.metrics(), b.metrics())
    small = d.GroundTruthProjector(ctx, v["width"] - 1, v["height"], Q_IMAGE, np.eye(4), K_IMAGE)
    assert code_of(lambda: a.addMapRender(wm, small)) == E.ERR_INVALID
    with pytest.raises(ValueError):
        a.addMapRender(wm, gts[0][:, :-1])
    # process.score_world_map over three frames == three manual render-and-add steps (one frame through the projector)
    a, b = new(), new()
    counts = proc.score_world_map(wm, a, [(poses[0], p), (poses[1], gts[1]), (poses[2], gts[2])], cam, v["min_depth"], v["max_depth"],
                                  splat=1, min_windows=1)
    manual = []
    for T_w_v, gt in zip(poses, [held, gts[1], gts[2]]):
        r = wm.render(d.invert_pose(T_w_v), *args, splat=1)
        b.add(r["depth"], r["mask"], gt)
        manual.append({k: r[k] for k in counts[0]})
    assert counts == manual and len(counts) == 3 and set(counts[0]) == set(rref.COUNTS) | {"width", "height"}
    assert b.metrics()["n_joint"] > 1500 and same_metrics(a.metrics(), b.metrics())
    for o in (p, small):
        o.close()


def test_invalidation_and_contexts(ctx):
    wm = d.WorldMap(ctx, 0.5, 8)
    score = d.DepthScore(ctx, 64, 0.6, 1.0)
    gt = np.ones((5, 7), np.float32)
    args = (IDENTITY, 7, 5, 1.0, 1.0, 3.0, 2.0, 0.5, 100.0)
    assert code_of(wm.fetchRender) == E.ERR_INVALID                 # before the first render
    wm.integrate(np.float32([[0.25, 0.25, 2.25]]), IDENTITY)
    wm.render(*args)
    assert wm.fetchRender()["hits"].sum() == 1
    score.addMapRender(wm, gt)
    wm.integrate(np.zeros((0, 3), np.float32), IDENTITY)            # any integrate call, even an empty one
    assert code_of(wm.fetchRender) == E.ERR_INVALID
    assert code_of(lambda: score.addMapRender(wm, gt)) == E.ERR_INVALID
    wm.render(*args, fetch=False)
    assert wm.fetchRender()["hits"].sum() == 1
    wm.reset()
    assert code_of(wm.fetchRender) == E.ERR_INVALID
    assert code_of(lambda: score.addMapRender(wm, gt)) == E.ERR_INVALID
    p = d.GroundTruthProjector(ctx, 7, 5, Q_IMAGE, np.eye(4), K_IMAGE)
    assert code_of(lambda: score.addMapRender(wm, p)) == E.ERR_INVALID
    assert wm.render(*args)["n_cells"] == 0                         # an empty map renders an empty image
    assert not wm.fetchRender()["mask"].any()
    # a bad view leaves the last render standing
    assert code_of(lambda: wm.render(*args, splat=5)) == E.ERR_INVALID
    assert not wm.fetchRender()["mask"].any()
    # a score or a projector of another context
    other = d.Context(0)
    foreign = d.DepthScore(other, 64, 0.6, 1.0)
    assert code_of(lambda: foreign.addMapRender(wm, gt)) == E.ERR_CONTEXT
    q = d.GroundTruthProjector(other, 7, 5, Q_IMAGE, np.eye(4), K_IMAGE)
    assert code_of(lambda: score.addMapRender(wm, q)) == E.ERR_CONTEXT
    assert code_of(lambda: foreign.addMapRender(wm, q)) == E.ERR_CONTEXT
    for o in (q, foreign, p, score, wm):
        o.close()
    other.close()
