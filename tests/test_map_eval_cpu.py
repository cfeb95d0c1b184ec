"""The world map's 3-D scoring without a GPU (include/dsi_map_eval.h; DESIGN.md 7j "Scoring the map in 3-D"): the numpy
restatement (tests/map_eval_reference.py) against a brute-force nearest neighbour, hand cases, the conditions the GPU
tests' scene must meet, the argument checks and symbols of the four dsx_* entry points, and the new kernels' metadata."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.spatial import cKDTree

import dvs_mcemvs_amd as d
import map_eval_reference as mref
import world_map_reference as ref
import world_map_render_reference as rref
from dvs_mcemvs_amd import engine as E
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = rref.IDENTITY
NEW = ("dsx_map_integrate_depth", "dsx_map_integrate_depth_gt", "dsx_map_compare", "dsx_map_compare_fetch")
NEW_KERNELS = ("k_map_integrate_depth", "k_map_compare", "k_map_compare_gather")


def cells(points, leaf):
    """the extraction of a map of one call of the points given"""
    rm = ref.ReferenceMap(leaf)
    assert rm.integrate(np.asarray(points, np.float32).reshape(-1, 3), IDENTITY) == 0
    return rm.extract()


@pytest.fixture(scope="module")
def scene():
    a, b = mref.scene_maps()
    return a.extract(), b.extract()


def cases(scene):
    """the six cases: (name, cells of the first map, cells of the second, the second's leaf, radius)"""
    ca, cb = scene
    for radius in mref.RADII:
        yield "a->b r=%g" % radius, ca, cb, mref.LEAF_B, radius
        yield "b->a r=%g" % radius, cb, ca, mref.LEAF_A, radius


def brute_force(ca, cb, radius):
    """float64 distance to the nearest centroid within radius, inf without one: the neighbours from a k-d tree (a ball a
    little larger than the radius, so that no rounding of the tree's own can lose one), the value from the same d2
    expression, the minimum over the ball"""
    p, q = ca["xyz"].astype(np.float64), cb["xyz"].astype(np.float64)
    out = np.full(len(p), np.inf)
    if len(q) == 0:
        return out
    balls = cKDTree(q).query_ball_point(p, float(radius) * (1.0 + 1e-9))
    for i, ball in enumerate(balls):
        if ball:
            dx, dy, dz = p[i, 0] - q[ball, 0], p[i, 1] - q[ball, 1], p[i, 2] - q[ball, 2]
            dd = np.sqrt((((dx * dx) + dy * dy) + dz * dz).min())
            if dd <= radius:
                out[i] = dd
    return out


def test_restatement_equals_brute_force_nearest_neighbour(scene):
    assert len(scene[0]["keys"]) == 19619
    for name, ca, cb, leaf_b, radius in cases(scene):
        r = mref.compare(ca, cb, leaf_b, radius, mref.N_BINS)
        want = brute_force(ca, cb, radius).astype(np.float32)
        assert np.array_equal(r["dist"].view(np.uint32), want.view(np.uint32)), name
        assert r["n_matched"] == int(np.isfinite(want).sum()) and r["n_cells"] == len(want), name


def test_random_scene_is_not_vacuous(scene):
    """What the GPU comparison on this scene relies on (floors that keep it from being vacuous, not tolerances): matched and
    unmatched cells, every bin, winners in another cell than the query's own index, winners at the edge of the reach."""
    for name, ca, cb, leaf_b, radius in cases(scene):
        r = mref.compare(ca, cb, leaf_b, radius, mref.N_BINS, details=True)
        moved = r["matched"] & (r["offset"] != 0).any(axis=1)
        edge = r["matched"] & (np.abs(r["offset"]) == r["reach"]).any(axis=1)
        print("%s: reach %d, matched %d, unmatched %d, min bin %d, other-cell winners %d, winners at reach %d" %
              (name, r["reach"], r["n_matched"], r["n_unmatched"], int(r["hist"].min()), int(moved.sum()), int(edge.sum())))
        assert r["n_matched"] >= 5000 and r["n_unmatched"] >= 300, name
        assert (r["hist"] > 0).all() and int(r["hist"].sum()) == r["n_matched"], name
        assert int(moved.sum()) >= 1000 and int(edge.sum()) >= 10, name
        assert r["n_cells"] == r["n_matched"] + r["n_unmatched"] == len(ca["keys"]), name
    assert sorted({mref.reach_of(r, l) for r in mref.RADII for l in (mref.LEAF_A, mref.LEAF_B)}) == [1, 2, 3]


def test_a_centroid_exactly_at_the_radius_and_in_the_last_bin():
    # leaf 0.5: single points at odd multiples of 0.25 are their cells' centroids, exactly
    a = cells([[0.25, 0.25, 0.25]], 0.5)
    b = cells([[0.75, 0.25, 0.25]], 0.5)
    assert np.array_equal(a["xyz"], np.float32([[0.25, 0.25, 0.25]])) and np.array_equal(b["xyz"], np.float32([[0.75, 0.25, 0.25]]))
    r = mref.compare(a, b, 0.5, 0.5, 8)                                # d == radius: matched, clamped into the last bin
    assert r["reach"] == 1 and r["n_matched"] == 1 and r["dist"][0] == np.float32(0.5)
    assert r["hist"].tolist() == [0] * 7 + [1] and r["sum_q"] == 1 << 32
    r = mref.compare(a, b, 0.5, float(np.nextafter(0.5, 0.0)), 8)      # a radius an ulp smaller: unmatched
    assert r["n_matched"] == 0 and r["n_unmatched"] == 1 and np.isposinf(r["dist"][0]) and not r["hist"].any() and r["sum_q"] == 0
    r = mref.compare(a, b, 0.5, 0.5625, 8)                             # d / w = 7.11: the last bin on its own merit
    assert r["hist"].tolist() == [0] * 7 + [1] and r["sum_q"] == int(np.floor((0.5 / 0.5625) * 2.0 ** 32))
    r = mref.compare(a, b, 0.5, 1.0, 8)                                # d / w = 4 exactly: bin 4, reach 2
    assert r["reach"] == 2 and r["hist"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and r["sum_q"] == 1 << 31


def test_a_map_against_itself_and_against_an_empty_map(scene):
    ca, cb = scene
    r = mref.compare(ca, ca, mref.LEAF_A, 0.08, 16)
    assert r["n_matched"] == r["n_cells"] == len(ca["keys"]) and r["sum_q"] == 0 and not r["dist"].any()
    assert r["hist"].tolist() == [len(ca["keys"])] + [0] * 15
    empty = ref.ReferenceMap(mref.LEAF_B).extract()
    r = mref.compare(ca, empty, mref.LEAF_B, 0.08, 16)
    assert r["n_matched"] == 0 and r["n_unmatched"] == len(ca["keys"]) and np.isposinf(r["dist"]).all() and not r["hist"].any()
    r = mref.compare(empty, ca, mref.LEAF_A, 0.08, 16)
    assert r["n_cells"] == 0 and r["dist"].shape == (0,) and not r["hist"].any()
    f = mref.f_score(r, mref.compare(ca, empty, mref.LEAF_B, 0.08, 16), 0.08, 16)
    assert not f["precision"].any() and not f["recall"].any() and not f["f1"].any()


def test_a_neighbour_beyond_the_key_range_is_skipped():
    # leaf 1: the outermost cell 2^20 - 2, whose upper neighbours do not exist -- the sweep must skip, not wrap, them
    top = float(ref.CELL_MAX)
    a = cells([[top + 0.5, 0.5, 0.5]], 1.0)
    b = cells([[top - 0.5, 0.5, 0.5], [-top + 0.5, 0.5, 0.5]], 1.0)
    assert ref.unpack_key(a["keys"])[0, 0] == ref.CELL_MAX
    r = mref.compare(a, b, 1.0, 1.0, 4, details=True)
    assert r["n_matched"] == 1 and r["dist"][0] == np.float32(1.0) and r["offset"][0].tolist() == [-1, 0, 0]
    # the key just past the range would alias another cell's bits if it were packed: nothing may be found there
    r = mref.compare(b, a, 1.0, 1.0, 4)
    assert r["n_matched"] == 1 and r["n_unmatched"] == 1
    # the same at the lower end, with a finer second map: c + o runs below -(2^20 - 2)
    lo = cells([[-top + 0.5, 0.5, 0.5]], 1.0)
    r = mref.compare(lo, lo, 1.0, 3.0, 4)
    assert r["reach"] == 3 and r["n_matched"] == 1 and r["dist"][0] == 0.0


def test_back_projection_by_hand():
    depth = np.float32([[2.0, np.nan, 0.0], [np.inf, 4.0, 8.0]])
    pts = mref.backproject(depth, None, 2.0, 4.0, 1.0, 0.5, 1.0, 8.0)
    assert np.array_equal(pts, np.float32([[-1.0, -0.25, 2.0], [0.0, 0.5, 4.0], [4.0, 1.0, 8.0]]))
    pts = mref.backproject(depth, np.uint8([[0, 1, 1], [1, 7, 0]]), 2.0, 4.0, 1.0, 0.5, 1.0, 8.0)
    assert np.array_equal(pts, np.float32([[0.0, 0.5, 4.0]]))
    assert mref.backproject(depth, None, 2.0, 4.0, 1.0, 0.5, float(np.nextafter(np.float32(2.0), np.float32(3.0))),
                            float(np.nextafter(np.float32(8.0), np.float32(0.0)))).shape == (1, 3)
    dimg, mask, lo, hi = mref.depth_image(67, 5, 3)
    pts = mref.backproject(dimg, mask, 40.0, 40.0, 33.0, 2.0, lo, hi)
    assert 100 < len(pts) < 67 * 5 and np.isfinite(pts).all() and pts[:, 2].min() == np.float32(lo) and pts[:, 2].max() == np.float32(hi)


def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    core = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    assert len(set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", core))) == 176 and "dsx_" not in core
    header = open(os.path.join(ROOT, "include", "dsi_map_eval.h")).read()
    declared = set(re.findall(r"DSI_API[^;(]*?\b(ds[ix]_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NEW)
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name                      # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "176 entry points" in readme and "dsi_map_eval.h" in readme and "%d entry points" % len(NEW) in readme
    for name in ("integrateDepth", "integrateGroundTruth", "compare", "fetchDistances"):
        assert hasattr(d.WorldMap, name)
    assert hasattr(d, "map_f_score")
    from dvs_mcemvs_amd import process as proc
    assert hasattr(proc, "ground_truth_map") and hasattr(proc, "score_world_map_3d")
    hpp = open(os.path.join(ROOT, "include", "dsi_engine.hpp")).read()
    for name in ("integrateDepth", "integrateGroundTruth", "fetchDistances", "map_f_score"):
        assert name in hpp, name


FLT_MIN, FLT_MAX = rref.FLT_MIN, rref.FLT_MAX
GOOD_IMAGE = dict(width=64, height=48, fx=40.0, fy=40.0, cx=31.5, cy=23.5, min_depth=0.5, max_depth=5.0)
BAD_IMAGES = [("width", 0, b"1 x 1"), ("height", -3, b"1 x 1"), ("width", 1 << 30, b"2^26"), ("fx", 0.0, b"fx"),
              ("fy", float("nan"), b"fx"), ("fx", float("inf"), b"fx"), ("cx", float("nan"), b"cx"), ("cy", float("-inf"), b"cx"),
              ("min_depth", 0.0, b"depth"), ("min_depth", float(np.nextafter(np.float64(FLT_MIN), 0.0)), b"depth"),
              ("min_depth", 5.0, b"depth"), ("min_depth", 6.0, b"depth"), ("max_depth", float("inf"), b"depth"),
              ("max_depth", float(np.nextafter(np.float64(FLT_MAX), np.inf)), b"depth"), ("min_depth", float("nan"), b"depth")]


def integrate_depth(L, handle, depth, T, **kw):
    g = dict(GOOD_IMAGE, **kw)
    return L.dsx_map_integrate_depth(handle, depth, None, g["width"], g["height"], g["fx"], g["fy"], g["cx"], g["cy"], g["min_depth"],
                                     g["max_depth"], T, None, None)


def integrate_gt(L, handle, gt, T, **kw):
    g = dict(GOOD_IMAGE, **kw)
    return L.dsx_map_integrate_depth_gt(handle, gt, g["fx"], g["fy"], g["cx"], g["cy"], g["min_depth"], g["max_depth"], T, None, None)


def test_abi_argument_checks_need_no_gpu(built):
    L = d.load_library()
    INV = E.ERR_INVALID
    fake = C.c_void_p(0x1000)                                                   # never dereferenced: the checks come first
    depth = (C.c_float * 4)()
    T = (C.c_double * 12)(*IDENTITY.tolist())
    # NULL handles and arrays
    assert integrate_depth(L, None, depth, T) == INV and b"map is null" in L.dsi_last_error()
    assert integrate_depth(L, fake, None, T) == INV and b"depth_host is null" in L.dsi_last_error()
    assert integrate_depth(L, fake, depth, None) == INV and b"T_w_c is null" in L.dsi_last_error()
    assert integrate_gt(L, None, fake, T) == INV and b"null" in L.dsi_last_error()
    assert integrate_gt(L, fake, None, T) == INV and b"null" in L.dsi_last_error()
    # every bound of the image and its pinhole in turn: judged before the map is looked at
    for field, value, word in BAD_IMAGES:
        assert integrate_depth(L, None, depth, T, **{field: value}) == INV, (field, value)
        assert word in L.dsi_last_error(), (field, value, L.dsi_last_error())
        if field not in ("width", "height"):                                    # (the projector brings its own size)
            assert integrate_gt(L, None, None, T, **{field: value}) == INV, (field, value)
            assert word in L.dsi_last_error(), (field, value, L.dsi_last_error())
    # the bounds themselves are legal: the complaint is then the missing map
    for kw in (dict(width=1 << 26, height=1), dict(min_depth=FLT_MIN), dict(max_depth=FLT_MAX), dict(fx=-40.0)):
        assert integrate_depth(L, None, depth, T, **kw) == INV and b"map is null" in L.dsi_last_error(), kw
    # the compare: options first, then the maps
    info = E._MapCompareInfo()
    opts = lambda radius=0.1, n_bins=16: E._MapCompareOpts(1, 1, 1, 1, radius, n_bins)
    assert L.dsx_map_compare(fake, fake, None, None, C.byref(info)) == INV and b"opts is null" in L.dsi_last_error()
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        assert L.dsx_map_compare(None, None, C.byref(opts(radius=radius)), None, None) == INV and b"radius" in L.dsi_last_error()
    for n_bins in (0, -1, 4097):
        assert L.dsx_map_compare(None, None, C.byref(opts(n_bins=n_bins)), None, None) == INV and b"n_bins" in L.dsi_last_error()
    assert L.dsx_map_compare(None, None, C.byref(opts(radius=5e-324, n_bins=2)), None, None) == INV and b"underflows" in L.dsi_last_error()
    for n_bins in (1, 4096):
        assert L.dsx_map_compare(None, fake, C.byref(opts(n_bins=n_bins)), None, None) == INV and b"map is null" in L.dsi_last_error()
    assert L.dsx_map_compare(fake, None, C.byref(opts()), None, None) == INV and b"map is null" in L.dsi_last_error()
    n = C.c_size_t()
    assert L.dsx_map_compare_fetch(None, None, None, 0, C.byref(n)) == INV and b"null" in L.dsi_last_error()
    assert L.dsx_map_compare_fetch(fake, None, None, 0, None) == INV and b"null" in L.dsi_last_error()
    assert L.dsi_abi_version() == 10


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_new_kernels_use_no_scratch():
    text = kernel_asm_text()
    seen = {}
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = [k for k in NEW_KERNELS if re.search(r"\d+%sE" % k, name)]
        if not short:
            continue
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, name
        assert val("wavefront_size") == 64 and val("max_flat_workgroup_size") == 256, name
        seen[short[0]] = (val("vgpr_count"), val("sgpr_count"), val("group_segment_fixed_size"))
    print(seen)
    assert set(seen) == set(NEW_KERNELS), seen
    # the histogram (4096 u32), two counts and sum_q in LDS; eight waves of the compare fit a SIMD
    assert seen["k_map_compare"][2] <= 4096 * 4 + 64 and seen["k_map_compare"][0] <= 64
    # the lookups only read: the compare's atomics are its counters', never a compare-and-swap on a table
    m = re.search(r"^(_ZN\w*\d+k_map_compareE\w*):.*?$(.*?)s_endpgm", text, re.S | re.M)
    assert m and "atomic_cmpswap" not in m.group(2) and "global_atomic_add_x2" in m.group(2)
