"""The world map's render without a GPU: the numpy restatement (tests/world_map_render_reference.py) on hand cases, the
exact tie, the conditions the GPU tests' random scene must meet, and the argument checks and symbols of the four entry
points (include/dsi_engine.h "the map rendered into a camera view")."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import world_map_reference as ref
import world_map_render_reference as rref
from dvs_mcemvs_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = rref.IDENTITY
NEW = ("dsi_map_render", "dsi_map_render_fetch", "dsi_score_add_map_render", "dsi_score_add_map_render_gt")


def cloud(points, windows=None):
    """cells as extract() gives them, from float32 centroids given directly"""
    xyz = np.asarray(points, np.float32).reshape(-1, 3)
    return {"xyz": xyz, "windows": np.ones(len(xyz), np.uint32) if windows is None else np.asarray(windows, np.uint32)}


view = rref.hand_view


def test_one_cell_on_the_optical_axis():
    r = rref.render(cloud([[0, 0, 2]]), IDENTITY, **view())
    want = np.zeros((5, 7), np.float32)
    want[2, 3] = 2.0
    assert np.array_equal(r["depth"], want) and r["depth"].dtype == np.float32
    assert np.array_equal(r["mask"], want > 0) and np.array_equal(r["hits"], (want > 0).astype(np.uint32))
    assert np.array_equal(r["windows"], (want > 0).astype(np.uint32))
    assert [r[k] for k in rref.COUNTS] == [1, 0, 0, 1, 1]


def test_splat_at_a_corner_draws_four_of_nine():
    # X / Z = -3, Y / Z = -2: pixel (0, 0)
    r = rref.render(cloud([[-6, -4, 2]]), IDENTITY, splat=1, **view())
    assert r["hits"].sum() == 4 and (r["hits"][:2, :2] == 1).all() and r["n_pixels"] == 4 and r["n_drawn"] == 1
    assert (r["depth"][:2, :2] == 2.0).all() and r["depth"].sum() == 8.0
    # the opposite corner, and a cell one pixel off the image whose splat still reaches it
    r = rref.render(cloud([[6, 4, 2], [8, 0, 2]]), IDENTITY, splat=1, **view())
    assert r["hits"][3:, 5:].tolist() == [[1, 2], [1, 1]] and r["hits"][1:4, 6].tolist() == [1, 1, 2] and r["hits"].sum() == 7
    assert r["n_drawn"] == 2 and r["n_outside"] == 0 and r["n_pixels"] == 6
    assert rref.render(cloud([[8, 0, 2]]), IDENTITY, splat=0, **view())["n_outside"] == 1


def test_half_pixel_boundary_goes_up_and_just_left_of_the_image_is_outside():
    # u = 1.5 exactly: floor(2.0) = 2; one ulp below: pixel 1
    r = rref.render(cloud([[-1.5, 0, 1]]), IDENTITY, **view())
    assert r["hits"][2, 2] == 1 and r["hits"].sum() == 1
    x = np.nextafter(np.float32(-1.5), np.float32(-2))
    r = rref.render(cloud([[x, 0, 1]]), IDENTITY, **view())
    assert r["hits"][2, 1] == 1 and r["hits"].sum() == 1
    # u = -0.5 exactly is pixel 0; u = -0.5 - eps is pixel -1: outside at splat 0, drawn at splat 1
    r = rref.render(cloud([[-3.5, 0, 1]]), IDENTITY, **view())
    assert r["hits"][2, 0] == 1 and r["n_outside"] == 0
    x = np.nextafter(np.float32(-3.5), np.float32(-4))
    r = rref.render(cloud([[x, 0, 1]]), IDENTITY, **view())
    assert [r[k] for k in rref.COUNTS] == [1, 0, 1, 0, 0] and not r["hits"].any() and not r["depth"].any()
    r = rref.render(cloud([[x, 0, 1]]), IDENTITY, splat=1, **view())
    assert r["n_drawn"] == 1 and r["hits"][1:4, 0].tolist() == [1, 1, 1] and r["hits"].sum() == 3


def test_clip_planes_are_closed_and_an_ulp_beyond_is_clipped():
    lo, hi = np.float32(0.75), np.float32(12.5)
    below, above = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(100))
    r = rref.render(cloud([[0, 0, lo], [hi, 0, hi], [0, 0, below], [0, 0, above]]), IDENTITY, **view(lo=float(lo), hi=float(hi)))
    assert [r[k] for k in rref.COUNTS] == [4, 2, 0, 2, 2]
    assert r["depth"][2, 3] == lo and r["depth"][2, 4] == hi and r["hits"].sum() == 2
    # Z <= 0 and Z = 0 (a division by zero) are clipped, whatever the range's lower end
    r = rref.render(cloud([[0, 0, 0], [1, 1, 0], [0, 0, -2], [0, 0, -0.0]]), IDENTITY, **view(lo=float(np.finfo(np.float32).tiny)))
    assert [r[k] for k in rref.COUNTS] == [4, 4, 0, 0, 0] and not r["hits"].any()
    # a pose that makes a coordinate non-finite
    T = IDENTITY.copy()
    T[3] = np.inf
    assert rref.render(cloud([[0, 0, 2]]), T, **view())["n_clipped"] == 1
    T[3] = np.nan
    assert rref.render(cloud([[0, 0, 2]]), T, **view())["n_clipped"] == 1


def test_huge_pixel_coordinates_are_dropped_not_saturated():
    for f, r22 in rref.HUGE_CASES:
        r = rref.render(cloud(rref.HUGE_POINTS), rref.huge_pose(r22), splat=4, **view(f=f, lo=1e-35, hi=10.0))
        assert [r[k] for k in rref.COUNTS] == rref.HUGE_COUNTS, (f, r)
        assert (r["hits"] == 1).all() and (r["depth"] == np.float32(r22)).all()


def tie_maps(second_twice):
    rm = ref.ReferenceMap(0.5)
    for pts in rref.tie_calls(second_twice):
        rm.integrate(pts, IDENTITY)
    return rm


@pytest.mark.parametrize("second_twice", [True, False])
def test_exact_depth_tie_goes_to_the_cell_seen_by_more_windows(second_twice):
    cells = tie_maps(second_twice).extract()
    assert np.array_equal(cells["xyz"], np.float32([[0.25, 0.25, 10.25], [0.75, 0.25, 10.25]]))
    assert cells["windows"].tolist() == ([1, 2] if second_twice else [2, 1])
    r = rref.render(cells, IDENTITY, **view())
    # u = 0.024 + 3 and 0.073 + 3: both pixel (3, 2)
    assert r["hits"][2, 3] == 2 and r["hits"].sum() == 2 and r["windows"][2, 3] == 2 and r["depth"][2, 3] == np.float32(10.25)
    # the winner is a matter of the window count, not of the order: with min_windows = 2 only the winner is left
    one = rref.render(tie_maps(second_twice).extract(min_windows=2), IDENTITY, **view())
    assert one["hits"][2, 3] == 1 and one["windows"][2, 3] == 2
    # a nearer cell beats both whatever its count
    cells["xyz"][0 if second_twice else 1, 2] = np.nextafter(np.float32(10.25), np.float32(0))
    r = rref.render(cells, IDENTITY, **view())
    assert r["windows"][2, 3] == 1 and r["depth"][2, 3] < np.float32(10.25)


def scene_reference():
    rm = ref.ReferenceMap(rref.SCENE_LEAF)
    for pts in rref.scene_calls():
        assert rm.integrate(pts, IDENTITY) == 0
    return rm


def test_random_scene_is_not_vacuous():
    """What the GPU comparison on this scene relies on: contended pixels, clipped and outside cells, and enough cells seen
    by two windows.  (Caps that keep the comparison from being vacuous, not tolerances.)"""
    rm = scene_reference()
    cells = rm.extract()
    r = rref.render(cells, rref.scene_pose(), splat=0, **rref.SCENE_VIEW)
    covered = int((r["hits"] > 0).sum())
    print("cells %d, windows >= 2: %d, covered %.0f %%, hits >= 2: %.0f %% of the image, clipped %d, outside %d" %
          (len(cells["keys"]), int((cells["windows"] >= 2).sum()), 100.0 * covered / r["hits"].size,
           100.0 * (r["hits"] >= 2).sum() / r["hits"].size, r["n_clipped"], r["n_outside"]))
    assert 2 * int((r["hits"] >= 2).sum()) >= covered > 0
    assert r["n_clipped"] > 0 and r["n_outside"] > 0
    assert int((cells["windows"] >= 2).sum()) >= 100
    assert r["n_cells"] == len(cells["keys"]) == r["n_clipped"] + r["n_outside"] + r["n_drawn"] and r["n_pixels"] == covered
    two = rref.render(rm.extract(min_windows=2), rref.scene_pose(), splat=2, **rref.SCENE_VIEW)
    assert two["n_drawn"] > 50 and (two["windows"][two["mask"] > 0] >= 2).all()


def test_symbols_are_declared_exported_and_bound(built):
    L = d.load_library()
    header = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    declared = set(re.findall(r"DSI_API[^;(]*?\b(dsi_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert getattr(L, name).argtypes is not None, name                     # bound in engine.py, exported by the library
    assert L.dsi_abi_version() == 10
    assert len(declared) == 176
    assert "%d entry points" % len(declared) in open(os.path.join(ROOT, "README.md")).read()
    for name in ("render", "fetchRender", "renderImage"):
        assert hasattr(d.WorldMap, name)
    assert hasattr(d.DepthScore, "addMapRender")
    from dvs_mcemvs_amd import process as proc
    assert hasattr(proc, "score_world_map")


def good_view():
    v = E._MapView()
    v.width, v.height, v.splat, v.min_points, v.min_windows = 64, 48, 0, 1, 1
    v.fx, v.fy, v.cx, v.cy, v.min_depth, v.max_depth = 40.0, 40.0, 31.5, 23.5, 0.5, 5.0
    v.T_v_w[:] = IDENTITY.tolist()
    return v


FLT_MIN, FLT_MAX = rref.FLT_MIN, rref.FLT_MAX
BAD_VIEWS = [("width", 0, b"1 x 1"), ("height", -3, b"1 x 1"), ("width", 1 << 30, b"2^26"), ("splat", -1, b"splat"),
             ("splat", 5, b"splat"), ("fx", 0.0, b"fx"), ("fy", float("nan"), b"fx"), ("fx", float("inf"), b"fx"),
             ("cx", float("nan"), b"cx"), ("cy", float("-inf"), b"cx"), ("min_depth", 0.0, b"depth"),
             ("min_depth", float(np.nextafter(np.float64(FLT_MIN), 0.0)), b"depth"), ("min_depth", 5.0, b"depth"),
             ("min_depth", 6.0, b"depth"), ("max_depth", float("inf"), b"depth"),
             ("max_depth", float(np.nextafter(np.float64(FLT_MAX), np.inf)), b"depth"), ("min_depth", float("nan"), b"depth")]


def test_abi_argument_checks_need_no_gpu(built):
    L = d.load_library()
    INV = E.ERR_INVALID
    info = E._MapRenderInfo()
    gt = (C.c_float * 4)()
    fake = C.c_void_p(0x1000)                                                  # never dereferenced: the checks come first
    # NULL handles
    assert L.dsi_map_render(None, C.byref(good_view()), C.byref(info)) == INV and b"map is null" in L.dsi_last_error()
    assert L.dsi_map_render(fake, None, C.byref(info)) == INV and b"view is null" in L.dsi_last_error()
    assert L.dsi_map_render_fetch(None, None, None, None, None) == INV and b"null" in L.dsi_last_error()
    assert L.dsi_score_add_map_render(None, fake, gt) == INV
    assert L.dsi_score_add_map_render(fake, None, gt) == INV
    assert L.dsi_score_add_map_render(fake, fake, None) == INV
    assert L.dsi_score_add_map_render_gt(None, fake, fake) == INV
    assert L.dsi_score_add_map_render_gt(fake, None, fake) == INV
    assert L.dsi_score_add_map_render_gt(fake, fake, None) == INV and b"null" in L.dsi_last_error()
    # every bound of dsi_map_view_t in turn: the view is judged before the map is looked at
    for field, value, word in BAD_VIEWS:
        v = good_view()
        setattr(v, field, value)
        assert L.dsi_map_render(None, C.byref(v), None) == INV, (field, value)
        assert word in L.dsi_last_error(), (field, value, L.dsi_last_error())
    # the bounds themselves are legal: the complaint is then the missing map
    for field, value in (("width", 1 << 26), ("splat", 4), ("min_depth", FLT_MIN), ("max_depth", FLT_MAX), ("fx", -40.0)):
        v = good_view()
        if field == "width":
            v.height = 1
        setattr(v, field, value)
        assert L.dsi_map_render(None, C.byref(v), None) == INV and b"map is null" in L.dsi_last_error(), field
    assert L.dsi_abi_version() == 10
