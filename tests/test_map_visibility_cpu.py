"""The visibility tally's restatement (tests/map_visibility_reference.py; include/dsi_map_visibility.h; DESIGN.md 7j
"Visibility") proved without a GPU: a constructed scene whose verdicts are known by plain reasoning, a brute-force scalar loop
in Python floats, the edge values of every comparison, the self-consistency of a map with its own render, the properties that
the GPU tests' layouts rely on, and the option checking of the stream stage."""
import math

import numpy as np
import pytest

import map_layout_cases as lc
import map_pca_reference as pr
import map_visibility_reference as vr
import world_map_reference as ref
import world_map_render_reference as rref
from dvs_mcemvs_amd import process as proc


# ---- 1. the constructed scene ----
def test_constructed_scene_has_the_verdicts_that_plain_reasoning_gives():
    s, rm = vr.wall_scene(), vr.wall_reference()
    depth, mask = vr.wall_depth()
    assert len(rm.keys) == len(s["points"])                                    # one cell per point
    cells = rm.extract(0, 0)
    ok, c, _ = ref.cells(s["points"], vr.IDENTITY, vr.WALL_LEAF)
    row = np.searchsorted(cells["keys"], ref.pack_key(c))
    assert ok.all() and np.array_equal(cells["xyz"][row], s["points"])         # the centroids are the points
    want = vr.wall_expected()
    tally = vr.Tally(rm)
    counts = tally.observe(depth, mask, window=0, **vr.WALL_VIEW)
    assert np.array_equal(tally.last[row], want)
    kind = np.array(vr.KINDS)[s["kind"]]
    assert set(want[kind == "wall"]) == {vr.AGREE} and set(want[kind == "clipped"]) == {vr.CLIPPED} and set(want[kind == "outside"]) == {vr.OUTSIDE}
    assert set(want[kind == "floater"]) == {vr.THROUGH, vr.UNSEEN} and set(want[kind == "behind"]) == {vr.BEHIND, vr.UNSEEN}
    assert all(counts[name] > 0 for name in vr.VERDICTS) and counts["n_cells"] == len(want) == sum(counts[n] for n in vr.VERDICTS)
    assert counts["n_valid_pixels"] == int(mask.sum()) == int((kind == "wall").sum()) and counts["views"] == 1
    rows = tally.rows()
    assert np.array_equal(rows["seen"][row], (want >= vr.AGREE).astype(np.uint32))
    assert np.array_equal(rows["agree"][row], (want == vr.AGREE).astype(np.uint32))
    assert np.array_equal(rows["through"][row], (want == vr.THROUGH).astype(np.uint32))
    sel = tally.select(1, 1)                                                   # one view that looks through carves: the floaters on wall pixels
    assert np.array_equal(sel["reason"][row], (want == vr.THROUGH).astype(np.uint8)) and sel["n_removed"] == counts["n_through"]
    # window 1 closes the holes of the wall's render: nothing in the frustum stays unseen, and a wall cell still agrees
    wide = vr.Tally(rm).observe(depth, mask, window=1, **vr.WALL_VIEW)
    assert wide["n_unseen"] == 0 and wide["n_agree"] == counts["n_agree"] and wide["n_through"] > counts["n_through"]


# ---- 2. the restatement against a scalar loop ----
def scalar_verdict(p, depth, mask, K, min_depth, max_depth, T, window, abs_tol, rel_tol):
    """one cell in Python floats: every operation a double, rounded on its own"""
    x, y, z = (float(v) for v in p)
    T = [float(v) for v in T]
    X, Y, Z = (((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3] for a in range(3))
    if not (math.isfinite(X) and math.isfinite(Y) and math.isfinite(Z) and min_depth <= Z <= max_depth):
        return vr.CLIPPED
    fx, fy, cx, cy = (float(v) for v in K)
    iu, iv = math.floor(((fx * (X / Z)) + cx) + 0.5), math.floor(((fy * (Y / Z)) + cy) + 0.5)
    height, width = depth.shape
    if not (0 <= iu <= width - 1 and 0 <= iv <= height - 1):
        return vr.OUTSIDE
    tol = (rel_tol * Z) + abs_tol
    lo, hi = Z - tol, Z + tol
    valid = agree = through = 0
    for dy in range(-window, window + 1):
        for dx in range(-window, window + 1):
            u, v = iu + dx, iv + dy
            if not (0 <= u < width and 0 <= v < height) or (mask is not None and mask[v, u] == 0):
                continue
            d = float(depth[v, u])
            if not (math.isfinite(d) and min_depth <= d <= max_depth):
                continue
            valid += 1
            agree += lo <= d <= hi
            through += d > hi
    return vr.UNSEEN if valid == 0 else vr.AGREE if agree else vr.THROUGH if through == valid else vr.BEHIND


@pytest.mark.parametrize("which", (0, 1))
def test_restatement_equals_the_scalar_loop(which):
    cells = pr.scene_reference().extract(0, 0)
    views = vr.scene_views(which)
    assert [v[6] for v in views] == [0, 1, 3] and [v[1] is None for v in views] == [True, False, False]
    seen = set()
    for depth, mask, K, lo, hi, T, window, abs_tol, rel_tol in views:
        d = depth[np.ones_like(depth, bool) if mask is None else mask > 0]
        assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d == 0).any() and (d > hi).any()
        got = vr.verdicts(cells["xyz"], depth, mask, K, lo, hi, T, window, abs_tol, rel_tol)
        want = [scalar_verdict(p, depth, mask, K, lo, hi, T, window, abs_tol, rel_tol) for p in cells["xyz"]]
        assert got.tolist() == want
        seen |= set(want)
    assert seen >= {vr.UNSEEN, vr.AGREE, vr.THROUGH, vr.BEHIND} and (which == 1 or vr.OUTSIDE in seen) and (which == 0 or vr.CLIPPED in seen)
    tally, counts = vr.scene_tally(which)
    assert [c["views"] for c in counts] == [1, 2, 3] and tally.seen.max() == 3
    assert np.array_equal(tally.seen.astype(np.int64), sum((vr.verdicts(cells["xyz"], *v) >= vr.AGREE).astype(np.int64) for v in views))
    assert (tally.agree + tally.through <= tally.seen).all()


# ---- 3. edge values ----
def one_cell(p, depth, mask=None, K=(1.0, 1.0, 0.0, 0.0), window=0, abs_tol=0.0, rel_tol=0.0, lo=0.5, hi=100.0):
    return int(vr.verdicts(np.float32([p]), np.float32(depth), mask, K, lo, hi, vr.IDENTITY, window, abs_tol, rel_tol)[0])


def test_tolerance_bounds_are_inclusive():
    up, down = (lambda v: np.nextafter(np.float32(v), np.float32(np.inf))), (lambda v: np.nextafter(np.float32(v), np.float32(-np.inf)))
    kw = dict(abs_tol=0.25)                                                     # Z = 2: lo = 1.75, hi = 2.25, all exact
    assert one_cell((0, 0, 2), [[1.75]], **kw) == vr.AGREE and one_cell((0, 0, 2), [[2.25]], **kw) == vr.AGREE
    assert one_cell((0, 0, 2), [[down(1.75)]], **kw) == vr.BEHIND and one_cell((0, 0, 2), [[up(2.25)]], **kw) == vr.THROUGH
    kw = dict(rel_tol=0.125)                                                    # the same bounds from the relative term
    assert one_cell((0, 0, 2), [[1.75]], **kw) == vr.AGREE and one_cell((0, 0, 2), [[up(2.25)]], **kw) == vr.THROUGH
    kw = dict(rel_tol=0.0625, abs_tol=0.125)                                    # and from both
    assert one_cell((0, 0, 2), [[2.25]], **kw) == vr.AGREE and one_cell((0, 0, 2), [[down(1.75)]], **kw) == vr.BEHIND
    assert one_cell((0, 0, 2), [[2.0]]) == vr.AGREE and one_cell((0, 0, 2), [[up(2.0)]]) == vr.THROUGH      # tolerance 0
    # the verdict's order: one agreeing pixel wins; without one, one nearer pixel protects the cell
    far, near = 9.0, 1.0
    assert one_cell((1, 1, 2), [[far, far, far], [far, 2.0, near], [far, far, far]], K=(2.0, 2.0, 0.0, 0.0), window=1) == vr.AGREE
    assert one_cell((1, 1, 2), [[far, far, far], [far, far, near], [far, far, far]], K=(2.0, 2.0, 0.0, 0.0), window=1) == vr.BEHIND
    assert one_cell((1, 1, 2), [[far, far, far], [far, far, np.nan], [far, 200.0, 0.0]], K=(2.0, 2.0, 0.0, 0.0), window=1) == vr.THROUGH
    mask = np.uint8([[1, 1, 1], [1, 1, 0], [1, 1, 1]])
    assert one_cell((1, 1, 2), [[far, far, far], [far, far, near], [far, far, far]], mask, K=(2.0, 2.0, 0.0, 0.0), window=1) == vr.THROUGH
    assert one_cell((1, 1, 2), [[far] * 3] * 3, np.zeros((3, 3), np.uint8), K=(2.0, 2.0, 0.0, 0.0), window=1) == vr.UNSEEN
    # the depth range is inclusive for the cell and for the pixel
    assert one_cell((0, 0, 0.5), [[0.5]]) == vr.AGREE and one_cell((0, 0, down(0.5)), [[0.5]]) == vr.CLIPPED
    assert one_cell((0, 0, 100), [[100.0]]) == vr.AGREE and one_cell((0, 0, 2), [[up(100.0)]]) == vr.UNSEEN


def test_pixel_rounding_and_the_centre_rule():
    img = [[9.0] * 3] * 3
    # u = x / 2 with K = (1, 1, 0, 0) at Z = 2: u = -0.5 rounds to pixel 0, the next double below it to pixel -1
    assert one_cell((-1, 0, 2), img) == vr.THROUGH
    assert one_cell((np.nextafter(np.float32(-1), np.float32(-2)), 0, 2), img) == vr.OUTSIDE
    assert one_cell((0, -1, 2), img) == vr.THROUGH and one_cell((0, np.nextafter(np.float32(-1), np.float32(-2)), 2), img) == vr.OUTSIDE
    # u = 2.5 rounds up to pixel 3, outside a 3 x 3 image, though its window reaches pixels 0..2; just below it is pixel 2
    assert one_cell((5, 0, 2), img, window=3) == vr.OUTSIDE
    assert one_cell((np.nextafter(np.float32(5), np.float32(0)), 0, 2), img, window=3) == vr.THROUGH
    assert one_cell((-1.5, 0, 2), img, window=1) == vr.OUTSIDE                  # pixel -1 with pixel 0 in its window
    # a corner cell reads only the pixels inside: the nearer pixel beyond the edge does not exist
    assert one_cell((0, 0, 2), [[9.0, 9.0, 1.0], [9.0, 9.0, 1.0], [1.0, 1.0, 1.0]], window=1) == vr.THROUGH
    assert one_cell((0, 0, 2), [[9.0, 9.0, 1.0], [9.0, 9.0, 1.0], [1.0, 1.0, 1.0]], window=2) == vr.BEHIND
    # huge and non-finite projections are dropped
    assert one_cell((1, 0, 2), img, K=(1e300, 1.0, 0.0, 0.0)) == vr.OUTSIDE and one_cell((3e38, 3e38, 2), img, K=(1e300, 1e300, 0.0, 0.0)) == vr.OUTSIDE


def hand_tally(seen, agree, through):
    t = vr.Tally(vr.wall_reference())
    n = len(seen)
    t.keys, t.seen, t.agree, t.through = t.keys[:n], np.uint32(seen), np.uint32(agree), np.uint32(through)
    return t


def test_selection_boundaries():
    t = hand_tally(seen=[5, 5, 5, 4, 3, 2, 0, 0xffffffff], agree=[2, 2, 2, 0, 3, 0, 0, 0x80000000], through=[2, 3, 1, 4, 0, 2, 0, 0x7fffffff])
    assert t.select(2, 1)["reason"].tolist() == [0, 1, 0, 1, 0, 1, 0, 0]       # through == agree_weight * agree is kept
    assert t.select(1, 1)["reason"].tolist() == [0, 1, 0, 1, 0, 1, 0, 0]
    assert t.select(3, 1)["reason"].tolist() == [0, 1, 0, 1, 0, 0, 0, 0]
    assert t.select(1, 0)["reason"].tolist() == [1, 1, 1, 1, 0, 1, 0, 1]       # agree_weight 0: any view that looks through carves
    assert t.select(2, 0)["reason"].tolist() == [1, 1, 0, 1, 0, 1, 0, 1]
    assert t.select(1, 2)["reason"].tolist() == [0, 0, 0, 1, 0, 1, 0, 0]
    assert t.select(1, 0xffffffff)["reason"].tolist() == [0, 0, 0, 1, 0, 1, 0, 0]    # the product needs 64 bits
    out = t.select(2, 1)
    assert out["n_cells"] == 8 and out["n_kept"] == 5 and out["n_removed"] == 3


# ---- 4. a map agrees with its own render ----
@pytest.mark.parametrize("scene", ("shapes", "render"))
def test_map_agrees_with_its_own_render(scene):
    rm = pr.scene_reference() if scene == "shapes" else vr.reference_of([(p, vr.IDENTITY) for p in rref.scene_calls()], rref.SCENE_LEAF)
    if scene == "shapes":
        T, (width, height), (fx, fy, cx, cy), (lo, hi) = vr.scene_views(0)[1][5], vr.VIEW_SIZE, vr.VIEW_K, vr.VIEW_RANGE
    else:
        T, v = rref.scene_pose(), rref.SCENE_VIEW
        width, height, fx, fy, cx, cy, lo, hi = (v[k] for k in ("width", "height", "fx", "fy", "cx", "cy", "min_depth", "max_depth"))
    r = rref.render(rm.extract(), T, width, height, fx, fy, cx, cy, lo, hi, splat=0)
    counts = vr.Tally(rm).observe(r["depth"], r["mask"], (fx, fy, cx, cy), lo, hi, T, window=0, rel_tol=2.0 ** -20)
    assert counts["n_through"] == 0 and counts["n_agree"] >= r["n_pixels"] > 100 and counts["n_unseen"] == 0
    assert counts["n_clipped"] == r["n_clipped"] and counts["n_outside"] == r["n_outside"] and counts["n_valid_pixels"] == r["n_pixels"]
    assert counts["n_agree"] + counts["n_behind"] == r["n_drawn"]


# ---- what the GPU tests' layouts rely on ----
@pytest.mark.parametrize("name", ("sparse", "dense"))
def test_layouts_get_every_verdict_in_both_rounds(name):
    rm = lc.sparse_reference() if name == "sparse" else lc.dense_reference()
    tally = vr.Tally(rm)
    tally.observe(*vr.layout_views(name)[0])
    for half in lc.halves(tally.keys):
        assert (np.bincount(tally.last[half], minlength=6) >= 10).all(), name
    whole, counts = vr.layout_tally(name)
    assert counts[1]["n_through"] == 0 and counts[1]["n_agree"] == counts[1]["n_valid_pixels"]   # the second view: its own render
    sel = whole.select(1, 1)
    assert all(20 <= int(sel["reason"][half].sum()) < int(half.sum()) for half in lc.halves(whole.keys))


def test_chain_observation_reaches_the_run_across_the_end():
    rm = lc.chain_reference("2^8")
    tally, counts = vr.tally_of(rm, vr.chain_views("2^8"))
    occ, run = lc.chain_run("2^8")
    assert run is not None and all(counts[0][k] >= 5 for k in ("n_unseen", "n_agree", "n_through", "n_behind", "n_outside"))


# ---- 5. the stream stage's options ----
def test_stream_stage_checks_its_options():
    stage = proc._MAP_STAGES[-1]                                               # the last row: it runs after the shapes stage
    assert stage.name == "world_map_carve" and [s.name for s in proc._MAP_STAGES].index("world_map_shapes") == len(proc._MAP_STAGES) - 2
    check = lambda opts, world_map=object(): proc._map_stage_options(stage, opts, world_map)
    good = dict(views=2, every=2, window=1, abs_tol=0.1, rel_tol=0.01, min_through=2, agree_weight=1, shrink=True)
    observe_opts, prune_opts, every, state = check(good)
    assert observe_opts == dict(window=1, abs_tol=0.1, rel_tol=0.01) and prune_opts == dict(min_through=2, agree_weight=1, shrink=True)
    assert every == 2 and state["ring"].maxlen == 2 and len(state["ring"]) == 0 and good["views"] == 2      # the caller's dict is not touched
    assert check(dict(views=3))[:3] == ({}, {}, 1)
    for bad, word in ((dict(good, radius=1.0), "unknown"), ({k: v for k, v in good.items() if k != "views"}, "views"), (dict(good, views=0), "views"),
                      (dict(good, views=1.5), "views"), (dict(good, views=True), "views"), (dict(good, every=0), "every"), (dict(good, every=1.5), "every"),
                      (dict(good, window=4), "window"), (dict(good, window=-1), "window"), (dict(good, abs_tol=-1.0), "abs_tol"),
                      (dict(good, rel_tol=float("nan")), "rel_tol"), (dict(good, abs_tol=float("inf")), "abs_tol"), (dict(good, min_through=0), "min_through"),
                      (dict(good, agree_weight=-1), "agree_weight")):
        with pytest.raises(ValueError, match=word):
            check(bad)
    with pytest.raises(ValueError, match="world_map_carve needs world_map"):
        check(good, world_map=None)
    # in full_sequence its keyword is checked first, before any other stage's and before anything touches a device
    with pytest.raises(ValueError, match="world_map_carve"):
        next(proc.full_sequence(None, None, None, None, None, 0.0, 1.0, 0.1, 0.1, world_map=object(), world_map_shapes=dict(keep=()),
                                world_map_carve=dict(good, bogus=1)))
    with pytest.raises(ValueError, match="world_map_carve needs world_map"):
        next(proc.full_sequence(None, None, None, None, None, 0.0, 1.0, 0.1, 0.1, world_map_carve=good))
    with pytest.raises(ValueError, match="no view"):
        proc.carve_world_map(_NoMap(), [], (1.0, 1.0, 0.0, 0.0), 0.5, 5.0)


class _NoMap:
    def clearVisibility(self):
        pass
