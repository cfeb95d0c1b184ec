"""The world map's visibility tally restated in numpy and Python ints (include/dsi_map_visibility.h; DESIGN.md 7j
"Visibility").  Elementwise float64 operations only, as world_map_render_reference.py: every product and sum is rounded on
its own.  The input is ReferenceMap.extract(0, 0): every occupied cell's float32 centroid, by ascending key.

    point      the extracted float32 centroid, widened; X = ((r00 x + r01 y) + r02 z) + t0, Y and Z alike
    clipped    X, Y or Z not finite, or not (Z >= min_depth and Z <= max_depth)
    pixel      iu = floor(((fx * (X / Z)) + cx) + 0.5), iv alike; outside unless 0 <= iu <= width - 1 and 0 <= iv <= height - 1
    window     (iu + dx, iv + dy), |dx|, |dy| <= window, each tested against the image; valid iff unmasked, finite and in range
    unseen     no valid pixel
    tolerance  tol = (rel_tol * Z) + abs_tol, lo = Z - tol, hi = Z + tol
    verdict    agree if any valid pixel has lo <= d <= hi; else through if every valid pixel has d > hi; else behind
    tally      seen, agree, through per cell over the observations
    selection  carved (1) iff through >= min_through and through > agree_weight * agree
"""
import functools

import numpy as np

import map_merge_reference as mref
import map_pca_reference as pr
import world_map_render_reference as rref

IDENTITY = rref.IDENTITY
CLIPPED, OUTSIDE, UNSEEN, AGREE, THROUGH, BEHIND = range(6)
VERDICTS = ("n_clipped", "n_outside", "n_unseen", "n_agree", "n_through", "n_behind")
COUNTS = ("n_cells",) + VERDICTS + ("n_valid_pixels", "views")


def pinhole(K):
    K = np.asarray(K, np.float64)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) if K.shape == (3, 3) else tuple(K.reshape(4))


def valid_pixels(depth, mask, min_depth, max_depth):
    """bool (height, width): the pixels an observation reads"""
    d = np.asarray(depth, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(d) & (d >= np.float64(min_depth)) & (d <= np.float64(max_depth))
    return ok if mask is None else ok & (np.asarray(mask, np.uint8) > 0)


def verdicts(xyz, depth, mask, K, min_depth, max_depth, T_v_w, window=1, abs_tol=0.0, rel_tol=0.0):
    """one view's verdict on every centroid of xyz (float32 (M, 3)): int64 [M] of CLIPPED .. BEHIND"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    depth = np.asarray(depth, np.float32)
    height, width = depth.shape
    ok = valid_pixels(depth, mask, min_depth, max_depth)
    d64 = depth.astype(np.float64)
    T = np.asarray(T_v_w, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(v) for v in pinhole(K))
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.full(len(xyz), CLIPPED, np.int64)
    with np.errstate(all="ignore"):
        X, Y, Z = [((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)]
        kept = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z >= np.float64(min_depth)) & (Z <= np.float64(max_depth))
        iu = np.floor(((fx * (X / Z)) + cx) + 0.5)
        iv = np.floor(((fy * (Y / Z)) + cy) + 0.5)
        inside = kept & (iu >= 0.0) & (iu <= np.float64(width - 1)) & (iv >= 0.0) & (iv <= np.float64(height - 1))
    out[kept & ~inside] = OUTSIDE
    j = np.flatnonzero(inside)
    pu, pv, Zj = iu[j].astype(np.int64), iv[j].astype(np.int64), Z[j]
    tol = (np.float64(rel_tol) * Zj) + np.float64(abs_tol)
    lo, hi = Zj - tol, Zj + tol
    n_valid, n_agree, n_through = (np.zeros(len(j), np.int64) for _ in range(3))
    for dy in range(-int(window), int(window) + 1):
        for dx in range(-int(window), int(window) + 1):
            qu, qv = pu + dx, pv + dy
            there = (qu >= 0) & (qu < width) & (qv >= 0) & (qv < height)
            cu, cv = np.clip(qu, 0, width - 1), np.clip(qv, 0, height - 1)
            v = there & ok[cv, cu]
            d = d64[cv, cu]
            with np.errstate(invalid="ignore"):
                n_valid += v
                n_agree += v & (d >= lo) & (d <= hi)
                n_through += v & (d > hi)
    out[j] = np.where(n_valid == 0, UNSEEN, np.where(n_agree > 0, AGREE, np.where(n_through == n_valid, THROUGH, BEHIND)))
    return out


class Tally:
    """The tally of one map as it stands: rows by ascending key, as WorldMap.fetchVisibility(sort=True) returns them"""

    def __init__(self, rm):
        cells = rm.extract(0, 0)
        self.keys, self.xyz = cells["keys"].copy(), cells["xyz"].copy()
        self.seen, self.agree, self.through = (np.zeros(len(self.keys), np.uint32) for _ in range(3))
        self.views = 0
        self.last = None

    def observe(self, depth, mask, K, min_depth, max_depth, T_v_w, window=1, abs_tol=0.0, rel_tol=0.0):
        """WorldMap.observe: the view's counts; the verdicts stay in self.last"""
        v = verdicts(self.xyz, depth, mask, K, min_depth, max_depth, T_v_w, window, abs_tol, rel_tol)
        self.last = v
        self.views += 1
        self.seen += (v >= AGREE).astype(np.uint32)
        self.agree += (v == AGREE).astype(np.uint32)
        self.through += (v == THROUGH).astype(np.uint32)
        out = {"n_cells": len(v), "n_valid_pixels": int(valid_pixels(depth, mask, min_depth, max_depth).sum()), "views": self.views}
        out.update({name: int((v == code).sum()) for code, name in enumerate(VERDICTS)})
        return out

    def rows(self):
        return {"keys": self.keys, "seen": self.seen, "agree": self.agree, "through": self.through}

    def select(self, min_through=2, agree_weight=1):
        """WorldMap.selectCarved in Python ints: dict of the counts and `reason` per cell"""
        assert min_through >= 1
        r = np.array([1 if int(t) >= min_through and int(t) > int(agree_weight) * int(a) else 0
                      for t, a in zip(self.through.tolist(), self.agree.tolist())], np.uint8).reshape(-1)
        return {"n_cells": len(r), "n_kept": int((r == 0).sum()), "n_removed": int((r == 1).sum()), "reason": r}

    def prune(self, rm, min_through=2, agree_weight=1):
        """WorldMap.pruneCarved on rm, the map this tally was made of; the tally is spent afterwards"""
        assert np.array_equal(rm.keys, self.keys)
        out = self.select(min_through, agree_weight)
        ok = out["reason"] == 0
        rm.keys, rm.n, rm.S = rm.keys[ok], rm.n[ok], rm.S[ok]
        rm.windows, rm.stamp = rm.windows[ok], rm.stamp[ok]
        return out


def assert_counts_equal(got, want):
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["n_cells"] == sum(got[k] for k in VERDICTS)


def assert_rows_equal(got, want):
    """array_equal on keys and the three columns of two tallies by ascending key"""
    for k in ("keys", "seen", "agree", "through"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def reference_of(calls, leaf):
    rm = mref.MergeReferenceMap(leaf)
    for pts, T in calls:
        rm.integrate(pts, T)
    return rm


# ---- the constructed scene: every verdict is known without the restatement ----
# Leaf 0.5 and one point per cell at the cell's centre: the centroids are the points, exactly.  Identity pose, f = 9 in a
# 33 x 25 image centred on (16, 12): a centre (x, y, z) lands on pixel (16 + 9 x / z, 12 + 9 y / z), rounded.  The wall's cells
# at z = 2.25 land on the odd pixels, so its render at splat 0 has holes on the even ones: a cell in front of a hole, or behind
# one, is UNSEEN at window 0.  The floaters at z = 0.75 land on odd pixels too: on the wall's.
WALL_LEAF = 0.5
WALL_VIEW = dict(K=(9.0, 9.0, 16.0, 12.0), min_depth=0.5, max_depth=4.0, T_v_w=IDENTITY)
WALL_SIZE = (33, 25)
KINDS = ("wall", "floater", "behind", "outside", "clipped")


def _centres(ix, iy, z):
    gx, gy = np.meshgrid(np.asarray(ix, np.float64), np.asarray(iy, np.float64), indexing="ij")
    return np.stack([0.25 + 0.5 * gx.ravel(), 0.25 + 0.5 * gy.ravel(), np.full(gx.size, z)], axis=1)


@functools.lru_cache(maxsize=None)
def wall_scene():
    """dict of points (float32 (N, 3), cell centres) and kind (index into KINDS per point): a wall of 16 x 12 cells at
    z = 2.25, floaters at z = 0.75 and z = 1.25 in front of it, cells at z = 3.25 behind it, cells at z = 2.25 far outside the frustum, and
    cells past max_depth (z = 4.75) and before min_depth (z = 0.25)"""
    parts = [_centres(range(-8, 8), range(-6, 6), 2.25), np.concatenate([_centres(range(-2, 2), range(-2, 2), 0.75), _centres(range(-3, 3), range(-2, 2), 1.25)]),
             _centres(range(-8, 8), range(-6, 6), 3.25), _centres((20, 21, -22), (0, 30), 2.25),
             np.concatenate([_centres(range(-2, 2), (0, 1), 4.75), _centres((0,), (0,), 0.25)])]
    kind = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    return {"points": np.concatenate(parts).astype(np.float32), "kind": kind}


@functools.lru_cache(maxsize=None)
def wall_reference():
    return reference_of([(wall_scene()["points"], IDENTITY)], WALL_LEAF)


@functools.lru_cache(maxsize=None)
def wall_depth():
    """the render of the wall alone at splat 0: (depth, mask)"""
    s = wall_scene()
    wall = reference_of([(s["points"][s["kind"] == 0], IDENTITY)], WALL_LEAF)
    fx, fy, cx, cy = WALL_VIEW["K"]
    r = rref.render(wall.extract(), IDENTITY, WALL_SIZE[0], WALL_SIZE[1], fx, fy, cx, cy, WALL_VIEW["min_depth"], WALL_VIEW["max_depth"], splat=0)
    return r["depth"], r["mask"]


def wall_expected():
    """per point of wall_scene(), by plain scalar reasoning at window 0 and tolerance 0: its verdict (CLIPPED .. BEHIND)"""
    s, (depth, mask) = wall_scene(), wall_depth()
    fx, fy, cx, cy = WALL_VIEW["K"]
    out = []
    for (x, y, z), kind in zip(s["points"].astype(np.float64).tolist(), s["kind"].tolist()):
        if KINDS[kind] == "clipped":
            out.append(CLIPPED)
            continue
        u, v = int(np.floor(fx * x / z + cx + 0.5)), int(np.floor(fy * y / z + cy + 0.5))
        if KINDS[kind] == "outside":
            assert not (0 <= u < WALL_SIZE[0] and 0 <= v < WALL_SIZE[1])
            out.append(OUTSIDE)
        elif not mask[v, u]:
            out.append(UNSEEN)                                                 # in front of (or behind) a hole of the wall's render
        else:
            assert depth[v, u] == np.float32(2.25)
            out.append({"wall": AGREE, "floater": THROUGH, "behind": BEHIND}[KINDS[kind]])
    return np.array(out, np.int64)


# ---- views of the local-shape scene (map_pca_reference.scene_calls): renders of the scene itself, disturbed ----
VIEW_SIZE = (64, 48)
VIEW_K = (20.0, 40.0, 31.5, 10.0)
VIEW_RANGE = (0.5, 4.6)


def _pose_y(angle, t):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c, 0.0, s, t[0], 0.0, 1.0, 0.0, t[1], -s, 0.0, c, t[2]], np.float64)


def disturbed_render(cells, T_v_w, size, K, depth_range, seed, splat=1):
    """(depth, mask): the reference render of `cells`, then per tile of 8 x 8 pixels kept, pulled nearer (x 0.7) or pushed away (x 1.4), and per pixel
    now and then replaced by NaN, +-inf, 0 or a depth beyond the range; the mask drops a fifth of the pixels at random"""
    fx, fy, cx, cy = K
    r = rref.render(cells, T_v_w, size[0], size[1], fx, fy, cx, cy, depth_range[0], depth_range[1], splat=splat)
    rng = np.random.default_rng(seed)
    depth = r["depth"].copy()
    tiles = rng.integers(0, 4, ((size[1] + 7) // 8, (size[0] + 7) // 8))        # per tile of 8 x 8 pixels: 0, 1 kept, 2 nearer, 3 away
    tile = np.kron(tiles, np.ones((8, 8), np.int64))[:size[1], :size[0]]
    depth[tile == 2] *= np.float32(0.7)
    depth[tile == 3] *= np.float32(1.4)
    what = rng.integers(0, 20, depth.shape)
    depth[what == 13] = np.nan
    depth[what == 14] = np.inf
    depth[what == 15] = 0.0
    depth[what == 16] = np.float32(2.0 * depth_range[1])
    depth[what == 17] = -np.inf
    mask = (r["mask"] * (rng.random(depth.shape) < 0.8)).astype(np.uint8) * np.uint8(3)
    return depth, mask


@functools.lru_cache(maxsize=None)
def scene_views(which=0):
    """two lists of three observations of the local-shape scene, as tuples of WorldMap.observe's arguments: windows 0, 1
    and 3, with and without mask, abs_tol and rel_tol at work"""
    cells = pr.scene_reference().extract(0, 0)
    poses = ((_pose_y(0.0, (0.0, 0.0, 2.0)), _pose_y(0.15, (0.2, -0.1, 2.5)), _pose_y(-0.2, (-0.5, 0.1, 1.5))),
             (_pose_y(0.05, (0.1, 0.0, 2.2)), _pose_y(-0.1, (0.0, 0.2, 3.0)), _pose_y(0.3, (0.4, 0.0, 2.0))))[which]
    settings = ((0, 0.02, 0.0, False), (1, 0.0, 0.01, True), (3, 0.01, 0.005, True))
    out = []
    for n, (T, (window, abs_tol, rel_tol, masked)) in enumerate(zip(poses, settings)):
        depth, mask = disturbed_render(cells, T, VIEW_SIZE, VIEW_K, VIEW_RANGE, 90 + 10 * which + n)
        out.append((depth, mask if masked else None, VIEW_K, VIEW_RANGE[0], VIEW_RANGE[1], T, window, abs_tol, rel_tol))
    return tuple(out)


def tally_of(rm, views):
    """(tally, the counts of every view) of the restatement"""
    t = Tally(rm)
    return t, [t.observe(*v) for v in views]


@functools.lru_cache(maxsize=None)
def scene_tally(which=0):
    return tally_of(pr.scene_reference(), scene_views(which))




# ---- the layouts (map_layout_cases): the view lc.SMALL_VIEW on the maps of two rounds and on the chain across the end ----
def observation_of(cells, view, window, abs_tol, rel_tol, splat=1, masked=True, disturb=None):
    """observe()'s arguments for the reference render of `cells` from `view` (a tuple as lc.SMALL_VIEW), disturbed as
    disturbed_render does with the seed `disturb`"""
    T, width, height, fx, fy, cx, cy, lo, hi = view
    if disturb is None:
        r = rref.render(cells, T, width, height, fx, fy, cx, cy, lo, hi, splat=splat)
        depth, mask = r["depth"], r["mask"]
    else:
        depth, mask = disturbed_render(cells, T, (width, height), (fx, fy, cx, cy), (lo, hi), disturb, splat)
    return (depth, mask if masked else None, (fx, fy, cx, cy), lo, hi, T, window, abs_tol, rel_tol)


@functools.lru_cache(maxsize=None)
def layout_views(name):
    """the observations of a table of two rounds: `sparse` sees the render of lc.other_reference() (another map of the
    same surface, noisier and with clutter), disturbed, and then its own render; `dense` the same other map and its own"""
    import map_layout_cases as lc
    own = (lc.sparse_reference() if name == "sparse" else lc.dense_reference()).extract(0, 0)
    view = lc.SMALL_VIEW if name == "sparse" else lc.SMALL_VIEW[:8] + (3.0,)      # (the dense block ends at z = 3.85: clip some of it)
    return (observation_of(lc.other_reference().extract(), view, 1, 0.05, 0.0, splat=0, disturb=97),
            observation_of(own, lc.SMALL_VIEW, 0, 0.0, 2.0 ** -20, splat=0, masked=False))


@functools.lru_cache(maxsize=None)
def layout_tally(name):
    import map_layout_cases as lc
    return tally_of(lc.sparse_reference() if name == "sparse" else lc.dense_reference(), layout_views(name))


CHAIN_VIEW = (_pose_y(0.1, (0.3, -0.2, 7.0)), 64, 48, 40.0, 40.0, 31.5, 23.5, 0.5, 12.0)


def chain_views(name):
    """the chain's map seen with the render of lc.chain_reference(name, ("first",)): the map before its second call"""
    import map_layout_cases as lc
    return (observation_of(lc.chain_reference(name, ("first",)).extract(), CHAIN_VIEW, 1, 0.0, 0.01, splat=0, disturb=98),)
