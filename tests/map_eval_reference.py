"""The world map's 3-D scoring restated in numpy (include/dsi_map_eval.h; DESIGN.md 7j "Scoring the map in 3-D").

Elementwise float64 operations only, as world_map_reference.py: every product and sum is rounded on its own.

    back-projection  pixel (u, v) of depth d is kept iff (mask is None or mask > 0) and d is finite and min <= d <= max;
                     x = float32(((u - cx) / fx) * d), y = float32(((v - cy) / fy) * d), z = d, in pixel order
    compare          for every cell of a (ReferenceMap.extract(): float32 centroids by ascending key):
                     c = floor(p / leaf_b) per axis; candidates: the cells of b at c + o, |o| <= reach per axis,
                     |c + o| <= 2^20 - 2; d2 = ((dx dx) + dy dy) + dz dz, the minimum kept; d = sqrt(min d2);
                     matched iff d <= radius; bin = min(floor(d / (radius / n_bins)), n_bins - 1);
                     sum_q += uint64(floor((d / radius) * 2^32)); dist = float32(d), +inf when unmatched
The lookup is sorted keys + np.searchsorted, swept over the (2 reach + 1)^3 offsets.
"""
import numpy as np

import world_map_reference as ref
import world_map_render_reference as rref

TWO32 = 4294967296.0
IDENTITY = rref.IDENTITY


def backproject(depth, mask, fx, fy, cx, cy, min_depth, max_depth):
    """(N, 3) float32 points of the pixels integrated, in pixel order (row-major)."""
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    d = depth.astype(np.float64)
    with np.errstate(all="ignore"):
        keep = np.isfinite(d) & (d >= np.float64(min_depth)) & (d <= np.float64(max_depth))
    if mask is not None:
        keep &= np.asarray(mask).reshape(h, w) > 0
    v, u = np.nonzero(keep)                                             # row-major: pixel order
    dd = d[v, u]
    x = ((u.astype(np.float64) - np.float64(cx)) / np.float64(fx)) * dd
    y = ((v.astype(np.float64) - np.float64(cy)) / np.float64(fy)) * dd
    with np.errstate(over="ignore"):
        return np.stack([x.astype(np.float32), y.astype(np.float32), depth[v, u]], axis=1)


def reach_of(radius, leaf_b):
    return int(np.ceil(np.float64(radius) / np.float64(leaf_b)))


def compare(cells_a, cells_b, leaf_b, radius, n_bins, details=False):
    """cells_a / cells_b: ReferenceMap.extract() (or WorldMap.extract()) of the two maps, already filtered, by ascending
    key.  Returns the dict WorldMap.compare(..., distances=True) returns: hist uint64 [n_bins], n_cells, n_matched,
    n_unmatched, sum_q, reach, keys (a's), dist float32.  details=True adds, per cell of a, `offset` (int64 [M][3], the
    winner's cell offset, 0 where unmatched or without candidate) and `found`."""
    radius, leaf_b = np.float64(radius), np.float64(leaf_b)
    reach = reach_of(radius, leaf_b)
    assert 1 <= reach <= 3 and 1 <= n_bins <= 4096
    p = np.asarray(cells_a["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    q_all = np.asarray(cells_b["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    keys_b = np.asarray(cells_b["keys"], np.uint64)
    assert (keys_b[1:] > keys_b[:-1]).all()
    M = p.shape[0]
    best = np.full(M, np.inf)
    found = np.zeros(M, bool)
    offset = np.zeros((M, 3), np.int64)
    with np.errstate(all="ignore"):
        c = np.floor(p / leaf_b)
        for oz in range(-reach, reach + 1):
            for oy in range(-reach, reach + 1):
                for ox in range(-reach, reach + 1):
                    if keys_b.shape[0] == 0:
                        continue
                    o = np.array([ox, oy, oz], np.float64)
                    v = c + o
                    inside = (np.abs(v) <= ref.CELL_MAX).all(axis=1)                # (NaN compares false)
                    key = ref.pack_key(np.where(inside[:, None], v, 0.0).astype(np.int64))
                    j = np.minimum(np.searchsorted(keys_b, key), keys_b.shape[0] - 1)
                    hit = inside & (keys_b[j] == key)
                    q = q_all[j]
                    dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
                    d2 = ((dx * dx) + dy * dy) + dz * dz
                    better = hit & (d2 < best)
                    best = np.where(better, d2, best)
                    offset[better] = (ox, oy, oz)
                    found |= hit
        d = np.sqrt(best)
        matched = d <= radius
        w = radius / np.float64(n_bins)
        dm = d[matched]
        bins = np.minimum(np.floor(dm / w), np.float64(n_bins - 1)).astype(np.int64)
        hist = np.bincount(bins, minlength=n_bins).astype(np.uint64)
        sum_q = int(np.floor((dm / radius) * TWO32).astype(np.uint64).sum(dtype=np.uint64))
        dist = np.where(matched, d, np.inf).astype(np.float32)
    out = {"hist": hist, "n_cells": M, "n_matched": int(matched.sum()), "n_unmatched": int(M - matched.sum()), "sum_q": sum_q,
           "reach": reach, "keys": np.asarray(cells_a["keys"], np.uint64), "dist": dist}
    if details:
        offset[~matched] = 0
        out.update(offset=offset, found=found, matched=matched, cell=c)
    return out


COUNTS = ("n_cells", "n_matched", "n_unmatched", "sum_q", "reach")


def assert_compares_equal(got, want, distances=True):
    """array_equal on the histogram, the counts and (by key) the float BITS of dist."""
    for k in COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], want["hist"]), "hist"
    if distances:
        assert np.array_equal(got["keys"], want["keys"]), "keys"
        assert got["dist"].dtype == np.float32 and want["dist"].dtype == np.float32
        assert np.array_equal(got["dist"].view(np.uint32), want["dist"].view(np.uint32)), "dist bits"


def f_score(fwd, bwd, radius, n_bins):
    """precision_completeness.py:44,60,76 from the integer counts of compare(est, gt) and compare(gt, est)."""
    w = np.float64(radius) / np.float64(n_bins)
    thresholds = (np.arange(n_bins, dtype=np.float64) + 1.0) * w
    with np.errstate(all="ignore"):
        P = 100.0 * np.cumsum(fwd["hist"]).astype(np.float64) / np.float64(fwd["n_cells"]) if fwd["n_cells"] else np.zeros(n_bins)
        R = 100.0 * np.cumsum(bwd["hist"]).astype(np.float64) / np.float64(bwd["n_cells"]) if bwd["n_cells"] else np.zeros(n_bins)
        f1 = np.where(P + R > 0, 2.0 * P * R / np.where(P + R > 0, P + R, 1.0), 0.0)
    return {"thresholds": thresholds, "precision": P, "recall": R, "f1": f1}


# ---- the scene the CPU and GPU tests compare (the issue's numbers) ----

LEAF_A, LEAF_B = 0.05, 0.04
RADII = (0.04, 0.08, 0.1)
N_BINS = 16


def scene_b_calls():
    """Map B's three calls: the scene's points with x < 1 plus Gaussian noise of sigma 0.02 (default_rng(5)) in two halves,
    then 3,000 uniform points."""
    rng = np.random.default_rng(5)
    pts = np.concatenate(rref.scene_calls())
    pts = pts[pts[:, 0] < 1]
    noisy = (pts.astype(np.float64) + rng.normal(0.0, 0.02, pts.shape)).astype(np.float32)
    half = len(noisy) // 2
    lo, hi = np.array([-2.0, -1.5, 1.0]), np.array([2.0, 1.5, 6.0])
    return [noisy[:half], noisy[half:], rng.uniform(lo, hi, size=(3000, 3)).astype(np.float32)]


def scene_maps():
    """(ReferenceMap A at leaf 0.05, ReferenceMap B at leaf 0.04)"""
    a, b = ref.ReferenceMap(LEAF_A), ref.ReferenceMap(LEAF_B)
    for pts in rref.scene_calls():
        assert a.integrate(pts, IDENTITY) == 0
    for pts in scene_b_calls():
        assert b.integrate(pts, IDENTITY) == 0
    return a, b


def depth_image(width, height, seed):
    """A depth image with every hostile value and a mask: (depth float32 (h, w), mask uint8 (h, w), lo, hi)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.float32(0.75), np.float32(6.5)
    depth = rng.uniform(0.5, 7.0, size=(height, width)).astype(np.float32)
    flat = depth.reshape(-1)
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(100)),
               np.nextafter(lo, np.float32(100)), np.nextafter(hi, np.float32(0))]
    where = rng.permutation(flat.shape[0])[:3 * len(special)]
    for k, i in enumerate(where):
        flat[i] = special[k % len(special)]
    mask = (rng.random((height, width)) < 0.8).astype(np.uint8) * np.uint8(rng.integers(1, 255))
    mask.reshape(-1)[where[:len(special)]] = 1                          # the first set of special values is not masked away
    return depth, mask, float(lo), float(hi)


def camera_pose(k=0):
    """camera -> world, 12 doubles: rotated about y, shifted"""
    a = 0.07 * (k + 1)
    return np.array([np.cos(a), 0, np.sin(a), 0.1 * k, 0, 1, 0, -0.05, -np.sin(a), 0, np.cos(a), 0.2 + 0.1 * k], np.float64)
