"""The world map's render restated in numpy (include/dsi_engine.h "the map rendered into a camera view").

Elementwise float64 operations only, as world_map_reference.py: every product and sum is rounded on its own.  The input
is ReferenceMap.extract() (or WorldMap.extract()): float32 centroids and their window counts, already filtered.

    point       the extracted float32 centroid, widened to double
    transform   X = ((r00 x + r01 y) + r02 z) + t0                       (rows 1, 2 for Y, Z)
    clipped     X, Y or Z not finite, or not (Z >= min_depth and Z <= max_depth)
    pixel       u = (fx * (X / Z)) + cx, iu = floor(u + 0.5); v, iv alike
    footprint   (iu + dx, iv + dy), |dx|, |dy| <= splat, each tested in double against the image
    outside     no footprint pixel inside the image
    drawn       per footprint pixel hits += 1, zkey = min(zkey, bits(float32(Z)) << 32 | (0xFFFFFFFF - windows))
    images      depth = float32(Z) of the winner (0 where hits == 0), windows, hits, mask = hits > 0
"""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTS = ("n_cells", "n_clipped", "n_outside", "n_drawn", "n_pixels")


def render(cells, T_v_w, width, height, fx, fy, cx, cy, min_depth, max_depth, splat=0):
    """cells: dict with xyz float32 (M, 3) and windows uint32 (M,).  Returns the dict WorldMap.render returns."""
    xyz = np.asarray(cells["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    win = np.asarray(cells["windows"], np.uint32).astype(np.uint64)
    T = np.asarray(T_v_w, np.float64).reshape(3, 4)
    fx, fy, cx, cy = np.float64(fx), np.float64(fy), np.float64(cx), np.float64(cy)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        X, Y, Z = [((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)]
        keep = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z >= np.float64(min_depth)) & (Z <= np.float64(max_depth))
        X, Y, Z, win = X[keep], Y[keep], Z[keep], win[keep]
        iu = np.floor(((fx * (X / Z)) + cx) + 0.5)
        iv = np.floor(((fy * (Y / Z)) + cy) + 0.5)
        key = (Z.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - win)
        npix = int(width) * int(height)
        zkey = np.full(npix, EMPTY, np.uint64)
        hits = np.zeros(npix, np.uint32)
        drawn = np.zeros(Z.shape[0], bool)
        for dy in range(-int(splat), int(splat) + 1):
            for dx in range(-int(splat), int(splat) + 1):
                pu, pv = iu + np.float64(dx), iv + np.float64(dy)               # still doubles: inf and NaN fail the tests
                inside = (pu >= 0.0) & (pu < np.float64(width)) & (pv >= 0.0) & (pv < np.float64(height))
                p = pv[inside].astype(np.int64) * int(width) + pu[inside].astype(np.int64)
                np.minimum.at(zkey, p, key[inside])
                np.add.at(hits, p, np.uint32(1))
                drawn |= inside
    covered = hits > 0
    depth = np.where(covered, (zkey >> np.uint64(32)).astype(np.uint32), np.uint32(0)).astype(np.uint32).view(np.float32)
    windows = np.where(covered, np.uint64(0xFFFFFFFF) - (zkey & np.uint64(0xFFFFFFFF)), np.uint64(0)).astype(np.uint32)
    shape = (int(height), int(width))
    n_cells, n_kept, n_drawn = int(keep.shape[0]), int(keep.sum()), int(drawn.sum())
    return {"width": int(width), "height": int(height), "n_cells": n_cells, "n_clipped": n_cells - n_kept,
            "n_outside": n_kept - n_drawn, "n_drawn": n_drawn, "n_pixels": int(covered.sum()),
            "depth": depth.reshape(shape), "windows": windows.reshape(shape), "hits": hits.reshape(shape),
            "mask": covered.astype(np.uint8).reshape(shape)}


def assert_renders_equal(got, want):
    """array_equal on the depth BITS, windows, hits, mask and the five counts."""
    for k in COUNTS + ("width", "height"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["depth"].dtype == np.float32 and want["depth"].dtype == np.float32
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), "depth bits"
    for k in ("windows", "hits", "mask"):
        assert got[k].dtype == want[k].dtype, k
        assert np.array_equal(got[k], want[k]), k


# ---- hand cases that the CPU tests put through the restatement and the GPU tests through the engine ----

FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)


def hand_view(width=7, height=5, f=1.0, cx=3.0, cy=2.0, lo=0.5, hi=100.0):
    return dict(width=width, height=height, fx=f, fy=f, cx=cx, cy=cy, min_depth=lo, max_depth=hi)


# Two cells far off the image on either side and one on the optical axis, whose splat of 4 covers a 7 x 5 image.  Per case
# (fx, r22): the third row of the pose is (0, 0, r22, 0), so Z = r22 and |u| = fx / r22 + 3 -- beyond 2^31, beyond 2^63,
# and infinite (1e300 * 1e30 overflows).  Dropped, never saturated: [n_cells, clipped, outside, drawn, pixels] = HUGE_COUNTS.
HUGE_POINTS = np.float32([[1, 1, 1], [-1, -1, 1], [0, 0, 1]])
HUGE_CASES = ((1e12, 1.0), (1e30, 1.0), (1e300, 1e-30))
HUGE_COUNTS = [3, 0, 2, 1, 35]


def huge_pose(r22):
    T = IDENTITY.copy()
    T[10] = r22
    return T


def tie_calls(second_twice):
    """leaf 0.5: (0.25, 0.25, 10.25) and (0.75, 0.25, 10.25) are the centres of two cells, on one pixel of hand_view() at
    one float depth; the second (or the first) of them is integrated in two calls"""
    a, b = np.float32([[0.25, 0.25, 10.25]]), np.float32([[0.75, 0.25, 10.25]])
    first, twice = (a, b) if second_twice else (b, a)
    return [np.concatenate([first, twice]), twice]


# ---- the random scene the GPU tests render (the issue's numbers) ----

SCENE_LEAF = 0.05
SCENE_VIEW = dict(width=64, height=48, fx=40.0, fy=40.0, cx=31.5, cy=23.5, min_depth=0.5, max_depth=5.0)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def scene_calls(seed=11, calls=5, n=4000):
    """Five calls of 4,000 float32 points, uniform in [-2, 2] x [-1.5, 1.5] x [1, 6]."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-2.0, -1.5, 1.0]), np.array([2.0, 1.5, 6.0])
    return [rng.uniform(lo, hi, size=(n, 3)).astype(np.float32) for _ in range(calls)]


def scene_pose():
    """The view: rotated 0.1 rad about y, t = (0.1, -0.05, 0.2); world -> view, 12 doubles."""
    c, s = np.cos(0.1), np.sin(0.1)
    return np.array([c, 0.0, s, 0.1, 0.0, 1.0, 0.0, -0.05, -s, 0.0, c, 0.2], np.float64)
