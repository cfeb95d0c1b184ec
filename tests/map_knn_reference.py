"""The world map's k nearest cells and its statistical outliers restated in numpy (include/dsi_map_knn.h; DESIGN.md 7j
"Neighbours and statistical outliers"): the box rule of the neighbours, the self query with its exact integer moments
(Python ints), the threshold, the selection and the prune, and the scenes that the GPU tests and the CPU tests share.
Every floating-point operation is a numpy float64 operation rounded on its own, in the order the header states."""
import functools
import itertools
import math

import numpy as np

import map_merge_reference as mref
import map_prune_reference as pref
import world_map_reference as ref

IDENTITY = pref.IDENTITY
Q_ONE = 1 << 30
MAX_K = 16


def reach_of(radius, leaf):
    return int(np.ceil(np.float64(radius) / np.float64(leaf)))


def neighbours(points, cells, leaf, radius, k, exclude=None):
    """points float64 (N, 3); cells: a ReferenceMap.extract() already filtered, by ascending key; exclude: None or uint64 [N],
    per query the key that is no candidate.  Returns dict of keys uint64 (N, k) padded with 0, d2 and d float64 (N, k) padded
    with +inf, dist float32 (N, k), found uint8 [N] and admitted int64 [N]."""
    radius, leaf = np.float64(radius), np.float64(leaf)
    reach = reach_of(radius, leaf)
    assert 1 <= reach <= 3 and 1 <= k <= MAX_K
    p = np.asarray(points, np.float64).reshape(-1, 3)
    N = p.shape[0]
    q_all = np.asarray(cells["xyz"], np.float32).reshape(-1, 3).astype(np.float64)
    keys_b = np.asarray(cells["keys"], np.uint64)
    assert (keys_b[1:] > keys_b[:-1]).all()
    span = range(-reach, reach + 1)
    offsets = list(itertools.product(span, span, span))
    D2 = np.full((N, len(offsets)), np.inf)
    KEY = np.full((N, len(offsets)), ~np.uint64(0), np.uint64)
    with np.errstate(all="ignore"):
        c = np.floor(p / leaf)
        if keys_b.shape[0] and N:
            for col, (oz, oy, ox) in enumerate(offsets):
                v = c + np.array([ox, oy, oz], np.float64)
                inside = (np.abs(v) <= ref.CELL_MAX).all(axis=1)                    # (NaN compares false)
                key = ref.pack_key(np.where(inside[:, None], v, 0.0).astype(np.int64))
                j = np.minimum(np.searchsorted(keys_b, key), keys_b.shape[0] - 1)
                hit = inside & (keys_b[j] == key)
                if exclude is not None:
                    hit &= key != np.asarray(exclude, np.uint64)
                q = q_all[j]
                dx, dy, dz = p[:, 0] - q[:, 0], p[:, 1] - q[:, 1], p[:, 2] - q[:, 2]
                d2 = ((dx * dx) + dy * dy) + dz * dz
                admitted = hit & (np.sqrt(d2) <= radius)
                D2[:, col] = np.where(admitted, d2, np.inf)
                KEY[:, col] = np.where(admitted, key, ~np.uint64(0))
    order = np.lexsort((KEY, D2), axis=1)[:, :k]                                   # by (d2, key): a total order
    d2 = np.take_along_axis(D2, order, axis=1)
    keys = np.take_along_axis(KEY, order, axis=1)
    if d2.shape[1] < k:                                                            # (k above the number of offsets cannot happen: 27 >= 16)
        raise AssertionError
    admitted = np.isfinite(D2).sum(axis=1)
    has = np.isfinite(d2)
    d = np.sqrt(d2)
    return {"keys": np.where(has, keys, np.uint64(0)), "d2": d2, "d": d, "dist": d.astype(np.float32),
            "found": np.minimum(admitted, k).astype(np.uint8), "admitted": admitted, "reach": reach}


def query(rm, points, k, radius, min_points=1, min_windows=1):
    """WorldMap.query: the float32 points widened"""
    pts = np.asarray(points, np.float32)[:, :3].astype(np.float64)
    out = neighbours(pts, rm.extract(min_points, min_windows), rm.leaf, radius, k)
    return {f: out[f] for f in ("keys", "dist", "found")}


def self_query(rm, k, radius, min_found=1, min_points=1, min_windows=1):
    """WorldMap.knn and fetchKnn(sort=True) in one dict: the counts and moments (sum_q2 a Python int), and per query keys,
    found, mean float32 and q uint32; `rows` holds the neighbours' rows for the tests that look at them"""
    assert 1 <= min_found <= k
    cells = rm.extract(min_points, min_windows)
    p = cells["xyz"].astype(np.float64)
    nb = neighbours(p, cells, rm.leaf, radius, k, exclude=cells["keys"])
    found = nb["found"].astype(np.int64)
    s = np.zeros(len(found))
    with np.errstate(all="ignore"):
        for j in range(k):
            s = np.where(j < found, s + nb["d"][:, j], s)                          # (((d_1 + d_2) + ...) + d_found)
        m = s / found.astype(np.float64)
        q = np.where(found > 0, np.floor((m / np.float64(radius)) * np.float64(Q_ONE)), 0.0).astype(np.uint64)
    mean = np.where(found > 0, m, np.inf).astype(np.float32)
    scored = found >= min_found
    qs = [int(v) for v in q[scored]]
    return {"n_cells": len(found), "n_unqueried": len(rm.keys) - len(found), "n_scored": int(scored.sum()),
            "n_isolated": int((~scored).sum()), "sum_q": sum(qs), "sum_q2": sum(v * v for v in qs), "reach": nb["reach"],
            "keys": cells["keys"], "found": nb["found"], "mean": mean, "q": q.astype(np.uint32), "rows": nb,
            "min_found": min_found, "filter": (min_points, min_windows)}


COUNTS = ("n_cells", "n_unqueried", "n_scored", "n_isolated", "sum_q", "sum_q2", "reach")


def threshold(N, sum_q, sum_q2, std_mult):
    """dsx_map_knn_threshold with Python ints: int -> float rounds to nearest even, as the C conversions do"""
    N, sum_q, sum_q2 = int(N), int(sum_q), int(sum_q2)
    V = N * sum_q2 - sum_q * sum_q
    assert V >= 0
    if N == 0:
        return {"mu": 0.0, "sigma": 0.0, "T_q": Q_ONE, "V": V}
    mu = float(sum_q) / float(N)
    sigma = math.sqrt(float(V) / (float(N) * float(N - 1))) if N >= 2 else 0.0
    T = mu + float(std_mult) * sigma
    T_q = Q_ONE if T >= float(Q_ONE) else 0 if T < 0.0 else int(math.floor(T))
    return {"mu": mu, "sigma": sigma, "T_q": T_q, "V": V}


def select(rm, sq, std_mult):
    """WorldMap.selectOutliers on the self query sq of rm: dict of the counts, the threshold, and per OCCUPIED cell (by
    ascending key) `all_reason`; `reason` is the queries' (fetchKnn's)"""
    thr = threshold(sq["n_scored"], sq["sum_q"], sq["sum_q2"], std_mult)
    r = np.zeros(len(sq["keys"]), np.uint8)
    if std_mult >= 0:
        r[sq["q"].astype(np.uint64) > np.uint64(thr["T_q"])] = 3
    r[sq["found"].astype(np.int64) < sq["min_found"]] = 2                          # (written last = found first)
    every = np.ones(len(rm.keys), np.uint8)
    every[np.searchsorted(rm.keys, sq["keys"])] = r
    return {"n_cells": len(every), "n_kept": int((every == 0).sum()), "n_removed": [int((every == v).sum()) for v in (1, 2, 3)],
            "T_q": thr["T_q"], "mu": thr["mu"], "sigma": thr["sigma"], "reason": r, "all_reason": every}


class KnnReferenceMap(mref.MergeReferenceMap):
    def prune_outliers(self, sq, std_mult):
        out = select(self, sq, std_mult)
        keep = out["all_reason"] == 0
        self.keys, self.n, self.S = self.keys[keep], self.n[keep], self.S[keep]
        self.windows, self.stamp = self.windows[keep], self.stamp[keep]
        return out


def reference_of(calls, leaf):
    rm = KnnReferenceMap(leaf)
    for pts, T in calls:
        rm.integrate(pts, T)
    return rm


def brute_force(points, cells, radius, k, exclude=None):
    """all pairs, no cells: per query the candidates with sqrt(d2) <= radius ordered by (d2, key), cut at k"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    q = np.asarray(cells["xyz"], np.float32).astype(np.float64)
    keys = np.asarray(cells["keys"], np.uint64)
    out_k = np.zeros((len(p), k), np.uint64)
    out_d = np.full((len(p), k), np.inf)
    found = np.zeros(len(p), np.uint8)
    for i in range(len(p)):
        dx, dy, dz = p[i, 0] - q[:, 0], p[i, 1] - q[:, 1], p[i, 2] - q[:, 2]
        d2 = ((dx * dx) + dy * dy) + dz * dz
        ok = np.sqrt(d2) <= np.float64(radius)
        if exclude is not None:
            ok &= keys != exclude[i]
        idx = np.flatnonzero(ok)
        idx = idx[np.lexsort((keys[idx], d2[idx]))][:k]
        out_k[i, :len(idx)], out_d[i, :len(idx)], found[i] = keys[idx], np.sqrt(d2[idx]), len(idx)
    return {"keys": out_k, "d": out_d, "found": found}


# ---- the scenes ----
LEAF = 0.05
LATTICE_RADII = (0.05, 0.1, 0.15)                                               # reach 1, 2, 3
LATTICE_KS = (1, 3, 8, 16)


@functools.lru_cache(maxsize=None)
def lattice_calls():
    """2,028 cells, 13 x 13 x 12 with the same index range on every axis, one point per cell centre: neighbours along
    different axes lie at the same distance bit for bit wherever the indices agree, and the key decides"""
    g = np.arange(-6, 7)
    c = np.stack([a.ravel() for a in np.meshgrid(g, g, g[:-1], indexing="ij")], axis=1)
    pts = ((c + 0.5) * LEAF).astype(np.float32)
    pts = pts[np.random.default_rng(61).permutation(len(pts))]
    return ((pts[:1000], IDENTITY), (pts[1000:], IDENTITY))


@functools.lru_cache(maxsize=None)
def lattice_queries():
    rng = np.random.default_rng(62)
    centres = np.concatenate([p for p, _ in lattice_calls()])[::7]                 # on centroids: ties among the six neighbours
    anywhere = rng.uniform(-0.4, 0.4, (300, 3)).astype(np.float32)                 # inside, at the rim and outside
    return np.concatenate([centres, anywhere])


SPARSE_RADIUS, SPARSE_K = 0.12, 8                                               # reach 3


@functools.lru_cache(maxsize=None)
def sparse_calls():
    """700 points of a unit cube seen by three calls, about 60 % each: about five neighbours within the radius, so that
    admitted < k, = k and > k all happen; with min_windows = 2 some cells leave the candidates"""
    rng = np.random.default_rng(63)
    base = rng.uniform(-0.5, 0.5, (700, 3))
    calls = []
    for _ in range(3):
        pick = rng.random(len(base)) < 0.6
        calls.append(((base[pick] + rng.normal(0.0, 0.002, (int(pick.sum()), 3))).astype(np.float32), IDENTITY))
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def sparse_queries():
    rng = np.random.default_rng(64)
    return rng.uniform(-0.6, 0.6, (500, 4)).astype(np.float32)                     # stride 4


FACE_LEAF = 0.125


@functools.lru_cache(maxsize=None)
def face_calls():
    """the face and face +- 1 ulp points of test_gpu_world_map.py, one call: below a face the fraction is just under 1 and
    around 0 it rounds to 1, so the float32 centroid of such a cell lies ON its upper face -- in the next index"""
    k = np.arange(-9, 10, dtype=np.float32) * np.float32(FACE_LEAF)
    faces = np.stack(np.meshgrid(k, k[:5], k[:3], indexing="ij"), axis=-1).reshape(-1, 3)
    up = np.nextafter(faces, np.float32(np.inf))
    down = np.nextafter(faces, np.float32(-np.inf))
    pts = np.concatenate([faces, up, down])
    return ((pts[np.random.default_rng(65).permutation(len(pts))], IDENTITY),)


def moved_cells(rm):
    """the cells of rm whose extracted centroid floors into another index than their own (bool per key)"""
    cells = rm.extract(0, 0)
    with np.errstate(all="ignore"):
        c = np.floor(cells["xyz"].astype(np.float64) / np.float64(rm.leaf))
    return (c != ref.unpack_key(cells["keys"]).astype(np.float64)).any(axis=1)


PATCH_LEAF, PATCH_SPACING = 0.05, 0.1                                            # every second cell: spacing 2 leaves
PATCH_RADIUS, PATCH_PAIR = 0.135, 0.13                                           # reach 3; the patch's diagonals (0.141) lie outside


@functools.lru_cache(maxsize=None)
def patch_calls():
    """first principles: a planar 12 x 12 lattice patch of spacing s = 0.1 at z = 1.025, three pairs 0.13 apart far from the
    patch and from each other, five singletons farther still.  Coordinates are multiples of 1/40 plus a quarter leaf, exact in
    float32 as far as the sums below need"""
    g = np.arange(12)
    patch = np.stack([a.ravel() for a in np.meshgrid(g, g, indexing="ij")], axis=1) * 0.1 + 0.0125
    patch = np.column_stack([patch, np.full(len(patch), 1.0125)])
    pairs = np.array([[3.0125 + 2.0 * i, 0.0125, 1.0125] for i in range(3)])
    pairs = np.concatenate([pairs, pairs + np.array([0.13, 0.0, 0.0])])
    singles = np.array([[-3.0125 - 2.0 * i, 0.0125, 1.0125] for i in range(5)])
    pts = np.concatenate([patch, pairs, singles]).astype(np.float32)
    return ((pts, IDENTITY),), len(patch)


EDGE_LEAF = 0.5


@functools.lru_cache(maxsize=None)
def edge_calls():
    """cells at |c| = 2^20 - 2 on every axis and one step inside: a query there skips the offsets that leave the key range"""
    top = ref.CELL_MAX
    c = np.array([[top, 0, 0], [top - 1, 0, 0], [top, 1, 0], [-top, -top, -top], [-top + 1, -top, -top], [-top, -top + 1, -top + 1],
                  [0, top, -top], [0, top - 1, -top], [1, top, -top + 1]], np.float64)
    pts = ((c + 0.5) * EDGE_LEAF).astype(np.float32)                               # (2^20 leaves of 0.5 need 20 bits: exact)
    return ((pts, IDENTITY),)


# ---- the layout cases (tests/map_layout_cases.py) ----
DENSE_K, DENSE_RADIUS = 8, 0.05                                                  # reach 1 at the layout cases' leaf


@functools.lru_cache(maxsize=None)
def dense_self_query():
    """the self query of the layout cases' dense scene (300,007 cells in a table of 2^19 slots: two rounds of every stride)"""
    import map_layout_cases as lc
    rm = lc.dense_reference()
    return self_query(rm, DENSE_K, DENSE_RADIUS)


def assert_self_queries_equal(info, rows, want):
    """info: WorldMap.knn's dict; rows: fetchKnn(sort=True)'s; want: self_query's.  array_equal on everything, the means by
    their float bits."""
    for f in COUNTS:
        assert info[f] == want[f], (f, info[f], want[f])
    for f in ("keys", "found", "q"):
        assert rows[f].dtype == want[f].dtype and np.array_equal(rows[f], want[f]), f
    assert rows["mean"].dtype == np.float32 and np.array_equal(rows["mean"].view(np.uint32), want["mean"].view(np.uint32)), "mean bits"


def assert_queries_equal(got, want):
    assert got["keys"].dtype == np.uint64 and np.array_equal(got["keys"], want["keys"]), "keys"
    assert got["found"].dtype == np.uint8 and np.array_equal(got["found"], want["found"]), "found"
    assert got["dist"].dtype == np.float32 and np.array_equal(got["dist"].view(np.uint32), want["dist"].view(np.uint32)), "dist bits"
