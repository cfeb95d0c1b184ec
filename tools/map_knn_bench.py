"""The world map's k nearest cells (engine.WorldMap.knn / fetchKnn / query, DESIGN.md 7j "Neighbours and statistical
outliers") on the three maps of tools/world_map_bench.py -- 16 windows of 1,097, 8,041 and 53,749 points, leaf 0.05, the
table that holds them without doubling -- and, with --dense, on the 300,007-cell dense map of tests/map_layout_cases.py:
k = 8 at reach 1 and 2 (radius = one and two leaves), the self query and `--points` random point queries drawn around the
map's own centroids.  Beside every device figure the HOST STAND-IN on the same cells: scipy.spatial.cKDTree.query with
workers=16 and distance_upper_bound=radius -- not the reference (which has no such stage): what a user of the extracted
cloud would otherwise run on the host.  The tool asserts that both give the same neighbours, and that the first rows equal
the restatement of tests/map_knn_reference.py bit for bit.

Wall-clock per call is printed by the tool itself: knn = one memset, one kernel, the read-back of seven counters and one
synchronisation; query = the upload of the points, one kernel, the three arrays to pageable host memory.  Per-kernel times:
run the tool under rocprofv3 --kernel-trace --stats, in a run without counters; the dispatches of k_map_knn_self<8> and
k_map_knn_points<8> come in the order of the rows printed here, --reps + 1 of each per row."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from scipy.spatial import cKDTree  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
import map_knn_reference as kref  # noqa: E402
import map_layout_cases as lc  # noqa: E402
from world_map_bench import SIZES, windows  # noqa: E402

K = 8
CHECK_ROWS = 2000                                                               # rows compared with the restatement bit for bit


def median_ms(v):
    return round(float(np.median(v)), 4)


def same_neighbours(got_keys, got_dist, found, tree, keys, points, radius, exclude_self):
    """the device's rows against cKDTree's on the same centroids.  The tree sums the squares in its own order and cuts at the
    bound in its own way, so the distances agree to a few ulp and a neighbour within 1e-9 of the radius may fall on either
    side; where two neighbours tie to that precision the tree's order is its own.  Rows without such a case must name the
    same cells in the same order.  Returns the number of rows compared in full."""
    k = got_keys.shape[1]
    td, ti = tree.query(points, k=k + 2, distance_upper_bound=radius * (1 + 1e-9), workers=16)
    if exclude_self:                                                            # the cell's own centroid comes first, at distance 0
        td, ti = td[:, 1:], ti[:, 1:]
    near_cut = (np.abs(td - radius) <= 1e-9).any(axis=1)
    td = np.where(td <= radius, td, np.inf)
    with np.errstate(invalid="ignore"):                                         # (inf - inf beyond the last neighbour)
        tied = (np.diff(td, axis=1) <= 1e-12 * radius)[:, :k] & np.isfinite(td[:, 1:k + 1])
    clear = ~near_cut & ~tied.any(axis=1)
    if exclude_self:
        clear &= td[:, 0] > 0                                                   # (another cell with the same centroid)
    td, ti = td[:, :k], ti[:, :k]
    want_found = np.isfinite(td).sum(axis=1)
    want_keys = np.where(np.isfinite(td), keys[np.minimum(ti, len(keys) - 1)], np.uint64(0))
    assert np.array_equal(found[clear], want_found[clear])
    assert np.array_equal(got_keys[clear], want_keys[clear])
    both = np.isfinite(td) & clear[:, None]
    assert np.allclose(got_dist[both], td[both], rtol=1e-6, atol=0)             # (float32 rows)
    return int(clear.sum())


def run(ctx, name, calls, leaf, cap, args):
    wm = d.WorldMap(ctx, leaf, cap)
    for xyz, T in calls:
        wm.integrate(xyz, T)
    cells = wm.extract()
    xyz64 = cells["xyz"].astype(np.float64)
    rng = np.random.default_rng(11)
    pick = rng.integers(0, len(cells["keys"]), args.points)
    points = (xyz64[pick] + rng.normal(0.0, leaf, (args.points, 3))).astype(np.float32)
    rm = None
    if not args.no_standin:
        rm = kref.reference_of(calls, leaf)
        t = time.perf_counter()
        tree = cKDTree(xyz64)
        tree_ms = round((time.perf_counter() - t) * 1e3, 2)
    for reach in (1, 2):
        radius = reach * leaf
        row = dict(map=name, leaf=leaf, capacity=1 << cap, cells=len(cells["keys"]), k=K, reach=reach, radius=radius, points=args.points)
        self_ms, fetch_ms, query_ms = [], [], []
        for rep in range(args.reps + 1):                # (the first repetition allocates the buffers and is dropped)
            t = time.perf_counter()
            info = wm.knn(K, radius)
            t1 = time.perf_counter()
            rows = wm.fetchKnn()
            t2 = time.perf_counter()
            if rep:
                self_ms.append((t1 - t) * 1e3)
                fetch_ms.append((t2 - t1) * 1e3)
        for rep in range(args.reps + 1):
            t = time.perf_counter()
            got = wm.query(points, K, radius)
            if rep:
                query_ms.append((time.perf_counter() - t) * 1e3)
        assert info["reach"] == reach
        row.update(knn_ms=median_ms(self_ms), fetch_ms=median_ms(fetch_ms), query_ms=median_ms(query_ms), n_scored=info["n_scored"],
                   n_isolated=info["n_isolated"], mean_found_self=round(float(rows["found"].mean()), 3),
                   mean_found_points=round(float(got["found"].mean()), 3))
        if not args.no_standin:
            row["ckdtree_build_ms"] = tree_ms
            t = time.perf_counter()
            tree.query(xyz64, k=K + 1, distance_upper_bound=radius, workers=16)
            row["ckdtree_self_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            t = time.perf_counter()
            tree.query(points.astype(np.float64), k=K, distance_upper_bound=radius, workers=16)
            row["ckdtree_points_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            row["rows_equal_ckdtree_points"] = same_neighbours(got["keys"], got["dist"], got["found"], tree, cells["keys"],
                                                               points.astype(np.float64), radius, False)
            head = slice(0, CHECK_ROWS)
            kref.assert_queries_equal({f: v[head] for f, v in got.items()}, kref.query(rm, points[head], K, radius))
            part = kref.neighbours(xyz64[head], cells, leaf, radius, K, exclude=cells["keys"][head])
            assert np.array_equal(rows["keys"][head], cells["keys"][head]) and np.array_equal(rows["found"][head], part["found"])
            nb = wm.query(cells["xyz"], K + 1, radius)                            # the self query's rows, through the point query
            row["rows_equal_ckdtree_self"] = same_neighbours(nb["keys"][:, 1:], nb["dist"][:, 1:], np.maximum(nb["found"], 1) - 1, tree,
                                                             cells["keys"], xyz64, radius, True)
        print(json.dumps(row), flush=True)
    wm.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=0, help="one cloud size (points per window) instead of the three")
    ap.add_argument("--dense", action="store_true", help="the 300,007-cell dense map as well")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-standin", action="store_true", help="skip cKDTree and the restatement (and the comparison with them)")
    args = ap.parse_args()
    ctx = d.Context(0)
    for n in ((args.size,) if args.size else SIZES):
        cap = max(8, int(np.ceil(np.log2(n * args.windows * 4 / 3))))
        run(ctx, "%d x %d points" % (args.windows, n), windows(n, args.windows, 7), args.leaf, cap, args)
    if args.dense:
        run(ctx, "dense %d cells" % lc.DENSE_CELLS, lc.dense_calls(), lc.LEAF, lc.BIG_LOG2, args)
    ctx.close()


if __name__ == "__main__":
    main()
