"""The world map's local shape (engine.WorldMap.pca / fetchPca, DESIGN.md 7j "Local shape") on the maps of
tools/map_knn_bench.py -- 16 windows of 1,097, 8,041 or 53,749 points, leaf 0.05, the table that holds them without doubling,
or with --dense the 300,007-cell dense map of tests/map_layout_cases.py -- at one k and one reach per process: the pass does
the self query's scan plus a few dozen f64 operations per cell, so the YARDSTICK beside every figure is WorldMap.knn (the
parent commit's code path, untouched) on the same map, k and radius, never a run of the pass itself.  k = 0, the radius
search, has no self query of its own: its yardstick is knn at k = 16, the same walk with the longest list.

One row of JSON per process (one timed step per process: a job script chains the processes with && and gives each its own
time limit).  pca and knn alternate inside the repetitions, so that both see the same machine; the first repetition allocates
the buffers and is dropped; every call ends in a synchronise, so wall-clock per call is one memset, one kernel, the read-back
of the counters and the synchronisation.  The first rows are compared with the restatement of tests/map_pca_reference.py bit
for bit unless --no-check.  Per-kernel times: run the tool under rocprofv3 --kernel-trace --stats, in a run without counters."""
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

import dvs_mcemvs_amd as d  # noqa: E402
import map_layout_cases as lc  # noqa: E402
import map_pca_reference as pr  # noqa: E402
from world_map_bench import windows  # noqa: E402

CHECK_ROWS = 2000                                                               # rows compared with the restatement bit for bit


def median_ms(v):
    return round(float(np.median(v)), 4)


def check_head(wm, rows, leaf, radius, k):
    """the first CHECK_ROWS rows by key against the restatement run on the whole map's cells (only those rows are solved)"""
    cells = wm.extract()
    mo = pr.moments(cells, leaf, radius, k)
    head = slice(0, CHECK_ROWS)
    found = mo["found"][head]
    sol = pr.solve(found + 1, mo["s"][head], mo["ss"][head], pr.quantum_of(leaf))
    solved = found >= 2
    assert np.array_equal(rows["keys"][head], cells["keys"][head]) and np.array_equal(rows["members"][head], (found + 1).astype(np.uint16))
    assert np.array_equal(rows["moments"][head], np.concatenate([mo["s"], mo["ss"]], axis=1)[head])
    assert np.array_equal(rows["label"][head][solved], sol["label"][solved]) and (rows["label"][head][~solved] == 0).all()
    for f in ("normal", "tangent", "eval"):
        assert np.array_equal(pr.bits(rows[f][head][solved]), pr.bits(sol[f][solved])), f
    return int(solved.sum())


def run(ctx, name, calls, leaf, cap, args):
    wm = d.WorldMap(ctx, leaf, cap)
    for xyz, T in calls:
        wm.integrate(xyz, T)
    radius = float("%.12g" % (args.reach * leaf))              # (3 * 0.05 lies above 0.15 and would ask for a reach of 4)
    knn_k = args.k if args.k else 16
    row = dict(map=name, leaf=leaf, capacity=1 << cap, cells=wm.info()["occupied"], k=args.k, knn_k=knn_k, reach=args.reach, radius=radius)
    pca_ms, knn_ms, fetch_ms = [], [], []
    for rep in range(args.reps + 1):                    # (the first repetition allocates the buffers and is dropped)
        t = time.perf_counter()
        info = wm.pca(args.k, radius)
        t1 = time.perf_counter()
        wm.knn(knn_k, radius)
        t2 = time.perf_counter()
        if rep:
            pca_ms.append((t1 - t) * 1e3)
            knn_ms.append((t2 - t1) * 1e3)
    for rep in range(2):
        t = time.perf_counter()
        wm.fetchPca()
        fetch_ms.append((time.perf_counter() - t) * 1e3)
    assert info["reach"] == args.reach
    row.update(pca_ms=median_ms(pca_ms), knn_ms=median_ms(knn_ms), pca_over_knn=round(float(np.median(pca_ms) / np.median(knn_ms)), 3),
               pca_ms_min=round(min(pca_ms), 4), pca_ms_max=round(max(pca_ms), 4), knn_ms_min=round(min(knn_ms), 4),
               knn_ms_max=round(max(knn_ms), 4), fetch_ms=round(fetch_ms[1], 4), reps=args.reps, n_sparse=info["n_sparse"],
               n_label=info["n_label"], mean_members=round(info["sum_members"] / max(info["n_cells"], 1), 3))
    if not args.no_check:
        wm.pca(args.k, radius, keep_moments=True)
        row["rows_equal_restatement"] = check_head(wm, wm.fetchPca(sort=True), leaf, radius, args.k)
    print(json.dumps(row), flush=True)
    wm.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=8041, help="points per window: 1097, 8041 or 53749")
    ap.add_argument("--dense", action="store_true", help="the 300,007-cell dense map instead")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--k", type=int, default=8, help="0: the radius search")
    ap.add_argument("--reach", type=int, default=1, help="radius in leaves: 1..3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the restatement")
    args = ap.parse_args()
    ctx = d.Context(0)
    if args.dense:
        run(ctx, "dense %d cells" % lc.DENSE_CELLS, lc.dense_calls(), lc.LEAF, lc.BIG_LOG2, args)
    else:
        cap = max(8, int(np.ceil(np.log2(args.size * args.windows * 4 / 3))))
        run(ctx, "%d x %d points" % (args.windows, args.size), windows(args.size, args.windows, 7), args.leaf, cap, args)
    ctx.close()


if __name__ == "__main__":
    main()
