"""Pruning the world map (engine.WorldMap.classifyPrune / prune, DESIGN.md 7j "Pruning") on the three maps of
tools/world_map_bench.py -- 16 windows of 1,097, 8,041 and 53,749 points, leaf 0.05, the table that holds them without
doubling -- with every criterion evaluated: min_points 1 and min_windows 1 (these sparse maps hold one point per cell:
a larger bound would remove them all before anything else is looked at), max_age 8 (half of the windows), a box of
+-(15, 10, 30) m around the last window's position, reach 1 with min_neighbors 2 (up to 26 lookups per surviving cell, the
sweep stopping at the second supporter), shrink.  Beside every device figure
the HOST STAND-IN: the numpy restatement of tests/map_prune_reference.py on the same windows -- not the reference (which
has no such stage).  The tool asserts that both give the same counts, verdicts and pruned map, bit for bit.  The one
comparison recorded: classify with criterion 5 alone at reach 1 and min_neighbors 26 (no early stop: 26 lookups for every
cell) against WorldMap.compare of the map with itself at reach 1 (the same walk, 27 lookups, plus a centroid per candidate).

Wall-clock per call is printed by the tool itself: classify = one memset, two kernels, the read-back of six counters and
one synchronisation; prune = that plus the new table's allocation and memset, the rebuild and the counters' read-back (a
prune changes the map, so every repetition integrates the windows again first); fetch = count, scan, gather and the two
arrays to pageable host memory.  Per-kernel times: run one case under rocprofv3 --kernel-trace --stats
(--size N --no-standin), in a run without counters."""
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
import map_prune_reference as pref  # noqa: E402
import world_map_reference as ref  # noqa: E402
from world_map_bench import SIZES, windows  # noqa: E402


def build(ctx, wins, leaf, cap):
    wm = d.WorldMap(ctx, leaf, cap)
    for xyz, T in wins:
        wm.integrate(xyz, T)
    return wm


def run(ctx, n, args):
    wins = windows(n, args.windows, 7)
    cap = max(8, int(np.ceil(np.log2(n * args.windows * 4 / 3))))
    t_last = np.asarray(wins[-1][1], np.float64)[[3, 7, 11]]
    half = np.array([15.0, 10.0, 30.0])
    opts = dict(min_points=1, min_windows=1, max_age=args.windows // 2, box=(t_last - half, t_last + half), reach=1, min_neighbors=2)
    wm = build(ctx, wins, args.leaf, cap)
    classify_ms, fetch_ms, compare_ms, prune_ms, sweep_ms = [], [], [], [], []
    for rep in range(args.reps + 1):                    # (the first repetition allocates the buffers and is dropped)
        t = time.perf_counter()
        info = wm.classifyPrune(**opts)
        t1 = time.perf_counter()
        verdicts = wm.fetchPruneReasons(sort=False)
        t2 = time.perf_counter()
        wm.compare(wm, args.leaf, 16)
        t3 = time.perf_counter()
        sweep = wm.classifyPrune(reach=1, min_neighbors=26)
        t4 = time.perf_counter()
        if rep:
            classify_ms.append((t1 - t) * 1e3)
            fetch_ms.append((t2 - t1) * 1e3)
            compare_ms.append((t3 - t2) * 1e3)
            sweep_ms.append((t4 - t3) * 1e3)
    wm.close()
    for rep in range(args.prune_reps + 1):
        wm = build(ctx, wins, args.leaf, cap)
        t = time.perf_counter()
        done = wm.prune(shrink=True, **opts)
        if rep:
            prune_ms.append((time.perf_counter() - t) * 1e3)
        if rep < args.prune_reps:
            wm.close()
    row = dict(points_per_window=n, windows=args.windows, leaf=args.leaf, capacity=1 << cap, cells=info["n_cells"], kept=info["n_kept"],
               removed=info["n_removed"], capacity_after=done["capacity"], classify_ms=round(float(np.median(classify_ms)), 4),
               fetch_ms=round(float(np.median(fetch_ms)), 4), prune_ms=round(float(np.median(prune_ms)), 4),
               classify_full_sweep_reach1_ms=round(float(np.median(sweep_ms)), 4), full_sweep_kept=sweep["n_kept"],
               compare_self_reach1_ms=round(float(np.median(compare_ms)), 4))
    if not args.no_standin:
        rm = pref.PruneReferenceMap(args.leaf)
        for xyz, T in wins:
            rm.integrate(xyz, T)
        t = time.perf_counter()
        want = rm.classify(**opts)
        row["numpy_standin_classify_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        t = time.perf_counter()
        rm.prune(**opts)
        row["numpy_standin_prune_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        order = np.argsort(verdicts["keys"], kind="stable")
        assert np.array_equal(verdicts["keys"][order], want["keys"]) and np.array_equal(verdicts["reason"][order], want["reason"])
        assert (info["n_cells"], info["n_kept"], info["n_removed"]) == (want["n_cells"], want["n_kept"], want["n_removed"])
        assert done["n_removed"] == want["n_removed"] and done["capacity"] == pref.shrunk_capacity(want["n_kept"])
        ref.assert_maps_equal(wm.extract(), rm.extract())                       # the same pruned map, bit for bit
    wm.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=0, help="one cloud size (points per window) instead of the three")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--prune-reps", type=int, default=3)
    ap.add_argument("--no-standin", action="store_true", help="skip the numpy stand-in (and the comparison with it)")
    args = ap.parse_args()
    ctx = d.Context(0)
    for n in ((args.size,) if args.size else SIZES):
        run(ctx, n, args)
    ctx.close()


if __name__ == "__main__":
    main()
