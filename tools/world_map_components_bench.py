"""The world map's connected components (engine.WorldMap.components / fetchComponents / listComponents / selectComponents /
pruneComponents, DESIGN.md 7j "Components") on the three maps of tools/world_map_bench.py -- 16 windows of 1,097, 8,041 and
53,749 points, leaf 0.05, the table that holds them without doubling -- and on the 300,007-cell dense map of
tests/map_layout_cases.py (one component: every union ends in one root), at connectivity 26 and 124.  Beside every device
figure the HOST STAND-IN: the numpy / scipy restatement of tests/map_components_reference.py on the same calls -- not the
reference (which has no such stage).  The tool asserts that both give the same counts, rows, list, reasons and pruned map,
bit for bit.  The one comparison recorded: WorldMap.classifyPrune(reach=1, min_neighbors=26) on the same map -- 26 read-only
lookups for every cell, where labelling at connectivity 26 makes 13 lookups plus the unions.

Wall-clock per call is printed by the tool itself: components = two memsets, seven kernels, the read-back of the counters
and one synchronisation; select = two memsets, two kernels per rank of keep_largest and one more, the read-back; prune = the
select plus the new table's allocation and memset, the rebuild and the counters' read-back (a prune changes the map, so every
repetition integrates the calls and labels again first); fetch and list = count, scan, gather and the arrays to pageable
host memory.  Per-kernel times: run one case under rocprofv3 --kernel-trace --stats (--size N --no-standin, or --dense
--no-standin), in a run without counters."""
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
import map_components_reference as cref  # noqa: E402
import map_layout_cases as lc  # noqa: E402
import map_prune_reference as pref  # noqa: E402
import world_map_reference as ref  # noqa: E402
from world_map_bench import SIZES, windows  # noqa: E402

SELECTION = dict(min_cells=2, min_component_points=2, keep_largest=16)


def build(ctx, calls, leaf, cap):
    wm = d.WorldMap(ctx, leaf, cap)
    for xyz, T in calls:
        wm.integrate(xyz, T)
    return wm


def median_ms(v):
    return round(float(np.median(v)), 4)


def run(ctx, name, calls, leaf, cap, args):
    wm = build(ctx, calls, leaf, cap)
    row = dict(map=name, leaf=leaf, capacity=1 << cap, cells=wm.info()["occupied"])
    sweep_ms = []
    for rep in range(args.reps + 1):                    # (the first repetition allocates the buffers and is dropped)
        t = time.perf_counter()
        sweep = wm.classifyPrune(reach=1, min_neighbors=26)
        if rep:
            sweep_ms.append((time.perf_counter() - t) * 1e3)
    row["classify_full_sweep_reach1_ms"], row["full_sweep_kept"] = median_ms(sweep_ms), sweep["n_kept"]
    got = {}
    for conn in (26, 124):
        label_ms, fetch_ms, list_ms, select_ms = [], [], [], []
        for rep in range(args.reps + 1):
            t = time.perf_counter()
            info = wm.components(connectivity=conn)
            t1 = time.perf_counter()
            rows = wm.fetchComponents(sort=False)
            t2 = time.perf_counter()
            lst = wm.listComponents()
            t3 = time.perf_counter()
            sel = wm.selectComponents(**SELECTION)
            t4 = time.perf_counter()
            if rep:
                label_ms.append((t1 - t) * 1e3)
                fetch_ms.append((t2 - t1) * 1e3)
                list_ms.append((t3 - t2) * 1e3)
                select_ms.append((t4 - t3) * 1e3)
        reasons = wm.fetchComponents(sort=False)
        got[conn] = (info, rows, lst, sel, reasons)
        row["c%d" % conn] = dict(components=info["n_components"], singletons=info["n_singletons"], largest_cells=info["largest_cells"],
                                 kept=sel["n_kept"], components_ms=median_ms(label_ms), fetch_ms=median_ms(fetch_ms),
                                 list_ms=median_ms(list_ms), select_keep16_ms=median_ms(select_ms))
    wm.close()
    prune_ms = []
    for rep in range(args.prune_reps + 1):
        wm = build(ctx, calls, leaf, cap)
        wm.components(connectivity=26)
        t = time.perf_counter()
        done = wm.pruneComponents(shrink=True, **SELECTION)
        if rep:
            prune_ms.append((time.perf_counter() - t) * 1e3)
        if rep < args.prune_reps:
            wm.close()
    row["prune_components_ms"], row["capacity_after"] = median_ms(prune_ms), done["capacity"]
    if not args.no_standin:
        rm = cref.map_of(calls, leaf)
        for conn in (26, 124):
            info, rows, lst, sel, reasons = got[conn]
            t = time.perf_counter()
            comp = cref.components(rm, connectivity=conn)
            row["c%d" % conn]["scipy_standin_components_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            want = cref.select(rm, comp, **SELECTION)
            order = np.argsort(rows["keys"], kind="stable")
            assert info == comp["info"], (info, comp["info"])
            assert np.array_equal(rows["keys"][order], comp["keys"]) and np.array_equal(rows["labels"][order], comp["labels"])
            assert all(np.array_equal(lst[k], comp["list"][k]) for k in lst)
            assert (sel["n_cells"], sel["n_kept"], sel["n_removed"], sel["n_components_kept"]) == \
                (want["n_cells"], want["n_kept"], want["n_removed"], want["n_components_kept"])
            assert np.array_equal(reasons["reason"][np.argsort(reasons["keys"], kind="stable")], want["node_reason"])
        want = cref.prune_components(rm, cref.components(rm, connectivity=26), **SELECTION)
        assert done["n_removed"] == want["n_removed"] and done["capacity"] == pref.shrunk_capacity(want["n_kept"])
        ref.assert_maps_equal(wm.extract(), rm.extract())                       # the same pruned map, bit for bit
    wm.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=0, help="one cloud size (points per window) instead of the three")
    ap.add_argument("--dense", action="store_true", help="the 300,007-cell dense map alone")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--prune-reps", type=int, default=3)
    ap.add_argument("--no-standin", action="store_true", help="skip the numpy / scipy stand-in (and the comparison with it)")
    args = ap.parse_args()
    ctx = d.Context(0)
    if not args.dense:
        for n in ((args.size,) if args.size else SIZES):
            cap = max(8, int(np.ceil(np.log2(n * args.windows * 4 / 3))))
            run(ctx, "%d x %d points" % (args.windows, n), windows(n, args.windows, 7), args.leaf, cap, args)
    if args.dense or not args.size:
        run(ctx, "dense %d cells" % lc.DENSE_CELLS, lc.dense_calls(), lc.LEAF, lc.BIG_LOG2, args)
    ctx.close()


if __name__ == "__main__":
    main()
