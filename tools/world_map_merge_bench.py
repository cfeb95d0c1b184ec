"""Merging world maps (engine.WorldMap.merge / exportState / importState, DESIGN.md 7j "Merging") on the three maps of
tools/world_map_bench.py -- 16 windows of 1,097, 8,041 and 53,749 points, leaf 0.05, the table that holds them without
doubling -- split into halves by window: the first eight windows in one map, the last eight in another.

Wall-clock per call, printed by the tool itself: merge = the second half appended to the first on the device (one memset,
one kernel, the read-back of six counters, one synchronisation; no growth: the table holds both halves); export = count,
scan, gather and the five arrays of the WHOLE map to pageable host memory; import = the second half's exported state
appended to the first half (the upload, the scratch table's allocation and memset, the build, then the merge).  A merge
changes its destination, so every repetition builds the first half again first.  The one comparison recorded, in the same
process: appending the second half by merge against integrating its eight windows' points anew into the first half --
the only way to combine two maps without these entry points, and one that needs the clouds.

The tool asserts bit equality: the merged map's exported state equals the whole map's and, unless --no-standin, the state
of the numpy restatement (tests/map_merge_reference.py) fed with the same windows and merged the same way.  Per-kernel
times: run one case under rocprofv3 --kernel-trace --stats (--size N --no-standin), in a run without counters."""
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
import map_merge_reference as mref  # noqa: E402
from world_map_bench import SIZES, windows  # noqa: E402


def build(ctx, wins, leaf, cap):
    wm = d.WorldMap(ctx, leaf, cap)
    for xyz, T in wins:
        wm.integrate(xyz, T)
    return wm


def median_ms(v):
    return round(float(np.median(v)), 4)


def run(ctx, n, args):
    wins = windows(n, args.windows, 7)
    half = args.windows // 2
    cap = max(8, int(np.ceil(np.log2(n * args.windows * 4 / 3))))
    whole, second = build(ctx, wins, args.leaf, cap), build(ctx, wins[half:], args.leaf, cap)
    want = whole.exportState()
    second_state = second.exportState(sort=False)
    merge_ms, import_ms, integrate_ms, export_ms = [], [], [], []
    info = None
    for rep in range(args.reps + 1):                    # (the first repetition allocates the buffers and is dropped)
        t = time.perf_counter()
        whole.exportState(sort=False)
        t1 = time.perf_counter()
        first = build(ctx, wins[:half], args.leaf, cap)
        t2 = time.perf_counter()
        info = first.merge(second)
        t3 = time.perf_counter()
        mref.assert_states_equal(first.exportState(), want)
        first.close()
        first = build(ctx, wins[:half], args.leaf, cap)
        t4 = time.perf_counter()
        info_import = first.importState(second_state)
        t5 = time.perf_counter()
        mref.assert_states_equal(first.exportState(), want)
        first.close()
        first = build(ctx, wins[:half], args.leaf, cap)
        t6 = time.perf_counter()
        for xyz, T in wins[half:]:
            first.integrate(xyz, T)
        t7 = time.perf_counter()
        mref.assert_states_equal(first.exportState(), want)
        first.close()
        assert info == info_import and info["growths"] == 0
        if rep:
            export_ms.append((t1 - t) * 1e3)
            merge_ms.append((t3 - t2) * 1e3)
            import_ms.append((t5 - t4) * 1e3)
            integrate_ms.append((t7 - t6) * 1e3)
    row = dict(points_per_window=n, windows=args.windows, leaf=args.leaf, capacity=1 << cap, cells=len(want["keys"]),
               second_half_cells=info["n_src_cells"], new=info["n_new"], common=info["n_common"], merge_ms=median_ms(merge_ms),
               export_whole_ms=median_ms(export_ms), import_second_half_ms=median_ms(import_ms),
               integrate_second_half_anew_ms=median_ms(integrate_ms), second_half_points=int(sum(len(x) for x, _ in wins[half:])))
    if not args.no_standin:
        a, b = mref.reference_of(wins[:half], args.leaf), mref.reference_of(wins[half:], args.leaf)
        t = time.perf_counter()
        counts = a.merge(b)
        row["numpy_standin_merge_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        assert {k: info[k] for k in counts} == counts
        mref.assert_states_equal(want, a.export_state())                       # the same merged map, bit for bit
    whole.close()
    second.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=0, help="one cloud size (points per window) instead of the three")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-standin", action="store_true", help="skip the numpy stand-in (and the comparison with it)")
    args = ap.parse_args()
    ctx = d.Context(0)
    for n in ((args.size,) if args.size else SIZES):
        run(ctx, n, args)
    ctx.close()


if __name__ == "__main__":
    main()
