"""The world map scored in 3-D (engine.WorldMap.compare: map-to-map nearest-centroid distances, DESIGN.md 7j "Scoring the
map in 3-D") on the three maps of tools/world_map_bench.py -- 16 windows of 1,097, 8,041 and 53,749 points, leaf 0.05, the
table that holds them without doubling -- each against a noisy copy of itself (sigma 0.02 on every point, the same leaf)
at radius 0.05 (reach 1, 27 lookups per cell) and 0.1 (reach 2, 125 lookups).  Beside every device figure the HOST
STAND-IN: the numpy restatement of tests/map_eval_reference.py on the two extracted maps -- not the reference (which has
no such stage): what a user of dsi_map_extract would otherwise run on the host.  The tool asserts that both give the same
histogram, counts and distances, bit for bit.

Wall-clock per call is printed by the tool itself: compare = two memsets, one kernel, the read-back of the histogram and
three counters and one synchronisation; fetch = count, scan, gather and the two arrays to pageable host memory.
Per-kernel times: run one case under rocprofv3 --kernel-trace --stats (--size N --radius R --no-standin)."""
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
import map_eval_reference as mref  # noqa: E402
from world_map_bench import SIZES, windows  # noqa: E402

RADII = (0.05, 0.1)
N_BINS = 16


def run(ctx, n, radius, args):
    wins = windows(n, args.windows, 7)
    rng = np.random.default_rng(8)
    cap = max(8, int(np.ceil(np.log2(n * args.windows * 4 / 3))))
    a, b = d.WorldMap(ctx, args.leaf, cap), d.WorldMap(ctx, args.leaf, cap)
    for xyz, T in wins:
        a.integrate(xyz, T)
        b.integrate((xyz.astype(np.float64) + rng.normal(0.0, args.sigma, xyz.shape)).astype(np.float32), T)
    compare_ms, fetch_ms = [], []
    for rep in range(args.reps + 1):                    # (the first repetition allocates the compare's buffers and is dropped)
        t = time.perf_counter()
        got = a.compare(b, radius, N_BINS)
        t1 = time.perf_counter()
        got.update(a.fetchDistances(sort=False))
        t2 = time.perf_counter()
        if rep:
            compare_ms.append((t1 - t) * 1e3)
            fetch_ms.append((t2 - t1) * 1e3)
    row = dict(points_per_window=n, windows=args.windows, leaf=args.leaf, capacity=a.info()["capacity"], radius=radius,
               compare_ms=round(float(np.median(compare_ms)), 4), fetch_ms=round(float(np.median(fetch_ms)), 4),
               cells_b=b.count(), max_bin=int(got["hist"].max()), mean=round(got["mean"], 6),
               **{k: got[k] for k in mref.COUNTS})
    if not args.no_standin:
        t = time.perf_counter()
        ca, cb = a.extract(), b.extract()
        row["extract_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        t = time.perf_counter()
        want = mref.compare(ca, cb, args.leaf, radius, N_BINS)
        row["numpy_standin_compare_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        order = np.argsort(got["keys"], kind="stable")
        got["keys"], got["dist"] = got["keys"][order], got["dist"][order]
        mref.assert_compares_equal(got, want)                                   # the same result, bit for bit
    a.close()
    b.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=0, help="one cloud size (points per window) instead of the three")
    ap.add_argument("--radius", type=float, default=0.0, help="one radius instead of 0.05 and 0.1")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-standin", action="store_true", help="skip the numpy stand-in (and the comparison with it)")
    args = ap.parse_args()
    ctx = d.Context(0)
    for n in ((args.size,) if args.size else SIZES):
        for radius in ((args.radius,) if args.radius else RADII):
            run(ctx, n, radius, args)
    ctx.close()


if __name__ == "__main__":
    main()
