"""Aligning world maps (engine.WorldMap.alignStep / align: ICP on exact integer moments, DESIGN.md 7j "Aligning") on the
three maps of tools/world_map_bench.py -- 16 windows of 1,097, 8,041 and 53,749 points, leaf 0.05, the table that holds
them without doubling -- each against a noisy copy of itself (sigma 0.02 on every point, the same leaf; the maps of
tools/map_eval_bench.py) seen from a frame turned by 1 degree and moved by half a leaf, at radius 0.05 (reach 1, 27 lookups
per cell) and 0.1 (reach 2, 125 lookups).  Beside every figure of the step the YARDSTICK: WorldMap.compare on the same two
maps at the same reach -- the kernel that makes the same lookups and keeps only the distance.

Wall-clock per call is printed by the tool itself: step = one memset, one kernel, the read-back of 27 words and one
synchronisation; align10 = ten rounds of that plus the host solve (eps 0: no early end).  Per-kernel times: run one case
under rocprofv3 --kernel-trace --stats (--size N --radius R) and read k_map_align_step beside k_map_compare."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
import map_align_reference as ar  # noqa: E402
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
    T_true = ar.axis_angle_pose((0.3, -0.5, 0.8), math.radians(1.0), (0.3 * args.leaf, -0.32 * args.leaf, 0.24 * args.leaf))
    moved = d.WorldMap(ctx, args.leaf, cap)                 # a, seen from a frame that lies at T_true in b's
    moved.integrateMap(a, d.invert_pose(T_true))
    step_ms, compare_ms, align_ms = [], [], []
    for rep in range(args.reps + 1):                        # (the first repetition allocates the buffers and is dropped)
        t = time.perf_counter()
        m = moved.alignStep(b, radius)
        t1 = time.perf_counter()
        c = moved.compare(b, radius, N_BINS)
        t2 = time.perf_counter()
        try:
            T, info = moved.align(b, radius, max_iterations=10, min_matched=3, eps_rot=0.0, eps_trans=0.0)
        except d.DsiError as e:                             # (a round without enough matches: the figures of the rounds run)
            T, info = e.T, e.info
        t3 = time.perf_counter()
        if rep:
            step_ms.append((t1 - t) * 1e3)
            compare_ms.append((t2 - t1) * 1e3)
            align_ms.append((t3 - t2) * 1e3)
    assert (m["n_cells"], m["n_matched"]) == (c["n_cells"], c["n_matched"])      # the same lookups, the same matches
    err = ar.pose_error(T, T_true)
    row = dict(points_per_window=n, windows=args.windows, leaf=args.leaf, capacity=moved.info()["capacity"], radius=radius,
               reach=m["reach"], n_cells=m["n_cells"], cells_b=b.count(), n_matched=m["n_matched"],
               step_ms=round(float(np.median(step_ms)), 4), compare_ms=round(float(np.median(compare_ms)), 4),
               align10_ms=round(float(np.median(align_ms)), 4), iterations=info["iterations"],
               rms_first=round(info["rms_first"], 6), rms_last=round(info["rms_last"], 6),
               pose_error_rad=round(err[0], 6), pose_error_trans=round(err[1], 6))
    for o in (a, b, moved):
        o.close()
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
    args = ap.parse_args()
    ctx = d.Context(0)
    for n in ((args.size,) if args.size else SIZES):
        for radius in ((args.radius,) if args.radius else RADII):
            run(ctx, n, radius, args)
    ctx.close()


if __name__ == "__main__":
    main()
