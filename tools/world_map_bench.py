"""The world map (engine.WorldMap: per-window clouds fused in a voxel hash) at the three cloud sizes of the
point-cloud table of DESIGN.md 7a -- what the radius filter leaves of a configs[1], configs[2] and configs[4] window:
1,097, 8,041 and 53,749 points -- over `--windows` integrate calls from poses that move along the scene, then count and
extract.  Two regimes: "steady" (the table is large enough from the start) and "growth" (it starts at 2^8 slots and
doubles on the way, k_map_rehash moving the cells).  Beside every device figure the HOST STAND-IN: the numpy restatement
of tests/world_map_reference.py on the same clouds -- not PCL, not the reference (which has no such stage): what a
user of the per-window clouds would otherwise run on the host.

Wall-clock per call is printed by the tool itself (upload, kernel, the read-back of the counters, one synchronisation).
Per-kernel times: run one case under rocprofv3 --kernel-trace --stats (--size N --regime steady|growth)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
import world_map_reference as ref  # noqa: E402

SIZES = (1097, 8041, 53749)


def windows(n, n_windows, seed):
    """n points per window on surfaces 5 - 60 m ahead of a rig that advances 0.18 m per window: (cloud, T_w_rv) pairs"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_windows):
        z = rng.choice([5.0, 12.0, 25.0, 40.0, 60.0], n) + rng.normal(0, 0.05, n)
        xyz = np.stack([rng.uniform(-0.6, 0.6, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], axis=1).astype(np.float32)
        yaw = 0.01 * np.sin(0.7 * k)
        T = np.array([np.cos(yaw), 0, np.sin(yaw), 0.05 * np.sin(0.3 * k), 0, 1, 0, 0, -np.sin(yaw), 0, np.cos(yaw), 0.18 * k])
        out.append((xyz, T))
    return out


def run(ctx, n, regime, args):
    wins = windows(n, args.windows, 7)
    # steady: the smallest table that holds every window's points without doubling
    cap = 8 if regime == "growth" else max(8, int(np.ceil(np.log2(n * args.windows * 4 / 3))))
    ms = []
    for rep in range(args.reps + 1):                    # (the first repetition warms the allocator and is dropped)
        wm = d.WorldMap(ctx, args.leaf, cap)
        per_call = []
        for xyz, T in wins:
            t = time.perf_counter()
            wm.integrate(xyz, T)
            per_call.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        cells = wm.count()
        count_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        out = wm.extract(sort=False)
        extract_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        twice = wm.extract(min_windows=2)
        extract2_ms = (time.perf_counter() - t) * 1e3
        info = wm.info()
        wm.close()
        if rep:
            ms.append((float(np.median(per_call)), float(np.max(per_call)), count_ms, extract_ms, extract2_ms))
    ms = np.median(np.array(ms), axis=0)
    row = dict(points_per_window=n, windows=args.windows, regime=regime, leaf=args.leaf, cells=int(cells),
               cells_seen_twice=len(twice["keys"]), capacity=info["capacity"], growths=info["growths"],
               integrate_ms_median=round(ms[0], 4), integrate_ms_max=round(ms[1], 4), count_ms=round(ms[2], 4),
               extract_ms=round(ms[3], 4), extract_min_windows_2_sorted_ms=round(ms[4], 4))
    if not args.no_standin:
        rm = ref.ReferenceMap(args.leaf)
        t = time.perf_counter()
        for xyz, T in wins:
            rm.integrate(xyz, T)
        row["numpy_standin_integrate_ms_per_window"] = round((time.perf_counter() - t) * 1e3 / len(wins), 2)
        t = time.perf_counter()
        want = rm.extract()
        row["numpy_standin_extract_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        order = np.argsort(out["keys"], kind="stable")
        ref.assert_maps_equal({k: v[order] for k, v in out.items()}, want)       # the same map, bit for bit
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=0, help="one cloud size (points per window) instead of the three")
    ap.add_argument("--regime", choices=("steady", "growth", "both"), default="both")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-standin", action="store_true", help="skip the numpy stand-in (and the comparison with it)")
    args = ap.parse_args()
    ctx = d.Context(0)
    for n in ((args.size,) if args.size else SIZES):
        for regime in (("steady", "growth") if args.regime == "both" else (args.regime,)):
            run(ctx, n, regime, args)
    ctx.close()


if __name__ == "__main__":
    main()
