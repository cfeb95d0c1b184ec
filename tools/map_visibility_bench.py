"""The world map's visibility tally (engine.WorldMap.observe / pruneCarved, DESIGN.md 7j "Visibility") on the largest map of
the tools -- 16 windows of 53,749 points, leaf 0.05, the table that holds them without doubling -- seen from the rig's last
pose through tools/world_map_render_bench.py's 640 x 480 view: the depth image is the map's own render at splat 2, every
eighth column pushed away by a factor 1.5 so that all three verdicts occur.  For ORIENTATION, not as a gate (nobody has
measured this kernel before): k_map_render at splat 0 on the same map and view, in the same process turn -- the same walk
over the slots with the same projection per cell, with two atomics per cell where the observation has (2 window + 1)^2
loads and three read-modify-writes.  observe and render alternate inside the repetitions, so that both see the same
machine; the first repetition allocates the buffers and is dropped.  observe_ms is the wall clock of one observe() from host
arrays: two uploads (1.5 MB), three memsets on the tally's first view, one kernel, the read-back of the counters and the
synchronisation; render_splat0_ms is one render without its fetch: three memsets (6.4 MB), two kernels, the read-back and the
synchronisation.  prune_ms is one pruneCarved() on a fresh tally of three views.  One row of JSON per window setting; the counts of the first view are compared with the
restatement of tests/map_visibility_reference.py unless --no-check.  Per-kernel times: run the tool under
rocprofv3 --kernel-trace --stats, in a run without counters."""
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
import map_visibility_reference as vr  # noqa: E402
from world_map_bench import windows  # noqa: E402
from world_map_render_bench import VIEW  # noqa: E402


def median_ms(v):
    return round(float(np.median(v)), 4)


def build(ctx, wins, leaf, cap):
    wm = d.WorldMap(ctx, leaf, cap)
    for xyz, T in wins:
        wm.integrate(xyz, T)
    return wm


def run(ctx, window, args):
    wins = windows(args.size, args.windows, 7)
    cap = max(8, int(np.ceil(np.log2(args.size * args.windows * 4 / 3))))
    wm = build(ctx, wins, args.leaf, cap)
    T_v_w = d.invert_pose(wins[-1][1])
    pos = (T_v_w,) + tuple(VIEW[k] for k in ("width", "height", "fx", "fy", "cx", "cy", "min_depth", "max_depth"))
    K, lo, hi = tuple(VIEW[k] for k in ("fx", "fy", "cx", "cy")), VIEW["min_depth"], VIEW["max_depth"]
    image = wm.render(*pos, splat=2)
    depth, mask = image["depth"].copy(), image["mask"]
    depth[:, ::8] *= np.float32(1.5)
    obs = (depth, mask, K, lo, hi, T_v_w, window, 0.0, 0.01)
    observe_ms, render_ms = [], []
    for rep in range(args.reps + 1):                    # (the first repetition allocates the buffers and is dropped)
        t = time.perf_counter()
        counts = wm.observe(*obs)
        t1 = time.perf_counter()
        wm.render(*pos, splat=0, fetch=False)
        t2 = time.perf_counter()
        if rep:
            observe_ms.append((t1 - t) * 1e3)
            render_ms.append((t2 - t1) * 1e3)
    assert counts["views"] == args.reps + 1
    info = wm.info()
    row = dict(points_per_window=args.size, windows=args.windows, leaf=args.leaf, capacity=info["capacity"], cells=info["occupied"],
               view="%dx%d" % (VIEW["width"], VIEW["height"]), window=window, observe_ms=median_ms(observe_ms),
               observe_ms_min=round(min(observe_ms), 4), observe_ms_max=round(max(observe_ms), 4), render_splat0_ms=median_ms(render_ms),
               render_ms_min=round(min(render_ms), 4), render_ms_max=round(max(render_ms), 4),
               observe_over_render=round(float(np.median(observe_ms) / np.median(render_ms)), 3), reps=args.reps,
               **{k: counts[k] for k in vr.COUNTS if k != "views"})
    fetch_ms = []
    for rep in range(2):
        t = time.perf_counter()
        wm.fetchVisibility(sort=False)
        fetch_ms.append((time.perf_counter() - t) * 1e3)
    row["fetch_ms"] = round(fetch_ms[1], 4)
    if not args.no_check:
        cells = wm.extract(0, 0)
        want = vr.verdicts(cells["xyz"], *obs)
        assert all(counts[name] == int((want == code).sum()) for code, name in enumerate(vr.VERDICTS)), (counts, np.bincount(want, minlength=6))
        row["counts_equal_restatement"] = True
    prune_ms = []
    for rep in range(args.prune_reps + 1):              # (every prune needs a map of its own: the first one warms the code up)
        fresh = build(ctx, wins, args.leaf, cap)
        for _ in range(3):
            fresh.observe(*obs)
        t = time.perf_counter()
        pruned = fresh.pruneCarved(2, 1)
        if rep:
            prune_ms.append((time.perf_counter() - t) * 1e3)
        fresh.close()
    row.update(prune_ms=median_ms(prune_ms), prune_reps=args.prune_reps, n_kept=pruned["n_kept"], n_removed=pruned["n_removed"])
    wm.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=53749, help="points per window: 1097, 8041 or 53749")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--window", type=int, default=-1, help="one window (0..3) instead of 0, 1 and 3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prune-reps", type=int, default=3)
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the restatement")
    ap.add_argument("--out", default=None, help="append the rows to this file (profiles/map_visibility.jsonl)")
    args = ap.parse_args()
    ctx = d.Context(0)
    rows = [run(ctx, w, args) for w in ((0, 1, 3) if args.window < 0 else (args.window,))]
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
