"""The world map's render (engine.WorldMap.render: the map as a pinhole camera sees it, DESIGN.md 7j "Rendering") on the
three maps of tools/world_map_bench.py -- 16 windows of 1,097, 8,041 and 53,749 points, leaf 0.05, the table that holds
them without doubling -- into a 640 x 480 view from the rig's last pose, at splat 0 and 2.  Beside every device figure
the HOST STAND-IN: the numpy restatement of tests/world_map_render_reference.py on the extracted map -- not the reference
(which has no such stage): what a user of dsi_map_extract would otherwise run on the host.  The tool asserts that both
give the same image, bit for bit.

Wall-clock per call is printed by the tool itself: render = two memsets, two kernels, the read-back of five counters and
one synchronisation; fetch = the four images to pageable host arrays.  Per-kernel times: run one case under
rocprofv3 --kernel-trace --stats (--size N --splat S --no-standin)."""
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
import world_map_render_reference as rref  # noqa: E402
from world_map_bench import SIZES, windows  # noqa: E402

VIEW = dict(width=640, height=480, fx=556.0, fy=556.0, cx=319.5, cy=239.5, min_depth=0.5, max_depth=100.0)


def run(ctx, n, splat, args):
    wins = windows(n, args.windows, 7)
    cap = max(8, int(np.ceil(np.log2(n * args.windows * 4 / 3))))
    wm = d.WorldMap(ctx, args.leaf, cap)
    for xyz, T in wins:
        wm.integrate(xyz, T)
    T_v_w = d.invert_pose(wins[-1][1])
    pos = (T_v_w,) + tuple(VIEW[k] for k in ("width", "height", "fx", "fy", "cx", "cy", "min_depth", "max_depth"))
    render_ms, fetch_ms = [], []
    for rep in range(args.reps + 1):                    # (the first repetition allocates the view's buffers and is dropped)
        t = time.perf_counter()
        counts = wm.render(*pos, splat=splat, fetch=False)
        t1 = time.perf_counter()
        images = wm.fetchRender()
        t2 = time.perf_counter()
        if rep:
            render_ms.append((t1 - t) * 1e3)
            fetch_ms.append((t2 - t1) * 1e3)
    info = wm.info()
    row = dict(points_per_window=n, windows=args.windows, leaf=args.leaf, capacity=info["capacity"], splat=splat,
               view="%dx%d" % (VIEW["width"], VIEW["height"]), render_ms=round(float(np.median(render_ms)), 4),
               fetch_ms=round(float(np.median(fetch_ms)), 4),
               max_hits=int(images["hits"].max()), **{k: counts[k] for k in rref.COUNTS})
    if not args.no_standin:
        t = time.perf_counter()
        cells = wm.extract(sort=False)
        row["extract_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        t = time.perf_counter()
        want = rref.render(cells, T_v_w, splat=splat, **VIEW)
        row["numpy_standin_render_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        counts.update(images)
        rref.assert_renders_equal(counts, want)                                 # the same image, bit for bit
    wm.close()
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=0, help="one cloud size (points per window) instead of the three")
    ap.add_argument("--splat", type=int, default=-1, help="one splat instead of 0 and 2")
    ap.add_argument("--windows", type=int, default=16)
    ap.add_argument("--leaf", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-standin", action="store_true", help="skip the numpy stand-in (and the comparison with it)")
    args = ap.parse_args()
    ctx = d.Context(0)
    for n in ((args.size,) if args.size else SIZES):
        for splat in ((0, 2) if args.splat < 0 else (args.splat,)):
            run(ctx, n, splat, args)
    ctx.close()


if __name__ == "__main__":
    main()
