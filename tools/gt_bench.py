"""Ground-truth depth from a disparity image on the device, beside its numpy yardstick in the same run and
on the same data: one 480 x 640 frame, the size of the reference's script.
  project        GroundTruthProjector.project_png16 (2 bytes per pixel uploaded, the clears, k_gt_project, k_gt_write) and
                 .project (4 bytes per pixel): device-event time of `--reps` back-to-back calls on the context's stream,
                 per call, upload inside
  numpy          tests/ground_truth_reference.py's project() of the same frame (host clock), median of `--host-reps`
One JSON line per case, appended to profiles/gt_bench.jsonl with --record.  Cross-check the per-kernel split with
rocprofv3 --kernel-trace --stats, in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
import ground_truth_reference as gr  # noqa: E402
from dvs_mcemvs_amd import engine  # noqa: E402

H, W, BASELINE = 480, 640, 0.6


def scene(seed):
    rng = np.random.default_rng(seed)
    cx, cy, f = 320.4, 240.2, 569.8
    Q = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, 1.0 / BASELINE, 0]], np.float64)
    a = 0.01
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    K = np.zeros((3, 4))
    K[0, 0] = K[1, 1] = 0.97 * f
    K[0, 2], K[1, 2], K[2, 2] = cx, cy, 1.0
    raw = rng.integers(256, 20000, (H, W)).astype(np.uint16)
    raw[rng.random((H, W)) < 0.3] = 0
    return Q, T, K, raw


def timed(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/gt_bench.jsonl")
    args = ap.parse_args()
    ctx = d.Context(0)
    Q, T, K, raw = scene(1)
    disp = engine.disparity_from_png16(raw)
    rows = []
    want = None
    host = []
    for _ in range(args.host_reps):
        t = time.perf_counter()
        want = gr.project(disp, Q, T, K, gr.DROP_OUTSIDE)
        host.append((time.perf_counter() - t) * 1e3)
    for mode_name, mode in (("drop_outside", engine.GT_DROP_OUTSIDE), ("as_script", engine.GT_AS_SCRIPT)):
        p = d.GroundTruthProjector(ctx, W, H, Q, T, K, mode)
        ms_u16 = timed(ctx, lambda: p.project_png16(raw), args.reps)
        ms_f32 = timed(ctx, lambda: p.project(disp), args.reps)
        depth, n, o = p.fetch()
        same = np.array_equal(depth, want[0]) and (n, o) == want[1:]     # (the frame has no point outside: both modes agree)
        rows.append(dict(op="project", shape="%dx%d" % (W, H), mode=mode_name, write="recompute", n_points=n, n_outside=o,
                         ms_png16=round(ms_u16, 4), ms_f32=round(ms_f32, 4), numpy_ms=round(statistics.median(host), 1),
                         equal_to_numpy=bool(same)))
        p.close()
    for r in rows:
        print(json.dumps(r))
    if args.record:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "gt_bench.jsonl"), "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
