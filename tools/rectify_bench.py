"""The lens rectification table on the device, beside its numpy yardstick in the same run: both models at
346 x 260 and 1280 x 720.
  kernel_ms      k_rectify_lut alone: rectify_lut_dev into device memory, device-event time of `--reps` back-to-back launches
                 on the context's stream, per launch
  call_ms        dsi_rectify_lut as a caller sees it: the kernel, the copy of the table to the host and the synchronise,
                 device-event time per call
  numpy_ms       tests/rectify_reference.py's rectify_lut of the same lens (host clock), median of `--host-reps`
This runs once per mapper: the figures are a record, not a gate.  One JSON line per case, appended to
profiles/rectify_bench.jsonl with --record."""
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
import rectify_reference as rr  # noqa: E402


def lens_of(model, w, h):
    f = 0.65 * w if model == "plumb_bob" else 0.82 * w
    K = [[f, 0, 0.5 * w + 0.6], [0, 0.998 * f, 0.5 * h - 0.3], [0, 0, 1]]
    D = (-0.09, 0.19, 8e-5, 2e-3) if model == "plumb_bob" else (-0.04, 0.003, -0.002, 0.0003)
    a = np.deg2rad(2.0)
    R = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    P = [[0.9 * f, 0, 0.51 * w, -0.1 * f], [0, 0.9 * f, 0.49 * h, 0], [0, 0, 1, 0]]
    return d.Lens(model, K, D, R, P)


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
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/rectify_bench.jsonl")
    args = ap.parse_args()
    ctx = d.Context(0)
    rows = []
    for w, h in ((346, 260), (1280, 720)):
        for model in ("plumb_bob", "fisheye"):
            lens = lens_of(model, w, h)
            host = []
            for _ in range(args.host_reps):
                t = time.perf_counter()
                want = rr.rectify_lut(lens, w, h)
                host.append((time.perf_counter() - t) * 1e3)
            g = d.Grid3D(ctx, w, h, 2)
            kernel_ms = timed(ctx, lambda: d.rectify_lut_dev(ctx, lens, w, h, g.device_ptr), args.reps)
            call_ms = timed(ctx, lambda: d.rectify_lut(ctx, lens, w, h), args.reps)
            got = d.rectify_lut(ctx, lens, w, h)
            differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            g.close()
            rows.append(dict(op="rectify_lut", model=model, shape="%dx%d" % (w, h), kernel_ms=round(kernel_ms, 4),
                             call_ms=round(call_ms, 4), numpy_ms=round(statistics.median(host), 1),
                             entries_differing_from_numpy=differ))
    for r in rows:
        print(json.dumps(r))
    if args.record:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "rectify_bench.jsonl"), "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
