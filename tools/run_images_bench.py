"""The run's pictures on the device, beside their host yardstick in the same run.
Event image of one camera (dsi_batch_event_image_dev: the events already on the device, as in an EventBatch pipeline):
500 k, 2 M and 10 M events on a 346 x 260 sensor, 10 M events on 16 pixels, 10 M events on 640 x 480 --
  event_image_polarity   use_polarity = 1: includes the upload of one polarity byte per event from page-locked memory
  event_image_counts     use_polarity = 0: nothing is uploaded, the three kernels alone
The two depth images (dsi_depth_images, host maps in and images out, so the copies are inside) at 346 x 260 and
1024 x 1024.  Times are device-event times of `--reps` back-to-back calls on the context's stream, per call.
host_loop: tools/accumulate_events_host.cpp, the reference's loop on one host thread (built here with g++ -O2 when absent).
Cross-check the per-kernel split with rocprofv3 --kernel-trace --stats, in a run of its own.  One JSON line per case."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
from dvs_mcemvs_amd.engine import _check as check, _ptr as ptr  # noqa: E402

CASES = [(346, 260, 500_000, 0), (346, 260, 2_000_000, 0), (346, 260, 10_000_000, 0), (346, 260, 10_000_000, 16),
         (640, 480, 10_000_000, 0)]


def timed(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def host_tool():
    exe = os.path.join(ROOT, "tools", "accumulate_events_host")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O2", src, "-o", exe])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    ctx = d.Context(0)
    L = d.load_library()
    rows = []
    out = d.Grid3D(ctx, 1024, 1024, 1)                                  # 4 MiB of device memory for the images
    for width, height, n, hot in CASES:
        rng = np.random.default_rng(n + hot)
        if hot:
            px = rng.choice(width * height, hot, replace=False)[rng.integers(0, hot, n)]
        else:
            px = rng.integers(0, width * height, n)
        x, y = (px % width).astype(np.uint16), (px // width).astype(np.uint16)
        pol = d.PinnedArray((n,), np.uint8)
        pol.a[:] = rng.random(n) < 0.5
        b = d.EventBatch(ctx, x, y, np.zeros((0, 12), np.float32))
        for name, use_polarity in (("event_image_polarity", 1), ("event_image_counts", 0)):
            ms = timed(ctx, lambda: check(L.dsi_batch_event_image_dev(b._h, ptr(pol.a, C.c_uint8), width, height, use_polarity,
                                                                      C.c_void_p(out.device_ptr), None)), args.reps)
            read = n * (4 + use_polarity)
            rows.append(dict(op=name, sensor="%dx%d" % (width, height), events=n, hot_pixels=hot, ms=round(ms, 4),
                             events_per_us=round(n / (ms * 1e3), 1), event_read_gb_s=round(read / (ms * 1e-3) / 1e9, 1)))
        ctx.synchronize()
        b.close()
        pol.close()
        if not args.skip_host:
            r = subprocess.run([host_tool(), str(width), str(height), str(n), str(hot), str(args.host_reps)], capture_output=True,
                               text=True, check=True)
            rows.append(json.loads(r.stdout))
    for rows_, cols in ((260, 346), (1024, 1024)):
        rng = np.random.default_rng(rows_)
        depth = rng.uniform(4.0, 200.0, (rows_, cols)).astype(np.float32)
        conf = rng.gamma(1.0, 3.0, (rows_, cols)).astype(np.float32)
        mask = (rng.random((rows_, cols)) < 0.3).astype(np.uint8)
        neg = np.empty((rows_, cols), np.uint8)
        bgr = np.empty((rows_, cols, 3), np.uint8)
        ms = timed(ctx, lambda: check(L.dsi_depth_images(ctx._h, ptr(depth, C.c_float), ptr(conf, C.c_float), ptr(mask, C.c_uint8),
                                                         rows_, cols, 4.0, 200.0, None, ptr(neg, C.c_uint8), ptr(bgr, C.c_uint8))),
                   args.reps)
        rows.append(dict(op="depth_images_host_maps", shape="%dx%d" % (cols, rows_), ms=round(ms, 4)))
    out.close()
    for r in rows:
        print(json.dumps(r))
    ctx.close()


if __name__ == "__main__":
    main()
