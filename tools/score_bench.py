"""Depth-map scores on the device, beside their numpy yardstick in the same run and on the same data.
  add            one DepthScore.add-equivalent at 512 x 512 and at 1024 x 1024, two ways: dsi_score_add (host maps: the
                 three uploads are inside) and dsi_score_add_dev (maps already on the device: the two kernels alone).
                 Device-event time of `--reps` back-to-back calls on the context's stream, per call; the object is
                 reset before every timed series so that the buffer never overflows.
  metrics_curves metrics() plus curves() after 100 windows of 346 x 260 (host clock around calls that end in a
                 synchronise), median of `--reps`
  numpy          tests/score_reference.py's metrics() plus curves() of the same 100 windows as one stack, and of one
                 512 x 512 / 1024 x 1024 map (what scoring a window on the host costs), median of `--host-reps`
One JSON line per case.  Cross-check the per-kernel split with rocprofv3 --kernel-trace --stats, in a run of its own."""
import argparse
import ctypes as C
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
import score_reference as sr  # noqa: E402
from dvs_mcemvs_amd.engine import _check as check, _ptr as ptr  # noqa: E402

B, FOCAL = 0.6, 557.25


def maps(seed, shape):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(4.0, 50.0, shape).astype(np.float32)
    est = (gt.astype(np.float64) * np.exp(rng.normal(0.0, 0.1, shape))).astype(np.float32)
    mask = (rng.random(shape) < 0.3).astype(np.uint8)
    gt[rng.random(shape) >= 0.7] = 0.0
    return est, mask, gt


def timed(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def host_median(fn, reps):
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    ctx = d.Context(0)
    L = d.load_library()
    rows = []
    for side in (512, 1024):
        est, mask, gt = maps(side, (side, side))
        n = est.size
        score = d.DepthScore(ctx, (args.reps + 3) * n, B, FOCAL)
        # device copies of the three maps: one float grid holds depth | gt | mask bytes
        rows_ = (2 * n + (n + 3) // 4 + 1023) // 1024
        store = d.Grid3D(ctx, 1024, rows_, 1)
        packed = np.zeros(rows_ * 1024, np.float32)
        packed[:n], packed[n:2 * n] = est.ravel(), gt.ravel()
        packed[2 * n:].view(np.uint8)[:n] = mask.ravel()
        store.upload(packed.reshape(1, rows_, 1024))
        base = store.device_ptr
        score.reset()
        ms_host = timed(ctx, lambda: check(L.dsi_score_add(score._h, ptr(est, C.c_float), ptr(mask, C.c_uint8), ptr(gt, C.c_float), n)),
                        args.reps)
        ctx.synchronize()
        score.reset()
        ms_dev = timed(ctx, lambda: check(L.dsi_score_add_dev(score._h, C.c_void_p(base), C.c_void_p(base + 8 * n), C.c_void_p(base + 4 * n),
                                                              n)), args.reps)
        m = score.metrics()
        assert not m["overflow"] and m["n_joint"] == (args.reps + 3) * sr.metrics(est, mask, gt, B, FOCAL)["n_joint"]
        np_ms = host_median(lambda: (sr.metrics(est, mask, gt, B, FOCAL), sr.curves(est, mask, gt)), args.host_reps)
        rows.append(dict(op="add", shape="%dx%d" % (side, side), joint_share=round(m["n_joint"] / ((args.reps + 3) * n), 3),
                         ms_host_maps=round(ms_host, 4), ms_device_maps=round(ms_dev, 4),
                         device_maps_read_gb_s=round(9 * n / (ms_dev * 1e-3) / 1e9, 1), numpy_metrics_curves_ms=round(np_ms, 2)))
        score.close()
        store.close()
    windows, shape = 100, (260, 346)
    est, mask, gt = maps(7, (windows,) + shape)
    score = d.DepthScore(ctx, est.size, B, FOCAL)
    for w in range(windows):
        score.add(est[w], mask[w], gt[w])
    ctx.synchronize()
    out = {}

    def device_side():
        out["m"], out["c"] = score.metrics(), score.curves()

    device_side()
    ms = host_median(device_side, args.reps)
    ref = {}

    def numpy_side():
        ref["m"], ref["c"] = sr.metrics(est, mask, gt, B, FOCAL), sr.curves(est, mask, gt)

    np_ms = host_median(numpy_side, args.host_reps)
    same = (out["m"]["n_joint"] == ref["m"]["n_joint"] and out["m"]["median_abs"] == ref["m"]["median_abs"] and
            all(np.array_equal(out["c"][k], ref["c"][k]) for k in ref["c"]))
    rows.append(dict(op="metrics_curves", windows=windows, shape="%dx%d" % shape[::-1], n_joint=out["m"]["n_joint"],
                     bins=int(out["c"]["base"].size), ms=round(ms, 3), numpy_ms=round(np_ms, 1), equal_to_numpy=bool(same)))
    score.close()
    for r in rows:
        print(json.dumps(r))
    ctx.close()


if __name__ == "__main__":
    main()
