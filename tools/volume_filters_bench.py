"""The volume filters at 346 x 260 x 100 (configs[1]) and 512 x 512 x 200 beside their floor in the same run: a
device-to-device copy of the volume (one read and one write, 8 bytes per voxel -- what one pass over the volume cannot
beat).  Timed: the Laplacian (stencil + copy back), the shortest diffusion (sigma 0.3: two stencil passes; no schedule has
fewer), the full sigma = 1 diffusion (12 passes, with the time per step), each axis kernel of the IIR filter on its own (the
experiments flavour's dsi_test_iir_axis hook: the production ABI runs the three together), the whole sigma = (1, 1, 1)
filter, dsi_grid_mean_std and Moran's index.  Times are device-event times of `--reps` back-to-back calls on the context's
stream, per call (mean_std and Moran return values and wait for the stream in every call).  bytes = the compulsory traffic
of the operation (passes x 8 bytes per voxel; reads only: 4); ratio = time over the copy's time x passes.  Cross-check the
per-kernel split with rocprofv3 --kernel-trace --stats, and take counters in a run of their own.

    DSI_ENGINE_EXPERIMENTS=1 python tools/volume_filters_bench.py [--out profiles/volume_filters_bench.jsonl]

Prints (and with --out writes) one JSON line per (shape, operation).  Without DSI_ENGINE_EXPERIMENTS=1 the per-axis lines
are left out."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
from dvs_mcemvs_amd import engine  # noqa: E402
from dvs_mcemvs_amd.engine import _check as check  # noqa: E402

HIP_MEMCPY_D2D = 3


def timed(ctx, fn, reps):
    for _ in range(2):
        fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="346x260x100,512x512x200")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = d.Context(0)
    L = d.load_library()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = L.dsi_context_stream(ctx._h)
    rows = []

    for spec in args.shapes.split(","):
        nx, ny, nz = (int(v) for v in spec.split("x"))
        rng = np.random.default_rng(1)
        vol = rng.uniform(0.0, 50.0, (nz, ny, nx)).astype(np.float32)
        vol[rng.random(vol.shape) < 0.5] = 0.0
        g = d.Grid3D(ctx, nx, ny, nz)
        h = d.Grid3D(ctx, nx, ny, nz)
        g.upload(vol)
        vb = 4.0 * nx * ny * nz

        def copy():
            assert hip.hipMemcpyAsync(h.device_ptr, g.device_ptr, int(vb), HIP_MEMCPY_D2D, stream) == 0

        ms_copy = timed(ctx, copy, args.reps)

        def row(op, ms, passes, bytes_moved=None):
            moved = passes * 2 * vb if bytes_moved is None else bytes_moved
            rows.append(dict(shape=spec, op=op, ms=round(ms, 5), us=round(ms * 1e3, 1), passes=passes,
                             tb_s=round(moved / (ms * 1e-3) / 1e12, 3), copy_us=round(ms_copy * 1e3, 1),
                             ratio_to_copy=round(ms / (ms_copy * passes), 2)))

        row("copy_d2d", ms_copy, 1)
        row("laplacian", timed(ctx, g.laplacian, args.reps), 2)                       # stencil pass + copy back
        g.upload(vol)
        steps = C.c_int()
        ms = timed(ctx, lambda: check(L.dsi_grid_smooth_diffuse(g._h, 0.3, C.byref(steps))), args.reps)
        assert steps.value == 2
        row("diffuse_2_steps", ms, 2)                                                 # the shortest schedule: two passes, no copy
        rows[-1]["us_per_step"] = round(ms * 1e3 / 2, 1)
        g.upload(vol)
        ms = timed(ctx, lambda: check(L.dsi_grid_smooth_diffuse(g._h, 1.0, C.byref(steps))), args.reps)
        assert steps.value == 12
        row("diffuse_sigma1", ms, 12)
        rows[-1]["us_per_step"] = round(ms * 1e3 / 12, 1)
        if engine.experiments_requested():
            for axis, name in enumerate("xyz"):
                g.upload(vol)
                ms = timed(ctx, lambda: check(L.dsi_test_iir_axis(g._h, axis, 1.0, 3, int(axis == 2))), args.reps)
                row("iir_axis_" + name, ms, 1)
        g.upload(vol)
        row("iir_sigma1", timed(ctx, lambda: g.smooth_iir(1.0, 1.0, 1.0), args.reps), 3)
        g.upload(vol)
        row("mean_std", timed(ctx, g.mean_std, args.reps), 1, 2 * vb)                 # two read passes
        # mean_std (2 reads), standardize (1 read, 2 writes), three IIR passes (3 x 2), the sum (2 reads)
        row("moran_sigma1", timed(ctx, lambda: g.moran_index(1.0), max(2, args.reps // 2)), 6.5, 13 * vb)
        ctx.synchronize()
        g.close()
        h.close()
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
