"""Grid3D's min/max, the four voxel-wise members that are no camera fusion, and the 8-bit slice images of imwriteSlices
 at 346 x 260 x 100 (configs[1]), 512 x 512 x 200 and 1024 x 1024 x 256, beside their yardsticks in the same
run: dsi_grid_mean_square (one read pass) for min/max, dsi_grid_fuse2 (two reads, one write) for the binary ops, and the
dim_idx 2 orientation (no transposition) for the transposing orientations.  Times are device-event times of `--reps`
back-to-back calls on the context's stream, per call (min/max and mean-square return a value and therefore wait for the
stream in every call, both alike); TB/s = compulsory traffic over that time.  Cross-check the per-kernel split with
rocprofv3 --kernel-trace --stats, in a run of its own.  Prints one JSON line per (shape, operation)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
from dvs_mcemvs_amd.engine import _check as check  # noqa: E402

OPS = {1: "subtract", 2: "ratio", 3: "quadratic_mean", 4: "cubic_mean"}


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="346x260x100,512x512x200,1024x1024x256")
    args = ap.parse_args()
    ctx = d.Context(0)
    L = d.load_library()
    rows = []

    def row(spec, op, ms, bytes_moved, versus, base):
        rows.append(dict(shape=spec, op=op, ms=round(ms, 5), us=round(ms * 1e3, 1),
                         tb_s=round(bytes_moved / (ms * 1e-3) / 1e12, 3), versus=versus, ratio=round(ms / base, 2)))

    for spec in args.shapes.split(","):
        nx, ny, nz = (int(v) for v in spec.split("x"))
        rng = np.random.default_rng(1)
        vol = rng.uniform(0.0, 50.0, (nz, ny, nx)).astype(np.float32)
        vol[rng.random(vol.shape) < 0.5] = 0.0
        g = d.Grid3D(ctx, nx, ny, nz)
        h = d.Grid3D(ctx, nx, ny, nz)
        out = d.Grid3D(ctx, nx, ny, nz)                # device memory for the images (a quarter of it is used)
        h.upload(np.roll(vol, 1, axis=0))
        vb = 4.0 * nx * ny * nz
        # one read pass
        g.upload(vol)
        v = C.c_double()
        ms_sq = timed(ctx, lambda: check(L.dsi_grid_mean_square(g._h, C.byref(v))), args.reps)
        row(spec, "mean_square", ms_sq, vb, "mean_square", ms_sq)
        lo, hi = C.c_float(), C.c_float()
        lp, hp = C.c_uint64(), C.c_uint64()
        ms = timed(ctx, lambda: check(L.dsi_grid_min_max(g._h, C.byref(lo), C.byref(hi), C.byref(lp), C.byref(hp))), args.reps)
        row(spec, "min_max", ms, vb, "mean_square", ms_sq)
        # two reads, one write
        ms_f2 = timed(ctx, lambda: check(L.dsi_grid_fuse2(g._h, h._h, d.FUSE_AM)), args.reps)
        row(spec, "fuse2_am", ms_f2, 3 * vb, "fuse2_am", ms_f2)
        for op, name in OPS.items():
            g.upload(vol)
            ms = timed(ctx, lambda: check(L.dsi_grid_binary_op(g._h, h._h, op)), args.reps)
            row(spec, name, ms, 3 * vb, "fuse2_am", ms_f2)
        # the slice images: one read of the volume (two with the extremes' pass), a quarter of it written
        g.upload(vol)
        base = {}
        for dim in (2, 0, 1):
            for by_minmax in (1, 0):
                ms = timed(ctx, lambda: check(L.dsi_grid_slices_u8_dev(g._h, dim, by_minmax, C.c_void_p(out.device_ptr))),
                           args.reps)
                if dim == 2:
                    base[by_minmax] = ms
                row(spec, "slices_u8_dim%d_%s" % (dim, "minmax" if by_minmax else "per_slice"), ms, 2.25 * vb,
                    "slices_u8_dim2", base[by_minmax])
        ctx.synchronize()
        for o in (g, h, out):
            o.close()
    for r in rows:
        print(json.dumps(r))
    ctx.close()


if __name__ == "__main__":
    main()
