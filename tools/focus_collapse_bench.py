"""The focus-based collapses (getDepthMapFromDSI's method 0..4: k_focus_tile + k_focus_finish) and the local-focus
transform (computeLocalFocusInPlace into another grid) at 346 x 260 x 100 (configs[1]), 512 x 512 x 200 and
1024 x 1024 x 256, beside the arg-max (k_collapse_max_z<Identity, 8>, method -1) at the same shape.  Times are
device-event times of `--reps` back-to-back calls on the context's stream, per call; TB/s = compulsory traffic (the
volume read once, the maps or the new volume written once) over that time.  Cross-check the per-kernel split with
rocprofv3 --kernel-trace --stats.  Prints one JSON line per (shape, operation)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
from dvs_mcemvs_amd.engine import _check as check  # noqa: E402

NAMES = {-1: "argmax", 0: "local_var", 1: "local_ms", 2: "grad_mag", 3: "laplacian_mag", 4: "dog"}


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
    ap.add_argument("--shapes", default="346x260x100,512x512x200,1024x1024x256")
    args = ap.parse_args()
    ctx = d.Context(0)
    L = d.load_library()
    rows = []
    for spec in args.shapes.split(","):
        nx, ny, nz = (int(v) for v in spec.split("x"))
        rng = np.random.default_rng(1)
        vol = rng.uniform(0.0, 8.0, (nz, ny, nx)).astype(np.float32)
        vol[rng.random(vol.shape) < 0.5] = 0.0
        g = d.Grid3D(ctx, nx, ny, nz)
        g.upload(vol)
        dst = d.Grid3D(ctx, nx, ny, nz)
        m = d.MapperEMVS(ctx, (nx, ny, nx / 2, nx / 2, nx / 2, ny / 2), d.ShapeDSI(0, 0, nz, 4.0, 200.0, 0.0))
        vol_bytes = 4.0 * nx * ny * nz
        map_bytes = 9.0 * nx * ny                     # conf f32 + idx u8 + depth f32
        base = None
        for method in (-1, 0, 1, 2, 3, 4):
            ms = timed(ctx, lambda: check(L.dsi_mapper_depth_map_of_focus(m._h, g._h, method)), args.reps)
            base = ms if method == -1 else base
            rows.append(dict(shape=spec, op=NAMES[method], method=method, ms=round(ms, 5), us=round(ms * 1e3, 1),
                             tb_s=round((vol_bytes + map_bytes) / (ms * 1e-3) / 1e12, 3), x_argmax=round(ms / base, 2)))
        for f in (0, 1):
            ms = timed(ctx, lambda: check(L.dsi_grid_local_focus(dst._h, g._h, f)), args.reps)
            rows.append(dict(shape=spec, op="local_focus_%s" % ("ms" if f == 1 else "std"), ms=round(ms, 5),
                             us=round(ms * 1e3, 1), tb_s=round(2 * vol_bytes / (ms * 1e-3) / 1e12, 3),
                             x_argmax=round(ms / base, 2)))
        ctx.synchronize()
        for o in (m, dst, g):
            o.close()
    for r in rows:
        print(json.dumps(r))
    ctx.close()


if __name__ == "__main__":
    main()
