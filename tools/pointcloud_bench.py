"""The point cloud (MapperEMVS::getPointcloud: back-projection + radius outlier removal) on the device at the image sizes
of configs[1] (346 x 260), configs[2] (512 x 512) and configs[4] (1024 x 1024), with the point counts before and after
the filter, beside a CPU stand-in for PCL's kd-tree filter: scipy's cKDTree (build + pairs within r (1 + 1e-3)) plus the
exact fp32 recheck of the candidates, on the same clouds.  --stream: the configs[2] window stream
(process.full_sequence, 512 x 512 x 200) with the filtered maps, with point clouds on and off.

Maps: a semi-dense synthetic scene (fronto-parallel layers 4.8 - 60 m with a slope, `--fill` of the pixels masked) and, at
configs[4], also every pixel masked (1,048,576 points).  Per-kernel times: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import dvs_mcemvs_amd as d  # noqa: E402
from dvs_mcemvs_amd import process as proc, synthetic as syn  # noqa: E402


def scene(nx, ny, fill, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    layer = ((xx * 6 // nx) + (yy * 4 // ny)) % 6
    depth = (4.8 + 10.0 * layer + 0.002 * xx + rng.normal(0, 0.01, (ny, nx))).astype(np.float32)
    mask = (rng.random((ny, nx)) < fill).astype(np.uint8)
    return depth, mask


def kdtree_standin(xyz, r, k):
    """cKDTree + the exact fp32 recheck (the keep-set of the count rule); returns (keep, ms)."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    p = np.ascontiguousarray(xyz[:, :3], np.float32)
    pairs = cKDTree(p.astype(np.float64)).query_pairs(float(np.float32(r)) * (1 + 1e-3), output_type="ndarray")
    a, b = pairs[:, 0], pairs[:, 1]
    dx, dy, dz = p[a, 0] - p[b, 0], p[a, 1] - p[b, 1], p[a, 2] - p[b, 2]
    ok = ((dx * dx + dy * dy) + dz * dz).astype(np.float64) <= float(np.float32(r)) ** 2
    cnt = np.ones(len(p), np.int64) + np.bincount(a[ok], minlength=len(p)) + np.bincount(b[ok], minlength=len(p))
    return cnt >= k + 1, (time.perf_counter() - t0) * 1e3


def clouds(ctx, args, out):
    opts = d.OptionsPointCloud(args.radius, args.min_neighbors)
    cases = [("configs[1]", 346, 260, args.fill), ("configs[2]", 512, 512, args.fill), ("configs[4]", 1024, 1024, args.fill),
             ("configs[4] all pixels", 1024, 1024, 1.0)]
    for name, nx, ny, fill in cases:
        m = d.MapperEMVS(ctx, (nx, ny, nx / 2, nx / 2, nx / 2, ny / 2), d.ShapeDSI(0, 0, 8, 4.0, 200.0, 0.0))
        depth, mask = scene(nx, ny, fill, 5)
        for _ in range(2):
            pc = m.getPointcloud(depth, mask, opts)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            pc = m.getPointcloud(depth, mask, opts)
        call_ms = (time.perf_counter() - t0) / args.reps * 1e3
        n0 = m.n_unfiltered_
        full = m.getPointcloud(depth, mask, d.OptionsPointCloud(args.radius, 0))   # every point: the unfiltered cloud
        t0 = time.perf_counter()
        for _ in range(args.reps):
            d.radius_outlier_removal(ctx, full, args.radius, args.min_neighbors)
        ror_ms = (time.perf_counter() - t0) / args.reps * 1e3
        keep, kd_ms = kdtree_standin(full, args.radius, args.min_neighbors)
        assert int(keep.sum()) == len(pc), "device keep-set differs from the stand-in's"
        row = dict(case=name, width=nx, height=ny, points_before=int(n0), points_after=len(pc),
                   get_pointcloud_ms=round(call_ms, 3), radius_outlier_removal_ms=round(ror_ms, 3),
                   ckdtree_standin_ms=round(kd_ms, 1))
        print("%-22s %4d x %4d: %8d -> %8d points; getPointcloud (maps up, points down) %.3f ms; "
              "radius_outlier_removal (points up, flags down) %.3f ms; cKDTree stand-in %.1f ms" %
              (name, nx, ny, n0, len(pc), call_ms, ror_ms, kd_ms))
        out.append(row)
        m.close()


def stream(ctx, args, out):
    n_win, ev_win, dur, t0 = args.windows, 500_000, 0.05, 10.0
    rig = syn.stereo_rig(n_win * ev_win, width=640, height=480, t0=t0, duration=n_win * dur, seed=77, n_points=6000)
    cam = rig["cam"]
    shape = d.ShapeDSI(512, 512, 200, 4.0, 200.0, 0.0)
    a = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    opts_dm, opts_pc = d.OptionsDepthMap(), d.OptionsPointCloud(args.radius, args.min_neighbors)
    res = {}
    for rep in range(2):   # the first repetition warms the pools
        for label, kw in (("off", {}), ("on", {"options_point_cloud": opts_pc})):
            t = time.perf_counter()
            wins = list(proc.full_sequence(*a, options_depth_map=opts_dm, **kw))
            res[label] = (time.perf_counter() - t) * 1e3 / len(wins)
            if label == "on":
                pts = [len(w[4]) for w in wins]
                masked = [int((w[3] > 0).sum()) for w in wins]
    print("configs[2] window stream, %d windows, filtered maps: %.3f ms per window with point clouds off, %.3f ms on "
          "(+%.3f ms); points per window: %d masked pixels -> %d points (mean)" %
          (n_win, res["off"], res["on"], res["on"] - res["off"], np.mean(masked), np.mean(pts)))
    out.append(dict(case="configs[2] stream", ms_per_window_off=round(res["off"], 3), ms_per_window_on=round(res["on"], 3),
                    masked_mean=float(np.mean(masked)), points_mean=float(np.mean(pts))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--min-neighbors", type=int, default=3)
    ap.add_argument("--fill", type=float, default=0.25, help="fraction of masked pixels of the semi-dense maps")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stream", action="store_true", help="also the configs[2] window stream, point clouds on / off")
    ap.add_argument("--windows", type=int, default=16)
    args = ap.parse_args()
    ctx = d.Context(0)
    out = []
    clouds(ctx, args, out)
    if args.stream:
        stream(ctx, args, out)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
