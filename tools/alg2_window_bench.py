"""One Alg. 2 window (process_2, full_seq) two ways on the same seeded inputs: the DSI-less kernel
(MapperEMVS.computeDepthMapOfEventsAlg2: preparation of the 2 N batches + k_vote_fuse_argmax_alg2 + unpack) and the
materialising path (process_2's evaluateDSI per sub-interval and camera, camera fusion, temporal accumulation,
finalisation, camera_time fusion, then the arg-max of both DSIs).  Times are device-event times on the context's
stream, per window, over `--reps` windows with the batches already uploaded (the host packetisation is the same for
both paths and is not timed).  Cross-check the per-kernel split with rocprofv3 --kernel-trace --stats in a separate run.
Prints one JSON line per (shape, configuration)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dvs_mcemvs_amd as d  # noqa: E402
from dvs_mcemvs_amd import process, synthetic as syn  # noqa: E402

# name, sensor (w, h), DSI (nx, ny, nz) (0 = the sensor's), events per camera, N, (sf, tf) pairs
CONFIGS = [
    ("mvsec_like", (346, 260), (0, 0, 100), 1_000_000, 2, [(2, 4), (2, 2)]),
    ("configs2_like", (640, 480), (512, 512, 200), 500_000, 4, [(2, 4)]),
    ("configs3_like_step", (346, 260), (0, 0, 100), 10_000_000, 8, [(2, 2)]),
    # events and phases apart: the configs[3]-like N at a short window, and a long window at N = 2
    ("n8_short", (346, 260), (0, 0, 100), 1_000_000, 8, [(2, 2)]),
    ("n2_long", (346, 260), (0, 0, 100), 10_000_000, 2, [(2, 2)]),
    ("n4_mid", (346, 260), (0, 0, 100), 3_000_000, 4, [(2, 2)]),
]


def timed(ctx, fn, reps):
    fn()
    ctx.synchronize()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated config names")
    args = ap.parse_args()
    ctx = d.Context(0)
    for name, (w, h), (nx, ny, nz), n_ev, n_sub, fusions in CONFIGS:
        if args.only and name not in args.only.split(","):
            continue
        rig = syn.stereo_rig(n_ev, width=w, height=h, duration=0.05, seed=97, n_points=6000)
        cam = rig["cam"]
        shape = d.ShapeDSI(nx, ny, nz, 4.0, 200.0, 0.0)
        ts = rig["t0"] + 0.05
        mappers = [d.MapperEMVS(ctx, cam, shape) for _ in range(2)]
        out_tc, out_ct = d.MapperEMVS(ctx, cam, shape), d.MapperEMVS(ctx, cam, shape)
        batches = process.alg2_window_batches(ctx, rig["events"], rig["trajectories"], ts, n_sub, 2)
        for sf, tf in fusions:
            fused_ms = timed(ctx, lambda: out_tc.computeDepthMapOfEventsAlg2(out_ct, mappers, batches, n_sub, sf, tf), args.reps)
            info = out_tc.last_vote_info()
            fused_tc_ms = timed(ctx, lambda: out_tc.computeDepthMapOfEventsAlg2(None, mappers, batches, n_sub, sf, tf), args.reps)
            # the materialising path on the same batches: the grids of process_2, built once and reused
            m0, m1 = mappers
            dims = m0.dsi_.getDimensions()
            sub, left, right = (d.Grid3D(ctx, *dims) for _ in range(3))
            fused, cam_time = out_tc.dsi_, out_ct.dsi_

            def materialising():
                fused.resetGrid()
                left.resetGrid()
                right.resetGrid()
                for k in range(n_sub):
                    for m, b in ((m0, batches[2 * k]), (m1, batches[2 * k + 1])):
                        if b.n_packets:
                            m.evaluateDSI_batch(b)
                        else:
                            m.dsi_.resetGrid()
                    sub.setToFusionOf(m0.dsi_, m1.dsi_, sf)
                    acc = left.addInverseOfTwoGrids if tf == 2 else left.addTwoGrids
                    acc(m0.dsi_)
                    (right.addInverseOfTwoGrids if tf == 2 else right.addTwoGrids)(m1.dsi_)
                    (fused.addInverseOfTwoGrids if tf == 2 else fused.addTwoGrids)(sub)
                for g in (left, right, fused):
                    (g.computeHMfromSumOfInv if tf == 2 else g.computeAMfromSum)(n_sub)
                cam_time.setToFusionOf(left, right, {1: 1, 2: 2, 3: 4, 4: 3, 5: 5, 6: 6}[sf])
                out_tc.computeDepthMap(fused)
                out_ct.computeDepthMap(cam_time)

            mat_ms = timed(ctx, materialising, args.reps)
            print(json.dumps(dict(config=name, shape="%dx%dx%d" % dims, events_per_camera=n_ev, n_sub=n_sub, sf=sf, tf=tf,
                                  dsi_less_ms=round(fused_ms, 4), dsi_less_time_camera_only_ms=round(fused_tc_ms, 4),
                                  materialising_ms=round(mat_ms, 4), ratio=round(fused_ms / mat_ms, 3),
                                  bands=info["bands"], band_rows=info["band_rows"], lanes=info["packed"],
                                  planner=process.alg2_plan(n_sub, 2 * n_ev, dims[0]))), flush=True)
            for g in (sub, left, right):
                g.close()
        ctx.synchronize()
        for o in batches + mappers + [out_tc, out_ct]:
            o.close()
    ctx.close()


if __name__ == "__main__":
    main()
