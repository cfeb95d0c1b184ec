"""Child process of tests/test_gpu_fused_schedule.py: one case of the schedule-independence tests of the DSI-less kernels, run
with the EXPERIMENTS flavour of the engine (DSI_ENGINE_EXPERIMENTS=1 in this process's environment; the test hooks
dsi_test_fused_grid_blocks / dsi_test_fused_solo / dsi_test_fused_fixed_cost and the knob DSI_FUSED_INTERLEAVE exist only there).

    python fused_schedule_child.py CASE      prints one line per run and, last, "SCHEDULE_OK CASE" -- or exits with status 1

Every case: (1) the expected depth map by the engine's own unfused path at the default settings -- evaluateDSI_batch per
camera, the fusion materialised in a Grid3D, collapseMaxZSlice of that grid; (2) the tie / empty-column condition asserted on
the downloaded fused DSI; (3) the DSI-less kernel under every schedule of the case, `array_equal` on depth, confidence
and index.  Inputs (numpy only) are built by inputs(); the module imports nothing of the engine until main() runs.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dvs_mcemvs_amd import synthetic as syn  # noqa: E402  (numpy only)

FUSE_MIN = 1

# name -> kind, grid (nx, ny, nz), band_rows (0: as tall as the kernel allows), cameras, lane mapping (-1: the engine's),
# which cameras stand still at the reference pose, and the kernel the case must reach as dsi_test_fused_last_launch names it
# (1 k_vote_fuse_argmax, 2 k_vote_fuse_argmax_2cu, 3 the instantiation that defers camera 1's arg-max update, 4 four cameras,
# 5 k_vote_fuse_argmax_alg2)
CASES = {
    # --- the draw ORDER, pinned: one workgroup as workgroup 0 of XCD k (dsi_test_fused_solo), dealt mode, bands == 1
    "solo_packed": dict(kind="solo", grid=(160, 96, 64), band_rows=0, bands=1, cams=2, lanes=1, still=(0,), ks=(1, 4, 7), kernel=3),
    "solo_vfill": dict(kind="solo", grid=(160, 96, 64), band_rows=0, bands=1, cams=2, lanes=5, still=(0,), ks=(1, 4, 7), kernel=1),
    "solo_three": dict(kind="solo", grid=(160, 96, 64), band_rows=0, bands=1, cams=3, lanes=-1, still=(0,), ks=(1, 4, 7), kernel=1),
    "solo_four": dict(kind="solo", grid=(160, 96, 64), band_rows=0, bands=1, cams=4, lanes=-1, still=(0, 1, 2, 3), ks=(1, 4, 7),
                      kernel=4),
    # (a band of 34 x 160 cells: the solo launch is the one-per-CU kernel's, the device's own launch the two-per-CU kernel's)
    "solo_three_bands": dict(kind="solo", grid=(160, 96, 64), band_rows=32, bands=3, cams=2, lanes=1, still=(0,), ks=(7,),
                             kernel=3, own_kernel=2),
    # --- the workgroup COUNT, pinned (dsi_test_fused_grid_blocks); the order within a count is the hardware's
    "count_one_band": dict(kind="count", grid=(160, 96, 100), band_rows=0, bands=1, cams=2, lanes=1, still=(0,),
                           counts=(8, 32, 64, 0), modes=("pieces", "turn", "dealt", "balanced"), kernel=3),
    "count_three_bands": dict(kind="count", grid=(160, 96, 64), band_rows=32, bands=3, cams=2, lanes=5, still=(0,),
                              counts=(8, 32, 64, 0), modes=("pieces", "turn", "dealt", "balanced"), kernel=1),
    "count_three_bands_four_cameras": dict(kind="count", grid=(160, 96, 64), band_rows=32, bands=3, cams=4, lanes=-1,
                                           still=(0, 1, 2, 3), counts=(8, 32, 64, 0), modes=("pieces", "turn", "dealt"),
                                           kernel=4),
    # 12 bands x 20 planes = 240 pairs: a forced count of 256 leaves workgroups without a pair on every device.  The vector
    # fill (mapping 5) has no two-per-CU kernel: bands of 10 x 160 cells stay on the one-per-CU kernel, which deals
    "count_twelve_bands": dict(kind="count", grid=(160, 96, 20), band_rows=8, bands=12, cams=3, lanes=5, still=(0,),
                               counts=(8, 32, 64, 256, 0), modes=("pieces", "turn", "dealt"), kernel=1),
    # a band of at most half the LDS and 10 x 1024 cells on the packed stream: k_vote_fuse_argmax_2cu, 2 x count workgroups;
    # it reads no balanced partition, and its "dealt" is "in turn"
    "count_two_per_cu": dict(kind="count", grid=(96, 72, 32), band_rows=0, bands=1, cams=2, lanes=1, still=(0,),
                             counts=(8, 32, 64, 0), modes=("pieces", "turn", "dealt"), kernel=2),
    "count_two_per_cu_twelve_bands": dict(kind="count", grid=(160, 96, 20), band_rows=8, bands=12, cams=3, lanes=1, still=(0,),
                                          counts=(8, 32, 64, 256, 0), modes=("pieces", "turn", "dealt"), kernel=2),
    # one process_method-2 window: k_vote_fuse_argmax_alg2 against the DSI-writing Alg. 2 path
    "count_alg2": dict(kind="alg2", grid=(96, 72, 32), band_rows=0, cams=2, lanes=-1, still=(0,), counts=(8, 32, 64, 0),
                       kernel=5),
    "count_alg2_fifteen_bands": dict(kind="alg2", grid=(96, 72, 32), band_rows=5, cams=2, lanes=-1, still=(0,),
                                     counts=(8, 32, 64, 0), kernel=5),
}


def inputs(case):
    """Events and trajectories of CASES[case] that make the fused DSI rich in EXACT ties: a camera that stands still at the
    reference pose votes an event into the same pixels of every plane (its centre is the reference view's: the plane
    homographies are the identity), so its DSI repeats from plane to plane up to the last bit of a few coordinates; its
    events are few (about one per pixel) and leave the right fifth of the image and a fifth of the pixels elsewhere
    empty.  Fused by MIN with the dense DSIs of moving cameras the minimum is the still camera's value on every plane
    the others exceed it on -- a tie over several planes, beginning anywhere --, and zero on every plane where the still
    camera has nothing.  Four cameras are fused by the geometric-mean tree: a product, tied only where every factor is:
    all four stand still.  Returns a synthetic.stereo_rig dict (+ "n_cams")."""
    c = CASES[case]
    nx, ny, nz = c["grid"]
    n_cams = c["cams"]
    n_moving = 60_000 if nx > 100 else 30_000
    rig = syn.stereo_rig(n_moving, width=nx, height=ny, duration=0.3, seed=401 + nx + nz, n_points=900, n_cams=n_cams)
    T_w_rv = syn.pose_inverse(rig["T_rv_w"])
    times = rig["trajectories"][0][0]
    still_traj = (times.copy(), np.tile(T_w_rv, (times.shape[0], 1)))
    for i in c["still"]:
        rng = np.random.default_rng(977 + 13 * i + nz)
        n = int(1.6 * 0.8 * nx * ny) // 1024 * 1024 + 1024 + 1     # (whole packets: evaluateDSI drops the tail)
        x = rng.integers(0, int(0.8 * nx), n).astype(np.uint16)
        y = rng.integers(0, ny, n).astype(np.uint16)
        ts = np.sort(rng.uniform(rig["t0"], rig["t1"], n))
        rig["events"][i] = (x, y, ts)
        rig["trajectories"][i] = still_traj
    rig["n_cams"] = n_cams
    return rig


def tie_statistics(fused, k=None, bands=1, band_rows=0):
    """Columns of the fused DSI [nz][ny][nx]: how many are empty (zero on every plane), how many have a non-zero maximum
    attained on two or more planes and -- k given: the solo launch as XCD k, which begins at pair P k / 8 of the band-major
    list of P = bands nz pairs, i.e. in the middle of a band (bands == 1: at plane k nz / 8) that it re-enters from plane 0
    after the wrap -- how many columns of THAT band have their first tied plane below the first plane voted and another
    tied plane at or above it."""
    nz = fused.shape[0]
    mx = fused.max(axis=0)
    at_max = fused == mx[None]
    tied = (mx > 0) & (at_max.sum(axis=0) >= 2)
    out = dict(columns=int(mx.size), empty=int((mx == 0).sum()), tied=int(tied.sum()))
    if k is not None:
        band, first_voted = divmod((bands * nz * k) // 8, nz)
        assert first_voted > 0
        first = at_max.argmax(axis=0)
        across = tied & (first < first_voted) & at_max[first_voted:].any(axis=0)
        if bands > 1:
            across[:band * band_rows] = False
            across[(band + 1) * band_rows:] = False
        out["tied_across_the_wrap"] = int(across.sum())
    return out


def assert_tie_rich(stats, what, key="tied"):
    n = stats["columns"]
    msg = "%s: %d columns, %d empty, %d tied%s" % (what, n, stats["empty"], stats["tied"],
                                                   ", %d tied across the wrap" % stats[key] if key != "tied" else "")
    print("INPUT " + msg)
    assert stats[key] >= 100 and stats[key] * 100 >= n, "too few tied columns -- " + msg
    assert stats["empty"] * 10 >= n, "fewer than 10 %% of the columns are empty -- " + msg


def compare(got, want, what, failures):
    diff = [int((g != w).sum()) for g, w in zip(got, want)]
    ok = all(np.array_equal(g, w) for g, w in zip(got, want))
    print("%s %s: depth / confidence / index differ at %d / %d / %d pixels" % ("SAME" if ok else "DIFFERENT", what, *diff))
    if not ok:
        failures.append(what)


def main(case):
    assert os.environ.get("DSI_ENGINE_EXPERIMENTS", "0") not in ("", "0") and "DSI_FUSED_INTERLEAVE" not in os.environ
    import dvs_mcemvs_amd as d
    from dvs_mcemvs_amd import process
    c = CASES[case]
    nx, ny, nz = c["grid"]
    rig = inputs(case)
    n = rig["n_cams"]
    L = d.load_library()
    assert L.dsi_build_flavour() == 1
    ctx = d.Context(0)
    shape = d.ShapeDSI(0, 0, nz, 4.0, 150.0, 0.0)
    failures = []

    def set_count(count):
        assert L.dsi_test_fused_grid_blocks(int(count)) == 0

    def assert_launched(blocks, interleave, kernel, splits=0):
        """What the engine says it launched last: the forced count (0: the device's own, whole groups of 8; twice the count for
        two workgroups per CU; 1: a solo launch), the forced mode, the kernel the case is about, a balanced partition."""
        import ctypes
        got = [ctypes.c_int(-9) for _ in range(4)]
        assert L.dsi_test_fused_last_launch(*[ctypes.byref(g) for g in got]) == 0
        got = [g.value for g in got]
        per_cu = 2 if kernel == 2 else 1
        assert got[1:] == [interleave, kernel, splits], (got, blocks, interleave, kernel, splits)
        if blocks:
            assert got[0] == blocks * per_cu if blocks > 1 else got[0] == 1, (got, blocks)
        else:
            assert got[0] >= 8 * per_cu and got[0] % (8 * per_cu) == 0, got

    if c["kind"] == "alg2":
        # one process_method-2 window, two sub-intervals, cameras fused by MIN, sub-intervals by the arithmetic mean
        ts, n_sub, sf, tf = rig["t0"] + 0.2, 2, FUSE_MIN, 4
        cams2 = [rig["cam"], rig["cam"]]
        fused, cam_time = d.MapperEMVS(ctx, rig["cam"], shape), d.MapperEMVS(ctx, rig["cam"], shape)
        out = process.process_2(ctx, cams2, shape, rig["events"], rig["trajectories"], n_sub, fused, cam_time, ts, sf, tf)
        out["left"].close()
        out["right"].close()
        want = [fused.getDepthMapFromDSI(), cam_time.getDepthMapFromDSI()]
        assert_tie_rich(tie_statistics(fused.dsi_.download().reshape(nz, ny, nx)), case + " time_camera")
        assert_tie_rich(tie_statistics(cam_time.dsi_.download().reshape(nz, ny, nx)), case + " camera_time")
        mappers = [d.MapperEMVS(ctx, rig["cam"], shape) for _ in range(2)]
        out_tc, out_ct = d.MapperEMVS(ctx, rig["cam"], shape), d.MapperEMVS(ctx, rig["cam"], shape)
        if c["band_rows"]:
            out_tc.set_band_params(c["band_rows"], 0, 0)
        batches = process.alg2_window_batches(ctx, rig["events"], rig["trajectories"], ts, n_sub, 2)
        for count in c["counts"]:
            set_count(count)
            out_tc.computeDepthMapOfEventsAlg2(out_ct, mappers, batches, n_sub, sf, tf)
            compare(out_tc.fetchDepthMap(), want[0], "%s time_camera, %d workgroups" % (case, count), failures)
            compare(out_ct.fetchDepthMap(), want[1], "%s camera_time, %d workgroups" % (case, count), failures)
            assert_launched(count, 0, c["kernel"])
            if c["band_rows"]:
                assert out_tc.last_vote_info()["band_rows"] == c["band_rows"]
        set_count(0)
    else:
        batches = []
        for i in range(n):
            first, Rt = d.packetize(rig["events"][i][2], rig["trajectories"][i], rig["T_rv_w"])
            batches.append(d.EventBatch(ctx, rig["events"][i][0], rig["events"][i][1], Rt, first))
        assert sum(int(b.n_packets) for b in batches) * 1024 <= 400_000
        # the expected map: vote, fuse (process1.cpp:126-191 / the geometric-mean tree), collapse -- default settings
        ref_m = [d.MapperEMVS(ctx, rig["cam"], shape) for _ in range(n)]
        for m, b in zip(ref_m, batches):
            m.evaluateDSI_batch(b)
        F = d.Grid3D(ctx, nx, ny, nz)
        if n == 4:
            F.setToFusionOfN([m.dsi_ for m in ref_m], d.ACC_GM_TREE)
        else:
            F.resetGrid()
            F.addTwoGrids(ref_m[0].dsi_)
            F.fuseTwoGrids(ref_m[1].dsi_, FUSE_MIN)
            if n == 3:
                F.minTwoGrids(ref_m[2].dsi_)
        want = ref_m[0].getDepthMapFromDSI(F)
        fused_host = F.download().reshape(nz, ny, nx)
        assert np.array_equal(want[2], fused_host.argmax(axis=0)) and np.array_equal(want[1], fused_host.max(axis=0))
        fus_m = [d.MapperEMVS(ctx, rig["cam"], shape) for _ in range(n + 1)]
        out = fus_m[-1]                     # (the fused path reads its knobs from the OUTPUT mapper of the call)
        for m in fus_m:
            m.set_packed_lanes(c["lanes"])
            m.set_band_params(c["band_rows"], 0, 0)

        def run():
            if n == 4:
                out.computeDepthMapOfEventsN(fus_m[:4], batches)
            else:
                out.computeDepthMapOfEvents(fus_m[:n], batches, FUSE_MIN)
            info = out.last_vote_info()
            assert info["algo"] == d.VOTE_FUSED_ARGMAX and info["bands"] == c["bands"], info
            if c["lanes"] >= 0:
                assert info["packed"] == c["lanes"], info
            return out.fetchDepthMap()

        if c["kind"] == "solo":
            for k in c["ks"]:
                assert_tie_rich(tie_statistics(fused_host, k, c["bands"], c["band_rows"]), "%s, XCD %d" % (case, k),
                                "tied_across_the_wrap")
            for k in c["ks"]:
                assert L.dsi_test_fused_solo(out._h, k) == 0
                compare(run(), want, "%s, one workgroup as XCD %d" % (case, k), failures)
                assert_launched(1, 2, c["kernel"])
            assert L.dsi_test_fused_solo(out._h, -1) == 0
            compare(run(), want, "%s, the device's own launch" % case, failures)
            assert_launched(0, 0, c.get("own_kernel", c["kernel"]))      # (inputs this small: contiguous pieces)
        else:
            assert_tie_rich(tie_statistics(fused_host), case)
            # what launch_vote_fuse_argmax asks of a band for two workgroups per CU: the packed stream, two or three cameras, at
            # most half the LDS and 10 x 1024 cells -- true of the two-per-CU cases only
            info = (run(), out.last_vote_info())[1]
            small = info["lds_bytes"] * 2 <= 160 * 1024 and (info["band_rows"] + 2) * nx <= 10 * 1024
            assert (small and info["packed"] in (1, 3) and n < 4) == (c["kernel"] == 2), info
            for count in c["counts"]:
                set_count(count)
                for mode in c["modes"]:
                    interleave = {"pieces": 0, "turn": 1, "dealt": 2, "balanced": 0}[mode]
                    os.environ["DSI_FUSED_INTERLEAVE"] = str(interleave)
                    assert L.dsi_test_fused_fixed_cost(out._h, 64 if mode == "balanced" else -1) == 0
                    # (dealt: twice on the same output mapper -- the counters behind the keys must be zero again)
                    for call in range(2 if mode == "dealt" else 1):
                        compare(run(), want, "%s, %d workgroups, %s, call %d" % (case, count, mode, call), failures)
                        assert_launched(count, interleave, c["kernel"], int(mode == "balanced"))
            del os.environ["DSI_FUSED_INTERLEAVE"]
            assert L.dsi_test_fused_fixed_cost(out._h, -1) == 0
            set_count(0)
    ctx.synchronize()
    if failures:
        print("SCHEDULE_FAILED %s: %d runs differ" % (case, len(failures)))
        return 1
    print("SCHEDULE_OK " + case)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
