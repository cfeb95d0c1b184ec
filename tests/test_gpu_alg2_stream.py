"""Alg. 2 windows (process_2 / process_5) without a DSI: MapperEMVS.computeDepthMapOfEventsAlg2 and the process_method 2 / 5
stream against the materialising path -- process.process_2 followed by the depth maps of mapper_fused.dsi_ (time_camera)
and mapper_fused_camera_time.dsi_ (camera_time) -- bit for bit: depth, confidence as uint32 and indices."""
import numpy as np
import pytest

import dvs_mcemvs_amd as d
from dvs_mcemvs_amd import engine as E, process, synthetic as syn
from oracle_pipeline import OracleMapper, argmax_report, oracle_process_2

pytestmark = pytest.mark.gpu


def assert_maps_equal(got, ref, what=""):
    depth_g, conf_g, idx_g = got
    depth_r, conf_r, idx_r = ref
    assert np.array_equal(idx_g, idx_r), "%s: %d indices differ" % (what, int((idx_g != idx_r).sum()))
    assert np.array_equal(conf_g.view(np.uint32), conf_r.view(np.uint32)), what
    assert np.array_equal(depth_g.view(np.uint32), depth_r.view(np.uint32)), what


def materialized(ctx, cam, shape, events, trajs, ts, n_sub, sf, tf, pm):
    """The yardstick: process_2 (process_5), then the arg-max of each DSI."""
    fused, cam_time = d.MapperEMVS(ctx, cam, shape), d.MapperEMVS(ctx, cam, shape)
    out = process.process_2(ctx, [cam, cam], shape, events, trajs, n_sub, fused, cam_time, ts, sf, tf,
                            shuffle_right=pm == 5)
    out["left"].close()
    out["right"].close()
    res = []
    for m in (fused, cam_time):
        res.append(m.getDepthMapFromDSI())
        m.close()
    return res


def dsi_less(ctx, cam, shape, events, trajs, ts, n_sub, sf, tf, pm, camera_time=True, band_rows=0, lanes=-1):
    mappers = [d.MapperEMVS(ctx, cam, shape) for _ in range(2)]
    out_tc = d.MapperEMVS(ctx, cam, shape)
    out_ct = d.MapperEMVS(ctx, cam, shape) if camera_time else None
    if band_rows:
        out_tc.set_band_params(band_rows=band_rows)
    if lanes >= 0:
        out_tc.set_packed_lanes(lanes)
    batches = process.alg2_window_batches(ctx, events, trajs, ts, n_sub, pm)
    out_tc.computeDepthMapOfEventsAlg2(out_ct, mappers, batches, n_sub, sf, tf)
    res = [out_tc.fetchDepthMap(), out_ct.fetchDepthMap() if out_ct is not None else None]
    for o in batches + mappers + [out_tc] + ([out_ct] if out_ct is not None else []):
        o.close()
    return res


@pytest.fixture(scope="module")
def small():
    rig = syn.stereo_rig(24_000 + 333, width=96, height=72, duration=0.3, seed=71, n_points=800)
    return rig, d.ShapeDSI(0, 0, 32, 4.0, 150.0, 0.0), rig["t0"] + 0.2


@pytest.mark.parametrize("pm", [2, 5])
def test_small_every_fusion(ctx, small, pm):
    rig, shape, ts = small
    for sf in range(1, 7):
        for tf in range(1, 7):
            ref = materialized(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 2, sf, tf, pm)
            got = dsi_less(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 2, sf, tf, pm)
            assert_maps_equal(got[0], ref[0], "time_camera pm=%d sf=%d tf=%d" % (pm, sf, tf))
            assert_maps_equal(got[1], ref[1], "camera_time pm=%d sf=%d tf=%d" % (pm, sf, tf))


@pytest.mark.parametrize("n_sub", [1, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("sf,tf", [(2, 2), (2, 4), (4, 2)])
def test_small_subinterval_counts(ctx, small, n_sub, sf, tf):
    rig, shape, ts = small
    for pm in (2, 5):
        ref = materialized(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, n_sub, sf, tf, pm)
        got = dsi_less(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, n_sub, sf, tf, pm)
        assert_maps_equal(got[0], ref[0], "time_camera N=%d pm=%d" % (n_sub, pm))
        assert_maps_equal(got[1], ref[1], "camera_time N=%d pm=%d" % (n_sub, pm))
        tc_only = dsi_less(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, n_sub, sf, tf, pm, camera_time=False)
        assert tc_only[1] is None
        assert_maps_equal(tc_only[0], ref[0], "time_camera alone N=%d pm=%d" % (n_sub, pm))


@pytest.mark.parametrize("lanes", [1, 3, 5, 6])
@pytest.mark.parametrize("band_rows", [0, 5, 17])
def test_small_forced_bands_and_lanes(ctx, small, lanes, band_rows):
    rig, shape, ts = small
    ref = materialized(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 3, 2, 4, 5)
    got = dsi_less(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 3, 2, 4, 5, band_rows=band_rows,
                   lanes=lanes)
    assert_maps_equal(got[0], ref[0], "time_camera")
    assert_maps_equal(got[1], ref[1], "camera_time")


def test_short_subintervals_empty_camera_dropped_tail(ctx):
    rig = syn.stereo_rig(9_000 + 7, width=96, height=72, duration=0.3, seed=73, n_points=600)
    shape = d.ShapeDSI(0, 0, 32, 4.0, 150.0, 0.0)
    ts = rig["t0"] + 0.25
    ev = rig["events"]
    cases = {
        "below 1024 per sub-interval": ([tuple(a[:8_000] for a in ev[c]) for c in range(2)], 8),   # 1000 events each
        "one camera below 1024": ([ev[0], tuple(a[:5_000] for a in ev[1])], 8),
        "empty camera": ([ev[0], tuple(a[:0] for a in ev[1])], 4),
        "dropped tail": ([tuple(a[:8_191] for a in ev[0]), ev[1]], 4),
    }
    for what, (events, n_sub) in cases.items():
        for sf, tf, pm in ((2, 2, 2), (4, 4, 5), (1, 2, 5)):
            ref = materialized(ctx, rig["cam"], shape, events, rig["trajectories"], ts, n_sub, sf, tf, pm)
            got = dsi_less(ctx, rig["cam"], shape, events, rig["trajectories"], ts, n_sub, sf, tf, pm)
            assert_maps_equal(got[0], ref[0], what)
            assert_maps_equal(got[1], ref[1], what)


@pytest.mark.parametrize("sf", [2, 4])
@pytest.mark.parametrize("tf", [2, 4])
def test_mvsec_like(ctx, sf, tf):
    rig = syn.stereo_rig(1_000_000, width=346, height=260, duration=0.05, seed=81, n_points=5000)
    shape = d.ShapeDSI(0, 0, 100, 4.0, 200.0, 0.0)
    ts = rig["t0"] + 0.05
    ref = materialized(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 2, sf, tf, 2)
    got = dsi_less(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 2, sf, tf, 2)
    assert_maps_equal(got[0], ref[0], "time_camera")
    assert_maps_equal(got[1], ref[1], "camera_time")


def test_configs2_like(ctx):
    rig = syn.stereo_rig(500_000, width=640, height=480, duration=0.05, seed=83, n_points=6000)
    shape = d.ShapeDSI(512, 512, 200, 4.0, 200.0, 0.0)
    ts = rig["t0"] + 0.05
    for pm in (2, 5):
        ref = materialized(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 4, 2, 4, pm)
        got = dsi_less(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 4, 2, 4, pm)
        assert_maps_equal(got[0], ref[0], "time_camera pm=%d" % pm)
        assert_maps_equal(got[1], ref[1], "camera_time pm=%d" % pm)


@pytest.mark.parametrize("pm", [2, 5])
def test_full_sequence_stream(ctx, pm):
    n_win, ev_win, dur, t0 = 8, 40_000, 0.05, 10.0
    rig = syn.stereo_rig(n_win * ev_win, width=128, height=96, t0=t0, duration=n_win * dur, seed=87, n_points=1500)
    cam = rig["cam"]
    shape = d.ShapeDSI(0, 0, 40, 4.0, 150.0, 0.0)
    opts_dm, opts_pc = d.OptionsDepthMap(), d.OptionsPointCloud(0.5, 3)
    args = (ctx, (cam, cam), shape, rig["events"], rig["trajectories"], t0, t0 + n_win * dur + 1e-9, dur, dur)
    kw = dict(fusion_method=2, process_method=pm, num_subintervals=3, temporal_fusion=2)
    got = list(process.full_sequence(*args, options_depth_map=opts_dm, options_point_cloud=opts_pc, concurrent=True, **kw))
    raw = list(process.full_sequence(*args, **kw))
    assert len(got) == len(raw) == n_win
    for (ts, tc, ct), (ts2, tc_raw, ct_raw), (w0, w1) in zip(got, raw, process.window_bounds(t0, t0 + n_win * dur + 1e-9, dur, dur)):
        assert ts == ts2 == w1
        assert (ct is None) == (pm == 5) and (ct_raw is None) == (pm == 5)
        ev = [process.window_events(rig["events"][c], w0, w1) for c in range(2)]
        fused, cam_time = d.MapperEMVS(ctx, cam, shape), d.MapperEMVS(ctx, cam, shape)
        out = process.process_2(ctx, [cam, cam], shape, ev, rig["trajectories"], 3, fused, cam_time, ts, 2, 2,
                                shuffle_right=pm == 5)
        out["left"].close()
        out["right"].close()
        for mine, mine_raw, m in ((tc, tc_raw, fused), (ct, ct_raw, cam_time)):
            if mine is None:
                continue
            assert_maps_equal(mine_raw, m.getDepthMapFromDSI(), "raw window %g" % ts)
            depth, conf, mask = m.getDepthMapFromDSI(options_depth_map=opts_dm)
            for a, b in zip(mine[:3], (depth, conf, mask)):
                assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))
            pc = m.getPointcloud(options_pc=opts_pc)
            assert np.array_equal(mine[3].view(np.uint32), pc.view(np.uint32))
        fused.close()
        cam_time.close()


def test_stream_planner_materializes_beyond_eight(ctx, small):
    rig, shape, ts = small
    ws = process.WindowStream(ctx, (rig["cam"], rig["cam"]), shape, fusion_method=2, process_method=2,
                              num_subintervals=9, temporal_fusion=4)
    slot = ws.submit(rig["events"], rig["trajectories"], ts)
    assert ws.last_plan == "materialize"
    tc, ct = ws.fetch(slot)
    ws.close()
    ref = materialized(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 9, 2, 4, 2)
    assert_maps_equal(tc, ref[0], "time_camera")
    assert_maps_equal(ct, ref[1], "camera_time")
    assert process.alg2_plan(8, 1000, 96) == "fused" and process.alg2_plan(9, 1000, 96) == "materialize"


def test_stream_refuses_options_without_effect(ctx, small):
    rig, shape, ts = small
    cams = (rig["cam"], rig["cam"])
    for kw in (dict(fused_vote=True), dict(exact_ties=True), dict(materialize_fused=False)):
        with pytest.raises(ValueError):
            process.WindowStream(ctx, cams, shape, process_method=2, **kw)
    ws = process.WindowStream(ctx, cams, shape, process_method=5, num_subintervals=2)
    with pytest.raises(ValueError):
        ws.submit(rig["events"], rig["trajectories"], ts, asynchronous=True)
    with pytest.raises(ValueError):
        ws.submit(rig["events"], rig["trajectories"], ts, rv_pos=0.1)
    ws.close()


def test_cpp_stream(built, tmp_path):
    """dsi::full_sequence_depth_maps_alg2 against ::process_2 / ::process_5 + getDepthMapFromDSI per window (memcmp of the
    raw maps, the filtered maps and the point clouds), the materialising path of the planner and the argument errors."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_alg2_stream")
    pkg = os.path.join(root, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(root, "tests", "cpp", "test_alg2_stream.cpp"), "-I" + os.path.join(root, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_index_map_against_oracle(ctx):
    rig = syn.stereo_rig(16_000, width=64, height=48, duration=0.3, seed=89, n_points=500)
    shape = d.ShapeDSI(0, 0, 12, 4.0, 150.0, 0.0)
    ts = rig["t0"] + 0.15
    got = dsi_less(ctx, rig["cam"], shape, rig["events"], rig["trajectories"], ts, 4, 2, 2, 2)
    ref = oracle_process_2(lambda: OracleMapper(rig["cam"], dimZ=12, min_depth=4.0, max_depth=150.0),
                           rig["events"], rig["trajectories"], 4, ts, 2, 2)
    rep = argmax_report(got[0][2], ref["fused"], 2e-4)
    assert rep["violations"] == 0, rep
    rep = argmax_report(got[1][2], ref["camera_time"], 4e-4)
    assert rep["violations"] == 0, rep


def test_argument_errors(ctx, small):
    rig, shape, ts = small
    cam = rig["cam"]
    mappers = [d.MapperEMVS(ctx, cam, shape) for _ in range(2)]
    out_tc, out_ct = d.MapperEMVS(ctx, cam, shape), d.MapperEMVS(ctx, cam, shape)
    batches = process.alg2_window_batches(ctx, rig["events"], rig["trajectories"], ts, 2)
    L = E.load_library()

    def code(*args):
        with pytest.raises(d.DsiError) as e:
            out_tc.computeDepthMapOfEventsAlg2(*args)
        return e.value.code

    assert code(out_ct, mappers, batches, 2, 0, 2) == E.ERR_BAD_OP
    assert code(out_ct, mappers, batches, 2, 7, 4) == E.ERR_BAD_OP
    hm = (E.C.c_void_p * 2)(*[m._h for m in mappers])
    many = batches * 5
    hb = (E.C.c_void_p * len(many))(*[b._h for b in many])
    assert L.dsi_mapper_depth_map_of_events_alg2(out_tc._h, out_ct._h, hm, hb, 9, 2, 2) == E.ERR_INVALID
    assert L.dsi_mapper_depth_map_of_events_alg2(out_tc._h, out_ct._h, hm, hb, 0, 2, 2) == E.ERR_INVALID
    assert L.dsi_mapper_depth_map_of_events_alg2(None, out_ct._h, hm, hb, 2, 2, 2) == E.ERR_INVALID
    assert L.dsi_mapper_depth_map_of_events_alg2(out_tc._h, out_ct._h, None, hb, 2, 2, 2) == E.ERR_INVALID
    assert L.dsi_mapper_depth_map_of_events_alg2(out_tc._h, out_ct._h, hm, None, 2, 2, 2) == E.ERR_INVALID
    other = d.MapperEMVS(ctx, cam, d.ShapeDSI(0, 0, 16, 4.0, 150.0, 0.0))
    assert code(other, mappers, batches, 2, 2, 2) == E.ERR_SHAPE
    ctx2 = d.Context(ctx.device)
    foreign = d.MapperEMVS(ctx2, cam, shape)
    assert code(foreign, mappers, batches, 2, 2, 2) == E.ERR_CONTEXT
    foreign.close()
    ctx2.close()
    for o in batches + mappers + [out_tc, out_ct, other]:
        o.close()
