"""GPU tests of the ground truth from disparity images: dsi_gt_* against the fixture built the way the
reference's script builds it (tests/golden/dsec_ground_truth.npz) and against the numpy restatement
(tests/ground_truth_reference.py).  Every comparison is exact: array_equal on the maps, == on the counts, the bytes of
the metrics.  The feature has no tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import ground_truth_reference as gr
from dvs_mcemvs_amd import engine, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
B, FOCAL = 0.6, 557.25
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "dsec_ground_truth.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
MODES = (("script", engine.GT_AS_SCRIPT), ("drop", engine.GT_DROP_OUTSIDE))
REALS = ("sum_di", "sum_di2", "sum_are", "sum_abs", "max_gt", "silog", "are", "lrmse", "badp", "mean_abs", "median_abs")
# Q: (X, Y, Z) = (x, y, d); K: u = X, v = Y, value = Z -- with T = identity the depth map is the disparity image itself
Q_IMAGE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
K_IMAGE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)


def golden_case(name):
    return {k[len(name) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "_")}


def code_of(fn):
    try:
        fn()
    except d.DsiError as e:
        return e.code
    return engine.OK


def bits(m):
    return np.array([m[k] for k in REALS] + list(m["delta"]), np.float64).tobytes()


def same_metrics(a, b):
    ints = lambda m: {k: v for k, v in m.items() if k not in REALS and k != "delta"}
    return bits(a) == bits(b) and ints(a) == ints(b)


def same_curves(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("base", "precision", "recall", "f1", "outliers"))


def scene(seed, H, W, focal_scale=0.97, p_zero=0.3):
    """a calibration like DSEC's at H x W and the uint16 samples of a random disparity image"""
    rng = np.random.default_rng(seed)
    cx, cy, f = W / 2.0 + 0.3, H / 2.0 - 0.2, 0.9 * W
    Q = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, 1.0 / B, 0]], np.float64)
    a = 0.01
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    T[0, 3] = 0.12                                                           # carries a very near point out of the image
    K = np.zeros((3, 4))
    K[0, 0] = K[1, 1] = focal_scale * f
    K[0, 2], K[1, 2], K[2, 2] = cx, cy, 1.0
    raw = rng.integers(256, 3000, (H, W)).astype(np.uint16)
    raw[rng.random((H, W)) < p_zero] = 0
    return Q, T, K, raw


# ------------------------------------------------------------------------------------ the script's own results
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tag,mode", MODES)
def test_fixture_case(ctx, name, tag, mode):
    g = golden_case(name)
    H, W = g["d"].shape
    p = d.GroundTruthProjector(ctx, W, H, g["Q"], g["T"], g["K"], mode)
    want, (n_points, n_outside) = g[tag + "_depth"], (int(v) for v in g[tag + "_counts"])
    p.project(g["d"])
    depth, n, o = p.fetch()
    assert depth.dtype == F and np.array_equal(depth, want) and (n, o) == (n_points, n_outside)
    p.project_png16(g["raw"])
    depth, n, o = p.fetch()
    assert np.array_equal(depth, want) and (n, o) == (n_points, n_outside)
    p.close()


def test_png16_conversion_on_the_device_for_every_value(ctx):
    raw = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    p = d.GroundTruthProjector(ctx, 256, 256, Q_IMAGE, np.eye(4), K_IMAGE)
    p.project_png16(raw)
    depth, n, o = p.fetch()
    assert (n, o) == (65536, 0) and np.array_equal(depth, engine.disparity_from_png16(raw))
    assert np.array_equal(depth, np.divide(raw, 65535, dtype=np.float32) * 256)
    p.close()


# ------------------------------------------------------------------------------------- the winner and the reruns
def test_one_target_pixel_twice_and_tiny_frames(ctx):
    g = golden_case("one_pixel")
    H, W = g["d"].shape
    p = d.GroundTruthProjector(ctx, W, H, g["Q"], g["T"], g["K"])
    runs = []
    for _ in range(2):
        p.project(g["d"])
        runs.append(p.fetch())
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1:] == runs[1][1:]
    pt = gr.points(g["d"], g["Q"], g["T"], g["K"])
    last = int(np.flatnonzero(pt["kept"])[-1])                               # the last kept source pixel wins
    assert np.count_nonzero(runs[0][0]) == 1 and runs[0][0][pt["iv"][last], pt["iu"][last]] == pt["value"][last]
    assert runs[0][0][pt["iv"][last], pt["iu"][last]] != pt["value"][int(np.flatnonzero(pt["kept"])[0])]
    p.close()
    # 1 x 64: every pixel of the row lands on column 5; 1 x 1: the frame is its own target
    K5 = np.array([[0, 0, 0, 5], [0, 0, 0, 0], [0, 0, 0, 1]], np.float64)
    row = np.arange(1, 65, dtype=F).reshape(1, 64)
    row[0, 60:] = np.inf                                                     # dropped: pixel 59 is the last kept one
    for mode in (engine.GT_AS_SCRIPT, engine.GT_DROP_OUTSIDE):
        p = d.GroundTruthProjector(ctx, 64, 1, Q_IMAGE, np.eye(4), K5, mode)
        outs = []
        for _ in range(2):
            p.project(row)
            outs.append(p.fetch())
        want = gr.project(row, Q_IMAGE, np.eye(4), K5, mode)
        assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1:] == outs[1][1:] == want[1:] == (60, 0)
        assert np.array_equal(outs[0][0], want[0]) and outs[0][0][0, 5] == 60.0 and np.count_nonzero(outs[0][0]) == 1
        p.close()
        p = d.GroundTruthProjector(ctx, 1, 1, Q_IMAGE, np.eye(4), K_IMAGE, mode)
        for v, want in ((3.5, (3.5, 1, 0)), (np.inf, (0.0, 0, 0)), (np.nan, (0.0, 0, 0)), (-2.0, (-2.0, 1, 0))):
            p.project(np.array([[v]], F))
            depth, n, o = p.fetch()
            assert (float(depth[0, 0]), n, o) == want, v
        p.close()
    # before the first projection: zeros
    p = d.GroundTruthProjector(ctx, 7, 3, Q_IMAGE, np.eye(4), K_IMAGE)
    depth, n, o = p.fetch()
    assert not depth.any() and (n, o) == (0, 0) and p.device_ptr()
    p.close()


def test_projector_reused_for_three_frames(ctx):
    """a dense frame, then sparser ones: a winner table or an output map that was not cleared would show through"""
    H, W = 29, 37
    for mode in (engine.GT_AS_SCRIPT, engine.GT_DROP_OUTSIDE):
        Q, T, K, _ = scene(1, H, W, focal_scale=0.8)
        p = d.GroundTruthProjector(ctx, W, H, Q, T, K, mode)
        frames = [scene(2, H, W, p_zero=0.0)[3], scene(3, H, W, p_zero=0.8)[3], scene(4, H, W, p_zero=0.5)[3]]
        frames[1][0, 0] = 65535                                               # so near that it leaves the image: one outside
        seen = []
        for raw in frames:
            p.project_png16(raw)
            depth, n, o = p.fetch()
            want = gr.project(gr.disparity_from_png16(raw), Q, T, K, mode)
            assert np.array_equal(depth, want[0]) and (n, o) == want[1:]
            seen.append((np.count_nonzero(depth), o))
        assert seen[0][0] > seen[2][0] > 0 and seen[1][1] == 1
        assert (seen[1][0] == 0) == (mode == engine.GT_AS_SCRIPT)
        p.close()


def test_script_frame_size_once(ctx):
    H, W = 480, 640
    Q, T, K, raw = scene(5, H, W, focal_scale=0.97)
    disp = engine.disparity_from_png16(raw)
    want = gr.project(disp, Q, T, K, engine.GT_DROP_OUTSIDE)
    p = d.GroundTruthProjector(ctx, W, H, Q, T, K, engine.GT_DROP_OUTSIDE)
    p.project(disp)
    depth, n, o = p.fetch()
    assert np.array_equal(depth, want[0]) and (n, o) == want[1:]
    assert n > 200000 and np.count_nonzero(depth) > 150000
    p.close()


# ------------------------------------------------------------------------------------------------ the score
def test_add_gt_equals_add_of_the_fetched_map(ctx):
    H, W = 29, 37
    Q, T, K, raw = scene(6, H, W)
    p = d.GroundTruthProjector(ctx, W, H, Q, T, K, engine.GT_DROP_OUTSIDE)
    p.project_png16(raw)
    gt, n, _ = p.fetch()
    rng = np.random.default_rng(7)
    est = (np.where(gt > 0, gt, 5.0) * np.exp(rng.normal(0, 0.2, gt.shape))).astype(F)
    mask = (rng.random(gt.shape) < 0.6).astype(np.uint8)
    a, b = d.DepthScore(ctx, H * W, B, FOCAL), d.DepthScore(ctx, H * W, B, FOCAL)
    a.addGroundTruth(est, mask, p)
    b.add(est, mask, gt)
    ma, mb = a.metrics(), b.metrics()
    assert ma["n_joint"] > 100 and same_metrics(ma, mb) and same_curves(a.curves(), b.curves())
    # errors: maps of another size, shapes that differ, a projector of another context
    assert code_of(lambda: a.addGroundTruth(est[:-1], mask[:-1], p)) == engine.ERR_INVALID
    with pytest.raises(ValueError):
        a.addGroundTruth(est, mask[:-1], p)
    with pytest.raises(ValueError):
        p.project(np.zeros((H, W + 1), F))
    with pytest.raises(ValueError):
        p.project(np.zeros((H, W), np.float64))
    other = d.Context(0)
    q = d.GroundTruthProjector(other, W, H, Q, T, K)
    assert code_of(lambda: a.addGroundTruth(est, mask, q)) == engine.ERR_CONTEXT
    assert d.load_library().dsi_context_destroy(other._h) == engine.ERR_CONTEXT        # a live projector keeps its context
    q.close()
    other.close()
    assert same_metrics(a.metrics(), mb)                                               # the refused adds added nothing
    for o in (a, b, p):
        o.close()


def test_add_mapper_gt_equals_add_of_the_fetched_maps(ctx):
    rig = syn.stereo_rig(60000, width=120, height=90, duration=0.3, seed=5)
    m = d.MapperEMVS(ctx, rig["cam"], d.ShapeDSI(0, 0, 40, 4.0, 200.0, 0.0))
    H, W = m.dimY, m.dimX
    Q, T, K, raw = scene(8, H, W)
    p = d.GroundTruthProjector(ctx, W, H, Q, T, K, engine.GT_DROP_OUTSIDE)
    a, b = d.DepthScore(ctx, H * W, B, FOCAL), d.DepthScore(ctx, H * W, B, FOCAL)
    assert code_of(lambda: a.addMapperGroundTruth(m, p)) == engine.ERR_INVALID          # nothing computed yet
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    depth, conf, mask = m.getDepthMapFromDSI(options_depth_map=d.OptionsDepthMap(5, 4.0, 5, 0.0))
    assert 0 < (mask > 0).sum() < mask.size
    p.project_png16(raw)
    a.addMapperGroundTruth(m, p)
    gt, _, _ = p.fetch()
    b.add(depth, mask, gt)
    ma, mb = a.metrics(), b.metrics()
    assert ma["n_joint"] > 20 and same_metrics(ma, mb) and same_curves(a.curves(), b.curves())
    small = d.GroundTruthProjector(ctx, W - 1, H, Q, T, K)
    assert code_of(lambda: a.addMapperGroundTruth(m, small)) == engine.ERR_INVALID      # another pixel count
    small.close()
    other = d.Context(0)
    q = d.GroundTruthProjector(other, W, H, Q, T, K)
    assert code_of(lambda: a.addMapperGroundTruth(m, q)) == engine.ERR_CONTEXT
    q.close()
    other.close()
    for o in (a, b, p, m):
        o.close()


# ------------------------------------------------------------------------------------------------ the erosion
@pytest.mark.parametrize("shape", ((1, 1), (5, 7), (37, 29)))
def test_thicken_edges(ctx, shape):
    rng = np.random.default_rng(9)
    depth = rng.uniform(1, 60, shape).astype(F)
    for p_est in (0.0, 0.15, 1.0):
        mask = (rng.random(shape) < p_est).astype(np.uint8)
        got_d, got_m = d.thicken_edges(ctx, depth, mask)
        want_d, want_m = gr.erode_cross(depth, mask)
        assert got_d.dtype == F and got_m.dtype == np.uint8
        assert np.array_equal(got_d, want_d) and np.array_equal(got_m, want_m), p_est
    got_d, got_m = d.thicken_edges(ctx, depth, np.ones(shape, np.uint8) * 255, no_estimate=1000.0)
    want_d, want_m = gr.erode_cross(depth, np.ones(shape, np.uint8), no_estimate=1000.0)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_m, want_m)


# ------------------------------------------------------------------------------------------- the window stream
def test_full_sequence_scores_against_disparity_frames(ctx):
    rig = syn.stereo_rig(90_000, width=96, height=72, t0=3.0, duration=0.9, seed=5)
    shape = d.ShapeDSI(0, 0, 24, 4.0, 100.0, 0.0)
    cams = (rig["cam"],) * 2
    opts = d.OptionsDepthMap(5, 4.0, 5, 0.0)
    args = (ctx, cams, shape, rig["events"], rig["trajectories"], 3.0, 3.9, 0.3, 0.3)
    plain = list(proc.full_sequence(*args, options_depth_map=opts))
    assert len(plain) == 3
    H, W = plain[0][1].shape
    Q, T, K, _ = scene(10, H, W)
    frames = [scene(11 + i, H, W)[3] for i in range(3)]
    times = [w[0] for w in plain]
    # frame 2 is nearest to the first window, frame 0 to the third; the second window's nearest frame is 0.12 away
    gt_times = np.array([times[2] + 0.03, times[1] + 0.12, times[0] - 0.02])
    picks = [proc.nearest_ground_truth(gt_times, t) for t in times]
    assert picks == [2, None, 0]
    for thicken in (False, True):
        p = d.GroundTruthProjector(ctx, W, H, Q, T, K, engine.GT_DROP_OUTSIDE)
        score = d.DepthScore(ctx, 3 * H * W, B, FOCAL)
        asked = []

        def frame(i):
            asked.append(i)
            return frames[i]

        scored = list(proc.full_sequence(*args, options_depth_map=opts, score=score,
                                         ground_truth_disparity=(frame, gt_times, p), thicken_edges=thicken))
        assert asked == [2, 0] and len(scored) == 3
        for w, q in zip(scored, plain):
            assert len(w) == len(q) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(w[1:], q[1:]))
        # the existing path, with ground truth made on the host
        host = d.DepthScore(ctx, 3 * H * W, B, FOCAL)
        gts = {t: (None if i is None else gr.project(gr.disparity_from_png16(frames[i]), Q, T, K, gr.DROP_OUTSIDE)[0])
               for t, i in zip(times, picks)}
        if thicken:
            for w, t in zip(plain, times):
                if gts[t] is not None:
                    host.add(*gr.erode_cross(w[1], w[3]), gts[t])
        else:
            list(proc.full_sequence(*args, options_depth_map=opts, score=host, ground_truth=lambda ts: gts[ts]))
        ms, mh = score.metrics(), host.metrics()
        assert ms["n_joint"] > 20 and same_metrics(ms, mh) and same_curves(score.curves(), host.curves())
        for o in (score, host, p):
            o.close()
    # a sequence of frames works like a callable
    p = d.GroundTruthProjector(ctx, W, H, Q, T, K, engine.GT_DROP_OUTSIDE)
    score = d.DepthScore(ctx, 3 * H * W, B, FOCAL)
    list(proc.full_sequence(*args, options_depth_map=opts, score=score, ground_truth_disparity=(frames, gt_times, p)))
    assert score.metrics()["n_joint"] > 20
    score.close()
    p.close()


# ------------------------------------------------------------------------------------------------ C++ call sites
def test_cpp_adapter_on_the_fixture(built, ctx, tmp_path):
    exe = str(tmp_path / "test_ground_truth")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_ground_truth.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = tmp_path / "cases"
    out.mkdir()
    lines = []
    for name in CASES:
        g = golden_case(name)
        lines.append("%s %d %d" % ((name,) + g["d"].shape))
        g["d"].tofile(str(out / (name + ".d.f32")))
        g["raw"].tofile(str(out / (name + ".raw.u16")))
        np.concatenate([g["Q"].ravel(), g["T"].ravel(), g["K"].ravel()]).astype(np.float64).tofile(str(out / (name + ".calib.f64")))
    (out / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    results = [ln.split() for ln in (out / "results.txt").read_text().splitlines()]
    assert len(results) == 4 * len(CASES)
    for name, tag, inp, n_points, n_outside in results:
        g = golden_case(name)
        depth = np.fromfile(str(out / ("%s.%s.%s.depth.f32" % (name, tag, inp))), F).reshape(g["d"].shape)
        assert np.array_equal(depth, g[tag + "_depth"]), (name, tag, inp)
        assert [int(n_points), int(n_outside)] == [int(v) for v in g[tag + "_counts"]], (name, tag, inp)
