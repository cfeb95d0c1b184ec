"""GPU tests of the depth-map scores: dsi_score_* against the recorded output of the reference's own programs
(tests/golden/depth_scores.npz) and against the numpy restatement (tests/score_reference.py) on the shapes that take the
kernels' different paths.  Counts, ratios of counts, the largest ground-truth depth, the median and the four curves are
compared with ==; the float64 sums with math.fsum of the restatement's terms, within 1e-12 * sum |t_i| (DESIGN 1, row A13:
the fixed-order summation takes about 2e-15 of that at these sizes, the rest allows the device's log a few ulp per term)."""
import math
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import score_reference as sr
from dvs_mcemvs_amd import engine, process as proc, synthetic as syn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
B, FOCAL = 0.6, 557.25
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "depth_scores.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
REALS = ("sum_di", "sum_di2", "sum_are", "sum_abs", "max_gt", "silog", "are", "lrmse", "badp", "mean_abs", "median_abs")


def golden_case(name):
    g = {k[len(name) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "_")}
    g["b"], g["f"] = float(g["bf"][0]), float(g["bf"][1])
    return g


def code_of(fn):
    try:
        fn()
    except d.DsiError as e:
        return e.code
    return engine.OK


def bits(m):
    """every double of a metrics dict, as bytes (NaN-safe equality)"""
    return np.array([m[k] for k in REALS] + list(m["delta"]), np.float64).tobytes()


def random_maps(seed, shape, p_est=0.3, p_gt=0.7):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(1.0, 4.0, shape).astype(F)
    est = (gt.astype(np.float64) * np.exp(rng.normal(0.0, 0.15, shape))).astype(F)
    mask = (rng.random(shape) < p_est).astype(np.uint8)
    gt[rng.random(shape) >= p_gt] = 0.0
    return est, mask, gt


def check_against_restatement(m, est, mask, gt, b, f, printed=None):
    """m: DepthScore.metrics() of these maps.  printed: the reference's (silog, are, lrmse) where they were recorded."""
    ref = sr.metrics(est, mask, gt, b, f)
    t = sr.terms(est, mask, gt, b, f)
    for k in ("n_est", "n_gt", "n_joint", "n_delta", "n_bad"):
        assert m[k] == ref[k], k
    assert m["n_stored"] == ref["n_joint"] and not m["overflow"] and m["guard_intact"]
    n = ref["n_joint"]
    if ref["n_gt"]:
        assert m["max_gt"] == ref["max_gt"]
    else:
        assert math.isnan(m["max_gt"])
    if n == 0:
        assert all(math.isnan(m[k]) for k in ("silog", "are", "lrmse", "badp", "mean_abs", "median_abs"))
        assert all(math.isnan(v) for v in m["delta"])
        assert m["sum_di"] == m["sum_di2"] == m["sum_are"] == m["sum_abs"] == 0.0
        return ref
    assert m["delta"] == ref["delta"] and m["badp"] == ref["badp"] and m["median_abs"] == ref["median_abs"]
    exact = {}
    for key, term in (("sum_di", "di"), ("sum_di2", "di2"), ("sum_are", "are"), ("sum_abs", "err")):
        exact[key], bound = math.fsum(t[term]), 1e-12 * math.fsum(np.abs(t[term]))
        print("%s: got %.17g exact %.17g |diff| %.3g bound %.3g" % (key, m[key], exact[key], abs(m[key] - exact[key]), bound))
        assert abs(m[key] - exact[key]) <= bound, key
    assert abs(m["mean_abs"] - exact["sum_abs"] / n) <= 1e-12 * exact["sum_abs"] / n
    assert abs(m["are"] - exact["sum_are"] / n) <= 1e-12 * exact["sum_are"] / n
    silog = printed[0] if printed is not None else exact["sum_di2"] / n - (exact["sum_di"] / n) ** 2
    lrmse = printed[2] if printed is not None else math.sqrt(exact["sum_di2"] / n)
    sbound = 1e-12 * (exact["sum_di2"] / n + (exact["sum_di"] / n) ** 2)
    print("silog: got %.17g want %.17g |diff| %.3g bound %.3g" % (m["silog"], silog, abs(m["silog"] - silog), sbound))
    assert abs(m["silog"] - silog) <= sbound
    assert abs(m["lrmse"] - lrmse) <= 1e-12 * lrmse
    if printed is not None:
        assert abs(m["are"] - printed[1]) <= 1e-12 * printed[1]
    return ref


def check_curves(c, want):
    for k in ("base", "precision", "recall", "f1", "outliers"):
        assert np.array_equal(c[k], want[k], equal_nan=True), k


# ------------------------------------------------------------------------------- the reference's own programs
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("by_window", (False, True))
def test_fixture_case(ctx, name, by_window):
    g = golden_case(name)
    est, mask, gt = g["est"], g["mask"], g["gt"]
    s = d.DepthScore(ctx, est.size, g["b"], g["f"])
    if by_window:
        for w in range(est.shape[0]):
            s.add(est[w], mask[w], gt[w])
    else:
        s.add(est, mask, gt)
    m = s.metrics()
    assert [m["n_gt"], m["n_est"], m["n_joint"]] == [int(v) for v in g["counts"]]
    d1, d2, d3, silog, are, lrmse, badp = (float(v) for v in g["printed"])
    assert m["delta"] == [d1, d2, d3] and m["badp"] == badp
    assert m["max_gt"] == float(g["max_gt"]) and m["median_abs"] == float(g["median"]) == s.median()
    check_against_restatement(m, est, mask, gt, g["b"], g["f"], printed=(silog, are, lrmse))
    assert abs(m["mean_abs"] - float(g["mean"])) <= 1e-12 * float(g["mean"])
    c = s.curves()
    for tag, key in (("p", "precision"), ("c", "recall"), ("f", "f1"), ("o", "outliers")):
        assert np.array_equal(c["base"], g[tag + "_x"]), tag
        assert np.array_equal(c[key], g[tag + "_y"], equal_nan=True), key
    s.close()


# ---------------------------------------------------------------------------------------------------- shapes
def test_single_pixel_and_nothing_valid(ctx):
    s = d.DepthScore(ctx, 8, B, FOCAL)
    s.add(np.array([[2.0]], F), np.array([[1]], np.uint8), np.array([[2.5]], F))            # 1 x 1, valid
    m = s.metrics()
    check_against_restatement(m, [[2.0]], [[1]], [[2.5]], B, FOCAL)
    assert m["n_joint"] == 1 and m["median_abs"] == 0.5 and m["mean_abs"] == 0.5
    counts, lo, hi = s.histogram(0.01)
    assert (lo, hi) == (0.0, 1.0) and counts.size == 50 and counts[25] == 1 and counts.sum() == 1   # min == max: -+0.5
    assert s.histogram(1.0)[0].size == 0                                                    # int(0.5 / 1.0) = 0 bins
    s.reset()
    for est, mask, gt in (([[2.0]], [[0]], [[2.5]]), ([[np.nan]], [[1]], [[2.5]]), ([[2.0]], [[1]], [[0.01]]),
                          ([[2.0]], [[1]], [[np.inf]]), ([[-2.0]], [[1]], [[2.5]])):       # 1 x 1, invalid
        s.reset()
        s.add(np.array(est, F), np.array(mask, np.uint8), np.array(gt, F))
        m = s.metrics()
        check_against_restatement(m, est, mask, gt, B, FOCAL)
        assert m["n_joint"] == 0 and s.histogram()[0].size == 0 and math.isnan(s.median())
        assert all(v.size == 0 for v in s.curves().values())
    s.reset()
    est, _, gt = random_maps(1, (13, 17))
    s.add(est, np.zeros((13, 17), np.uint8), gt)                                            # everything masked
    m = s.metrics()
    check_against_restatement(m, est, np.zeros((13, 17), np.uint8), gt, B, FOCAL)
    assert m["n_est"] == 0 and m["n_gt"] > 0 and m["n_joint"] == 0
    s.close()


@pytest.mark.parametrize("n_joint", (1, 2))
def test_one_and_two_joint_pixels(ctx, n_joint):
    est, _, gt = random_maps(2, (9, 11), p_gt=1.0)
    mask = np.zeros((9, 11), np.uint8)
    mask.flat[[40, 7][:n_joint]] = 1
    s = d.DepthScore(ctx, 4, B, FOCAL)
    s.add(est, mask, gt)
    m = s.metrics()
    ref = check_against_restatement(m, est, mask, gt, B, FOCAL)
    assert ref["n_joint"] == n_joint
    check_curves(s.curves(0.001), sr.curves(est, mask, gt, binwidth=0.001))
    s.close()


@pytest.mark.parametrize("shape", ((37, 29), (260, 346)))
def test_odd_shape_and_several_blocks(ctx, shape):
    """37 x 29 is no multiple of a wave; 260 x 346 takes 352 blocks, so several partials per lane of the finish kernel"""
    est, mask, gt = random_maps(3, shape)
    s = d.DepthScore(ctx, est.size, B, FOCAL)
    s.add(est, mask, gt)
    check_against_restatement(s.metrics(), est, mask, gt, B, FOCAL)
    check_curves(s.curves(), sr.curves(est, mask, gt))
    s.close()


def test_three_adds_of_different_sizes(ctx):
    parts = [random_maps(10 + i, shape) for i, shape in enumerate(((5, 7), (64, 64), (131, 97)))]
    est, mask, gt = (np.concatenate([p[k].ravel() for p in parts]) for k in range(3))
    s = d.DepthScore(ctx, est.size, B, FOCAL)
    for p in parts:
        s.add(*p)
    check_against_restatement(s.metrics(), est, mask, gt, B, FOCAL)
    check_curves(s.curves(), sr.curves(est, mask, gt))
    s.close()


def test_histogram_in_lds_and_in_global_memory(ctx):
    """8192 bins are the most the LDS counters hold: one bin fewer and more than that, and 20 times as many"""
    est, mask, gt = random_maps(4, (120, 90))
    err = sr.terms(est, mask, gt, B, FOCAL)["err"]
    s = d.DepthScore(ctx, est.size, B, FOCAL)
    s.add(est, mask, gt)
    for nb in (8191, 8192, 8193, 163840):
        bw = float(err.max()) / (nb + 0.5)
        assert int(err.max() / bw) == nb
        counts, lo, hi = s.histogram(bw)
        want, wlo, whi = sr.histogram(err, bw)
        assert counts.size == nb and (lo, hi) == (wlo, whi) and np.array_equal(counts, want), nb
        assert np.array_equal(counts, np.histogram(err, bins=nb)[0])
    s.close()


def test_same_adds_after_reset_give_the_same_bits(ctx):
    parts = [random_maps(20 + i, shape) for i, shape in enumerate(((260, 346), (37, 29), (100, 100)))]
    s = d.DepthScore(ctx, sum(p[0].size for p in parts), B, FOCAL)
    runs = []
    for _ in range(2):
        s.reset()
        for p in parts:
            s.add(*p)
        m = s.metrics()
        c = s.curves()
        runs.append((bits(m), {k: v for k, v in m.items() if k not in REALS and k != "delta"},
                     b"".join(c[k].tobytes() for k in sorted(c))))
    assert runs[0] == runs[1]
    assert np.isfinite(np.frombuffer(runs[0][0], np.float64)).all()
    s.close()


def test_overflow_keeps_counts_refuses_median_and_stays_in_bounds(ctx):
    est, mask, gt = random_maps(5, (50, 70))
    ref = sr.metrics(est, mask, gt, B, FOCAL)
    assert ref["n_joint"] > 100
    s = d.DepthScore(ctx, ref["n_joint"] - 1, B, FOCAL)                                    # one short
    s.add(est, mask, gt)
    m = s.metrics()
    assert m["overflow"] and m["n_stored"] == ref["n_joint"] - 1 and m["guard_intact"]
    for k in ("n_est", "n_gt", "n_joint", "n_delta", "n_bad"):
        assert m[k] == ref[k], k
    assert m["delta"] == ref["delta"] and m["badp"] == ref["badp"] and m["max_gt"] == ref["max_gt"]
    assert abs(m["sum_abs"] - ref["sum_abs"]) <= 1e-12 * ref["sum_abs"] and math.isnan(m["median_abs"])
    assert code_of(s.median) == engine.ERR_INVALID
    assert b"overflow" in d.load_library().dsi_last_error()
    assert code_of(s.histogram) == engine.ERR_INVALID and code_of(s.curves) == engine.ERR_INVALID
    s.reset()                                                                               # and the object recovers
    s.add(est[:10], mask[:10], gt[:10])
    check_against_restatement(s.metrics(), est[:10], mask[:10], gt[:10], B, FOCAL)
    s.close()
    s = d.DepthScore(ctx, ref["n_joint"], B, FOCAL)                                        # exactly enough
    s.add(est, mask, gt)
    m = s.metrics()
    assert not m["overflow"] and m["median_abs"] == ref["median_abs"] and m["guard_intact"]
    s.close()


def test_error_returns_with_a_context(ctx):
    L = d.load_library()
    s = d.DepthScore(ctx, 16, B, FOCAL)
    with pytest.raises(ValueError):
        s.add(np.ones((2, 2), F), np.ones((2, 3), np.uint8), np.ones((2, 2), F))
    s.add(np.array([1.0, 2.0, 4.0], F), np.ones(3, np.uint8), np.array([1.5, 2.0, 5.0], F))
    n, lo, hi = (engine.C.c_size_t(), engine.C.c_double(), engine.C.c_double())
    counts = np.zeros(4, np.uint64)
    rc = L.dsi_score_histogram(s._h, 0.01, engine._ptr(counts, engine.C.c_uint64), 4, engine.C.byref(n), engine.C.byref(lo),
                               engine.C.byref(hi))
    assert rc == engine.ERR_INVALID and n.value == 100                                      # too small: the size is reported
    assert code_of(lambda: s.histogram(1e-9)) == engine.ERR_INVALID                         # more than 2^24 bins
    assert L.dsi_context_destroy(ctx._h) == engine.ERR_CONTEXT                              # a live score keeps its context
    s.close()
    assert code_of(lambda: d.DepthScore(ctx, 0, B, FOCAL)) == engine.ERR_INVALID
    assert code_of(lambda: d.DepthScore(ctx, 16, B, FOCAL, gt_min=0.0)) == engine.ERR_INVALID


# ------------------------------------------------------------------------------------- maps still on the device
def test_add_mapper_equals_add_of_the_fetched_maps(ctx):
    rig = syn.stereo_rig(60000, width=120, height=90, duration=0.3, seed=5)
    m = d.MapperEMVS(ctx, rig["cam"], d.ShapeDSI(0, 0, 40, 4.0, 200.0, 0.0))
    gt_shape = (m.dimY, m.dimX)
    rng = np.random.default_rng(6)
    a, b = d.DepthScore(ctx, m.dimY * m.dimX, B, FOCAL), d.DepthScore(ctx, m.dimY * m.dimX, B, FOCAL)
    assert code_of(lambda: a.addMapper(m, np.ones(gt_shape, F))) == engine.ERR_INVALID     # nothing computed yet
    assert m.evaluateDSI(rig["events"][0], rig["trajectories"][0], rig["T_rv_w"])
    depth, conf, mask = m.getDepthMapFromDSI(options_depth_map=d.OptionsDepthMap(5, 4.0, 5, 0.0))
    assert 0 < (mask > 0).sum() < mask.size
    gt = (np.where(mask > 0, depth, 10.0) * np.exp(rng.normal(0, 0.2, gt_shape))).astype(F)
    gt[rng.random(gt_shape) < 0.3] = 0.0
    a.addMapper(m, gt)
    b.add(depth, mask, gt)
    ma, mb = a.metrics(), b.metrics()
    assert ma["n_joint"] > 50 and bits(ma) == bits(mb)
    assert {k: v for k, v in ma.items() if k not in REALS and k != "delta"} == {k: v for k, v in mb.items() if k not in REALS and k != "delta"}
    check_against_restatement(ma, depth, mask, gt, B, FOCAL)
    check_curves(a.curves(), b.curves())
    check_curves(a.curves(), sr.curves(depth, mask, gt))
    with pytest.raises(ValueError):
        a.addMapper(m, gt[:-1])
    other = d.Context(0)
    c = d.DepthScore(other, 16, B, FOCAL)
    assert code_of(lambda: c.addMapper(m, gt)) == engine.ERR_CONTEXT
    c.close()
    other.close()
    m.computeDepthMap()                                                                     # a new raw map invalidates them
    assert code_of(lambda: a.addMapper(m, gt)) == engine.ERR_INVALID
    for o in (a, b, m):
        o.close()


def test_full_sequence_scores_every_window(ctx):
    rig = syn.stereo_rig(60_000, width=96, height=72, t0=3.0, duration=0.6, seed=5)
    shape = d.ShapeDSI(0, 0, 24, 4.0, 100.0, 0.0)
    cams = (rig["cam"],) * 2
    opts = d.OptionsDepthMap(5, 4.0, 5, 0.0)
    args = (ctx, cams, shape, rig["events"], rig["trajectories"], 3.0, 3.6, 0.3, 0.3)
    plain = list(proc.full_sequence(*args, options_depth_map=opts))
    assert len(plain) == 2
    rng = np.random.default_rng(7)
    gts = {w[0]: (np.where(w[3] > 0, w[1], 20.0) * np.exp(rng.normal(0, 0.2, w[1].shape))).astype(F) for w in plain}
    skipped = plain[1][0]
    score = d.DepthScore(ctx, 2 * plain[0][1].size, B, FOCAL)
    asked = []

    def ground_truth(ts):
        asked.append(ts)
        return None if ts == skipped else gts[ts]

    scored = list(proc.full_sequence(*args, options_depth_map=opts, score=score, ground_truth=ground_truth))
    assert asked == [w[0] for w in plain] and len(scored) == 2
    for w, p in zip(scored, plain):
        assert len(w) == len(p) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(w[1:], p[1:]))
    m = score.metrics()
    ts, depth, conf, mask = plain[0]
    assert m["n_joint"] > 20
    check_against_restatement(m, depth, mask, gts[ts], B, FOCAL)                            # the second window had no ground truth
    score.close()
    with pytest.raises(ValueError):
        next(proc.full_sequence(*args, score=score, ground_truth=ground_truth))             # no filtered maps


# ------------------------------------------------------------------------------------------------ C++ call sites
def test_cpp_adapter_on_the_fixture(built, ctx, tmp_path):
    exe = str(tmp_path / "test_score")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_score.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    g = golden_case("random3")
    out = tmp_path / "case"
    out.mkdir()
    (out / "case.txt").write_text("%d %d %d %r %r\n" % (g["est"].shape + (g["b"], g["f"])))
    g["est"].tofile(str(out / "est.f32"))
    g["mask"].tofile(str(out / "mask.u8"))
    g["gt"].tofile(str(out / "gt.f32"))
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    vals = dict(line.split() for line in (out / "metrics.txt").read_text().splitlines())
    m = {k: int(vals[k]) for k in ("n_est", "n_gt", "n_joint", "n_bad", "n_stored")}
    m["n_delta"] = [int(vals["n_delta%d" % k]) for k in range(3)]
    m["overflow"], m["guard_intact"] = bool(int(vals["overflow"])), bool(int(vals["guard_intact"]))
    for k in REALS:
        m[k] = float.fromhex(vals[k])
    m["delta"] = [float.fromhex(vals["delta%d" % k]) for k in range(3)]
    d1, d2, d3, silog, are, lrmse, badp = (float(v) for v in g["printed"])
    assert m["delta"] == [d1, d2, d3] and m["badp"] == badp and m["median_abs"] == float(g["median"])
    check_against_restatement(m, g["est"], g["mask"], g["gt"], g["b"], g["f"], printed=(silog, are, lrmse))
    nb = int(vals["n_bins"])
    curves = np.fromfile(str(out / "curves.f64"), np.float64).reshape(5, nb)
    for row, tag in zip(curves[1:], "pcfo"):
        assert np.array_equal(curves[0], g[tag + "_x"]) and np.array_equal(row, g[tag + "_y"], equal_nan=True), tag
    # and the same object through Python gives the same bits
    s = d.DepthScore(ctx, g["est"].size, g["b"], g["f"])
    for w in range(g["est"].shape[0]):
        s.add(g["est"][w], g["mask"][w], g["gt"][w])
    assert bits(s.metrics()) == bits(m)
    s.close()
