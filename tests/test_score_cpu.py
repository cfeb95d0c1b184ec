"""CPU tests of the depth-map scores: the numpy restatement in tests/score_reference.py against the recorded
output of the reference's own programs (tests/golden/depth_scores.npz, written by tests/golden/make_depth_scores.py), known
answers for the edge rules, nearest_ground_truth and load_depth_points, the exported symbols and their argument checks, the
C++ adapter's call sites, and the resource usage of the new kernels."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import score_reference as sr
from dvs_mcemvs_amd import engine, io as dio, process
from kernel_asm import _hipcc, kernel_asm_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW_SYMBOLS = ("dsi_score_create", "dsi_score_destroy", "dsi_score_reset", "dsi_score_add", "dsi_score_add_dev",
               "dsi_score_add_mapper", "dsi_score_metrics", "dsi_score_median", "dsi_score_histogram")
NEW_KERNELS = ("k_score_accumulate", "k_score_finish", "k_score_minmax", "k_score_histogram", "k_score_select")
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "depth_scores.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]


def golden_case(name):
    g = {k[len(name) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(name + "_")}
    g["b"], g["f"] = float(g["bf"][0]), float(g["bf"][1])
    return g


def fsum_bound(terms):
    """(math.fsum of the terms, 1e-12 * sum |t_i|): the project's figure for a float64 reduction"""
    return math.fsum(terms), 1e-12 * math.fsum(np.abs(terms))


# ------------------------------------------------------------------- the restatement against the reference's programs
def test_fixture_covers_the_cases_it_is_meant_to():
    assert CASES == ["random1", "random3", "ratios", "ties_a", "ties_b"]
    assert GOLDEN["random3_est"].shape == (3, 18, 24) and GOLDEN["random1_est"].shape == (1, 29, 37)
    assert int(GOLDEN["ties_a_counts"][2]) % 2 != int(GOLDEN["ties_b_counts"][2]) % 2       # both parities of n_joint
    for name in ("random1", "random3"):
        g = golden_case(name)
        t = sr.terms(g["est"], g["mask"], g["gt"], g["b"], g["f"])
        assert 2 * int((np.abs(t["di"]) >= 0.01).sum()) >= t["di"].size
    # the tie cases: errors are multiples of 2^-7 that repeat, the smallest and largest of them on the outer edges
    t = sr.terms(*[golden_case("ties_a")[k] for k in ("est", "mask", "gt")], 1.0, 1.0)
    assert np.array_equal(t["err"] * 128, np.round(t["err"] * 128)) and np.unique(t["err"]).size < t["err"].size // 10
    assert t["err"].min() == 0.25 and t["err"].max() == 1.25
    # the ratio case holds ratios of exactly 1.25, 1.25^2, 1.25^3
    t = sr.terms(*[golden_case("ratios")[k] for k in ("est", "mask", "gt")], 1.0, 1.0)
    assert all(int((t["ratio"] == th).sum()) >= 8 for th in sr.THRESHOLDS)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_programs(name):
    g = golden_case(name)
    m = sr.metrics(g["est"], g["mask"], g["gt"], g["b"], g["f"])
    assert [m["n_gt"], m["n_est"], m["n_joint"]] == [int(v) for v in g["counts"]]
    d1, d2, d3, silog, are, lrmse, badp = (float(v) for v in g["printed"])
    assert m["delta"] == [d1, d2, d3] and m["badp"] == badp                   # ratios of exact counts: ==
    assert m["median_abs"] == float(g["median"]) and m["max_gt"] == float(g["max_gt"])
    t = sr.terms(g["est"], g["mask"], g["gt"], g["b"], g["f"])
    for key, term in (("sum_di", "di"), ("sum_di2", "di2"), ("sum_are", "are"), ("sum_abs", "err")):
        exact, bound = fsum_bound(t[term])
        assert abs(m[key] - exact) <= bound, key
    n = m["n_joint"]
    assert abs(m["mean_abs"] - float(g["mean"])) <= 1e-12 * math.fsum(t["err"]) / n
    assert abs(m["silog"] - silog) <= 1e-12 * (m["sum_di2"] / n + (m["sum_di"] / n) ** 2)
    assert abs(m["are"] - are) <= 1e-12 * are and abs(m["lrmse"] - lrmse) <= 1e-12 * lrmse
    c = sr.curves(g["est"], g["mask"], g["gt"])
    for tag, key in (("p", "precision"), ("c", "recall"), ("f", "f1"), ("o", "outliers")):
        assert np.array_equal(c["base"], g[tag + "_x"]), tag
        assert np.array_equal(c[key], g[tag + "_y"], equal_nan=True), key


def test_restated_histogram_is_numpys_bin_for_bin():
    rng = np.random.default_rng(3)
    for n, scale in ((1, 1.0), (2, 0.3), (500, 2.0), (5000, 0.11), (70000, 7.0)):
        err = np.abs(rng.normal(0, scale, n))
        err[rng.integers(0, n, n // 3)] = np.round(err[rng.integers(0, n, n // 3)], 2)       # values on and near bin edges
        nb = int(err.max() / 0.01)
        counts, lo, hi = sr.histogram(err, 0.01)
        if nb < 1:
            assert counts.size == 0
            continue
        want, edges = np.histogram(err, bins=nb)
        assert np.array_equal(counts, want) and np.array_equal(sr.edges(lo, hi, nb), edges)


# --------------------------------------------------------------------------------------------- known answers
def test_validity_rules():
    est = np.array([2.0, 2.0, np.nan, np.inf, 0.0, -1.0, 2.0, 2.0, 2.0, 2.0], F)
    mask = np.array([1, 0, 1, 1, 1, 1, 255, 1, 1, 1], np.uint8)
    gt = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, np.nan, 0.04, 0.05], F)
    ev, gv = sr.validity(est, mask, gt)
    assert list(ev) == [True, False, False, False, False, False, True, True, True, True]
    # float32(0.05) is a little above the double 0.05: valid; a non-finite ground truth is invalid, not poison
    assert list(gv) == [True] * 7 + [False, False, True]
    m = sr.metrics(est, mask, gt, 0.6, 500.0)
    assert (m["n_est"], m["n_gt"], m["n_joint"]) == (5, 8, 3) and m["max_gt"] == 2.0
    assert np.isfinite(m["sum_di"]) and np.isfinite(m["mean_abs"])


def test_thresholds_are_strict_and_badp_needs_both():
    g = np.array([4.0, 4.0, 4.0, 4.0], F)
    est = np.array([5.0, 6.25, 7.8125, 2.0], F)                     # ratios 1.25, 1.5625, 1.953125 exactly, and 2 the other way
    m = sr.metrics(est, np.ones(4, np.uint8), g, 0.6, 500.0)
    assert m["n_delta"] == [0, 1, 2] and m["delta"] == [0.0, 0.25, 0.5]
    # e = |1/d - 1/g| b f, r = e g / b / f: d = 1, g = 1.04 -> e = 11.5 > 5 but r = 0.04 -> not bad; g = 1.2 -> bad;
    # d = 50, g = 100 -> r = 1 but e = 3 -> not bad
    m = sr.metrics(np.array([1.0, 1.0, 50.0], F), np.ones(3, np.uint8), np.array([1.04, 1.2, 100.0], F), 0.6, 500.0)
    assert m["n_bad"] == 1 and m["badp"] == 1 / 3


def test_empty_and_tiny_scores():
    m = sr.metrics(np.zeros((2, 3), F), np.zeros((2, 3), np.uint8), np.ones((2, 3), F), 0.6, 500.0)
    assert (m["n_est"], m["n_gt"], m["n_joint"]) == (0, 6, 0) and m["max_gt"] == 1.0
    assert all(math.isnan(m[k]) for k in ("silog", "are", "lrmse", "badp", "mean_abs", "median_abs")) and math.isnan(m["delta"][0])
    assert sr.histogram(np.zeros(0))[0].size == 0
    assert sr.median(np.array([3.0])) == 3.0 and sr.median(np.array([3.0, 1.0])) == 2.0
    assert sr.median(np.array([1.0, 7.0, 2.0, 4.0])) == 3.0


def test_histogram_edge_rules():
    # all errors equal: the range is widened by 0.5 either way and every error lands in the middle bin
    counts, lo, hi = sr.histogram(np.full(5, 0.25), 0.01)
    assert (lo, hi, counts.size) == (-0.25, 0.75, 25) and counts[12] == 5 and counts.sum() == 5
    # fewer than one bin: numpy raises, the score answers with no bins
    assert sr.histogram(np.array([0.001, 0.009]), 0.01)[0].size == 0
    # the maximum belongs to the last bin (closed on the right), the minimum to the first
    err = np.array([0.5, 1.0, 1.5, 1.5])
    counts, lo, hi = sr.histogram(err, 0.5)
    assert counts.tolist() == [1, 1, 2] and (lo, hi) == (0.5, 1.5)
    want, _ = np.histogram(err, bins=3)
    assert np.array_equal(counts, want)


def test_nearest_ground_truth():
    times = np.array([0.0, 0.1, 0.2, 0.45])
    assert process.nearest_ground_truth(times, 0.12) == 1
    assert process.nearest_ground_truth(times, 0.15) in (1, 2)
    assert process.nearest_ground_truth(times, 0.25) == 2
    assert process.nearest_ground_truth(times, 0.325) is None                 # 0.125 from both neighbours: skipped
    assert process.nearest_ground_truth(times, 0.55) is None                  # dt >= 0.1 is skipped, as in the script
    assert process.nearest_ground_truth(times, 0.549) == 3
    assert process.nearest_ground_truth(times, 0.5, max_dt=0.01) is None
    assert process.nearest_ground_truth([], 0.5) is None


def test_load_depth_points_round_trip(tmp_path):
    rng = np.random.default_rng(8)
    depth = rng.uniform(1, 60, (7, 9)).astype(F)
    mask = (rng.random((7, 9)) < 0.4).astype(np.uint8)
    depth[2, 3], mask[2, 3] = 255.0, 1                                       # the script reads exactly 255 as "no estimate"
    p = str(tmp_path / "depth_points_fused_2.txt")
    n = dio.save_depth_points(p, depth, mask)
    got, gmask = dio.load_depth_points(p, 7, 9)
    want_mask = mask.copy()
    want_mask[2, 3] = 0
    assert n == int(mask.sum()) and np.array_equal(gmask, want_mask) and got.dtype == F
    want = np.array([float("%g" % v) for v in depth.ravel()], F).reshape(7, 9)   # the file holds six significant digits
    assert np.array_equal(got[gmask > 0], want[gmask > 0]) and not got[gmask == 0].any()
    open(p, "w").close()
    got, gmask = dio.load_depth_points(p, 7, 9)
    assert not gmask.any() and got.shape == (7, 9)
    with open(p, "w") as f:
        f.write("9 0 2.5\n")
    with pytest.raises(ValueError):
        dio.load_depth_points(p, 7, 9)


# ------------------------------------------------------------------------------------------- the built library
def test_new_symbols_are_exported_declared_and_bound(built):
    L = d.load_library()
    header = open(os.path.join(ROOT, "include", "dsi_engine.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"DSI_API int %s\(" % name, header), name
    assert L.dsi_abi_version() == 10
    assert hasattr(d, "DepthScore") and "DepthScore" in d.__all__
    for name in ("add", "addMapper", "metrics", "curves", "reset", "median", "histogram"):
        assert hasattr(d.DepthScore, name)
    assert hasattr(process, "nearest_ground_truth") and hasattr(dio, "load_depth_points")
    assert ctypes.sizeof(engine._ScoreMetrics) == 8 * 8 + 8 + 5 * 8 + 9 * 8


def test_new_entry_points_validate_arguments_without_gpu(built):
    L = d.load_library()
    h = ctypes.c_void_p()
    fake = ctypes.c_void_p(0x1000)                                            # never dereferenced: the checks come first
    f32 = (ctypes.c_float * 4)()
    u8 = (ctypes.c_uint8 * 4)()
    assert L.dsi_score_create(None, 16, 0.6, 500.0, 0.05, ctypes.byref(h)) == engine.ERR_INVALID
    assert b"null" in L.dsi_last_error()
    assert L.dsi_score_create(fake, 16, 0.6, 500.0, 0.05, None) == engine.ERR_INVALID
    for cap, b, f, gt_min in ((0, 0.6, 500.0, 0.05), (16, 0.0, 500.0, 0.05), (16, -0.6, 500.0, 0.05), (16, 0.6, 0.0, 0.05),
                              (16, 0.6, math.nan, 0.05), (16, math.inf, 500.0, 0.05), (16, 0.6, 500.0, 0.0),
                              (16, 0.6, 500.0, -1.0), (16, 0.6, 500.0, math.nan)):
        assert L.dsi_score_create(fake, cap, b, f, gt_min, ctypes.byref(h)) == engine.ERR_INVALID, (cap, b, f, gt_min)
        assert not h.value
    assert L.dsi_score_add(None, f32, u8, f32, 4) == engine.ERR_INVALID
    assert L.dsi_score_add(fake, None, u8, f32, 4) == engine.ERR_INVALID
    assert L.dsi_score_add(fake, f32, None, f32, 4) == engine.ERR_INVALID
    assert L.dsi_score_add(fake, f32, u8, None, 4) == engine.ERR_INVALID
    assert L.dsi_score_add(fake, f32, u8, f32, 0) == engine.ERR_INVALID
    assert L.dsi_score_add_dev(None, fake, fake, fake, 4) == engine.ERR_INVALID
    assert L.dsi_score_add_dev(fake, fake, fake, fake, 0) == engine.ERR_INVALID
    assert L.dsi_score_add_mapper(None, fake, f32) == engine.ERR_INVALID
    assert L.dsi_score_add_mapper(fake, None, f32) == engine.ERR_INVALID
    assert L.dsi_score_add_mapper(fake, fake, None) == engine.ERR_INVALID
    assert L.dsi_score_metrics(None, None) == engine.ERR_INVALID
    assert L.dsi_score_metrics(fake, None) == engine.ERR_INVALID
    assert L.dsi_score_median(fake, None) == engine.ERR_INVALID
    n, lo, hi = ctypes.c_size_t(), ctypes.c_double(), ctypes.c_double()
    assert L.dsi_score_histogram(None, 0.01, None, 0, ctypes.byref(n), ctypes.byref(lo), ctypes.byref(hi)) == engine.ERR_INVALID
    assert L.dsi_score_histogram(fake, 0.01, None, 0, None, ctypes.byref(lo), ctypes.byref(hi)) == engine.ERR_INVALID
    for bw in (0.0, -0.01, math.nan, math.inf):
        assert L.dsi_score_histogram(fake, bw, None, 0, ctypes.byref(n), ctypes.byref(lo), ctypes.byref(hi)) == engine.ERR_INVALID
    assert b"binwidth" in L.dsi_last_error()
    assert L.dsi_score_reset(None) == engine.ERR_INVALID
    assert L.dsi_score_destroy(None) == engine.OK                            # like the other destroy calls
    with pytest.raises(ValueError):
        process.full_sequence(None, None, None, None, None, 0, 1, 0.1, 0.1, score=object()).__next__()
    with pytest.raises(ValueError):
        process.full_sequence(None, None, None, None, None, 0, 1, 0.1, 0.1, score=object(), ground_truth=lambda t: None).__next__()


def test_cpp_call_sites_compile_and_refuse_without_gpu(built, tmp_path):
    exe = str(tmp_path / "test_score")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "test_score.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    if d.device_count() == 0:   # (with a GPU, tests/test_gpu_score.py runs the program)
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no HIP device" in (r.stdout + r.stderr)


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not available")
def test_score_kernels_use_no_scratch():
    text = kernel_asm_text()
    seen = set()
    for block in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if not any(k in name for k in NEW_KERNELS):
            continue
        seen.add(name)
        val = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        assert val("private_segment_fixed_size") == 0 and val("vgpr_spill_count") == 0 and val("sgpr_spill_count") == 0, name
        assert val("vgpr_count") <= 64 and val("wavefront_size") == 64, name
    # accumulate, finish, minmax, both histogram instances, select and its pick
    assert len(seen) == 7, seen
    # the sums are reduced without floating-point atomics; the cursor and the counts are integer atomics
    m = re.search(r"^(_ZN\w*k_score_accumulate\w*):.*?$(.*?)s_endpgm", text, re.S | re.M)
    assert m, "k_score_accumulate not found"
    body = m.group(2)
    assert "global_atomic_add_x2" in body and not re.search(r"atomic_\w*(f64|f32)", body)
