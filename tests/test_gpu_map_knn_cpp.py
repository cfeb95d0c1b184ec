"""dsi::WorldMap::query / knn / pruneOutliers and dsi::knn_threshold (tests/cpp/test_map_knn.cpp) on the sparse scene of
tests/map_knn_reference.py: the files the program dumps equal the restatement, array_equal on the neighbours' rows, the
moments, the threshold, the counts and the pruned map."""
import os
import subprocess

import numpy as np
import pytest

import map_knn_reference as kref
import map_layout_cases as lc
import map_prune_reference as pref
import world_map_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER, K, MIN_FOUND, STD_MULT = (1, 2), 5, 2, 1.0


def test_cpp_map_knn_on_the_sparse_scene(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_knn")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_knn.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    calls, radius = kref.sparse_calls(), kref.SPARSE_RADIUS
    np.asarray([kref.LEAF, len(calls), *FILTER, K, MIN_FOUND, radius, STD_MULT], np.float64).tofile(str(tmp_path / "opts.f64"))
    for k, (pts, _) in enumerate(calls):
        np.asarray(pts, np.float32).tofile(str(tmp_path / ("call_%d.f32" % k)))
    points = kref.sparse_queries()
    points.tofile(str(tmp_path / "points.f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    rm = kref.reference_of(calls, kref.LEAF)
    flt = dict(min_points=FILTER[0], min_windows=FILTER[1])
    got = {"keys": load("query.keys.u64", np.uint64).reshape(-1, K), "dist": load("query.dist.f32", np.float32).reshape(-1, K),
           "found": load("query.found.u8", np.uint8)}
    kref.assert_queries_equal(got, kref.query(rm, points, K, radius, **flt))
    sq = kref.self_query(rm, K, radius, MIN_FOUND, **flt)
    want = rm.prune_outliers(sq, STD_MULT)
    assert want["n_kept"] >= 5 and min(want["n_removed"]) >= 1
    moments = [sq["n_cells"], sq["n_unqueried"], sq["n_scored"], sq["n_isolated"], sq["sum_q"], sq["sum_q2"] & (2 ** 64 - 1), sq["sum_q2"] >> 64,
               sq["reach"], want["T_q"]]
    counts = [want["n_cells"], want["n_kept"]] + want["n_removed"] + [want["T_q"], pref.shrunk_capacity(want["n_kept"])]
    assert lc.grown_from(calls, kref.LEAF, 8) > pref.shrunk_capacity(want["n_kept"])
    assert load("info.u64", np.uint64).tolist() == moments + counts
    assert load("threshold.f64", np.float64).tolist() == [want["mu"], want["sigma"]] * 2
    cells = {"keys": load("cells.keys.u64", np.uint64), "n": load("cells.n.u32", np.uint32), "windows": load("cells.windows.u32", np.uint32),
             "xyz": load("cells.xyz.f32", np.float32).reshape(-1, 3)}
    ref.assert_maps_equal(cells, rm.extract())
