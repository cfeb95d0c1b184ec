"""dsi::WorldMap::observe / fetchVisibility / selectCarved / pruneCarved (tests/cpp/test_map_visibility.cpp) on the scene of
tests/map_pca_reference.py with the three views of tests/map_visibility_reference.py: the files the program dumps equal the
Python rows and the restatement, array_equal on the rows, the counts and the pruned map."""
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_pca_reference as pr
import map_prune_reference as pref
import map_visibility_reference as vr
import world_map_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_THROUGH, AGREE_WEIGHT = 1, 1


def test_cpp_map_visibility_on_the_scene(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_visibility")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_visibility.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    calls, views = pr.scene_calls(), vr.scene_views(0)
    np.asarray([pr.LEAF, len(calls), len(views), MIN_THROUGH, AGREE_WEIGHT], np.float64).tofile(str(tmp_path / "opts.f64"))
    for k, (pts, _) in enumerate(calls):
        np.asarray(pts, np.float32).tofile(str(tmp_path / ("call_%d.f32" % k)))
    for k, (depth, mask, K, lo, hi, T, window, abs_tol, rel_tol) in enumerate(views):
        stem = str(tmp_path / ("view_%d" % k))
        np.asarray([depth.shape[1], depth.shape[0], window, *K, lo, hi, abs_tol, rel_tol, *T], np.float64).tofile(stem + ".obs.f64")
        np.asarray(depth, np.float32).tofile(stem + ".depth.f32")
        (np.zeros(0, np.uint8) if mask is None else np.asarray(mask, np.uint8)).tofile(stem + ".mask.u8")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    got = {"keys": load("rows.keys.u64", np.uint64), "seen": load("rows.seen.u32", np.uint32), "agree": load("rows.agree.u32", np.uint32),
           "through": load("rows.through.u32", np.uint32), "reason": load("rows.reason.u8", np.uint8)}
    # the Python rows of the same observations
    wm = d.WorldMap(ctx, pr.LEAF, 8)
    for pts, T in calls:
        wm.integrate(pts, T)
    py_counts = [wm.observe(*v) for v in views]
    py_select = wm.selectCarved(MIN_THROUGH, AGREE_WEIGHT, shrink=True)
    py = wm.fetchVisibility(sort=True)
    assert set(py) == set(got)
    for f in got:
        assert py[f].dtype == got[f].dtype and np.array_equal(py[f], got[f]), f
    wm.close()
    # and the restatement
    rm = vr.reference_of(calls, pr.LEAF)
    tally, want_counts = vr.tally_of(rm, views)
    info = load("info.u64", np.uint64).tolist()
    names = ("n_cells", "n_clipped", "n_outside", "n_unseen", "n_agree", "n_through", "n_behind", "n_valid_pixels", "views")
    for k, (mine, want) in enumerate(zip(py_counts, want_counts)):
        counts = dict(zip(names, info[9 * k:9 * k + 9]))
        assert counts == mine
        vr.assert_counts_equal(counts, want)
    vr.assert_rows_equal(got, tally.rows())
    sel = tally.select(MIN_THROUGH, AGREE_WEIGHT)
    assert np.array_equal(got["reason"], sel["reason"]) and sel["n_removed"] >= 100
    pruned = tally.prune(rm, MIN_THROUGH, AGREE_WEIGHT)
    grown = py_select["capacity"]
    assert info[27:31] == [sel["n_cells"], sel["n_kept"], sel["n_removed"], grown] == [py_select[f] for f in ("n_cells", "n_kept", "n_removed", "capacity")]
    assert info[31:] == [pruned["n_cells"], pruned["n_kept"], pruned["n_removed"], pref.shrunk_capacity(pruned["n_kept"])]
    cells = {"keys": load("cells.keys.u64", np.uint64), "n": load("cells.n.u32", np.uint32), "windows": load("cells.windows.u32", np.uint32),
             "xyz": load("cells.xyz.f32", np.float32).reshape(-1, 3)}
    ref.assert_maps_equal(cells, rm.extract())
