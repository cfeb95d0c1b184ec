"""dsi::WorldMap::pca / fetchPca / pruneShapes and dsi::pca_solve (tests/cpp/test_map_pca.cpp) on the scene of
tests/map_pca_reference.py at one setting: the files the program dumps equal the Python rows and the restatement, array_equal
on the rows, the moments, the counts and the pruned map."""
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_layout_cases as lc
import map_pca_reference as pr
import map_prune_reference as pref
import world_map_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER, K, MIN_FOUND, RADIUS, KEEP = (1, 2), 5, 3, 0.1, 3


def test_cpp_map_pca_on_the_scene(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_pca")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_pca.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    calls = pr.scene_calls()
    np.asarray([pr.LEAF, len(calls), *FILTER, K, MIN_FOUND, RADIUS, *pr.VIEWPOINT, KEEP], np.float64).tofile(str(tmp_path / "opts.f64"))
    for k, (pts, _) in enumerate(calls):
        np.asarray(pts, np.float32).tofile(str(tmp_path / ("call_%d.f32" % k)))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    got = {"keys": load("rows.keys.u64", np.uint64), "normal": load("rows.normal.f32", np.float32).reshape(-1, 3),
           "tangent": load("rows.tangent.f32", np.float32).reshape(-1, 3), "eval": load("rows.eval.f32", np.float32).reshape(-1, 3),
           "members": load("rows.members.u16", np.uint16), "label": load("rows.label.u8", np.uint8), "flags": load("rows.flags.u8", np.uint8),
           "moments": load("rows.moments.i64", np.int64).reshape(-1, 9)}
    flt = dict(min_points=FILTER[0], min_windows=FILTER[1])
    # the Python rows of the same pass; two tables hold their cells in slots of their own, so both are put in key order
    wm = d.WorldMap(ctx, pr.LEAF, 8)
    for pts, T in calls:
        wm.integrate(pts, T)
    py_info = wm.pca(K, RADIUS, MIN_FOUND, True, pr.VIEWPOINT, keep_moments=True, **flt)
    py = wm.fetchPca(sort=True)
    order = np.argsort(got["keys"], kind="stable")
    got = {f: v[order] for f, v in got.items()}
    assert set(py) == set(got)
    for f in got:
        assert py[f].dtype == got[f].dtype and np.array_equal(py[f].view(np.uint8), got[f].view(np.uint8)), f
    wm.close()
    # and the restatement
    rm = pr.reference_of(calls, pr.LEAF)
    want = pr.shape_pass(rm, K, RADIUS, MIN_FOUND, True, pr.VIEWPOINT, **flt)
    info = load("info.u64", np.uint64).tolist()
    counts = {"n_cells": info[0], "n_unqueried": info[1], "n_sparse": info[2], "n_label": info[3:6], "n_normal_determined": info[6],
              "n_tangent_determined": info[7], "sum_members": info[8], "reach": info[9]}
    assert counts == py_info
    pr.assert_passes_equal(counts, got, want)
    pruned = rm.prune_shapes(want, KEEP, True)
    assert pruned["n_kept"] >= 100 and min(pruned["n_removed"]) >= 5
    assert lc.grown_from(calls, pr.LEAF, 8) > pref.shrunk_capacity(pruned["n_kept"])
    assert info[10:] == [pruned["n_cells"], pruned["n_kept"]] + pruned["n_removed"] + [pref.shrunk_capacity(pruned["n_kept"])]
    cells = {"keys": load("cells.keys.u64", np.uint64), "n": load("cells.n.u32", np.uint32), "windows": load("cells.windows.u32", np.uint32),
             "xyz": load("cells.xyz.f32", np.float32).reshape(-1, 3)}
    ref.assert_maps_equal(cells, rm.extract())
