"""dsi::WorldMap::components / fetchComponents / listComponents / selectComponents / pruneComponents
(tests/cpp/test_map_components.cpp) on the random scene of tests/map_prune_reference.py: the files the program dumps equal
the restatement of tests/map_components_reference.py, array_equal on the rows, the list, the counts and the pruned map."""
import copy
import os
import subprocess

import numpy as np
import pytest

import map_components_reference as cref
import map_layout_cases as lc
import map_prune_reference as pref
import world_map_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER, CONNECTIVITY = (2, 1), 18
SELECTION = dict(min_cells=2, min_component_points=6, keep_largest=3)


def test_cpp_map_components_on_the_random_scene(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_components")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_components.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    calls = pref.scene_calls()
    row = [pref.LEAF, len(calls), *FILTER, CONNECTIVITY, SELECTION["min_cells"], SELECTION["min_component_points"], SELECTION["keep_largest"]]
    np.asarray(row, np.float64).tofile(str(tmp_path / "opts.f64"))
    for k, (pts, _) in enumerate(calls):
        np.asarray(pts, np.float32).tofile(str(tmp_path / ("call_%d.f32" % k)))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    load = lambda name, dtype: np.fromfile(str(tmp_path / name), dtype)
    rm = copy.deepcopy(cref.scene_reference())
    comp = cref.scene_components(*FILTER, CONNECTIVITY)
    want = cref.select(rm, comp, **SELECTION)
    assert np.array_equal(load("rows.keys.u64", np.uint64), comp["keys"]) and np.array_equal(load("rows.labels.u64", np.uint64), comp["labels"])
    assert np.array_equal(load("rows.reason.u8", np.uint8), want["node_reason"])
    for k in ("labels", "cells", "points"):
        assert np.array_equal(load("list.%s.u64" % k, np.uint64), comp["list"][k]), k
    counts = [want["n_cells"], want["n_kept"]] + want["n_removed"] + [want["n_components_kept"]]
    labelling = [comp["info"][k] for k in ("n_cells", "n_unlabelled", "n_components", "n_singletons", "largest_label", "largest_cells",
                                            "largest_points")]
    assert want["n_kept"] >= 5 and min(want["n_removed"]) >= 1
    assert load("info.u64", np.uint64).tolist() == labelling + counts + [lc.grown_from(calls, pref.LEAF, 8)] + counts + [pref.shrunk_capacity(want["n_kept"])]
    cref.prune_components(rm, comp, **SELECTION)
    got = {"keys": load("cells.keys.u64", np.uint64), "n": load("cells.n.u32", np.uint32), "windows": load("cells.windows.u32", np.uint32),
           "xyz": load("cells.xyz.f32", np.float32).reshape(-1, 3)}
    ref.assert_maps_equal(got, rm.extract())
