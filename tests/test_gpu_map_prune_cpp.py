"""dsi::WorldMap::prune / classifyPrune / fetchPruneReasons (tests/cpp/test_map_prune.cpp) on the hand cases of
tests/map_prune_reference.py: the files the program dumps equal the numpy restatement and the cases' stated verdicts,
array_equal on the keys, the reasons, the counts and the pruned map's cells."""
import os
import subprocess

import numpy as np
import pytest

import map_prune_reference as pref
import world_map_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_map_prune_on_the_hand_cases(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_prune")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_prune.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    cases = pref.hand_cases()
    for i, case in enumerate(cases):
        o = dict(pref.DEFAULTS, **case["opts"])
        lo, hi = o["box"] if o["box"] is not None else ((0, 0, 0), (0, 0, 0))
        row = [case["leaf"], len(case["calls"]), o["min_points"], o["min_windows"], -1 if o["max_age"] is None else o["max_age"],
               0 if o["box"] is None else 1, *lo, *hi, o["reach"], o["min_neighbors"]]
        np.asarray(row, np.float64).tofile(str(tmp_path / ("case_%d.opts.f64" % i)))
        for k, (pts, _) in enumerate(case["calls"]):
            np.asarray(pts, np.float32).tofile(str(tmp_path / ("case_%d_%d.f32" % (i, k))))
    r = subprocess.run([exe, str(tmp_path), str(len(cases))], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    for i, case in enumerate(cases):
        base = str(tmp_path / ("case_%d" % i))
        rm = pref.run_hand_case(case, pref.PruneReferenceMap)
        want = rm.classify(**case["opts"])
        keys, reasons = pref.wanted_reasons(case)
        got_keys, got_reasons = np.fromfile(base + ".keys.u64", np.uint64), np.fromfile(base + ".reason.u8", np.uint8)
        assert np.array_equal(got_keys, want["keys"]) and np.array_equal(got_reasons, want["reason"]), case["name"]
        assert np.array_equal(got_keys, keys) and np.array_equal(got_reasons, reasons), case["name"]
        counts = [want["n_cells"], want["n_kept"]] + want["n_removed"]
        info = np.fromfile(base + ".info.u64", np.uint64).tolist()
        assert info == counts + [256] + counts + [pref.shrunk_capacity(want["n_kept"])], case["name"]
        rm.prune(**case["opts"])
        got = {"keys": np.fromfile(base + ".cells.keys.u64", np.uint64), "n": np.fromfile(base + ".cells.n.u32", np.uint32),
               "windows": np.fromfile(base + ".cells.windows.u32", np.uint32),
               "xyz": np.fromfile(base + ".cells.xyz.f32", np.float32).reshape(-1, 3)}
        ref.assert_maps_equal(got, rm.extract())
