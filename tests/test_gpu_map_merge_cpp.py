"""dsi::WorldMap::merge / exportState / importState (tests/cpp/test_map_merge.cpp) on two cuts of the scene of
tests/map_prune_reference.py: the states the program dumps equal the numpy restatement's, array_equal on every array,
and the merges' counts equal its counts."""
import os
import subprocess

import numpy as np
import pytest

import map_merge_reference as mref
import map_prune_reference as pref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (3, 5)


def load(base):
    header = np.fromfile(base + ".header.f64", np.float64)
    return {"leaf": float(header[0]), "calls": int(header[1]), "accepted": int(header[2]), "rejected": int(header[3]),
            "keys": np.fromfile(base + ".keys.u64", np.uint64), "n": np.fromfile(base + ".n.u32", np.uint32),
            "S": np.fromfile(base + ".S.u64", np.uint64).reshape(-1, 3), "windows": np.fromfile(base + ".windows.u32", np.uint32),
            "stamp": np.fromfile(base + ".stamp.u32", np.uint32)}


def test_cpp_map_merge_on_two_cuts_of_the_scene(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_merge")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_merge.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    calls = pref.scene_calls()
    for k, (pts, _) in enumerate(calls):
        np.asarray(pts, np.float32).tofile(str(tmp_path / ("call_%d.f32" % k)))
    r = subprocess.run([exe, str(tmp_path), repr(pref.LEAF), str(len(calls))] + [str(c) for c in CUTS], capture_output=True, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    whole = mref.reference_of(calls).export_state()
    for cut in CUTS:
        base = str(tmp_path / ("cut_%d" % cut))
        first, rest = mref.reference_of(calls[:cut]), mref.reference_of(calls[cut:])
        occupied = len(first.keys)
        want = first.merge(rest)
        mref.assert_states_equal(load(base + ".merged"), first.export_state())
        mref.assert_states_equal(load(base + ".merged"), whole)
        mref.assert_states_equal(load(base + ".imported"), whole)
        info = np.fromfile(base + ".info.u64", np.uint64).tolist()
        assert info[:3] == [want["n_src_cells"], want["n_new"], want["n_common"]] and want["n_new"] >= 100 and want["n_common"] >= 400
        assert info[3] >= 4 * (occupied + want["n_src_cells"]) / 3 and info[3] & (info[3] - 1) == 0
        assert info[5:] == [1640, 1640, 0] + list(mref.grown_capacity(256, 0, 1640))
