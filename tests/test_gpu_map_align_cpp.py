"""dsi::WorldMap::align_step / align / integrate_map and dsi::compose_pose (tests/cpp/test_map_align.cpp) on the first scene
of tests/map_align_reference.py: the moments, the poses and the moved map the program writes equal the Python path's, bit
for bit."""
import os
import subprocess

import numpy as np
import pytest

import dvs_mcemvs_amd as d
import map_align_reference as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_map_align_on_scene_1(built, ctx, tmp_path):
    exe = str(tmp_path / "test_map_align")
    pkg = os.path.join(ROOT, "dvs_mcemvs_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "test_map_align.cpp"), "-I" + os.path.join(ROOT, "include"),
                           "-L" + pkg, "-ldsi_engine", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    ca, cb = ar.scene1_calls()
    for name, calls in (("a", ca), ("b", cb)):
        for k, pts in enumerate(calls):
            np.asarray(pts, np.float32).tofile(str(tmp_path / ("%s_%d.f32" % (name, k))))
    ar.T_TRUE_1.tofile(str(tmp_path / "T_step.f64"))
    o = ar.SCENE1_LOOP
    r = subprocess.run([exe, str(tmp_path), repr(ar.LEAF_A), str(len(ca)), repr(ar.LEAF_B), str(len(cb)), repr(o["radius"]),
                        str(o["max_iterations"]), str(o["min_matched"]), repr(o["eps_rot"]), repr(o["eps_trans"])],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    # the Python path on the same maps
    a, b = d.WorldMap(ctx, ar.LEAF_A, 12), d.WorldMap(ctx, ar.LEAF_B, 12)
    for wm, calls in ((a, ca), (b, cb)):
        for pts in calls:
            assert wm.integrate(pts, ar.IDENTITY) == 0
    m = a.alignStep(b, o["radius"], ar.T_TRUE_1)
    want = [m["n_cells"], m["n_matched"], m["n_unmatched"]] + m["su"] + m["sv"] + m["suv_hi"] + m["suv_lo"] + [m["e2"], m["reach"]]
    assert np.fromfile(str(tmp_path / "moments.i64"), np.int64).tolist() == want and m["n_matched"] >= 1500
    T_delta, _ = d.solve_alignment(m)
    assert np.array_equal(np.fromfile(str(tmp_path / "T_solve.f64"), np.float64), d.compose_pose(T_delta, ar.T_TRUE_1))
    T, info = a.align(b, **o)
    assert np.array_equal(np.fromfile(str(tmp_path / "T_out.f64"), np.float64), T)
    got = np.fromfile(str(tmp_path / "info.f64"), np.float64).tolist()
    assert got == [float(info[k]) for k in ("iterations", "converged", "stopped", "n_matched_first", "n_matched_last", "rms_first",
                                            "rms_last", "angle_last", "trans_last")]
    assert ar.pose_error(T, ar.T_TRUE_1) == ar.SCENE1_LOOP_RESULT["pose_error"]
    moved = d.WorldMap(ctx, ar.LEAF_B, 8)
    moved.integrateMap(a, T, 2, 1)
    s = moved.exportState()
    assert np.array_equal(np.fromfile(str(tmp_path / "moved.keys.u64"), np.uint64), s["keys"]) and len(s["keys"]) > 1000
    assert np.array_equal(np.fromfile(str(tmp_path / "moved.n.u32"), np.uint32), s["n"])
    assert np.array_equal(np.fromfile(str(tmp_path / "moved.S.u64"), np.uint64).reshape(-1, 3), s["S"])
    for wm in (a, b, moved):
        wm.close()
